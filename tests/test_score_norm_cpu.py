"""Score normalisation without a GPU: the golden file against a float64 restatement, the argument checks that run before any device
call, and the export tables."""
import os

import numpy
import pytest

import sidekit_amd
from sidekit_amd import score_normalization as sn
from sidekit_amd.bosaris import Scores


def _ids(prefix, n):
    return numpy.array([f"{prefix}{i:04d}" for i in range(n)], dtype="|O")


def _scores(models, segs, mat):
    s = Scores()
    s.modelset, s.segset, s.scoremat, s.scoremask = models, segs, numpy.array(mat, dtype=numpy.float64), numpy.ones(mat.shape, dtype="bool")
    return s


def test_golden_agrees_with_a_float64_restatement(golden_dir):
    fx = numpy.load(os.path.join(golden_dir, "score_norm.npz"))
    e, t, c = (fx[k].astype(numpy.float64) for k in ("enrol", "test", "cohort"))
    assert e.shape == (37, 256) and t.shape == (53, 256) and c.shape == (301, 256)
    for x in (e, t, c):
        numpy.testing.assert_allclose(numpy.linalg.norm(x, axis=1), 1.0, atol=1e-6)
    s, imp_test, enrol_imp = e @ t.T, c @ t.T, e @ c.T
    assert min(imp_test.std(0).min(), enrol_imp.std(1).min()) > 1e-3          # the conditioning the fixture promises
    numpy.testing.assert_allclose(fx["min_cohort_std"], min(imp_test.std(0).min(), enrol_imp.std(1).min()), rtol=1e-9)
    # 1e-10: the reference and this restatement differ by the order of float64 sums, amplified by 1 / std < 1e3
    numpy.testing.assert_allclose(fx["tnorm"], (s - imp_test.mean(0)) / imp_test.std(0), rtol=1e-10, atol=1e-10)
    numpy.testing.assert_allclose(fx["znorm"], (s - enrol_imp.mean(1)[:, None]) / enrol_imp.std(1)[:, None], rtol=1e-10, atol=1e-10)


def test_xvector_shape_checks_fire_before_any_device_call():
    x, c = numpy.zeros((5, 8), dtype=numpy.float32), numpy.zeros((7, 8), dtype=numpy.float32)
    with pytest.raises(ValueError, match="multiple of 4"):
        sn.cohort_stats_device(x, numpy.zeros((7, 12), dtype=numpy.float32))          # D mismatch
    with pytest.raises(ValueError, match="multiple of 4"):
        sn.cohort_stats_device(numpy.zeros((5, 6), dtype=numpy.float32), numpy.zeros((7, 6), dtype=numpy.float32))   # D % 4
    with pytest.raises(ValueError, match="topk"):
        sn.cohort_stats_device(x, c, topk=8)                                            # topk > M
    with pytest.raises(ValueError, match="topk"):
        sn.asnorm_trials(x, x, c, topk=200)
    with pytest.raises(ValueError, match="empty"):
        sn.cohort_stats_device(x, numpy.zeros((0, 8), dtype=numpy.float32))
    with pytest.raises(ValueError, match="together"):
        sn.cohort_stats_device(x, c, col_shift=numpy.zeros(7, dtype=numpy.float32))
    with pytest.raises(ValueError, match="one entry per cohort row"):
        sn.cohort_stats_device(x, c, col_shift=numpy.zeros(6, dtype=numpy.float32), col_scale=numpy.ones(6, dtype=numpy.float32))
    for fn in (sn.znorm_device, sn.tnorm_device):
        with pytest.raises(ValueError, match="multiple of 4"):
            fn(None, x, numpy.zeros((7, 12), dtype=numpy.float32))
    for fn in (sn.snorm_device, sn.ztnorm_device):
        with pytest.raises(ValueError, match="multiple of 4"):
            fn(None, x, numpy.zeros((3, 12), dtype=numpy.float32), c)


def test_matrix_checks_fire_before_any_device_call():
    with pytest.raises(ValueError, match="square"):
        sn.matrix_moments_device(numpy.zeros((3, 4), dtype=numpy.float32), 1, skip_diag=True)   # skip_diag on a non-square matrix
    with pytest.raises(ValueError, match="axis"):
        sn.matrix_moments_device(numpy.zeros((3, 3), dtype=numpy.float32), 2)
    lib = sidekit_amd._lib.lib()                                                               # the C entry points say the same
    assert lib.sc_matrix_moments(1, 3, 4, 1, 1, 1, 1, None) == sidekit_amd._lib.SK_EARG and "square" in sidekit_amd._lib.last_error()
    assert lib.sc_cohort_moments(None, 4, None, 0, 8, None, None, -1, None, None, None) == sidekit_amd._lib.SK_EARG    # M == 0
    assert lib.sc_cohort_moments(None, 1, None, 1, 8, None, None, 0, None, None, None) == sidekit_amd._lib.SK_EARG     # the row keeps no pair
    assert lib.sc_cohort_moments(None, 0, None, 5, 8, None, None, -1, None, None, None) == sidekit_amd._lib.SK_OK      # N == 0: nothing to do
    assert lib.sc_norm_apply(1, 2, 2, None, None, None, None, None) == sidekit_amd._lib.SK_EARG                        # neither pair


def test_scores_objects_must_share_their_sets():
    rs = numpy.random.RandomState(0)
    et = _scores(_ids("enr", 3), _ids("tst", 4), rs.randn(3, 4))
    with pytest.raises(ValueError, match="segset"):
        sn.tnorm(et, _scores(_ids("imp", 5), _ids("tst", 3), rs.randn(5, 3)))
    with pytest.raises(ValueError, match="segset"):
        sn.tnorm(et, _scores(_ids("imp", 5), _ids("seg", 4), rs.randn(5, 4)))
    with pytest.raises(ValueError, match="modelset"):
        sn.znorm(et, _scores(_ids("mod", 3), _ids("imp", 5), rs.randn(3, 5)))
    with pytest.raises(ValueError, match="square"):
        sn.znorm(et, _scores(_ids("enr", 3), _ids("imp", 5), rs.randn(3, 5)), sym=True)
    with pytest.raises(ValueError, match="modelset"):                                         # ztnorm: the first znorm already objects
        sn.ztnorm(et, _scores(_ids("mod", 3), _ids("imp", 5), rs.randn(3, 5)), _scores(_ids("imp", 5), _ids("tst", 4), rs.randn(5, 4)),
                  _scores(_ids("imp", 5), _ids("imp", 5), rs.randn(5, 5)))
    assert et.scoremat.shape == (3, 4)                                                        # the first argument is never touched


def test_new_names_are_exported():
    names = ("znorm", "tnorm", "ztnorm", "asnorm_trials", "cohort_stats_device", "znorm_device", "tnorm_device", "snorm_device",
             "ztnorm_device")
    for name in names:
        assert sidekit_amd._LAZY[name] == "score_normalization"
        assert getattr(sidekit_amd, name) is getattr(sn, name)
    for sym in ("sc_cohort_moments", "sc_norm_apply", "sc_matrix_moments"):
        assert sym in sidekit_amd._lib.SIGNATURES
    import inspect
    assert list(inspect.signature(sn.znorm).parameters) == ["enrol_test_scores", "enrol_imp_scores", "sym"]                 # :44
    assert list(inspect.signature(sn.tnorm).parameters) == ["enrol_test_scores", "imp_test_scores"]                          # :75
    assert list(inspect.signature(sn.ztnorm).parameters) == ["enrol_test_scores", "enrol_imp_scores", "imp_test_scores", "imp_imp_scores"]   # :96
