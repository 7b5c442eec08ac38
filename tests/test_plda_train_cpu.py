"""PLDA training, the parts that need no GPU: the tests' numpy yardstick is pinned by the reference's own output, the module imports,
the model file round-trips in the reference's layout, and the new entry points reject bad arguments before touching a device."""
import os
import subprocess
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plda_em_numpy as pen  # noqa: E402

H5PY_PYTHON = "/opt/conda/bin/python3.9"


def _assert_model(got, want, tol, what):
    mu, F, Sigma = got
    mu_r, F_r, Sigma_r = want
    errs = {"mu": numpy.abs(mu - mu_r).max() / numpy.abs(mu_r).max(), "Sigma": pen.rel(Sigma, Sigma_r),
            "FF'": pen.rel(F.dot(F.T), F_r.dot(F_r.T)), "F": pen.rel(pen.sign_align(F, F_r), F_r)}
    print(what, {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < tol, f"{what}: {k} differs from the reference by {v:.3e} (relative max-norm, bound {tol})"


@pytest.mark.parametrize("eigen_form", [False, True])
def test_restatement_matches_the_reference_on_config5(golden_dir, eigen_form):
    """400 speakers x 8 sessions, D 256, rank 128, 10 iterations: config5.npz holds what the reference's FactorAnalyser.plda trained."""
    sys.path.insert(0, golden_dir)
    import config5_inputs as c5
    fx = numpy.load(os.path.join(golden_dir, "config5.npz"))
    X, lab = c5.plda_training_set()
    numpy.testing.assert_array_equal(c5.digest(X), fx["X_digest"])
    _assert_model(pen.em(X, lab, c5.PLDA_RANK, 10, eigen_form=eigen_form), (fx["mu"], fx["F"], fx["Sigma"]), 1e-12, f"config5 eigen_form={eigen_form}")


@pytest.mark.parametrize("eigen_form", [False, True])
@pytest.mark.parametrize("k", [0, 1])
def test_restatement_matches_the_reference_on_the_ragged_set(golden_dir, k, eigen_form):
    """60 classes of 1-12 sessions, string ids, shuffled rows, scaling_factor 1.0 and 0.7 (tests/golden/make_plda_train_golden.py)."""
    fx = numpy.load(os.path.join(golden_dir, "plda_train.npz"))
    X, ids = pen.ragged_set()
    numpy.testing.assert_array_equal(X, fx["X"])
    assert list(ids) == list(fx["modelset"]) and numpy.unique(ids, return_counts=True)[1].min() == 1
    got = pen.em(X, ids, int(fx["rank"]), int(fx["nb_iter"]), float(fx["scalings"][k]), eigen_form=eigen_form)
    _assert_model(got, (fx[f"mean_{k}"], fx[f"F_{k}"], fx[f"Sigma_{k}"]), 1e-12, f"ragged scaling={fx['scalings'][k]} eigen_form={eigen_form}")


def test_module_imports_and_is_wired_into_the_package():
    import sidekit_amd
    from sidekit_amd import factor_analyser
    assert "factor_analyser" in sidekit_amd.SUBMODULES
    assert sidekit_amd.FactorAnalyser is factor_analyser.FactorAnalyser
    fa = factor_analyser.FactorAnalyser(mean=numpy.zeros(3))
    assert fa.F is None and fa.G is None and fa.H is None and fa.Sigma is None and fa.mean.shape == (3,)


def test_class_index_is_a_csr_of_slices_that_never_straddle_a_class():
    from sidekit_amd.factor_analyser import SLICE_ROWS, ClassIndex
    rs = numpy.random.RandomState(0)
    labels = numpy.concatenate((rs.randint(0, 7, 500), numpy.full(3 * SLICE_ROWS + 5, 9), [11]))
    rs.shuffle(labels)
    ix = ClassIndex(labels)
    assert list(ix.ids) == sorted(set(labels)) and ix.counts.sum() == labels.shape[0]
    assert ix.slice_off[0] == 0 and ix.slice_off[-1] == labels.shape[0] and (numpy.diff(ix.slice_off) > 0).all()
    assert numpy.diff(ix.slice_off).max() <= SLICE_ROWS
    for c in range(ix.ids.shape[0]):
        rows = ix.rows[ix.slice_off[ix.class_slice_off[c]]:ix.slice_off[ix.class_slice_off[c + 1]]]
        assert (ix.inverse[rows] == c).all() and rows.shape[0] == ix.counts[c] and (numpy.diff(rows) > 0).all()


def test_sum_stat_per_model_matches_a_per_model_scan():
    """On a machine without a GPU this is the host grouping; with one, the class-sum kernel."""
    from sidekit_amd.statserver import StatServer
    X, ids = pen.ragged_set()
    s = StatServer.from_arrays(ids, numpy.array([f"s{i}" for i in range(X.shape[0])], dtype="|O"), X)
    out, sessions = s.sum_stat_per_model()
    assert list(out.modelset) == sorted(set(ids)) and out.validate()
    for i, m in enumerate(out.modelset):
        numpy.testing.assert_allclose(out.stat1[i], X[ids == m].sum(axis=0), rtol=1e-13, atol=1e-15)
        assert out.stat0[i, 0] == sessions[i] == (ids == m).sum()


def test_write_read_round_trip(tmp_path):
    from sidekit_amd.factor_analyser import FactorAnalyser
    rs = numpy.random.RandomState(1)
    full = FactorAnalyser(mean=rs.randn(48), F=rs.randn(48, 16), G=rs.randn(48, 4), H=rs.randn(48), Sigma=rs.randn(48, 48))
    full.write(str(tmp_path / "sub" / "full.h5"))
    for back in (FactorAnalyser.read(str(tmp_path / "sub" / "full.h5")), FactorAnalyser(str(tmp_path / "sub" / "full.h5"))):
        for name in ("mean", "F", "G", "H", "Sigma"):
            got = getattr(back, name)
            assert got.dtype == numpy.float64
            numpy.testing.assert_array_equal(got, getattr(full, name))
    part = FactorAnalyser(mean=full.mean, F=full.F, Sigma=full.Sigma)      # what plda() leaves: no G, no H
    part.write(str(tmp_path / "plda.h5"))
    back = FactorAnalyser.read(str(tmp_path / "plda.h5"))
    assert back.G is None and back.H is None
    numpy.testing.assert_array_equal(back.F, full.F)
    numpy.testing.assert_array_equal(back.Sigma, full.Sigma)


@pytest.mark.skipif(not os.path.exists(H5PY_PYTHON), reason="no interpreter with h5py on this machine")
def test_h5py_reads_the_model_file(tmp_path):
    from sidekit_amd.factor_analyser import FactorAnalyser
    if subprocess.run([H5PY_PYTHON, "-c", "import h5py"], capture_output=True).returncode != 0:
        pytest.skip("that interpreter has no h5py")
    rs = numpy.random.RandomState(2)
    fa = FactorAnalyser(mean=rs.randn(8), F=rs.randn(8, 3), G=rs.randn(8, 2), H=rs.randn(8), Sigma=rs.randn(8, 8))
    path = str(tmp_path / "fa.h5")
    fa.write(path)
    code = ("import h5py, sys\n"
            "with h5py.File(sys.argv[1], 'r') as f:\n"
            "    print(sorted(f['fa'].keys()), f['fa/kind'][()].tolist(), str(f['fa/kind'].dtype), f['fa/f'].shape, float(f['fa/sigma'][()].sum()))\n")
    out = subprocess.run([H5PY_PYTHON, "-c", code, path], capture_output=True, text=True, check=True).stdout
    assert out.startswith("['f', 'g', 'h', 'kind', 'mean', 'sigma'] [1, 1, 1, 1, 1] int16 (8, 3)"), out
    assert abs(float(out.split()[-1]) - fa.Sigma.sum()) < 1e-12


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    from sidekit_amd import _lib
    lib = _lib.lib()
    assert lib.sc_class_sums(None, _lib.XT_F32, 10, 4, None, None, 1, None, 1, None, None, None) == _lib.SK_EARG
    assert "sc_class_sums" in _lib.last_error() and "null" in _lib.last_error()
    assert lib.sc_gemm_tn(None, None, _lib.XT_F64, 10, 4, 4, None, None, None, None, None) == _lib.SK_EARG
    assert "sc_gemm_tn" in _lib.last_error()
    assert lib.sc_dgemm_nn(None, None, 4, 4, 4, 1.0, None, None, _lib.SC_EPI_RANK1, None, None) == _lib.SK_EARG
    assert "sc_dgemm_nn" in _lib.last_error()
    one = 8   # any non-null address: the size checks come before any use of it
    assert lib.sc_class_sums(one, _lib.XT_BF16, 10, 4, one, one, 1, one, 1, one, None, None) == _lib.SK_EARG
    assert lib.sc_class_sums(one, _lib.XT_F32, 0, 4, one, one, 1, one, 1, one, None, None) == _lib.SK_EARG
    assert lib.sc_gemm_tn(one, one, _lib.XT_F32, 0, 4, 4, None, None, None, one, None) == _lib.SK_EARG
    assert lib.sc_gemm_tn(one, one, _lib.XT_I16, 10, 4, 4, None, None, None, one, None) == _lib.SK_EARG
    assert lib.sc_dgemm_nn(one, one, 4, 0, 4, 1.0, None, None, _lib.SC_EPI_RANK1, one, None) == _lib.SK_EARG
    assert lib.sc_dgemm_nn(one, one, 4, 4, 4, 1.0, None, None, _lib.SC_EPI_POSTERIOR, one, None) == _lib.SK_EARG
    assert lib.sc_dgemm_nn(one, one, 4, 4, 4, 1.0, None, None, 7, one, None) == _lib.SK_EARG


def test_resolves_under_the_reference_name():
    code = ("import sidekit_amd\n"
            "sidekit_amd.install_as_sidekit()\n"
            "import sidekit.factor_analyser\n"
            "from sidekit.factor_analyser import FactorAnalyser\n"
            "import sidekit\n"
            "assert sidekit.FactorAnalyser is FactorAnalyser and FactorAnalyser.__module__ == 'sidekit_amd.factor_analyser'\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr
