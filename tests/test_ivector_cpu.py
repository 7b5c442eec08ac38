"""Total variability without a GPU (sidekit_amd/factor_analyser.py, csrc/ivector.hip): the numpy restatement the GPU tests lean on
against the reference's own output (tests/golden/ivector.npz, written by make_ivector_golden.py from the imported reference module), the
host M-step against the fixture's accumulators, the entry points' own header against their binding table and the built library, their
argument checks through the C ABI, the refusals, the packed index, the reference's parameter lists and the i-vector ``StatServer`` file.

The restatement is held to 1e-12 relative max-norm, the bar make_backend_golden.py sets for a restatement of float64 algebra (the
generator measured at most 1.5e-15 on this set, whose inverted and solved matrices have condition numbers below 20).
"""
import inspect
import os
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ivector_numpy as ivn  # noqa: E402

from sidekit_amd import _lib, factor_analyser  # noqa: E402
from sidekit_amd.factor_analyser import FactorAnalyser  # noqa: E402
from sidekit_amd.mixture import Mixture  # noqa: E402
from sidekit_amd.statserver import StatServer  # noqa: E402

RESTATEMENT_TOL = 1e-12
C, D, R, N = 6, 5, 7, 40


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(numpy.load(os.path.join(golden_dir, "ivector.npz")))


def _batches(fx):
    n, size = fx["stat0"].shape[0], int(fx["batch_size"])
    return numpy.array_split(numpy.arange(n), int(numpy.floor(n / float(size) + 0.999)))


def _ubm(fx):
    m = Mixture()
    m.w, m.mu, m.invcov = (numpy.array(fx[k], dtype=numpy.float64) for k in ("w", "mu", "invcov"))
    m.cov_var_ctl = 1.0 / m.invcov
    m.cst, m.det = numpy.zeros(m.w.shape), numpy.zeros(m.w.shape)
    m._compute_all()
    return m


def _assert_all(errs, tol=RESTATEMENT_TOL):
    print({k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < tol, f"{k} differs by {v:.3e} (relative max-norm, bound {tol})"


def test_fixture_is_the_set_its_generator_describes(fx):
    assert fx["stat0"].shape == (N, C) and fx["stat1"].shape == (N, C * D) and fx["tv_init"].shape == (C * D, R)
    assert [len(b) for b in _batches(fx)] == [14, 13, 13]
    assert numpy.all(fx["stat0"] > 0) and 25 < fx["stat0"].sum(1).min() and fx["stat0"].sum(1).max() < 75
    for k in ("stat0", "stat1"):   # a StatServer file stores float32: the fixture's statistics survive it bit for bit
        numpy.testing.assert_array_equal(fx[k], fx[k].astype(numpy.float32).astype(numpy.float64))
    assert fx["e_h"].shape == (N, R) and fx["e_hh"].shape == (N, R * (R + 1) // 2) and fx["A"].shape == (C, 28) and fx["C"].shape == (R, C * D)
    assert fx["iv"].shape == fx["iv_sigma"].shape == (N, R)
    lam = numpy.eye(R)[None] + ivn.unpack(fx["stat0"].dot(ivn.gram(fx["tv_init"], C, D)), R)
    assert max(numpy.linalg.cond(m) for m in lam) <= 1e3
    assert max(numpy.linalg.cond(m) for m in ivn.unpack(fx["A"], R)) <= 1e4 and numpy.linalg.cond(ivn.unpack(fx["R"] / N, R)) <= 1e4


def test_restatement_matches_the_reference_fixture(fx):
    s0, s1, mu, ic, b = fx["stat0"], fx["stat1"], fx["mu"], fx["invcov"], _batches(fx)
    _, acc, e_h, e_hh = ivn.em_iteration(s0, s1, mu, ic, fx["tv_init"], b, True)
    errs = {"e_h": ivn.rel(e_h, fx["e_h"]), "e_hh": ivn.rel(e_hh, fx["e_hh"]), "_A": ivn.rel(acc[0], fx["A"]), "_C": ivn.rel(acc[1], fx["C"]),
            "_R": ivn.rel(acc[2], fx["R"])}
    for tag, min_div in (("md", True), ("nomd", False)):
        for i, F in enumerate(ivn.train(s0, s1, mu, ic, fx["tv_init"], 3, b, min_div)):
            errs[f"F {tag} it{i}"] = ivn.rel(F, fx[f"F_{tag}_it{i}"])
    iv, sigma = ivn.extract(s0, s1, mu, ic, fx["F_md_it2"])
    errs.update({"iv": ivn.rel(iv, fx["iv"]), "iv_sigma": ivn.rel(sigma, fx["iv_sigma"]),
                 "whitened stat1": ivn.rel(ivn.whiten(s0, s1, mu, ic), fx["stat1_whitened"])})
    _assert_all(errs)


def test_host_m_step_against_the_fixture(fx):
    errs = {"M-step and minimum divergence": ivn.rel(factor_analyser.tv_m_step(fx["A"], fx["C"], fx["R"], N, True), fx["F_md_it0"]),
            "M-step alone": ivn.rel(factor_analyser.tv_m_step(fx["A"], fx["C"], fx["R"], N, False), fx["F_nomd_it0"]),
            "restatement's M-step": ivn.rel(ivn.m_step(fx["A"], fx["C"], fx["R"], N, True), fx["F_md_it0"])}
    _assert_all(errs)
    A, Cm, Rm = fx["A"].copy(), fx["C"].copy(), fx["R"].copy()
    factor_analyser.tv_m_step(A, Cm, Rm, N, True)
    assert numpy.array_equal(A, fx["A"]) and numpy.array_equal(Cm, fx["C"]) and numpy.array_equal(Rm, fx["R"]), "the accumulators are left as they are"


def test_packed_index_is_numpy_triu_order():
    for rank in (1, 2, 7, 64, 65, 192):
        rows, cols = numpy.triu_indices(rank)
        want = numpy.arange(rows.shape[0])
        numpy.testing.assert_array_equal(rows * rank - rows * (rows - 1) // 2 + (cols - rows), want)
        numpy.testing.assert_array_equal([ivn.packed_index(i, j, rank) for i, j in zip(rows[:300], cols[:300])], want[:300])
        assert factor_analyser.packed_size(rank) == want.shape[0]
        full = numpy.random.RandomState(rank).randn(rank, rank)
        full = full + full.T
        numpy.testing.assert_array_equal(factor_analyser._unpack(ivn.pack(full), rank), full)
        numpy.testing.assert_array_equal(ivn.unpack(ivn.pack(full), rank), full)


def test_header_binding_table_and_library_agree():
    """What tests/test_abi.py checks for include/sidekit_amd.h, for the i-vector header and table."""
    import ctypes
    import re
    src = open(os.path.join(ROOT, "include", "sidekit_amd", "ivector.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?(?:int|char\s*\*|void)\s*\**\s*((?:xt|sc|sk)_\w+)\s*\(", src, flags=re.M)))
    assert declared == ["sc_tv_gram", "sc_tv_posterior"]
    assert sorted(_lib.IVECTOR_SIGNATURES) == declared, "ctypes binding table and header disagree"
    assert not set(_lib.IVECTOR_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.GAUSSIAN_SIGNATURES) | set(_lib.MIXTURE_SIGNATURES))
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(cdll, name), f"{name} declared in include/sidekit_amd/ivector.h but not exported"
    lib = _lib.lib()
    for name, (res, args) in _lib.IVECTOR_SIGNATURES.items():
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    ctype = {"void*": _lib._P, "int32_t": _lib._I32, "int64_t": _lib._I64, "double": _lib._F64}
    flat = re.sub(r"\s+", " ", src)
    for name, (_, args) in _lib.IVECTOR_SIGNATURES.items():
        params = re.search(r"int %s\((.*?)\);" % name, flat).group(1).split(",")
        kinds = ["void*" if "*" in q else q.replace("const", "").split()[0] for q in params]
        assert [ctype[k] for k in kinds] == args, (name, kinds)
    cap = int(re.search(r"#define SC_TV_MAX_RANK (\d+)", src).group(1))
    assert cap == factor_analyser.TV_MAX_RANK == 192
    assert (cap * (cap + 1) // 2 + 3 * cap + 2 * 256) * 8 <= 163840, "the packed triangle, three vectors and the partial sums fit the LDS a workgroup may declare"


def test_entry_points_check_their_arguments_before_anything_is_enqueued():
    """SK_EARG through the C ABI on a host with no GPU: nothing was enqueued, or there would have been a HIP error instead."""
    lib = _lib.lib()
    p = 4096   # any non-null address: a refused call dereferences nothing

    def gram(F=p, C=3, D=4, R=5, G=p):
        return lib.sc_tv_gram(F, C, D, R, G, None)

    def post(Lp=p, B=p, N=2, R=5, Eh=p, Ehh=p, diag=p):
        return lib.sc_tv_posterior(Lp, B, N, R, Eh, Ehh, diag, None)

    cases = {"gram F null": gram(F=None), "gram G null": gram(G=None), "gram R = 0": gram(R=0), "gram R = 193": gram(R=193), "gram R < 0": gram(R=-1),
             "gram C = 0": gram(C=0), "gram C < 0": gram(C=-3), "gram D = 0": gram(D=0), "gram D < 0": gram(D=-1),
             "posterior Lp null": post(Lp=None), "posterior B null": post(B=None), "posterior Eh null": post(Eh=None),
             "posterior both outputs null": post(Ehh=None, diag=None), "posterior R = 0": post(R=0), "posterior R = 193": post(R=193),
             "posterior R < 0": post(R=-2), "posterior N = 0": post(N=0), "posterior N < 0": post(N=-1)}
    assert all(rc == _lib.SK_EARG for rc in cases.values()), cases
    assert "sc_tv_posterior" in _lib.last_error()


def _server(fx):
    names = numpy.array([f"s{i:02d}" for i in range(N)], dtype="|O")
    s = StatServer()
    s.modelset, s.segset = names.copy(), names.copy()
    s.start, s.stop = numpy.empty(N, dtype="|O"), numpy.empty(N, dtype="|O")
    s.stat0, s.stat1 = fx["stat0"].copy(), fx["stat1"].copy()
    return s


def test_rank_above_the_cap_and_full_covariances_are_refused(fx):
    ubm, server = _ubm(fx), _server(fx)
    fa = FactorAnalyser()
    with pytest.raises(ValueError, match="192"):
        fa.total_variability(server, ubm, 193, nb_iter=1)
    with pytest.raises(ValueError, match="192"):
        fa.total_variability_single(server, ubm, 0, nb_iter=1)
    with pytest.raises(ValueError, match="192"):
        factor_analyser.total_variability_device(None, None, ubm, 193)
    fa.F = numpy.zeros((C * D, 193))
    for call in (lambda: fa.extract_ivectors(ubm, server), lambda: fa.extract_ivectors_single(ubm, server),
                 lambda: factor_analyser.extract_ivectors_device(None, None, ubm, fa.F)):
        with pytest.raises(ValueError, match="192"):
            call()
    numpy.testing.assert_array_equal(server.stat1, fx["stat1"])   # refused before anything was whitened
    full = _ubm(fx)
    full.invcov = numpy.stack([numpy.diag(v) for v in full.invcov])
    assert full.validate()
    fa.F = fx["tv_init"]
    for call in (lambda: fa.total_variability(server, full, R, nb_iter=1), lambda: fa.total_variability_single(server, full, R, nb_iter=1),
                 lambda: fa.extract_ivectors(full, server), lambda: fa.extract_ivectors_single(full, server),
                 lambda: factor_analyser.total_variability_device(None, None, full, R),
                 lambda: factor_analyser.extract_ivectors_device(None, None, full, fa.F)):
        with pytest.raises(NotImplementedError, match="full-covariance"):
            call()
    for name in ("total_variability_raw", "weighted_likelihood_plda"):
        assert not hasattr(FactorAnalyser, name)


def test_without_a_gpu_training_and_extraction_raise(fx, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    ubm, server = _ubm(fx), _server(fx)
    fa = FactorAnalyser(F=fx["tv_init"])
    for call in (lambda: fa.total_variability(server, ubm, R, nb_iter=1), lambda: fa.extract_ivectors(ubm, server),
                 lambda: fa.extract_ivectors_single(ubm, server)):
        with pytest.raises(RuntimeError, match="no GPU is visible"):
            call()
    numpy.testing.assert_array_equal(server.stat1, fx["stat1"])


def test_reference_parameter_lists():
    expect = {"total_variability": "(self, stat_server_filename, ubm, tv_rank, nb_iter=20, min_div=True, tv_init=None, batch_size=300, "
                                   "save_init=False, output_file_name=None, num_thread=1)",
              "total_variability_single": "(self, stat_server_filename, ubm, tv_rank, nb_iter=20, min_div=True, tv_init=None, batch_size=300, "
                                          "save_init=False, output_file_name=None)",
              "extract_ivectors": "(self, ubm, stat_server_filename, prefix='', batch_size=300, uncertainty=False, num_thread=1)",
              "extract_ivectors_single": "(self, ubm, stat_server, uncertainty=False)"}
    for name, sig in expect.items():
        assert str(inspect.signature(getattr(FactorAnalyser, name))) == sig, name
    device = {"tv_posterior_device": "(stat0, stat1_w, F, G=None, want='packed')",
              "total_variability_device": "(stat0, stat1, ubm, tv_rank, nb_iter=20, min_div=True, tv_init=None, max_workspace_bytes=1073741824, "
                                          "after_iteration=None)",
              "extract_ivectors_device": "(stat0, stat1, ubm, F, uncertainty=False, max_workspace_bytes=1073741824)"}
    for name, sig in device.items():
        assert str(inspect.signature(getattr(factor_analyser, name))) == sig, name
    # the device batch: P + C D + C + 2 R doubles per session, one session at least
    per = 8 * (R * (R + 1) // 2 + C * D + C + 2 * R)
    assert factor_analyser._batch_rows(N, C, D, R, 13 * per + per - 1) == 13 and factor_analyser._batch_rows(N, C, D, R, 1) == 1
    assert factor_analyser._batch_rows(N, C, D, R, 1 << 30) == N


def test_ivector_statserver_round_trips_through_its_file(fx, tmp_path):
    server = _server(fx)
    iv = factor_analyser._ivector_server(server, fx["iv"].astype(numpy.float32).astype(numpy.float64))
    assert iv.validate() and numpy.array_equal(iv.stat0, numpy.ones((N, 1))) and iv.modelset is not server.modelset
    path = str(tmp_path / "iv.h5")
    iv.write(path)
    back = StatServer.read(path)
    for name in ("modelset", "segset", "stat0", "stat1"):
        numpy.testing.assert_array_equal(getattr(back, name), getattr(iv, name))
    assert back.start.shape == (N,) and all(v is None for v in back.start) and all(v is None for v in back.stop)
    assert back.stat1.shape == (N, R)


def test_save_init_needs_an_output_file_name(fx):
    with pytest.raises(AssertionError, match="output_file_name"):
        FactorAnalyser().total_variability(_server(fx), _ubm(fx), R, nb_iter=1, save_init=True)
