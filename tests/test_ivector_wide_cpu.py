"""Total variability at ranks above 192 without a GPU (sidekit_amd/factor_analyser_wide.py, csrc/ivector_wide.hip): the entry points'
header against their binding table and the built library, their argument checks through the C ABI, the scratch size, the refusals, the
parameter lists, and the host-side algebra of the device M-step against the reference's own output (tests/golden/ivector.npz) with the
inverses injected from numpy."""
import ctypes
import inspect
import os
import re
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ivector_numpy as ivn  # noqa: E402

from sidekit_amd import _lib, factor_analyser, factor_analyser_wide as faw  # noqa: E402
from sidekit_amd.factor_analyser import FactorAnalyser  # noqa: E402
from sidekit_amd.factor_analyser_wide import WideFactorAnalyser  # noqa: E402
from sidekit_amd.mixture import Mixture  # noqa: E402
from sidekit_amd.statserver import StatServer  # noqa: E402

RESTATEMENT_TOL = 1e-12   # tests/test_ivector_cpu.py's bar for float64 algebra on this fixture (condition numbers below 20)
C, D, R, N = 6, 5, 7, 40


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(numpy.load(os.path.join(golden_dir, "ivector.npz")))


def _ubm(fx):
    m = Mixture()
    m.w, m.mu, m.invcov = (numpy.array(fx[k], dtype=numpy.float64) for k in ("w", "mu", "invcov"))
    m.cov_var_ctl = 1.0 / m.invcov
    m.cst, m.det = numpy.zeros(m.w.shape), numpy.zeros(m.w.shape)
    m._compute_all()
    return m


def _server(fx):
    names = numpy.array([f"s{i:02d}" for i in range(N)], dtype="|O")
    s = StatServer()
    s.modelset, s.segset = names.copy(), names.copy()
    s.start, s.stop = numpy.empty(N, dtype="|O"), numpy.empty(N, dtype="|O")
    s.stat0, s.stat1 = fx["stat0"].copy(), fx["stat1"].copy()
    return s


def test_header_binding_table_and_library_agree():
    """What tests/test_ivector_cpu.py checks for ivector.h, for the wide header and table."""
    src = open(os.path.join(ROOT, "include", "sidekit_amd", "ivector_wide.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?(?:int|char\s*\*|void)\s*\**\s*((?:xt|sc|sk)_\w+)\s*\(", src, flags=re.M)))
    assert declared == ["sc_tvw_gram", "sc_tvw_posterior", "sc_tvw_workspace"]
    assert sorted(_lib.IVECTOR_WIDE_SIGNATURES) == declared, "ctypes binding table and header disagree"
    others = [name for name in dir(_lib) if name.endswith("SIGNATURES") and name != "IVECTOR_WIDE_SIGNATURES"]
    assert "IVECTOR_SIGNATURES" in others and "SIGNATURES" in others and len(others) >= 14
    for name in others:
        assert not set(_lib.IVECTOR_WIDE_SIGNATURES) & set(getattr(_lib, name)), name
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(cdll, name), f"{name} declared in include/sidekit_amd/ivector_wide.h but not exported"
    lib = _lib.lib()
    for name, (res, args) in _lib.IVECTOR_WIDE_SIGNATURES.items():
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    ctype = {"void*": _lib._P, "int32_t": _lib._I32, "int64_t": _lib._I64, "double": _lib._F64}
    flat = re.sub(r"\s+", " ", src)
    for name, (_, args) in _lib.IVECTOR_WIDE_SIGNATURES.items():
        params = re.search(r"int %s\((.*?)\);" % name, flat).group(1).split(",")
        kinds = ["void*" if "*" in q else q.replace("const", "").split()[0] for q in params]
        assert [ctype[k] for k in kinds] == args, (name, kinds)
    cap = int(re.search(r"#define SC_TVW_MAX_RANK (\d+)", src).group(1))
    assert cap == faw.TVW_MAX_RANK == _lib.SC_TVW_MAX_RANK == 1024
    assert factor_analyser.TV_MAX_RANK == 192, "the narrow surface keeps its cap"


def _workspace(n, r):
    need = ctypes.c_int64(-1)
    rc = _lib.lib().sc_tvw_workspace(n, r, ctypes.byref(need))
    return rc, need.value


def test_entry_points_check_their_arguments_before_anything_is_enqueued():
    """SK_EARG through the C ABI on a host with no GPU: nothing was enqueued, or there would have been a HIP error instead."""
    lib = _lib.lib()
    p = 4096   # any non-null address: a refused call dereferences nothing
    enough = _workspace(2, 5)[1]

    def gram(F=p, C=3, D=4, R=5, G=p):
        return lib.sc_tvw_gram(F, C, D, R, G, None)

    def post(Lp=p, B=p, N=2, R=5, shift=1.0, Eh=p, Ehh=p, diag=p, work=p, nbytes=enough):
        return lib.sc_tvw_posterior(Lp, B, N, R, shift, Eh, Ehh, diag, work, nbytes, None)

    cases = {"gram F null": gram(F=None), "gram G null": gram(G=None), "gram R = 0": gram(R=0), "gram R = 1025": gram(R=1025),
             "gram R < 0": gram(R=-1), "gram C = 0": gram(C=0), "gram D = 0": gram(D=0),
             "workspace bytes null": lib.sc_tvw_workspace(2, 5, None), "workspace N = 0": _workspace(0, 5)[0],
             "workspace R = 0": _workspace(2, 0)[0], "workspace R = 1025": _workspace(2, 1025)[0],
             "posterior Lp null": post(Lp=None), "posterior work null": post(work=None),
             "posterior B null with Eh set": post(B=None), "posterior Eh null with B set": post(Eh=None),
             "posterior both outputs null": post(Ehh=None, diag=None), "posterior R = 0": post(R=0), "posterior R = 1025": post(R=1025),
             "posterior R < 0": post(R=-2), "posterior N = 0": post(N=0), "posterior N < 0": post(N=-1),
             "posterior shift < 0": post(shift=-1e-300), "posterior shift nan": post(shift=float("nan")),
             "posterior shift inf": post(shift=float("inf")), "posterior one byte short": post(nbytes=enough - 1),
             "posterior one byte short at rank 1024": post(R=1024, nbytes=_workspace(2, 1024)[1] - 1)}
    assert all(rc == _lib.SK_EARG for rc in cases.values()), cases
    assert "sc_tvw_posterior" in _lib.last_error()


def test_workspace_is_monotone_and_within_its_bound():
    """N sessions of 2 Rp^2 + O(Rp) doubles, Rp = R rounded up to 64"""
    last = 0
    for r in range(1, 1025):
        rc, one = _workspace(1, r)
        assert rc == _lib.SK_OK
        rp = (r + 63) // 64 * 64
        assert 8 * 2 * rp * rp <= one <= 8 * (2 * rp * rp + 64 * rp), r
        assert one >= last, "monotone in R"
        last = one
        if r in (1, 64, 65, 400, 1024):
            sizes = [_workspace(n, r)[1] for n in (1, 2, 3, 260, 100000)]
            assert sizes == sorted(sizes) and sizes[1] == 2 * one and sizes[4] == 100000 * one, "monotone (linear) in N"
            assert faw.workspace_bytes(3, r) == sizes[2]
    assert _workspace(2 ** 31 - 1, 1024)[1] == (2 ** 31 - 1) * 8 * 2 * 1024 * 1024, "no 32-bit product on the way"
    # the device batch counts the scratch: P + C D + C + 2 R + 2 Rp^2 doubles per session, one session at least
    per = 8 * (200 * 201 // 2 + 8 * 26 + 8 + 2 * 200) + faw.workspace_bytes(1, 200)
    assert faw._batch_rows(260, 8, 26, 200, 100 * per + per - 1) == 100 and faw._batch_rows(260, 8, 26, 200, 1) == 1
    assert faw._batch_rows(260, 8, 26, 200, 1 << 40) == 260


def test_rank_above_the_cap_and_full_covariances_are_refused(fx):
    ubm, server = _ubm(fx), _server(fx)
    fa = WideFactorAnalyser()
    with pytest.raises(ValueError, match="1024"):
        fa.total_variability(server, ubm, 1025, nb_iter=1)
    with pytest.raises(ValueError, match="1024"):
        fa.total_variability_single(server, ubm, 0, nb_iter=1)
    with pytest.raises(ValueError, match="1024"):
        faw.total_variability_wide_device(None, None, ubm, 1025)
    fa.F = numpy.zeros((C * D, 1025))
    for call in (lambda: fa.extract_ivectors(ubm, server), lambda: fa.extract_ivectors_single(ubm, server),
                 lambda: faw.extract_ivectors_wide_device(None, None, ubm, fa.F)):
        with pytest.raises(ValueError, match="1024"):
            call()
    numpy.testing.assert_array_equal(server.stat1, fx["stat1"])   # refused before anything was whitened
    full = _ubm(fx)
    full.invcov = numpy.stack([numpy.diag(v) for v in full.invcov])
    assert full.validate()
    fa.F = fx["tv_init"]
    for call in (lambda: fa.total_variability(server, full, 400, nb_iter=1), lambda: fa.total_variability_single(server, full, R, nb_iter=1),
                 lambda: fa.extract_ivectors(full, server), lambda: fa.extract_ivectors_single(full, server),
                 lambda: faw.total_variability_wide_device(None, None, full, 400),
                 lambda: faw.extract_ivectors_wide_device(None, None, full, fa.F)):
        with pytest.raises(NotImplementedError, match="full-covariance"):
            call()
    # the narrow class still refuses 193, now naming this module
    with pytest.raises(ValueError, match="192.*factor_analyser_wide"):
        FactorAnalyser().total_variability(server, ubm, 193, nb_iter=1)
    for name in ("total_variability_raw", "weighted_likelihood_plda"):
        assert not hasattr(WideFactorAnalyser, name)


def test_without_a_gpu_training_and_extraction_raise(fx, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    ubm, server = _ubm(fx), _server(fx)
    fa = WideFactorAnalyser(F=fx["tv_init"])
    for call in (lambda: fa.total_variability(server, ubm, 400, nb_iter=1), lambda: fa.extract_ivectors(ubm, server)):
        with pytest.raises(RuntimeError, match="no GPU is visible"):
            call()


def test_parameter_lists():
    for name in ("total_variability", "total_variability_single", "extract_ivectors", "extract_ivectors_single"):
        assert inspect.signature(getattr(WideFactorAnalyser, name)) == inspect.signature(getattr(FactorAnalyser, name)), name
    for name in ("plda", "read", "write"):
        assert getattr(WideFactorAnalyser, name) is getattr(FactorAnalyser, name), name
    assert issubclass(WideFactorAnalyser, FactorAnalyser)
    expect = {"tv_gram_wide_device": "(F, C)",
              "tv_posterior_wide_device": "(stat0, stat1_w, F, G=None, want='packed')",
              "tv_m_step_device": "(_A, _C, _R, nb_sessions, min_div=True)",
              "total_variability_wide_device": "(stat0, stat1, ubm, tv_rank, nb_iter=20, min_div=True, tv_init=None, "
                                               "max_workspace_bytes=1073741824, after_iteration=None, m_step='device')",
              "extract_ivectors_wide_device": "(stat0, stat1, ubm, F, uncertainty=False, max_workspace_bytes=1073741824)"}
    for name, sig in expect.items():
        assert str(inspect.signature(getattr(faw, name))) == sig, name


def test_m_step_algebra_against_the_fixture_with_injected_inverses(fx):
    """``tv_m_step_device`` = the kernel's inverses + ``m_step_from_inverses``; here the inverses come from numpy.  The fixture's
    ``A_c`` have condition numbers below 1e4 (asserted by tests/test_ivector_cpu.py), far inside the bar."""
    import torch
    inv = ivn.pack(numpy.linalg.inv(ivn.unpack(fx["A"], R)))
    t = lambda a: torch.as_tensor(numpy.ascontiguousarray(a))   # noqa: E731
    errs = {}
    for tag, min_div in (("md", True), ("nomd", False)):
        F = faw.m_step_from_inverses(t(inv), t(fx["C"]), t(fx["R"]), N, min_div).numpy()
        errs[f"F {tag}"] = ivn.rel(F, fx[f"F_{tag}_it0"])
        errs[f"F {tag} against tv_m_step"] = ivn.rel(F, factor_analyser.tv_m_step(fx["A"], fx["C"], fx["R"], N, min_div))
    errs["_R as (1, P)"] = ivn.rel(faw.m_step_from_inverses(t(inv), t(fx["C"]), t(fx["R"][None]), N, True).numpy(), fx["F_md_it0"])
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v < RESTATEMENT_TOL for v in errs.values()), errs
    # a component nobody occupies: its inverse is not finite, and the M-step says which
    bad = inv.copy()
    bad[[1, 4]] = numpy.nan
    with pytest.raises(numpy.linalg.LinAlgError, match=r"\[1, 4\]"):
        faw.m_step_from_inverses(t(bad), t(fx["C"]), t(fx["R"]), N, True)
