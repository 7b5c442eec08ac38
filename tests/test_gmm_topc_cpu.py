"""Top-C GMM-UBM scoring without a GPU (sidekit_amd/gmm_scoring.py, include/sidekit_amd/gmm_topc.h, csrc/gmm.hip, csrc/gmm_topc.hip): the
numpy restatement the GPU tests lean on (tests/tools/gmm_topc_numpy.py) against the dense restatement and against the reference's own
scores (tests/golden/gmm_scoring.npz), the signatures, the header against its binding table and the built library, the argument checks
of both entry points through the C ABI, and the Python refusals.

The restatement is held to 1e-12 relative max-norm, the bar of tests/test_gmm_scoring_cpu.py for float64 algebra restated in numpy.
"""
import inspect
import os
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gmm_scoring_numpy as gsn  # noqa: E402
import gmm_topc_numpy as gtn  # noqa: E402
import mixture_numpy as mxn  # noqa: E402

from sidekit_amd import _lib, gmm_scoring  # noqa: E402
from sidekit_amd.mixture import Mixture  # noqa: E402

RESTATEMENT_TOL = 1e-12
KEYS = ("w", "mu", "invcov", "cov_var_ctl")


@pytest.fixture(scope="module")
def fx(golden_dir):
    out = dict(numpy.load(os.path.join(golden_dir, "gmm_scoring.npz")))
    out.update({"mix_" + k: v for k, v in numpy.load(os.path.join(golden_dir, "mixture.npz")).items()})
    return out


def _ubm(fx):
    m = Mixture()
    m.w, m.mu, m.invcov, m.cov_var_ctl = (numpy.array(fx[f"mix_split4_{k}"], dtype=numpy.float64) for k in KEYS)
    m.cst, m.det = numpy.zeros(m.w.shape), numpy.zeros(m.w.shape)
    m._compute_all()
    return m


def _random_case(seed, C, D, lengths, M):
    rs = numpy.random.RandomState(seed)
    w = rs.rand(C) + 0.5
    ref = mxn.model(w / w.sum(), 2.0 * rs.randn(C, D), 1.0 / (0.5 + rs.rand(C, D)))
    models = (ref["mu"][None] + 0.3 * rs.randn(M, C, D)).reshape(M, C * D)
    n = int(sum(lengths))
    X = ref["mu"][rs.randint(0, C, n)] + 1.1 * rs.randn(n, D)
    return ref, models, X, numpy.concatenate(([0], numpy.cumsum(lengths)))


def test_all_components_is_the_dense_restatement():
    ref, models, X, off = _random_case(3, 12, 7, [5, 0, 40], 3)
    assert numpy.array_equal(gtn.lists(ref, X, 12), numpy.tile(numpy.arange(12, dtype=numpy.int32), (45, 1)))
    assert numpy.array_equal(gtn.lists(ref, X, 32), gtn.lists(ref, X, 12)), "top_c above C: every component"
    dense, lens = gsn.llk(ref, models, X, off)
    sparse, lens_t = gtn.llk(ref, models, X, off, top_c=12)
    err = mxn.rel(sparse, dense)
    print(f"top_c = C vs the dense restatement: {err:.2e}")
    assert err < RESTATEMENT_TOL and list(lens) == list(lens_t) and sparse[0, 1] == 0.0
    some = numpy.array([True, False, True])
    err = numpy.abs(gtn.llr(ref, models, X, off, top_c=12)[:, some] - gsn.llr(ref, models, X, off)[:, some]).max() / numpy.abs(dense[:, some] / lens[some]).max()
    print(f"ratios: {err:.2e}")
    assert err < RESTATEMENT_TOL and numpy.isnan(gtn.llr(ref, models, X, off, top_c=12)[:, 1]).all()


def test_lists_are_the_largest_ties_to_the_lower_index_stored_ascending():
    ref, _, X, _ = _random_case(4, 9, 5, [30], 1)
    lp = gtn.log_posteriors(ref, X)
    assert mxn.rel(lp, mxn.log_posteriors(ref, X)) < RESTATEMENT_TOL, "the direct form is the expanded form"
    for K in (1, 4, 9):
        idx = gtn.lists(ref, X, K)
        assert idx.dtype == numpy.int32 and idx.shape == (30, K) and numpy.all(numpy.diff(idx, axis=1) > 0)
        for n in range(30):
            rest = numpy.setdiff1d(numpy.arange(9), idx[n])
            assert rest.size == 0 or lp[n, idx[n]].min() > lp[n, rest].max()
    tied = numpy.array([[1.0, 3.0, 3.0, 0.0, 3.0]])
    assert gtn.lists(None, None, 2, tied).tolist() == [[1, 2]] and gtn.lists(None, None, 1, tied).tolist() == [[1]]
    assert gtn.lists(None, None, 4, tied).tolist() == [[0, 1, 2, 4]]


def test_restatement_matches_the_reference_fixture(fx):
    """C = 8: with every component listed the new arithmetic gives the reference's own scores"""
    m = mxn.model(*(fx[f"mix_split4_{k}"] for k in KEYS))
    X, off = fx["mix_X"], fx["mix_seg_off"]
    seg = [int(s[4:]) for s in fx["score_segset"]]
    order = [list(fx["enroll_modelset"]).index(n) for n in fx["score_modelset"]]
    sums, lens = gsn.llk(m, fx["enroll_stat1"][order], X, off)
    scale = numpy.abs(sums[:, seg] / lens[seg]).max()
    got = gtn.llr(m, fx["enroll_stat1"][order], X, off, top_c=8)
    errs = {"scores over the largest mean llk": numpy.abs(got[:, seg] - fx["scoremat"]).max() / scale,
            "masked scores": numpy.abs(gtn.llr(m, fx["enroll_stat1"][order], X, off, None, 8)[:, seg] * fx["masked_scoremask"] - fx["masked_scoremat"]).max() / scale}
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v < RESTATEMENT_TOL for v in errs.values()), errs
    assert numpy.isnan(got[:, 2]).all() and lens[2] == 0 and numpy.all(got[list(fx["score_modelset"]).index("ubm"), seg] == 0.0)


def test_fewer_components_give_less_and_more_give_more():
    ref, models, X, off = _random_case(5, 20, 6, [17, 64, 3], 4)
    dense, _ = gsn.llk(ref, models, X, off)
    before = None
    for K in (1, 2, 5, 10):   # the dropped terms stay far above the rounding of either form (1e-12): the last assertion
        sparse, _ = gtn.llk(ref, models, X, off, top_c=K)
        assert numpy.all(sparse <= dense), f"top_c = {K}: a sum over fewer non-negative terms"
        assert before is None or numpy.all(sparse >= before), f"top_c = {K}: not below the sum over fewer"
        before = sparse
    assert numpy.all(dense - before > 1e-9 * numpy.abs(dense)) and mxn.rel(before, dense) < 1e-2


def test_signatures():
    assert str(inspect.signature(gmm_scoring.gmm_top_components_device)) == "(ubm, frames, top_c=10)"
    topc = "(ubm, models, frames, seg_off=None, mask=None, top_c=10, components=None, max_workspace_bytes=1073741824)"
    assert str(inspect.signature(gmm_scoring.gmm_llk_topc_device)) == topc
    assert str(inspect.signature(gmm_scoring.gmm_llr_topc_device)) == topc
    assert str(inspect.signature(gmm_scoring.gmm_scoring_topc)) == "(ubm, enroll, ndx, feature_server, top_c=10, num_thread=1)"
    # and the reference's, as tests/test_gmm_scoring_cpu.py::test_reference_signatures pins them
    assert str(inspect.signature(gmm_scoring.gmm_scoring)) == "(ubm, enroll, ndx, feature_server, num_thread=1)"
    assert str(inspect.signature(gmm_scoring.gmm_scoring_singleThread)) == "(ubm, enroll, ndx, feature_server, score_mat, seg_idx=None)"
    assert str(inspect.signature(gmm_scoring.gmm_llk_device)) == "(ubm, models, frames, seg_off=None, mask=None, max_workspace_bytes=1073741824)"
    assert str(inspect.signature(gmm_scoring.gmm_llr_device)) == "(ubm, models, frames, seg_off=None, mask=None, max_workspace_bytes=1073741824)"
    assert "not built" not in gmm_scoring.__doc__


def test_header_binding_table_and_library_agree():
    """What tests/test_abi.py checks for include/sidekit_amd.h, for the top-C header and table."""
    import ctypes
    import re
    src = open(os.path.join(ROOT, "include", "sidekit_amd", "gmm_topc.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?(?:int|char\s*\*|void)\s*\**\s*((?:xt|sc|sk)_\w+)\s*\(", src, flags=re.M)))
    assert declared == ["sc_gmm_score_models_topc", "sc_gmm_top_components"]
    assert sorted(_lib.GMM_TOPC_SIGNATURES) == declared, "ctypes binding table and header disagree"
    others = (_lib.SIGNATURES, _lib.GAUSSIAN_SIGNATURES, _lib.MIXTURE_SIGNATURES, _lib.IVECTOR_SIGNATURES, _lib.GMM_SCORING_SIGNATURES,
              _lib.JFA_SIGNATURES, _lib.SVM_SIGNATURES, _lib.FEATURES_SIGNATURES, _lib.CEPSTRUM_SIGNATURES)
    assert not any(set(_lib.GMM_TOPC_SIGNATURES) & set(t) for t in others)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(cdll, name), f"{name} declared in include/sidekit_amd/gmm_topc.h but not exported"
    lib = _lib.lib()
    for name, (res, args) in _lib.GMM_TOPC_SIGNATURES.items():
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    ctype = {"void*": _lib._P, "int32_t": _lib._I32, "int64_t": _lib._I64, "double": _lib._F64}
    flat = re.sub(r"\s+", " ", src)
    for name, (_, args) in _lib.GMM_TOPC_SIGNATURES.items():
        params = re.search(r"int %s\((.*?)\);" % name, flat).group(1).split(",")
        kinds = ["void*" if "*" in q else q.replace("const", "").split()[0] for q in params]
        assert [ctype[k] for k in kinds] == args, (name, kinds)
    assert int(re.search(r"#define SC_GMM_TOPC_MAX (\d+)", src).group(1)) == _lib.SC_GMM_TOPC_MAX == gmm_scoring.MAX_TOP_C == 32
    assert '#include "gmm_scoring.h"' in src


def test_entry_points_check_their_arguments_before_anything_is_enqueued():
    """SK_EARG through the C ABI on a host with no GPU: nothing was enqueued, or there would have been a HIP error instead."""
    lib = _lib.lib()
    p, F32 = 4096, _lib.XT_F32   # any non-null address: a refused call dereferences nothing

    def top(X=p, dt=F32, N=5, D=4, mu=p, ic=p, A=p, C=3, K=2, idx=p):
        return lib.sc_gmm_top_components(X, dt, N, D, mu, ic, A, C, K, idx, None)

    cases = {"X null": top(X=None), "mu null": top(mu=None), "invcov null": top(ic=None), "A null": top(A=None), "idx null": top(idx=None),
             "bf16": top(dt=_lib.XT_BF16), "i64": top(dt=_lib.XT_I64), "i16": top(dt=_lib.XT_I16), "N = 0": top(N=0), "N = 2^31": top(N=1 << 31),
             "D = 0": top(D=0), "D = 129": top(D=129), "C = 0": top(C=0), "C > grid": top(C=65535 * 64 + 1), "K = 0": top(K=0), "K < 0": top(K=-1),
             "K > C": top(K=4), "K > 32": top(C=100, K=33)}
    assert all(rc == _lib.SK_EARG for rc in cases.values()), cases
    assert "sc_gmm_top_components" in _lib.last_error() and "K=33" in _lib.last_error()

    def score(X=p, dt=F32, N=5, D=4, mus=p, M=2, ic=p, B=p, C=3, off=p, S=1, max_len=5, mask=None, idx=p, K=2, llk=p):
        return lib.sc_gmm_score_models_topc(X, dt, N, D, mus, M, ic, B, C, off, S, max_len, mask, idx, K, llk, None)

    cases = {"X null": score(X=None), "mus null": score(mus=None), "invcov null": score(ic=None), "B null": score(B=None), "seg_off null": score(off=None),
             "idx null": score(idx=None), "llk null": score(llk=None), "M = 0": score(M=0), "M < 0": score(M=-1), "M > grid": score(M=65536),
             "C = 0": score(C=0), "C > grid": score(C=65535 * 64 + 1), "D = 0": score(D=0), "D = 129": score(D=129), "N = 0": score(N=0),
             "N = 2^31": score(N=1 << 31), "S = 0": score(S=0), "bf16": score(dt=_lib.XT_BF16), "i64": score(dt=_lib.XT_I64), "i16": score(dt=_lib.XT_I16),
             "max_len < 0": score(max_len=-1), "max_len > N": score(max_len=6), "K = 0": score(K=0), "K < 0": score(K=-1), "K > C": score(K=4),
             "K > 32": score(C=100, K=33)}
    assert all(rc == _lib.SK_EARG for rc in cases.values()), cases
    assert "sc_gmm_score_models_topc" in _lib.last_error() and "K=33" in _lib.last_error()


def test_refusals(fx):
    import torch
    ubm = _ubm(fx)
    X = fx["mix_X"]
    N, C = X.shape[0], ubm.mu.shape[0]
    models = ubm.mu.reshape(1, -1)
    calls = {"lists": lambda **kw: gmm_scoring.gmm_top_components_device(ubm, X, **kw),
             "llk": lambda **kw: gmm_scoring.gmm_llk_topc_device(ubm, models, X, **kw),
             "llr": lambda **kw: gmm_scoring.gmm_llr_topc_device(ubm, models, X, **kw)}
    for name, call in calls.items():
        for bad in (0, -3, 33):
            with pytest.raises(ValueError, match="top_c"):
                call(top_c=bad)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="top_c"):
            gmm_scoring.gmm_scoring_topc(ubm, _server(fx), _ndx(), None, top_c=bad)
    good = numpy.zeros((N, 3), dtype=numpy.int32)
    for name in ("llk", "llr"):
        for bad in (good[:-1], good[:, :2], good.astype(numpy.int64), good.astype(numpy.float64), good.ravel(), torch.zeros((N, 3), dtype=torch.int64),
                    torch.zeros((N, 4), dtype=torch.int32), good.tolist()):
            with pytest.raises(ValueError, match="components"):
                calls[name](top_c=3, components=bad)
        with pytest.raises(ValueError, match="components"):
            calls[name](top_c=12, components=numpy.zeros((N, 12), dtype=numpy.int32))   # K = min(top_c, C) = 8 columns
    full = _ubm(fx)
    full.invcov = numpy.stack([numpy.diag(v) for v in full.invcov])
    for call in (lambda: gmm_scoring.gmm_top_components_device(full, X), lambda: gmm_scoring.gmm_llk_topc_device(full, models, X),
                 lambda: gmm_scoring.gmm_llr_topc_device(full, models, X, top_c=99), lambda: gmm_scoring.gmm_scoring_topc(full, _server(fx), _ndx(), None)):
        with pytest.raises(NotImplementedError, match="full-covariance"):
            call()
    with pytest.raises(AssertionError, match="Mixture"):
        gmm_scoring.gmm_scoring_topc(object(), _server(fx), _ndx(), None)
    if not torch.cuda.is_available():
        for name, call in calls.items():
            with pytest.raises(RuntimeError, match="no GPU is visible"):
                call()
        with pytest.raises(RuntimeError, match="no GPU is visible"):
            calls["llk"](top_c=3, components=good)
    assert C == 8


def _server(fx):
    from sidekit_amd.statserver import StatServer
    s = StatServer()
    s.modelset = fx["enroll_modelset"].astype("|O")
    s.segset = s.modelset.copy()
    s.start, s.stop = numpy.empty(5, dtype="|O"), numpy.empty(5, dtype="|O")
    s.stat0, s.stat1 = numpy.ones((5, 1)), fx["enroll_stat1"].copy()
    return s


def _ndx():
    from sidekit_amd.bosaris import Ndx
    return Ndx(models=numpy.array(["ubm", "ubm"], dtype="|O"), testsegs=numpy.array(["show1", "show3"], dtype="|O"))
