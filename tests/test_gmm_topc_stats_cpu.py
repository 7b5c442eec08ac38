"""Top-C Baum-Welch statistics without a GPU (sidekit_amd/mixture.py, sidekit_amd/statserver.py, include/sidekit_amd/gmm_topc_stats.h,
csrc/gmm_topc_stats.hip): the numpy restatement the GPU tests lean on (tests/tools/gmm_topc_stats_numpy.py) against the dense
restatement, the signatures, the header against its binding table and the built library, the argument checks of both entry points
through the C ABI, and the Python refusals.

The restatement is held to 1e-12 relative max-norm, the bar of tests/test_gmm_topc_cpu.py for float64 algebra restated in numpy.
"""
import inspect
import os
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gmm_topc_numpy as gtn  # noqa: E402
import gmm_topc_stats_numpy as gsn  # noqa: E402
import mixture_numpy as mxn  # noqa: E402

from sidekit_amd import _lib, gmm_scoring, mixture  # noqa: E402
from sidekit_amd.mixture import Mixture  # noqa: E402
from sidekit_amd.statserver import StatServer  # noqa: E402

RESTATEMENT_TOL = 1e-12
KEYS = ("w", "mu", "invcov", "cov_var_ctl")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(numpy.load(os.path.join(golden_dir, "mixture.npz")))


def _ubm(fx):
    m = Mixture()
    m.w, m.mu, m.invcov, m.cov_var_ctl = (numpy.array(fx[f"split4_{k}"], dtype=numpy.float64) for k in KEYS)
    m.cst, m.det = numpy.zeros(m.w.shape), numpy.zeros(m.w.shape)
    m._compute_all()
    return m


def test_full_lists_are_the_dense_restatement(fx):
    """C = 8, D = 23, K = C: every component listed, the renormalisation is the dense one"""
    ref = mxn.model(*(fx[f"split4_{k}"] for k in KEYS))
    X, off = fx["X"], fx["seg_off"]
    assert list(numpy.diff(off)) == [3, 301, 0, 64, 130, 17, 700, 45]
    full = numpy.tile(numpy.arange(8, dtype=numpy.int32), (X.shape[0], 1))
    assert numpy.array_equal(gtn.lists(ref, X, 8), full)
    s0, s1, s2, llk, post, lse = gsn.stats(ref, X, full, off)
    d0, d1, d2, dl = mxn.stats(ref, X, off)
    dense_post, _ = mxn.sum_log_probabilities(mxn.log_posteriors(ref, X))
    errs = {"stat0": mxn.rel(s0, d0), "stat1": mxn.rel(s1, d1), "stat2": mxn.rel(s2, d2), "llk": mxn.rel(llk, dl), "post": mxn.rel(post, dense_post),
            "lse": mxn.rel(lse, mxn.frame_lse(mxn.log_posteriors(ref, X))), "rows of post": numpy.abs(post.sum(1) - 1.0).max()}
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v < RESTATEMENT_TOL for v in errs.values()), errs
    assert numpy.all(s0[2] == 0.0) and numpy.all(s1[2] == 0.0) and numpy.all(s2[2] == 0.0) and llk[2] == 0.0, "the empty segment"


def test_restatement_on_shorter_and_broken_lists(fx):
    ref = mxn.model(*(fx[f"split4_{k}"] for k in KEYS))
    X, off = fx["X"], fx["seg_off"]
    idx = gtn.lists(ref, X, 3)
    s0, s1, s2, llk, post, lse = gsn.stats(ref, X, idx, off)
    assert numpy.abs(post.sum(1) - 1.0).max() < RESTATEMENT_TOL and numpy.abs(s0.sum(1) - numpy.diff(off)).max() < RESTATEMENT_TOL * 700
    dense = mxn.frame_lse(mxn.log_posteriors(ref, X))
    assert numpy.all(lse <= dense + RESTATEMENT_TOL * numpy.abs(dense)), "a sum over fewer non-negative terms, up to the rounding of the two forms"
    broken = idx.copy()
    broken[5, 0], broken[5, 2], broken[7] = -1, 8, (-1, 8, 99)   # in the second segment
    b0, b1, b2, bllk, bpost, blse = gsn.stats(ref, X, broken, off)
    assert bpost[5, 0] == 0.0 and bpost[5, 2] == 0.0 and bpost[5, 1] == 1.0 and numpy.all(bpost[7] == 0.0) and blse[7] == -numpy.inf
    assert bllk[1] == -numpy.inf and numpy.isfinite(b0).all() and numpy.isfinite(b1).all()
    others = [0, 2, 3, 4, 5, 6, 7]
    assert numpy.array_equal(b0[others], s0[others]) and numpy.array_equal(b2[others], s2[others]) and numpy.array_equal(bllk[others], llk[others])
    assert abs(b0[1].sum() - 300.0) < RESTATEMENT_TOL * 300, "the frame without a valid entry adds nothing"


def test_signatures():
    assert str(inspect.signature(mixture.gmm_topc_posteriors_device)) == "(ubm, frames, top_c=10, components=None)"
    assert str(inspect.signature(mixture.gmm_stats_topc_device)) == \
        "(ubm, frames, seg_off=None, order=2, top_c=10, components=None, max_workspace_bytes=1073741824)"
    assert str(inspect.signature(StatServer.accumulate_stat_topc)) == \
        "(self, ubm, feature_server, top_c=10, seg_indices=None, channel_extension=('', '_b'), num_thread=1)"
    assert str(inspect.signature(StatServer.accumulate_stat_topc_device)) == "(self, ubm, frames, seg_off, top_c=10)"
    # and the dense ones, as tests/test_mixture_cpu.py pins them
    assert str(inspect.signature(mixture.gmm_stats_device)) == "(ubm, frames, seg_off=None, order=2, max_workspace_bytes=1073741824)"
    assert str(inspect.signature(StatServer.accumulate_stat)) == "(self, ubm, feature_server, seg_indices=None, channel_extension=('', '_b'), num_thread=1)"
    assert str(inspect.signature(StatServer.accumulate_stat_device)) == "(self, ubm, frames, seg_off)"


def test_header_binding_table_and_library_agree():
    """What tests/test_gmm_topc_cpu.py checks for gmm_topc.h, for the top-C statistics header and table."""
    import ctypes
    import re
    src = open(os.path.join(ROOT, "include", "sidekit_amd", "gmm_topc_stats.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?(?:int|char\s*\*|void)\s*\**\s*((?:xt|sc|sk)_\w+)\s*\(", src, flags=re.M)))
    assert declared == ["sc_gmm_topc_posteriors", "sc_gmm_topc_stats"]
    assert sorted(_lib.GMM_TOPC_STATS_SIGNATURES) == declared, "ctypes binding table and header disagree"
    others = (_lib.SIGNATURES, _lib.GAUSSIAN_SIGNATURES, _lib.MIXTURE_SIGNATURES, _lib.IVECTOR_SIGNATURES, _lib.GMM_SCORING_SIGNATURES,
              _lib.GMM_TOPC_SIGNATURES, _lib.JFA_SIGNATURES, _lib.SVM_SIGNATURES, _lib.FEATURES_SIGNATURES, _lib.CEPSTRUM_SIGNATURES)
    assert not any(set(_lib.GMM_TOPC_STATS_SIGNATURES) & set(t) for t in others)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(cdll, name), f"{name} declared in include/sidekit_amd/gmm_topc_stats.h but not exported"
    lib = _lib.lib()
    for name, (res, args) in _lib.GMM_TOPC_STATS_SIGNATURES.items():
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    ctype = {"void*": _lib._P, "int32_t": _lib._I32, "int64_t": _lib._I64, "double": _lib._F64}
    flat = re.sub(r"\s+", " ", src)
    for name, (_, args) in _lib.GMM_TOPC_STATS_SIGNATURES.items():
        params = re.search(r"int %s\((.*?)\);" % name, flat).group(1).split(",")
        kinds = ["void*" if "*" in q else q.replace("const", "").split()[0] for q in params]
        assert [ctype[k] for k in kinds] == args, (name, kinds)
    assert '#include "gmm_topc.h"' in src and "#define SC_" not in src, "the list's bound stays gmm_topc.h's"


def test_entry_points_check_their_arguments_before_anything_is_enqueued():
    """SK_EARG through the C ABI on a host with no GPU: nothing was enqueued, or there would have been a HIP error instead."""
    lib = _lib.lib()
    p, F32 = 4096, _lib.XT_F32   # any non-null address: a refused call dereferences nothing

    def post(X=p, dt=F32, N=5, D=4, mu=p, ic=p, B=p, C=3, idx=p, K=2, out=p, lse=p):
        return lib.sc_gmm_topc_posteriors(X, dt, N, D, mu, ic, B, C, idx, K, out, lse, None)

    cases = {"X null": post(X=None), "mu null": post(mu=None), "invcov null": post(ic=None), "B null": post(B=None), "idx null": post(idx=None),
             "post null": post(out=None), "lse null": post(lse=None), "bf16": post(dt=_lib.XT_BF16), "i64": post(dt=_lib.XT_I64),
             "i16": post(dt=_lib.XT_I16), "N = 0": post(N=0), "N = 2^31": post(N=1 << 31), "D = 0": post(D=0), "D = 129": post(D=129),
             "C = 0": post(C=0), "C > grid": post(C=65535 * 64 + 1), "K = 0": post(K=0), "K < 0": post(K=-1), "K > C": post(K=4),
             "K > 32": post(C=100, K=33)}
    assert all(rc == _lib.SK_EARG for rc in cases.values()), cases
    assert "sc_gmm_topc_posteriors" in _lib.last_error() and "K=33" in _lib.last_error()

    def stats(X=p, dt=F32, N=5, D=4, C=3, idx=p, po=p, K=2, lse=p, off=p, S=1, max_len=5, order=2, s0=p, s1=p, s2=p, llk=None):
        return lib.sc_gmm_topc_stats(X, dt, N, D, C, idx, po, K, lse, off, S, max_len, order, s0, s1, s2, llk, None)

    cases = {"X null": stats(X=None), "idx null": stats(idx=None), "post null": stats(po=None), "lse null": stats(lse=None),
             "seg_off null": stats(off=None), "stat0 null": stats(s0=None), "stat1 null": stats(s1=None), "order 2 without stat2": stats(s2=None),
             "order 0": stats(order=0), "order 3": stats(order=3), "bf16": stats(dt=_lib.XT_BF16), "i64": stats(dt=_lib.XT_I64),
             "i16": stats(dt=_lib.XT_I16), "N = 0": stats(N=0), "N = 2^31": stats(N=1 << 31), "D = 0": stats(D=0), "D = 129": stats(D=129),
             "C = 0": stats(C=0), "C > grid": stats(C=65535 * 64 + 1), "S = 0": stats(S=0), "max_len < 0": stats(max_len=-1),
             "max_len > N": stats(max_len=6), "K = 0": stats(K=0), "K < 0": stats(K=-1), "K > C": stats(K=4), "K > 32": stats(C=100, K=33)}
    assert all(rc == _lib.SK_EARG for rc in cases.values()), cases
    assert "sc_gmm_topc_stats" in _lib.last_error() and "K=33" in _lib.last_error()


def test_refusals(fx):
    import torch
    ubm = _ubm(fx)
    X = fx["X"]
    N, C = X.shape[0], ubm.mu.shape[0]
    names = numpy.array([f"show{i}" for i in range(8)], dtype="|O")
    server = StatServer()
    server.modelset, server.segset = names, names.copy()
    server.start, server.stop = numpy.empty(8, dtype="|O"), numpy.empty(8, dtype="|O")
    calls = {"posteriors": lambda **kw: mixture.gmm_topc_posteriors_device(ubm, X, **kw),
             "stats": lambda **kw: mixture.gmm_stats_topc_device(ubm, X, fx["seg_off"], **kw),
             "accumulate_stat_topc": lambda **kw: server.accumulate_stat_topc(ubm, None, **kw),
             "accumulate_stat_topc_device": lambda **kw: server.accumulate_stat_topc_device(ubm, X, fx["seg_off"], **kw)}
    for name, call in calls.items():
        for bad in (0, -3, 33):
            with pytest.raises(ValueError, match="top_c"):
                call(top_c=bad)
    good = numpy.zeros((N, 3), dtype=numpy.int32)
    for name in ("posteriors", "stats"):
        for bad in (good[:-1], good[:, :2], good.astype(numpy.int64), good.astype(numpy.float64), good.ravel(), torch.zeros((N, 3), dtype=torch.int64),
                    torch.zeros((N, 4), dtype=torch.int32), good.tolist()):
            with pytest.raises(ValueError, match="components"):
                calls[name](top_c=3, components=bad)
        with pytest.raises(ValueError, match="components"):
            calls[name](top_c=12, components=numpy.zeros((N, 12), dtype=numpy.int32))   # K = min(top_c, C) = 8 columns
    with pytest.raises(AssertionError, match="order"):
        mixture.gmm_stats_topc_device(ubm, X, order=3)
    full = _ubm(fx)
    full.invcov = numpy.stack([numpy.diag(v) for v in full.invcov])
    for call in (lambda: mixture.gmm_topc_posteriors_device(full, X), lambda: mixture.gmm_stats_topc_device(full, X, top_c=99),
                 lambda: server.accumulate_stat_topc(full, None), lambda: server.accumulate_stat_topc_device(full, X, fx["seg_off"])):
        with pytest.raises(NotImplementedError, match="full-covariance"):
            call()
    with pytest.raises(AssertionError, match="Mixture"):
        server.accumulate_stat_topc(object(), None)
    if not torch.cuda.is_available():
        for name in ("posteriors", "stats", "accumulate_stat_topc_device"):
            with pytest.raises(RuntimeError, match="no GPU is visible"):
                calls[name]()
        with pytest.raises(RuntimeError, match="no GPU is visible"):
            calls["stats"](top_c=3, components=good)
    assert C == 8 and gmm_scoring.MAX_TOP_C == 32
