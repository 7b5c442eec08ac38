"""Top-C EM without a GPU (sidekit_amd/mixture.py, include/sidekit_amd/gmm_topc_em.h, csrc/gmm_topc_em.hip): the header against its
binding table and the built library, the argument checks of the entry point through the C ABI, the Python refusals, and the numpy
restatement the GPU tests lean on (tests/tools/gmm_topc_em_numpy.py) against the dense restatement.

The restatement is held to 1e-12 relative max-norm, the bar of tests/test_gmm_topc_stats_cpu.py for float64 algebra restated in numpy.
"""
import inspect
import os
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gmm_topc_em_numpy as gem  # noqa: E402
import gmm_topc_numpy as gtn  # noqa: E402
import gmm_topc_stats_numpy as gsn  # noqa: E402
import mixture_numpy as mxn  # noqa: E402

import sidekit_amd  # noqa: E402
from sidekit_amd import _lib, mixture  # noqa: E402
from sidekit_amd.mixture import Mixture  # noqa: E402

RESTATEMENT_TOL = 1e-12
ITERATIONS = (1, 2, 2, 4)


def recipe():
    """the driver recipe of the GPU tests: 600 frames around 16 overlapping clusters in 5 dimensions"""
    rs = numpy.random.RandomState(0)
    ctr = 3 * rs.randn(16, 5)
    return ctr[rs.randint(16, size=600)] + rs.randn(600, 5) * (0.5 + rs.rand(600, 1))


def _ubm(C=4, D=3, seed=3):
    rs = numpy.random.RandomState(seed)
    m = Mixture()
    m.w, m.mu, m.invcov = numpy.full(C, 1.0 / C), rs.randn(C, D), 1.0 / (0.5 + rs.rand(C, D))
    m.cov_var_ctl, m.cst, m.det = 1.0 / m.invcov, numpy.zeros(C), numpy.zeros(C)
    m._compute_all()
    return m


# ---- bindings and refusals ----------------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree():
    """What tests/test_gmm_topc_stats_cpu.py checks for gmm_topc_stats.h, for the top-C EM header and table."""
    import ctypes
    import re
    src = open(os.path.join(ROOT, "include", "sidekit_amd", "gmm_topc_em.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?(?:int|char\s*\*|void)\s*\**\s*((?:xt|sc|sk)_\w+)\s*\(", src, flags=re.M)))
    assert declared == ["sc_gmm_topc_refine"]
    assert sorted(_lib.GMM_TOPC_EM_SIGNATURES) == declared, "ctypes binding table and header disagree"
    others = (_lib.SIGNATURES, _lib.GAUSSIAN_SIGNATURES, _lib.MIXTURE_SIGNATURES, _lib.IVECTOR_SIGNATURES, _lib.GMM_SCORING_SIGNATURES,
              _lib.GMM_TOPC_SIGNATURES, _lib.GMM_TOPC_STATS_SIGNATURES, _lib.JFA_SIGNATURES, _lib.SVM_SIGNATURES, _lib.FEATURES_SIGNATURES,
              _lib.CEPSTRUM_SIGNATURES)
    assert not any(set(_lib.GMM_TOPC_EM_SIGNATURES) & set(t) for t in others)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(cdll, name), f"{name} declared in include/sidekit_amd/gmm_topc_em.h but not exported"
    lib = _lib.lib()
    for name, (res, args) in _lib.GMM_TOPC_EM_SIGNATURES.items():
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    ctype = {"void*": _lib._P, "int32_t": _lib._I32, "int64_t": _lib._I64, "double": _lib._F64}
    flat = re.sub(r"\s+", " ", src)
    for name, (_, args) in _lib.GMM_TOPC_EM_SIGNATURES.items():
        params = re.search(r"int %s\((.*?)\);" % name, flat).group(1).split(",")
        kinds = ["void*" if "*" in q else q.replace("const", "").split()[0] for q in params]
        assert [ctype[k] for k in kinds] == args, (name, kinds)
    assert '#include "gmm_topc_stats.h"' in src
    assert re.findall(r"#define (SC_\w+) (\d+)", src) == [("SC_GMM_TOPC_CAND_MAX", "64")] and _lib.SC_GMM_TOPC_CAND_MAX == 64


def test_signatures_and_lazy_names():
    tail = "iterations=(1, 2, 2, 4, 4, 4, 4, 8, 8, 8, 8, 8, 8), top_c=10, "
    assert str(inspect.signature(mixture.split_candidates)) == "(idx, c_old)"
    assert str(inspect.signature(mixture.gmm_topc_refine_device)) == "(ubm, frames, candidates, top_c=10, posteriors=False)"
    assert str(inspect.signature(mixture.em_split_topc_device)) == \
        "(frames, distrib_nb, " + tail + "init_frames=None, ceil_cov=10, floor_cov=0.01, exact_lists_at=(), after_iteration=None)"
    assert str(inspect.signature(Mixture.EM_split_topc)) == \
        "(self, features_server, feature_list, distrib_nb, " + tail + \
        "num_thread=1, llk_gain=0.01, save_partial=False, output_file_name='ubm', ceil_cov=10, floor_cov=0.01, exact_lists_at=())"
    # and the dense ones, as tests/test_mixture_cpu.py pins them
    assert str(inspect.signature(mixture.em_split_device)) == \
        "(frames, distrib_nb, iterations=(1, 2, 2, 4, 4, 4, 4, 8, 8, 8, 8, 8, 8), init_frames=None, ceil_cov=10, floor_cov=0.01, after_iteration=None)"
    for name in ("split_candidates", "gmm_topc_refine_device", "em_split_topc_device"):
        assert getattr(sidekit_amd, name) is getattr(mixture, name)


def test_entry_point_checks_its_arguments_before_anything_is_enqueued():
    """SK_EARG through the C ABI on a host with no GPU: nothing was enqueued, or there would have been a HIP error instead."""
    lib = _lib.lib()
    p, F32 = 4096, _lib.XT_F32   # any non-null address: a refused call dereferences nothing

    def refine(X=p, dt=F32, N=5, D=4, mu=p, ic=p, B=p, C=3, cand=p, Kc=4, K=2, idx=p, post=p, lse=p):
        return lib.sc_gmm_topc_refine(X, dt, N, D, mu, ic, B, C, cand, Kc, K, idx, post, lse, None)

    cases = {"X null": refine(X=None), "mu null": refine(mu=None), "invcov null": refine(ic=None), "B null": refine(B=None),
             "cand null": refine(cand=None), "idx null": refine(idx=None), "post alone null": refine(post=None), "lse alone null": refine(lse=None),
             "bf16": refine(dt=_lib.XT_BF16), "i64": refine(dt=_lib.XT_I64), "i16": refine(dt=_lib.XT_I16), "N = 0": refine(N=0),
             "N = 2^31": refine(N=1 << 31), "D = 0": refine(D=0), "D = 129": refine(D=129), "C = 0": refine(C=0), "C > grid": refine(C=65535 * 64 + 1),
             "Kc = 0": refine(Kc=0), "Kc < 0": refine(Kc=-1), "Kc = 65": refine(Kc=65), "K = 0": refine(K=0), "K < 0": refine(K=-1),
             "K > C": refine(K=4), "K > 32": refine(C=100, K=33), "K > 32, lists only": refine(C=100, K=33, post=None, lse=None)}
    assert all(rc == _lib.SK_EARG for rc in cases.values()), cases
    assert "sc_gmm_topc_refine" in _lib.last_error() and "K=33" in _lib.last_error()
    assert refine(Kc=65) == _lib.SK_EARG and "Kc=65" in _lib.last_error()


def test_refusals():
    import torch
    ubm, X = _ubm(), numpy.zeros((7, 3))
    good = numpy.zeros((7, 4), dtype=numpy.int32)
    for bad in (0, -3, 33):
        with pytest.raises(ValueError, match="top_c"):
            mixture.gmm_topc_refine_device(ubm, X, good, top_c=bad)
        with pytest.raises(ValueError, match="top_c"):
            mixture.em_split_topc_device(X, 4, top_c=bad)
        with pytest.raises(ValueError, match="top_c"):
            Mixture().EM_split_topc(None, [], 4, top_c=bad)
    for bad in (good[:-1], numpy.zeros((7, 65), dtype=numpy.int32), numpy.zeros((7, 0), dtype=numpy.int32), good.astype(numpy.int64), good.ravel(),
                torch.zeros((7, 4), dtype=torch.int64), good.tolist()):
        with pytest.raises(ValueError, match="candidates"):
            mixture.gmm_topc_refine_device(ubm, X, bad)
    full = _ubm()
    full.invcov = numpy.stack([numpy.diag(v) for v in full.invcov])
    with pytest.raises(NotImplementedError, match="full-covariance"):
        mixture.gmm_topc_refine_device(full, X, good)
    if not torch.cuda.is_available():
        for call in (lambda: mixture.gmm_topc_refine_device(ubm, X, good), lambda: mixture.gmm_topc_refine_device(ubm, X, good, posteriors=True),
                     lambda: mixture.em_split_topc_device(X, 4), lambda: mixture.em_split_topc_device(X, 4, top_c=2, exact_lists_at=(4,))):
            with pytest.raises(RuntimeError, match="no GPU is visible"):
                call()


# ---- the numpy model ----------------------------------------------------------------------------------------------------------------------
def test_split_candidates_on_host_arrays():
    idx = numpy.array([[0, 2, 5], [1, -1, 7], [-1, -1, -1]], dtype=numpy.int32)
    want = numpy.array([[0, 2, 5, 8, 10, 13], [1, -1, 7, 9, -1, 15], [-1, -1, -1, -1, -1, -1]], dtype=numpy.int32)
    for got in (mixture.split_candidates(idx, 8), mixture.split_candidates(idx.astype(numpy.int64), 8), mixture.split_candidates(idx.tolist(), 8),
                gem.split_candidates(idx, 8)):
        assert isinstance(got, numpy.ndarray) and got.dtype == numpy.int32 and numpy.array_equal(got, want)
    # the children of component c of a split are c and c + C_old: mixture_numpy.split stacks the lower halves first
    m = mxn.split(mxn.model([0.25, 0.75], [[0.0, 1.0], [5.0, 5.0]], [[1.0, 4.0], [0.25, 1.0]]))
    assert numpy.array_equal(m["mu"], [[-1.0, 1.0], [3.0, 5.0], [1.0, 1.0], [7.0, 5.0]])


def test_refine_restatement():
    """all components as candidates: the exact lists; broken rows: what the header says of them"""
    rs = numpy.random.RandomState(2)
    C, D, N = 12, 6, 50
    m = mxn.model(numpy.full(C, 1.0 / C), rs.randn(C, D), 1.0 / (0.5 + rs.rand(C, D)))
    X = rs.randn(N, D)
    every = numpy.array([rs.permutation(C) for _ in range(N)], dtype=numpy.int32)
    idx, post, lse, gap = gem.refine(m, X, every, 4)
    assert numpy.array_equal(idx, gtn.lists(m, X, 4)) and abs(gap - gtn.gap(m, X, 4)[0]) < 1e-12
    rpost, rlse = gsn.posteriors(m, X, idx)
    assert numpy.array_equal(post, rpost) and numpy.array_equal(lse, rlse) and numpy.abs(post.sum(1) - 1.0).max() < RESTATEMENT_TOL
    broken = every[:, :5].copy()
    broken[0] = (3, 3, -1, C, 3)                  # one valid entry
    broken[1] = (-1, C, 2 ** 31 - 1, -2 ** 31, -7)   # none
    broken[2] = (5, 1, 5, 1, 9)                   # three
    idx, post, lse, gap = gem.refine(m, X, broken, 4)
    assert idx[0].tolist() == [3, -1, -1, -1] and post[0].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert idx[1].tolist() == [-1] * 4 and lse[1] == -numpy.inf and numpy.all(post[1] == 0.0)
    assert idx[2].tolist() == [1, 5, 9, -1] and post[2, 3] == 0.0 and abs(post[2].sum() - 1.0) < RESTATEMENT_TOL
    assert numpy.all(numpy.diff(idx[3:], axis=1) > 0), "ascending"
    assert gem.refine(m, X, every[:, :3], 4)[3] == numpy.inf, "K > Kc: nothing is left out"


def test_dense_agreement_when_top_c_covers_every_level():
    X = recipe()
    dense = mxn.em_split(X, 16, ITERATIONS)
    for top_c in (16, 32):
        trace, idx, gap = gem.em_split_topc(X, 16, ITERATIONS, top_c)
        assert idx is None and gap == numpy.inf and len(trace) == len(dense) == 9
        errs = {f"{k} after iteration {i}": mxn.rel(a[0][k], b[0][k]) for i, (a, b) in enumerate(zip(trace, dense)) for k in ("w", "mu", "invcov")}
        errs["llk"] = mxn.rel([a[1] for a in trace], [b[1] for b in dense])
        assert max(errs.values()) < RESTATEMENT_TOL, errs


def test_smallest_gap_on_the_driver_recipe():
    """8.7e-4 over all refinements (levels C = 4, 8, 16 at top_c = 3: two, two and four E-steps and one closing refinement each): far
    above what separates two float64 evaluations of one lp, so the GPU test may ask for equal lists"""
    X = recipe()
    trace, idx, gap = gem.em_split_topc(X, 16, ITERATIONS, 3)
    print(f"smallest candidate gap {gap:.4e}; llk {[round(float(l), 4) for _, l in trace]}")
    assert 8.65e-4 < gap < 8.75e-4
    assert idx.shape == (600, 3) and idx.min() >= 0 and idx.max() < 16 and numpy.all(numpy.diff(idx, axis=1) > 0)
    assert all(numpy.isfinite(m["mu"]).all() and (m["w"] > 0).all() for m, _ in trace), "no component died"
    dense = mxn.em_split(X, 16, ITERATIONS)
    assert abs(trace[-1][1] - dense[-1][1]) < 0.1, "the same quality as dense EM on this recipe"
    exact = gem.em_split_topc(X, 16, ITERATIONS, 3, exact_lists_at=(8, 16))
    assert exact[2] > 1e-6 and not numpy.array_equal(exact[0][-1][0]["mu"], trace[-1][0]["mu"]), "exact lists at 8 and 16 change the run"
