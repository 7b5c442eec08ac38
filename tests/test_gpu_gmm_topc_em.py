"""Top-C EM on the GPU (sidekit_amd/mixture.py gmm_topc_refine_device / em_split_topc_device / Mixture.EM_split_topc, csrc/gmm_topc_em.hip)
against the float64 numpy restatement (tests/tools/gmm_topc_em_numpy.py, held to the dense restatement by tests/test_gmm_topc_em_cpu.py),
against the posteriors kernel at the seam the two share (post and lse of a list, bit for bit) and against the dense lists.

TOL = 1e-9 relative max-norm, the project's bound for float64 quantities (tests/test_gpu_mixture.py).  Lists are integers: two
evaluations of one log posterior differ by rounding, so a frame's list is demanded only where the gap between its K-th and (K + 1)-th
candidate exceeds GAP = 1e-9 x max |lp|; at most 1 % of the frames may lie under it, and the seeds below are ones for which the numpy
restatement reports none (every test prints its count).  The bitwise tests are exact: no atomics, every sum in one fixed order.
"""
import os
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gmm_topc_em_numpy as gem  # noqa: E402
import gmm_topc_numpy as gtn  # noqa: E402
import mixture_numpy as mxn  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9
GAP = 1e-9
KEYS = ("w", "mu", "invcov", "cov_var_ctl")
ITERATIONS = (1, 2, 2, 4)
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def _mixture(ref):
    from sidekit_amd.mixture import Mixture
    m = Mixture()
    m.w, m.mu, m.invcov, m.cov_var_ctl = (numpy.array(ref[k], dtype=numpy.float64) for k in KEYS)
    m.cst, m.det = numpy.zeros(m.w.shape), numpy.zeros(m.w.shape)
    with numpy.errstate(divide="ignore"):   # a zero weight: log 0
        m._compute_all()
    return m


def _np(t):
    return t if isinstance(t, numpy.ndarray) else t.cpu().numpy()


def _check(errs):
    print({k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < TOL, f"{k} differs by {v:.3e} (relative max-norm, bound {TOL})"


def _synthetic(seed, C, D, n, dtype=numpy.float64):
    """a diagonal mixture drawn from a fixed seed and n frames around its components, which overlap (means 0.25 apart per dimension under
    unit noise), so a frame's posterior spreads over its list; the frames rounded to ``dtype`` and widened again: exact operands"""
    rs = numpy.random.RandomState(seed)
    w = rs.rand(C) + 0.5
    ref = mxn.model(w / w.sum(), 0.25 * rs.randn(C, D), 1.0 / (0.5 + rs.rand(C, D)))
    X = (ref["mu"][rs.randint(0, C, n)] + 1.1 * rs.randn(n, D)).astype(dtype)
    return ref, X, rs


def _rows(rs, N, C, Kc):
    """distinct, random, unsorted candidates"""
    return numpy.array([rs.permutation(C)[:Kc] for _ in range(N)], dtype=numpy.int32)


def _lists_agree(name, got, want, gaps, scale):
    """equal on every frame whose gap exceeds GAP x max |lp|; at most 1 % of the frames under it"""
    under = gaps <= GAP * scale
    print(f"{name}: {int(under.sum())} of {gaps.size} frames under the gap {GAP * scale:.2e}; smallest gap {gaps.min():.3e}")
    assert under.sum() <= 0.01 * gaps.size
    bad = numpy.flatnonzero((got != want).any(axis=1) & ~under)
    assert bad.size == 0, f"{name}: lists differ on frames {bad[:8].tolist()}: {got[bad[:3]].tolist()} for {want[bad[:3]].tolist()}"


def _refine(ubm, x, cand, K, posteriors=True):
    from sidekit_amd.mixture import gmm_topc_refine_device
    return gmm_topc_refine_device(ubm, x, cand, top_c=K, posteriors=posteriors)


# ---- 1. the kernel against the restatement ----------------------------------------------------------------------------------------------
SHAPES = [(130, 60, 150, 20, 10),    # two component tiles, two frame tiles plus two rows
          (1, 1, 2, 1, 1),
          (67, 128, 70, 64, 32),     # the second d trip, a full wave of candidates, SC_GMM_TOPC_MAX
          (130, 65, 40, 7, 10),      # K > Kc: padding
          (70, 64, 70, 10, 5),       # the last D a wave's 64 lanes cover in one pass; a full tile and six frames
          (70, 65, 70, 10, 5)]       # the first D with a second pass, one lane wide


@pytest.mark.parametrize("dtype", [numpy.float32, numpy.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N{}-D{}-C{}-Kc{}-K{}".format(*s))
def test_shapes_against_the_restatement(gpu, shape, dtype):
    import torch
    from sidekit_amd.mixture import gmm_topc_posteriors_device
    N, D, C, Kc, K = shape
    ref, X, rs = _synthetic(21, C, D, N, dtype)
    cand = _rows(rs, N, C, Kc)
    ubm, x, d_cand = _mixture(ref), torch.as_tensor(X).to(gpu), torch.as_tensor(cand).to(gpu)
    idx, post, lse = _refine(ubm, x, d_cand, K)
    assert idx.is_cuda and idx.dtype == torch.int32 and idx.shape == (N, K) and post.dtype == torch.float64 and post.shape == (N, K) and lse.shape == (N,)
    wide = X.astype(numpy.float64)
    want, gaps = gem.select(ref, wide, cand, K)
    _lists_agree(str(shape), _np(idx), want, gaps, numpy.abs(gtn.log_posteriors(ref, wide)).max())
    filled = min(K, Kc)
    assert bool((idx[:, filled:] == -1).all()) and bool((idx[:, :filled] >= 0).all()) and bool((idx[:, 1:filled] > idx[:, :filled - 1]).all()), "ascending, then -1"
    rpost, rlse = gem.gsn.posteriors(ref, wide, _np(idx))    # on the device's own lists: exact operands
    _check({"post": mxn.rel(_np(post), rpost), "lse": mxn.rel(_np(lse), rlse), "rows of post sum to 1": numpy.abs(_np(post).sum(1) - 1.0).max()})
    # bits: the posteriors kernel on the same lists; the lists without the posteriors; the same call again
    same = gmm_topc_posteriors_device(ubm, x, top_c=K, components=idx)
    assert torch.equal(same[1], post) and torch.equal(same[2], lse), "post and lse are sc_gmm_topc_posteriors' for the list"
    alone = _refine(ubm, x, d_cand, K, posteriors=False)
    assert torch.is_tensor(alone) and torch.equal(alone, idx), "the lists do not depend on whether the posteriors are requested"
    again = _refine(ubm, x, d_cand, K)
    assert torch.equal(again[0], idx) and torch.equal(again[1], post) and torch.equal(again[2], lse), "run to run"
    h_idx, h_post, h_lse = _refine(ubm, X, cand, K)   # a host array in gives host arrays out, with the same bits
    assert isinstance(h_idx, numpy.ndarray) and numpy.array_equal(h_idx, _np(idx)) and numpy.array_equal(h_post, _np(post)) and numpy.array_equal(h_lse, _np(lse))


def test_split_candidates_on_the_device(gpu):
    import torch
    from sidekit_amd.mixture import split_candidates
    idx = numpy.array([[0, 2, 5], [1, -1, 7], [-1, -1, -1]], dtype=numpy.int32)
    got = split_candidates(torch.as_tensor(idx).to(gpu), 8)
    assert got.is_cuda and got.dtype == torch.int32 and got.is_contiguous() and numpy.array_equal(_np(got), split_candidates(idx, 8))


# ---- 2. hostile candidates, ties, zero weight -------------------------------------------------------------------------------------------
def test_hostile_candidates(gpu):
    import torch
    C, D, N, Kc, K = 20, 7, 70, 8, 4
    ref, X, rs = _synthetic(5, C, D, N)
    cand = _rows(rs, N, C, Kc)
    cand[3] = (4, 4, -1, C, 4, I32_MAX, I32_MIN, 4)              # one valid entry, three times
    cand[10] = (-1, C, I32_MAX, I32_MIN, -5, C + 1, -1, C)       # none
    cand[11] = (7, 2, 7, 2, 9, 9, 7, 2)                          # three
    cand[64] = (19, I32_MAX, 0, 19, I32_MIN, 0, 5, C)            # in the second tile
    cand[20:30, 1] = cand[20:30, 0]                              # a repeat beside its first
    cand[30:40, 5] = -1
    cand[40:50, 2] = C
    X[50] = numpy.nan
    ubm, x = _mixture(ref), torch.as_tensor(X).to(gpu)
    idx, post, lse = _refine(ubm, x, torch.as_tensor(cand).to(gpu), K)
    ok = numpy.arange(N) != 50
    want, gaps = gem.select(ref, X[ok], cand[ok], K)
    _lists_agree("hostile rows", _np(idx)[ok], want, gaps, numpy.abs(gtn.log_posteriors(ref, X[ok])).max())
    assert _np(idx)[3].tolist() == [4, -1, -1, -1] and _np(post)[3].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert _np(idx)[10].tolist() == [-1] * 4 and float(lse[10]) == -numpy.inf and bool((post[10] == 0).all()), "a row with no valid entry"
    assert _np(idx)[11].tolist() == [2, 7, 9, -1] and _np(idx)[64].tolist() == [0, 5, 19, -1]
    assert _np(idx)[50].tolist() == sorted(cand[50].tolist())[:K], "a frame of nan: every lp ranks as -inf, the lower indices win"
    assert float(lse[50]) == -numpy.inf and bool((post[50] == 0).all())
    keep = ok & (numpy.arange(N) != 10)
    rpost, rlse = gem.gsn.posteriors(ref, X[keep], _np(idx)[keep])
    _check({"post": mxn.rel(_np(post)[keep], rpost), "lse": mxn.rel(_np(lse)[keep], rlse)})
    assert bool(torch.isfinite(post).all()) and bool(((idx >= -1) & (idx < C)).all())


def test_ties_go_to_the_lower_index(gpu):
    """rows c and c + C / 2 bit-identical, weights included: K = 5 takes two pairs and the lower half of a third"""
    import torch
    C, D, N, K = 16, 9, 70, 5
    rs = numpy.random.RandomState(8)
    half = mxn.model(numpy.full(C // 2, 2.0 / C), 0.5 * rs.randn(C // 2, D), 1.0 / (0.5 + rs.rand(C // 2, D)))
    ref = mxn.model(numpy.tile(half["w"], 2) * 0.5, numpy.tile(half["mu"], (2, 1)), numpy.tile(half["invcov"], (2, 1)))
    X = half["mu"][rs.randint(0, C // 2, N)] + 1.1 * rs.randn(N, D)
    cand = _rows(rs, N, C, C)
    scale = numpy.abs(gtn.log_posteriors(ref, X)).max()
    for k in (4, 6):   # between two pairs the gaps are wide
        assert gem.select(ref, X, cand, k)[1].min() > GAP * scale
    want, gaps = gem.select(ref, X, cand, K)
    assert bool((gaps == 0.0).all()), "the fifth and the sixth are one pair"
    idx = _np(_refine(_mixture(ref), torch.as_tensor(X).to(gpu), torch.as_tensor(cand).to(gpu), K, posteriors=False))
    assert numpy.array_equal(idx, want) and bool((numpy.diff(idx, axis=1) > 0).all())
    for row in idx:
        low = [c for c in row if c < C // 2]
        assert len(low) == 3 and sum(c + C // 2 in row for c in low) == 2, "one pair is cut: its lower index stays"


def test_zero_weight_component_ranks_last(gpu):
    import torch
    C, D, N, K, Z = 12, 6, 70, 4, 7
    rs = numpy.random.RandomState(13)
    w = rs.rand(C) + 0.5
    w[Z] = 0.0
    with numpy.errstate(divide="ignore"):
        ref = mxn.model(w / w.sum(), 0.25 * rs.randn(C, D), 1.0 / (0.5 + rs.rand(C, D)))
    X = ref["mu"][rs.randint(0, C, N)] + 1.1 * rs.randn(N, D)
    others = numpy.setdiff1d(numpy.arange(C), [Z])
    cand = numpy.full((N, 6), -1, dtype=numpy.int32)
    for n in range(N):
        pick = rs.permutation(others)
        row = [Z] + pick[:5].tolist() if n % 2 == 0 else [Z] + pick[:2].tolist()   # even: five others; odd: two, so Z is needed
        cand[n, :len(row)] = rs.permutation(row)
    idx, post, lse = _refine(_mixture(ref), torch.as_tensor(X).to(gpu), torch.as_tensor(cand).to(gpu), K)
    idx, post = _np(idx), _np(post)
    with numpy.errstate(invalid="ignore"):
        want, gaps = gem.select(ref, X, cand, K)
    _lists_agree("zero weight", idx, want, gaps, numpy.abs(gtn.log_posteriors(ref, X)[:, others]).max())
    assert not (idx[0::2] == Z).any(), "five finite candidates for four places: not listed"
    assert bool(((idx[1::2] == Z).sum(1) == 1).all()) and bool((idx[1::2, 3] == -1).all()), "two finite candidates: listed, then padding"
    assert bool((post[idx == Z] == 0.0).all()) and numpy.abs(post.sum(1) - 1.0).max() < TOL and bool(torch.isfinite(lse).all())


# ---- 3. independence, sentinels ---------------------------------------------------------------------------------------------------------
def test_a_frames_outputs_depend_on_that_frame_alone(gpu):
    import torch
    N, D, C, Kc, K = 130, 60, 150, 20, 10
    ref, X, rs = _synthetic(21, C, D, N)
    ubm, x, cand = _mixture(ref), torch.as_tensor(X).to(gpu), torch.as_tensor(_rows(rs, N, C, Kc)).to(gpu)
    inside = _refine(ubm, x, cand, K)
    alone = _refine(ubm, x[5:10].clone(), cand[5:10].clone(), K)
    assert all(torch.equal(a, b[5:10]) for a, b in zip(alone, inside)), "rows 5 .. 9 alone"
    late = _refine(ubm, x[60:].clone(), cand[60:].clone(), K)    # a tile boundary in another place
    assert all(torch.equal(a, b[60:]) for a, b in zip(late, inside))


def test_one_row_behind_every_output_is_untouched(gpu):
    import torch
    from sidekit_amd import _lib, mixture
    N, D, C, Kc, K = 130, 65, 40, 7, 10
    ref, X, rs = _synthetic(21, C, D, N)
    ubm, x, cand = _mixture(ref), torch.as_tensor(X).to(gpu), torch.as_tensor(_rows(rs, N, C, Kc)).to(gpu)
    want = _refine(ubm, x, cand, K)
    operands = mixture._topc_model(torch, ubm, gpu)
    for with_post in (True, False):
        idx = torch.full((N + 1, K), -77, dtype=torch.int32, device=gpu)
        post = torch.full((N + 1, K), 123.0, dtype=torch.float64, device=gpu)
        lse = torch.full((N + 1,), 123.0, dtype=torch.float64, device=gpu)
        _lib.launch("sc_gmm_topc_refine", gpu, x, _lib.XT_F64, N, D, *operands, C, cand, Kc, K, idx, post if with_post else None, lse if with_post else None)
        torch.cuda.synchronize()
        assert torch.equal(idx[:N], want[0]) and bool((idx[N] == -77).all())
        if with_post:
            assert torch.equal(post[:N], want[1]) and torch.equal(lse[:N], want[2]) and bool((post[N] == 123.0).all()) and float(lse[N]) == 123.0
        else:
            assert bool((post == 123.0).all()) and bool((lse == 123.0).all()), "not requested: not written"


# ---- 4. every component as a candidate: the dense lists ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [numpy.float32, numpy.float64], ids=["f32", "f64"])
def test_all_components_as_candidates_give_the_dense_lists(gpu, dtype):
    """C = 48, K = 10: sc_gmm_top_components forms lp by the half-GEMM, this kernel directly, so the demand is the gap's"""
    import torch
    from sidekit_amd.gmm_scoring import gmm_top_components_device
    C, D, N, K = 48, 23, 200, 10
    ref, X, rs = _synthetic(31, C, D, N, dtype)
    ubm, x = _mixture(ref), torch.as_tensor(X).to(gpu)
    idx = _refine(ubm, x, torch.as_tensor(_rows(rs, N, C, C)).to(gpu), K, posteriors=False)
    lp = gtn.log_posteriors(ref, X.astype(numpy.float64))
    ranked = -numpy.sort(-lp, axis=1)
    assert abs((ranked[:, K - 1] - ranked[:, K]).min() - gtn.gap(ref, X.astype(numpy.float64), K)[0]) == 0.0, "per frame what gmm_topc_numpy.gap reduces"
    _lists_agree("dense lists", _np(idx), _np(gmm_top_components_device(ubm, x, top_c=K)), ranked[:, K - 1] - ranked[:, K], numpy.abs(lp).max())


# ---- 5. the driver ----------------------------------------------------------------------------------------------------------------------
def recipe():
    rs = numpy.random.RandomState(0)
    ctr = 3 * rs.randn(16, 5)
    return ctr[rs.randint(16, size=600)] + rs.randn(600, 5) * (0.5 + rs.rand(600, 1))


@pytest.fixture(scope="module")
def trained(gpu):
    """the recipe at top_c = 3, once: the resident frames, the mixture, its llk list"""
    import torch
    from sidekit_amd.mixture import em_split_topc_device
    x = torch.as_tensor(recipe()).to(gpu)
    ubm, llk = em_split_topc_device(x, 16, ITERATIONS, top_c=3)
    return x, ubm, llk


def test_top_c_that_covers_every_level_is_em_split_device(gpu, trained):
    from sidekit_amd.mixture import em_split_device, em_split_topc_device
    x = trained[0]
    dense, dense_llk = em_split_device(x, 16, ITERATIONS)
    for top_c in (16, 32):
        ubm, llk = em_split_topc_device(x, 16, ITERATIONS, top_c=top_c)
        assert llk == dense_llk and len(llk) == 9
        assert numpy.array_equal(ubm.w, dense.w) and numpy.array_equal(ubm.mu, dense.mu) and numpy.array_equal(ubm.invcov, dense.invcov)


@pytest.mark.parametrize("exact", [(), (8, 16)], ids=["tree", "exact-lists-at-8-and-16"])
def test_driver_against_the_restatement(gpu, trained, exact):
    """the restatement's smallest candidate gap over all refinements of this recipe is 8.7e-4 (tests/test_gmm_topc_em_cpu.py): equal lists
    are a fair demand"""
    import torch
    from sidekit_amd.mixture import Mixture, em_split_topc_device
    x = trained[0]
    trace, want_idx, gap = gem.em_split_topc(recipe(), 16, ITERATIONS, 3, exact_lists_at=exact)
    print(f"smallest candidate gap of the restatement: {gap:.3e}")
    ubm = Mixture()
    llk, idx = ubm._em_split(x, 16, ITERATIONS, None, 10, 1e-2, top_c=3, exact_lists_at=exact)
    assert idx.is_cuda and idx.dtype == torch.int32 and numpy.array_equal(_np(idx), want_idx), "the lists the last level ended with"
    final = trace[-1][0]
    _check({"llk": mxn.rel(llk, [l for _, l in trace]), "w": mxn.rel(ubm.w, final["w"]), "mu": mxn.rel(ubm.mu, final["mu"]),
            "invcov": mxn.rel(ubm.invcov, final["invcov"])})
    public, public_llk = em_split_topc_device(x, 16, ITERATIONS, top_c=3, exact_lists_at=exact)
    assert public_llk == llk and numpy.array_equal(public.mu, ubm.mu) and numpy.array_equal(public.invcov, ubm.invcov) and numpy.array_equal(public.w, ubm.w)
    if not exact:
        assert public_llk == trained[2] and numpy.array_equal(public.mu, trained[1].mu), "two runs give the same bits"
    else:
        assert public_llk != trained[2], "exact lists at 8 and 16 components change the run"


def test_wiring(gpu, trained, tmp_path):
    from sidekit_amd.mixture import Mixture, em_split_topc_device
    x, ubm, llk = trained
    X = recipe()
    seen = []
    again, again_llk = em_split_topc_device(x, 16, ITERATIONS, top_c=3, after_iteration=lambda m, v: seen.append((m.get_distrib_nb(), v)))
    assert [c for c, _ in seen] == [2, 4, 4, 8, 8, 16, 16, 16, 16] and [v for _, v in seen] == again_llk == llk, "once per M-step"
    parts = numpy.array_split(X, 22)   # more than 20 sessions: the single Gaussian comes from the first 20
    sessions = [f"show{i}" for i in range(22)]

    class Server:
        calls = []

        def stack_features(self, shows, start_list=None, stop_list=None):
            self.calls.append(list(shows))
            return numpy.concatenate([parts[int(s[4:])] for s in shows])

    head = sum(p.shape[0] for p in parts[:20])
    direct, direct_llk = em_split_topc_device(x, 16, ITERATIONS, top_c=3, init_frames=head, exact_lists_at=(8,))
    m = Mixture()
    out = os.path.join(str(tmp_path), "ubm")
    got = m.EM_split_topc(Server(), sessions, 16, ITERATIONS, top_c=3, save_partial=True, output_file_name=out, exact_lists_at=(8,))
    assert Server.calls == [sessions[:20], sessions[20:]], "every session stacked once"
    assert got == direct_llk and numpy.array_equal(m.w, direct.w) and numpy.array_equal(m.mu, direct.mu) and numpy.array_equal(m.invcov, direct.invcov)
    assert sorted(os.listdir(str(tmp_path))) == ["ubm_1g.h5", "ubm_2g.h5", "ubm_4g.h5", "ubm_8g.h5"], "before every split"
    assert Mixture(out + "_8g.h5").mu.shape == (8, 5)
