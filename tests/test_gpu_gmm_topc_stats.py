"""Top-C Baum-Welch statistics on the GPU (sidekit_amd/mixture.py gmm_topc_posteriors_device / gmm_stats_topc_device, csrc/gmm_topc_stats.hip)
against the float64 numpy restatement (tests/tools/gmm_topc_stats_numpy.py, held to 1e-12 against the dense restatement by
tests/test_gmm_topc_stats_cpu.py), against the dense route (gmm_stats_device) with every component listed, and against top-C scoring
at the seam the two share (a frame's lse).

TOL = 1e-9 relative max-norm, the project's bound for float64 quantities.  The restatement is evaluated on the device's own lists
(exact operands), so a near-tie between two log posteriors cannot move a frame from one list to another between the two sides.  Every
comparison prints the error it measured.  The bitwise tests are exact: no floating-point atomics, every sum in an order that depends on
the segment's own frames and lists alone.
"""
import os
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gmm_topc_stats_numpy as gsn  # noqa: E402
import mixture_numpy as mxn  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9
KEYS = ("w", "mu", "invcov", "cov_var_ctl")
LENGTHS = [3, 301, 0, 64, 130, 17, 700, 45]   # the fixture's segments: one empty, one shorter than a tile, one cut into two slabs


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


def _equal(a, b):
    import torch
    return all((p is None and q is None) or torch.equal(p, q) for p, q in zip(a, b))


@pytest.fixture(scope="module")
def golden(golden_dir):
    """the fixture's final mixture (C = 8, D = 23), its restatement model, the 1 260 frames and the eight segments"""
    fx = dict(numpy.load(os.path.join(golden_dir, "mixture.npz")))
    ref = mxn.model(*(fx[f"split4_{k}"] for k in KEYS))
    assert list(numpy.diff(fx["seg_off"])) == LENGTHS
    return _mixture(ref), ref, fx["X"], fx["seg_off"]


@pytest.fixture(scope="module")
def three(gpu, golden):
    """K = 3 on the fixture, computed once and left unchanged: the resident frames, the device's lists, posteriors and statistics"""
    import torch
    from sidekit_amd.mixture import gmm_stats_topc_device, gmm_topc_posteriors_device
    ubm, ref, X, off = golden
    x = torch.as_tensor(X).to(gpu)
    idx, post, lse = gmm_topc_posteriors_device(ubm, x, top_c=3)
    stats = gmm_stats_topc_device(ubm, x, off, order=2, top_c=3)
    return x, idx, post, lse, stats


# ---- 1. the restatement on the device's lists -------------------------------------------------------------------------------------------
def test_fixture_against_the_restatement(gpu, golden, three):
    import torch
    from sidekit_amd.gmm_scoring import gmm_top_components_device
    from sidekit_amd.mixture import gmm_stats_topc_device, gmm_topc_posteriors_device
    ubm, ref, X, off = golden
    x, idx, post, lse, (s0, s1, s2, llk) = three
    assert idx.is_cuda and idx.dtype == torch.int32 and idx.shape == (1260, 3) and torch.equal(idx, gmm_top_components_device(ubm, x, top_c=3))
    assert post.is_cuda and post.dtype == torch.float64 and post.shape == (1260, 3) and lse.shape == (1260,)
    assert s0.is_cuda and s0.shape == (8, 8) and s1.shape == (8, 8, 23) and s2.shape == (8, 8, 23) and llk.shape == (8,)
    r0, r1, r2, rl, rpost, rlse = gsn.stats(ref, X, _np(idx), off)
    lens = numpy.diff(off)
    _check({"post": mxn.rel(_np(post), rpost), "lse": mxn.rel(_np(lse), rlse), "stat0": mxn.rel(_np(s0), r0), "stat1": mxn.rel(_np(s1), r1),
            "stat2": mxn.rel(_np(s2), r2), "llk": mxn.rel(_np(llk), rl), "rows of post sum to 1": numpy.abs(_np(post).sum(1) - 1.0).max(),
            "stat0 of a segment sums to its length": numpy.abs(_np(s0).sum(1) - lens).max() / lens.max()})
    assert bool((s0[2] == 0).all()) and bool((s1[2] == 0).all()) and bool((s2[2] == 0).all()) and float(llk[2]) == 0.0, "the empty segment: exact zeros"
    # a host array in gives host arrays out, with the same bits
    h_idx, h_post, h_lse = gmm_topc_posteriors_device(ubm, X, top_c=3)
    assert isinstance(h_post, numpy.ndarray) and numpy.array_equal(h_idx, _np(idx)) and numpy.array_equal(h_post, _np(post)) and numpy.array_equal(h_lse, _np(lse))
    h = gmm_stats_topc_device(ubm, X, off, order=2, top_c=3)
    assert all(isinstance(a, numpy.ndarray) and numpy.array_equal(a, _np(b)) for a, b in zip(h, (s0, s1, s2, llk)))


# ---- 2. every component: the dense route ------------------------------------------------------------------------------------------------
def test_every_component_is_the_dense_route(gpu, golden, three):
    import torch
    from sidekit_amd.mixture import frame_loglik_device, gmm_stats_device, gmm_stats_topc_device, gmm_topc_posteriors_device
    ubm, ref, X, off = golden
    x = three[0]
    d0, d1, d2, dl = gmm_stats_device(ubm, x, off, order=2)
    for top_c in (8, 32):
        idx, post, lse = gmm_topc_posteriors_device(ubm, x, top_c=top_c)
        assert idx.shape == (1260, 8) and bool((idx == torch.arange(8, dtype=torch.int32, device=gpu)).all())
        s0, s1, s2, llk = gmm_stats_topc_device(ubm, x, off, order=2, top_c=top_c)
        _check({"stat0": mxn.rel(_np(s0), _np(d0)), "stat1": mxn.rel(_np(s1), _np(d1)), "stat2": mxn.rel(_np(s2), _np(d2)), "llk": mxn.rel(_np(llk), _np(dl)),
                "lse": mxn.rel(_np(lse), _np(frame_loglik_device(ubm, x)))})


# ---- 3. bits ----------------------------------------------------------------------------------------------------------------------------
def test_bits(gpu, golden, three):
    import torch
    from sidekit_amd.mixture import gmm_stats_topc_device, gmm_topc_posteriors_device
    ubm, ref, X, off = golden
    x, idx, post, lse, stats = three
    assert _equal(gmm_stats_topc_device(ubm, x, off, order=2, top_c=3), stats) and _equal(gmm_topc_posteriors_device(ubm, x, top_c=3), (idx, post, lse)), "the same calls again"
    assert _equal(gmm_stats_topc_device(ubm, x, off, order=2, top_c=3, components=idx), stats), "lists passed in"
    o0, o1, o2, ol = gmm_stats_topc_device(ubm, x, off, order=1, top_c=3)
    assert o2 is None and _equal((o0, o1, ol), (stats[0], stats[1], stats[3])), "order 1 is order 2 without the second moments"
    front = x[100:137]
    for s in (0, 4, 6):   # shorter than a tile; three tiles; two slabs
        a, b = int(off[s]), int(off[s + 1])
        alone = gmm_stats_topc_device(ubm, x[a:b].clone(), None, order=2, top_c=3, components=idx[a:b].clone())
        assert all(torch.equal(t[0], u[s]) for t, u in zip(alone, stats)), f"segment {s} alone with its own rows of idx"
        moved = gmm_stats_topc_device(ubm, torch.cat((front, x[a:b])), [37, 37 + b - a], order=2, top_c=3, components=torch.cat((idx[100:137], idx[a:b])))
        assert all(torch.equal(t[0], u[s]) for t, u in zip(moved, stats)), f"segment {s} with 37 other frames in front of it in X"
        p_alone = gmm_topc_posteriors_device(ubm, x[a:b].clone(), top_c=3)
        assert _equal(p_alone, (idx[a:b], post[a:b], lse[a:b])), f"segment {s}'s frames alone: their lists, posteriors and lse"
    x32 = torch.as_tensor(X.astype(numpy.float32)).to(gpu)
    wide = x32.double()
    assert _equal(gmm_topc_posteriors_device(ubm, x32, top_c=3), gmm_topc_posteriors_device(ubm, wide, top_c=3)), "float32 frames are widened in the load"
    assert _equal(gmm_stats_topc_device(ubm, x32, off, order=2, top_c=3), gmm_stats_topc_device(ubm, wide, off, order=2, top_c=3))
    assert _equal(gmm_stats_topc_device(ubm, x, off, order=2, top_c=3, max_workspace_bytes=1), stats), "one segment per call"


# ---- 4. the seam with top-C scoring -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [23, 70])
def test_lse_is_the_scoring_kernels_frame_term(gpu, golden, D):
    """70 single-frame segments: a segment's llk under a model whose means are the UBM's is that frame's term, and lse has its bits"""
    import torch
    from sidekit_amd.gmm_scoring import gmm_llk_topc_device
    from sidekit_amd.mixture import gmm_topc_posteriors_device
    if D == 23:
        ubm, _, X, _ = golden
        X = X[300:370]
    else:
        ubm, _, X = _synthetic(7, 40, D, 70)
    x = torch.as_tensor(X).to(gpu)
    for K in (1, 3, 5):
        idx, post, lse = gmm_topc_posteriors_device(ubm, x, top_c=K)
        llk, lens = gmm_llk_topc_device(ubm, ubm.mu[None], x, numpy.arange(71), top_c=K, components=idx)
        assert llk.shape == (1, 70) and bool((lens == 1).all())
        assert torch.equal(llk[0], lse), f"D = {D}, K = {K}: largest difference {float((llk[0] - lse).abs().max()):.3e}"


# ---- 5. second trips --------------------------------------------------------------------------------------------------------------------
def _synthetic(seed, C, D, n, far=()):
    """a diagonal mixture drawn from a fixed seed and n frames around its components, which overlap (means 0.25 apart per dimension under
    unit noise), so a frame's posterior spreads over its list; the components `far` lie where no frame lists them"""
    rs = numpy.random.RandomState(seed)
    w = rs.rand(C) + 0.5
    mu = 0.25 * rs.randn(C, D)
    mu[list(far)] += 1000.0
    ref = mxn.model(w / w.sum(), mu, 1.0 / (0.5 + rs.rand(C, D)))
    near = numpy.setdiff1d(numpy.arange(C), far)
    X = ref["mu"][near[rs.randint(0, near.size, n)]] + 1.1 * rs.randn(n, D)
    return _mixture(ref), ref, X


def test_second_trips_against_the_restatement(gpu):
    """C = 150: three component blocks, the last one partial; D = 70: the second pass over d; K = 32: SC_GMM_TOPC_MAX; a segment of 1 100
    frames (three slabs) between two short ones"""
    import torch
    from sidekit_amd import mixture
    far = (5, 64, 149)
    lengths = [5, 1100, 9]
    assert mixture._slabs(1100) == 3
    ubm, ref, X = _synthetic(11, 150, 70, sum(lengths), far)
    off = numpy.concatenate(([0], numpy.cumsum(lengths)))
    x = torch.as_tensor(X).to(gpu)
    idx, post, lse = mixture.gmm_topc_posteriors_device(ubm, x, top_c=32)
    s0, s1, s2, llk = mixture.gmm_stats_topc_device(ubm, x, off, order=2, top_c=32, components=idx)
    lists = _np(idx)
    assert lists.shape == (1114, 32) and lists.min() >= 0 and lists.max() < 150 and not numpy.isin(lists, far).any()
    r0, r1, r2, rl, rpost, rlse = gsn.stats(ref, X, lists, off)
    _check({"post": mxn.rel(_np(post), rpost), "lse": mxn.rel(_np(lse), rlse), "stat0": mxn.rel(_np(s0), r0), "stat1": mxn.rel(_np(s1), r1),
            "stat2": mxn.rel(_np(s2), r2), "llk": mxn.rel(_np(llk), rl), "rows of post sum to 1": numpy.abs(_np(post).sum(1) - 1.0).max(),
            "stat0 of a segment sums to its length": numpy.abs(_np(s0).sum(1) - lengths).max() / max(lengths)})
    for s in range(3):
        unlisted = numpy.setdiff1d(numpy.arange(150), lists[off[s]:off[s + 1]])
        assert set(far) <= set(unlisted)
        print(f"segment {s}: {unlisted.size} components that no frame lists")
        assert bool((s0[s, unlisted] == 0).all()) and bool((s1[s, unlisted] == 0).all()) and bool((s2[s, unlisted] == 0).all()), "exact zeros"
    o0, o1, o2, ol = mixture.gmm_stats_topc_device(ubm, x, off, order=1, top_c=32, components=idx)
    assert o2 is None and torch.equal(o0, s0) and torch.equal(o1, s1) and torch.equal(ol, llk)


@pytest.mark.parametrize("D", [64, 65])
def test_posteriors_at_the_second_lane_pass_against_the_restatement(gpu, D):
    """D = 64: the last size a wave's 64 lanes cover in one pass; D = 65: the first with a second pass, one lane wide.  70 frames (a full
    tile and six frames), C = 70, K = 5"""
    import torch
    from sidekit_amd import mixture
    ubm, ref, X = _synthetic(D, 70, D, 70)
    off = numpy.array([0, 70])
    x = torch.as_tensor(X).to(gpu)
    idx, post, lse = mixture.gmm_topc_posteriors_device(ubm, x, top_c=5)
    s0, s1, s2, llk = mixture.gmm_stats_topc_device(ubm, x, off, order=2, top_c=5, components=idx)
    lists = _np(idx)
    assert lists.shape == (70, 5) and lists.min() >= 0 and lists.max() < 70
    r0, r1, r2, rl, rpost, rlse = gsn.stats(ref, X, lists, off)
    _check({"post": mxn.rel(_np(post), rpost), "lse": mxn.rel(_np(lse), rlse), "stat0": mxn.rel(_np(s0), r0), "stat1": mxn.rel(_np(s1), r1),
            "stat2": mxn.rel(_np(s2), r2), "llk": mxn.rel(_np(llk), rl), "rows of post sum to 1": numpy.abs(_np(post).sum(1) - 1.0).max()})


# ---- 6. the caller's lists --------------------------------------------------------------------------------------------------------------
def test_callers_lists_invalid_entries_and_zero_weight(gpu):
    import torch
    from sidekit_amd.mixture import gmm_stats_topc_device, gmm_topc_posteriors_device
    rs = numpy.random.RandomState(44)
    C, D, lengths = 4, 8, [30, 70, 5]
    with numpy.errstate(divide="ignore"):
        ref = mxn.model([0.5, 0.0, 0.25, 0.25], 2.0 * rs.randn(C, D), 1.0 / (0.5 + rs.rand(C, D)))
    ubm = _mixture(ref)
    X = ref["mu"][rs.randint(0, C, sum(lengths))] + 1.1 * rs.randn(sum(lengths), D)
    off = numpy.concatenate(([0], numpy.cumsum(lengths)))
    x = torch.as_tensor(X).to(gpu)
    clean = numpy.tile(numpy.array([3, 1, 0], dtype=numpy.int32), (105, 1))   # any order; component 1 has weight 0
    lists = clean.copy()
    lists[40] = (-1, 3, C)       # in the second segment: one valid entry
    lists[50] = (-1, C, 99)      # and a frame without any
    want = gsn.stats(ref, X, lists, off)
    idx, post, lse = gmm_topc_posteriors_device(ubm, x, top_c=3, components=lists)
    assert idx.is_cuda and numpy.array_equal(_np(idx), lists)
    s0, s1, s2, llk = gmm_stats_topc_device(ubm, x, off, order=2, top_c=3, components=torch.as_tensor(lists).to(gpu))
    ok = numpy.arange(105) != 50
    plain = ok & (numpy.arange(105) != 40)
    _check({"post": mxn.rel(_np(post), want[4]), "lse": mxn.rel(_np(lse)[ok], want[5][ok]), "stat0": mxn.rel(_np(s0), want[0]), "stat1": mxn.rel(_np(s1), want[1]),
            "stat2": mxn.rel(_np(s2), want[2]), "llk": mxn.rel(_np(llk)[[0, 2]], want[3][[0, 2]])})
    assert bool((_np(post)[plain][:, 1] == 0).all()) and bool((s0[:, 1] == 0).all()) and bool((s1[:, 1] == 0).all()), "a listed component of weight 0: posterior exactly 0"
    assert _np(post)[40].tolist() == [0.0, 1.0, 0.0], "an entry of -1 and an entry of C contribute nothing"
    assert float(lse[50]) == -numpy.inf and bool((post[50] == 0).all()) and float(llk[1]) == -numpy.inf and want[3][1] == -numpy.inf
    assert bool(torch.isfinite(s0).all()) and bool(torch.isfinite(s1).all()) and bool(torch.isfinite(s2).all())
    assert abs(float(s0[1].sum()) - 69.0) < TOL * 69, "the frame without a valid entry adds nothing to the statistics"
    base = gmm_stats_topc_device(ubm, x, off, order=2, top_c=3, components=clean)
    assert all(torch.equal(t[[0, 2]], u[[0, 2]]) for t, u in zip((s0, s1, s2, llk), base)), "every other segment's bits are unchanged"


# ---- 7. StatServer ----------------------------------------------------------------------------------------------------------------------
def test_accumulate_stat_topc_with_a_duck_typed_server(gpu, golden, three):
    import torch
    from sidekit_amd.mixture import gmm_stats_topc_device
    from sidekit_amd.statserver import StatServer
    ubm, ref, X, off = golden
    names = numpy.array([f"show{i}" for i in range(8)], dtype="|O")

    class Server:
        features_extractor = None

        def load(self, show, channel=0):
            i = int(show[4:])
            pad = numpy.full((2, X.shape[1]), 99.0)     # two frames the VAD labels drop
            cep = numpy.concatenate((pad[:1], X[off[i]:off[i + 1]], pad[1:]))
            vad = numpy.ones(cep.shape[0], dtype=bool)
            vad[0] = vad[-1] = False
            return cep, vad

    server = StatServer()
    server.modelset, server.segset = names, names.copy()
    server.start, server.stop = numpy.empty(8, dtype="|O"), numpy.empty(8, dtype="|O")
    server.accumulate_stat_topc(ubm, Server(), top_c=3)
    assert server.validate() and server.stat0.shape == (8, 8) and server.stat1.shape == (8, 8 * 23), "stat1: sessions x C D, what extract_ivectors_device takes"
    resident = StatServer()
    resident.modelset, resident.segset, resident.start, resident.stop = names, names.copy(), server.start, server.stop
    resident.accumulate_stat_topc_device(ubm, three[0], off, top_c=3)
    assert numpy.array_equal(resident.stat0, server.stat0) and numpy.array_equal(resident.stat1, server.stat1)
    s0, s1, _, _ = three[4]
    assert numpy.array_equal(resident.stat0, _np(s0)) and numpy.array_equal(resident.stat1, _np(s1).reshape(8, -1)), "gmm_stats_topc_device's bits"
    dense = StatServer()
    dense.modelset, dense.segset, dense.start, dense.stop = names, names.copy(), server.start, server.stop
    dense.accumulate_stat_device(ubm, three[0], off)
    diff = numpy.abs(dense.stat0 - server.stat0).max()
    print(f"top_c = 3 against accumulate_stat_device: stat0 differs by at most {diff:.3e}")
    assert diff > 0.0, "three of eight components: not the dense statistics"
    with pytest.raises(Exception, match="dimension of ubm and features differ: 23 / 22"):
        resident.accumulate_stat_topc_device(ubm, torch.zeros(4, 22, device=gpu), [0] * 9, top_c=3)
    assert gmm_stats_topc_device(ubm, three[0], off, order=1, top_c=3)[2] is None
