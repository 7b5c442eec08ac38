"""Top-C GMM-UBM scoring on the GPU (sidekit_amd/gmm_scoring.py, csrc/gmm.hip gmm_topc_kernel, csrc/gmm_topc.hip) against the float64 numpy
restatement (tests/tools/gmm_topc_numpy.py, held to 1e-12 against the dense restatement and the reference's own scores by
tests/test_gmm_topc_cpu.py) and against the reference's scores themselves (tests/golden/gmm_scoring.npz).

TOL = 1e-9 relative max-norm as in tests/test_gpu_gmm_scoring.py, for the log-likelihood sums and means; a ratio's bound is absolute,
TOL x the largest |mean llk| of the case.  Lists are compared exactly: before the device's lists are looked at, the test asserts on the
CPU that in every frame the K-th and the (K + 1)-th largest log posterior lie at least 100 x TOL x max |lp| apart -- a hundred times what
the two ways of forming lp may differ by -- so no frame is left out; the seeds are chosen so that this holds.  Every comparison prints
the error it measured.  The bitwise tests are exact: no floating-point atomics, every sum in an order that depends on the segment's own
length alone, every list a function of its own frame.
"""
import os
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gmm_scoring_numpy as gsn  # noqa: E402
import gmm_topc_numpy as gtn  # noqa: E402
import mixture_numpy as mxn  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9
KEYS = ("w", "mu", "invcov", "cov_var_ctl")


@pytest.fixture(scope="module")
def fx(golden_dir):
    out = dict(numpy.load(os.path.join(golden_dir, "gmm_scoring.npz")))
    out.update({"mix_" + k: v for k, v in numpy.load(os.path.join(golden_dir, "mixture.npz")).items()})
    return out


def _mixture(ref):
    from sidekit_amd.mixture import Mixture
    m = Mixture()
    m.w, m.mu, m.invcov, m.cov_var_ctl = (numpy.array(ref[k], dtype=numpy.float64) for k in KEYS)
    m.cst, m.det = numpy.zeros(m.w.shape), numpy.zeros(m.w.shape)
    with numpy.errstate(divide="ignore"):   # a zero weight: log 0
        m._compute_all()
    return m


def _random_case(seed, C, D, lengths, M, spread=0.3):
    """tests/test_gpu_gmm_scoring.py's draw -> (Mixture, restatement model, models (M, C D), X, seg_off)"""
    rs = numpy.random.RandomState(seed)
    w = rs.rand(C) + 0.5
    ref = mxn.model(w / w.sum(), 2.0 * rs.randn(C, D), 1.0 / (0.5 + rs.rand(C, D)))
    models = (ref["mu"][None] + spread * rs.randn(M, C, D)).reshape(M, C * D)
    n = int(sum(lengths))
    X = ref["mu"][rs.randint(0, C, n)] + 1.1 * rs.randn(n, D)
    return _mixture(ref), ref, models, X, numpy.concatenate(([0], numpy.cumsum(lengths)))


def _np(t):
    return t if isinstance(t, numpy.ndarray) else t.cpu().numpy()


def _assert_gap(ref, X, K):
    gap, top = gtn.gap(ref, X, K)
    print(f"K = {K}: smallest gap between the K-th and the next log posterior {gap:.2e}, bound {100 * TOL * top:.2e}")
    assert gap >= 100 * TOL * top, "the case does not separate its lists: choose another seed"


def _assert_valid(idx, C):
    idx = _np(idx)
    assert idx.dtype == numpy.int32 and idx.min() >= 0 and idx.max() < C
    assert numpy.all(numpy.diff(idx.astype(numpy.int64), axis=1) > 0), "a list is stored ascending, so its entries are distinct"


def _check_sums(name, llk, lens, ref, models, X, off, K, mask=None):
    """llk sums and means at TOL relative max-norm, the ratios at TOL x the largest |mean llk|; entries outside the mask are exactly 0"""
    want, want_lens = gtn.llk(ref, list(models) + [ref["mu"].flatten()], X, off, top_c=K)
    assert list(_np(lens)) == list(want_lens)
    got = _np(llk)
    if mask is not None:
        assert numpy.all(got[~mask] == 0.0), "entries without a trial are not written"
        got, want = numpy.where(mask, got, 0.0), numpy.where(mask, want, 0.0)
    some = want_lens > 0
    mean_got, mean_want = got[:, some] / want_lens[some], want[:, some] / want_lens[some]
    errs = {f"{name} llk": mxn.rel(got, want), f"{name} mean llk": mxn.rel(mean_got, mean_want)}
    if mask is None:
        errs[f"{name} llr over the largest mean"] = numpy.abs((mean_got[:-1] - mean_got[-1]) - (mean_want[:-1] - mean_want[-1])).max() / numpy.abs(mean_want).max()
    print({k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < TOL, f"{k} differs by {v:.3e} (bound {TOL})"
    assert numpy.all(got[:, ~some] == 0), "an empty segment's sum is exactly 0"


# ---- 1. lists -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("C,D", [(150, 23), (150, 70), (70, 23), (70, 70)], ids=["three_tiles_d23", "three_tiles_d70", "two_tiles_d23", "two_tiles_d70"])
def test_lists_are_the_restatements(gpu, C, D, dtype):
    """C = 150: two full component tiles and 22 more; N = 130: two frame tiles and two rows; K = 32: SC_GMM_TOPC_MAX"""
    import torch
    from sidekit_amd.gmm_scoring import gmm_top_components_device
    ubm, ref, _, X, _ = _random_case(1, C, D, [130], 1)
    X = X.astype(dtype)
    wide = X.astype(numpy.float64)   # float32 frames are widened in the load: the lists of the widened frames
    x = torch.as_tensor(X).to(gpu)
    for K in (1, 5, 32):
        _assert_gap(ref, wide, K)
        want = gtn.lists(ref, wide, K)
        got = gmm_top_components_device(ubm, x, top_c=K)
        assert got.is_cuda and got.dtype == torch.int32 and got.shape == (130, K)
        _assert_valid(got, C)
        wrong = int((numpy.sort(_np(got), axis=1) != want).any(axis=1).sum())
        print(f"C = {C}, D = {D}, {dtype}, K = {K}: {wrong} of 130 frames with another set")
        assert wrong == 0 and numpy.array_equal(_np(got), want)
    host = gmm_top_components_device(ubm, X, top_c=5)
    assert isinstance(host, numpy.ndarray) and numpy.array_equal(host, gtn.lists(ref, wide, 5))


# ---- 2. sparse sums -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [23, 70])
def test_sums_means_and_ratios(gpu, D):
    """segments: empty, one frame, the tile's edges, two slabs; M = 5 (and the UBM): not a multiple of the model group"""
    import torch
    from sidekit_amd import mixture
    from sidekit_amd.gmm_scoring import gmm_llk_topc_device, gmm_llr_topc_device
    lengths, C, K, M = [0, 1, 63, 64, 65, 700], 70, 5, 5
    assert mixture._slabs(700) == 2
    ubm, ref, models, X, off = _random_case(33, C, D, lengths, M)
    _assert_gap(ref, X, K)
    x = torch.as_tensor(X).to(gpu)
    stacked = numpy.concatenate((models, ref["mu"].reshape(1, -1)))
    llk, lens = gmm_llk_topc_device(ubm, stacked, x, off, top_c=K)
    assert llk.is_cuda and llk.shape == (M + 1, 6)
    _check_sums("device", llk, lens, ref, models, X, off, K)
    host_llk, host_lens = gmm_llk_topc_device(ubm, stacked.reshape(M + 1, C, D), X, off, top_c=K)
    assert isinstance(host_llk, numpy.ndarray) and numpy.array_equal(host_llk, _np(llk)) and list(host_lens) == lengths
    mask = numpy.ones((M + 1, 6), dtype=bool)
    mask[2] = False      # a model without a trial
    mask[:, 4] = False   # a segment without a trial
    masked, _ = gmm_llk_topc_device(ubm, stacked, x, off, mask, top_c=K)
    _check_sums("masked", masked, lens, ref, models, X, off, K, mask)
    d_mask = torch.as_tensor(mask).to(gpu)
    assert torch.equal(masked[d_mask], llk[d_mask]), "a trial's bits do not depend on the mask"
    llr = _np(gmm_llr_topc_device(ubm, models, x, off, mask[:M], top_c=K))
    want = gtn.llr(ref, models, X, off, mask[:M], top_c=K)
    bound = TOL * numpy.abs(gtn.llk(ref, stacked, X, off, top_c=K)[0][:, 1:] / numpy.diff(off)[1:]).max()
    assert numpy.isnan(llr[mask[:M][:, 0], 0]).all() and numpy.isnan(want[mask[:M][:, 0], 0]).all(), "a trial on the empty segment is the mean of nothing"
    assert numpy.all(llr[~mask[:M]] == 0.0)
    err = numpy.abs(llr[:, 1:] - want[:, 1:]).max()
    print(f"llr vs the restatement: {err:.2e}, bound {bound:.2e}")
    assert err < bound


# ---- 3. every component -------------------------------------------------------------------------------------------------------------------
def test_every_component_is_the_dense_score(gpu):
    """D = 3: the components overlap, so the two that top_c = 3 drops carry a weight (at least 1.7e-7 of a segment's sum, by the
    restatement) far above the rounding of either route"""
    import torch
    from sidekit_amd.gmm_scoring import gmm_llk_device, gmm_llk_topc_device, gmm_top_components_device
    ubm, ref, models, X, off = _random_case(41, 5, 3, [70, 3, 64], 3)
    x = torch.as_tensor(X).to(gpu)
    for top_c in (5, 10):
        idx = gmm_top_components_device(ubm, x, top_c=top_c)
        assert idx.shape == (137, 5) and bool((idx == torch.arange(5, dtype=torch.int32, device=gpu)).all())
    dense, _ = gmm_llk_device(ubm, models, x, off)
    sparse, _ = gmm_llk_topc_device(ubm, models, x, off, top_c=5)
    err = mxn.rel(_np(sparse), _np(dense))
    print(f"top_c = C against gmm_llk_device: {err:.2e}")
    assert err < TOL
    fewer, _ = gmm_llk_topc_device(ubm, models, x, off, top_c=3)
    print(f"top_c = 3: dense - sparse in [{float((dense - fewer).min()):.3e}, {float((dense - fewer).max()):.3e}]")
    assert bool((fewer <= dense).all()) and bool((fewer <= sparse).all())


# ---- 4. the UBM against itself ------------------------------------------------------------------------------------------------------------
def test_a_model_equal_to_the_ubm_scores_zero(gpu):
    import torch
    from sidekit_amd.gmm_scoring import gmm_llr_topc_device
    ubm, ref, models, X, off = _random_case(42, 70, 23, [5, 130, 600], 5)
    models[3] = ref["mu"].flatten()
    llr = gmm_llr_topc_device(ubm, models, torch.as_tensor(X.astype(numpy.float32)).to(gpu), off, top_c=7)
    assert llr.is_cuda and llr.shape == (5, 3) and bool((llr[3] == 0.0).all()) and bool((llr[[0, 1, 2, 4]] != 0.0).all()) and bool(torch.isfinite(llr).all())


# ---- 5. bits ------------------------------------------------------------------------------------------------------------------------------
def test_bits(gpu):
    import torch
    from sidekit_amd.gmm_scoring import gmm_llk_topc_device, gmm_top_components_device
    lengths, K = [3, 64, 0, 133], 6
    ubm, ref, models, X, off = _random_case(43, 130, 23, lengths, 7)
    x = torch.as_tensor(X).to(gpu)
    llk, _ = gmm_llk_topc_device(ubm, models, x, off, top_c=K)
    assert bool(torch.isfinite(llk).all()) and bool((llk[:, 2] == 0).all()) and bool((llk[:, [0, 1, 3]] != 0).all())
    for k in range(7):
        assert torch.equal(gmm_llk_topc_device(ubm, models[k:k + 1], x, off, top_c=K)[0][0], llk[k]), f"model {k} alone"
    perm = numpy.array([4, 0, 6, 2, 5, 1, 3])
    assert torch.equal(gmm_llk_topc_device(ubm, models[perm], x, off, top_c=K)[0], llk[torch.as_tensor(perm).to(gpu)]), "at another row"
    for k in (0, 3, 6):
        mask = numpy.zeros((7, 4), dtype=bool)
        mask[k] = True
        alone = gmm_llk_topc_device(ubm, models, x, off, mask, top_c=K)[0]
        assert torch.equal(alone[k], llk[k]) and bool((alone[numpy.arange(7) != k] == 0).all()), f"the others masked out around model {k}"
    # chunks of one model: with one slab the workspace is empty and every model fits, so the long segment below is there to cut
    rs = numpy.random.RandomState(6)
    long = torch.as_tensor(ref["mu"][rs.randint(0, 130, 700)] + rs.randn(700, 23)).to(gpu)
    seg3 = x[off[3]:off[4]].clone()
    xs, offs = torch.cat((long, seg3, x[off[1]:off[2]])), [0, 700, 833, 897]
    moved = gmm_llk_topc_device(ubm, models, xs, offs, top_c=K)[0]
    assert torch.equal(moved[:, 1], llk[:, 3]) and torch.equal(moved[:, 2], llk[:, 1]), "a segment elsewhere in X, behind one that is cut into slabs"
    assert torch.equal(gmm_llk_topc_device(ubm, models, xs, offs, top_c=K, max_workspace_bytes=1)[0], moved), "chunks of one model"
    assert torch.equal(gmm_llk_topc_device(ubm, models, seg3, top_c=K)[0][:, 0], llk[:, 3]), "the 133-frame segment alone"
    lists = gmm_top_components_device(ubm, x, top_c=K)
    assert torch.equal(gmm_llk_topc_device(ubm, models, x, off, top_c=K, components=lists)[0], llk), "lists passed in"
    assert numpy.array_equal(gmm_llk_topc_device(ubm, models, X, off, top_c=K, components=_np(lists))[0], _np(llk)), "lists passed in from the host"
    assert torch.equal(gmm_llk_topc_device(ubm, models, x, off, top_c=K)[0], llk) and torch.equal(gmm_top_components_device(ubm, x, top_c=K), lists), "the same calls again"
    for n in (0, 63, 64, 199):
        assert torch.equal(gmm_top_components_device(ubm, x[n:n + 1].clone(), top_c=K)[0], lists[n]), f"frame {n}'s list alone"
    assert torch.equal(gmm_top_components_device(ubm, x[37:150].clone(), top_c=K), lists[37:150]), "at another place in its tile"


# ---- 6. degenerate input ------------------------------------------------------------------------------------------------------------------
def test_zero_weight_and_nan(gpu):
    import torch
    from sidekit_amd.gmm_scoring import gmm_llk_topc_device, gmm_top_components_device
    rs = numpy.random.RandomState(44)
    C, D, lengths = 4, 8, [30, 70, 5]
    with numpy.errstate(divide="ignore"):
        ref = mxn.model([0.5, 0.0, 0.25, 0.25], 2.0 * rs.randn(C, D), 1.0 / (0.5 + rs.rand(C, D)))
    ubm = _mixture(ref)
    models = (ref["mu"][None] + 0.3 * rs.randn(3, C, D)).reshape(3, C * D)
    X = ref["mu"][rs.randint(0, C, sum(lengths))] + 1.1 * rs.randn(sum(lengths), D)
    X[50, 3] = numpy.nan   # in the second segment
    off = numpy.concatenate(([0], numpy.cumsum(lengths)))
    x = torch.as_tensor(X).to(gpu)
    for K in (4, 2, 1):
        idx = gmm_top_components_device(ubm, x, top_c=K)
        assert idx.shape == (105, K)
        _assert_valid(idx, C)
        clean = numpy.delete(_np(idx), 50, axis=0)
        assert K == 4 or not (clean == 1).any(), "three components have a finite lp: the zero-weight one is not among the best two"
    assert numpy.array_equal(_np(gmm_top_components_device(ubm, x, top_c=4)), numpy.tile(numpy.arange(4, dtype=numpy.int32), (105, 1)))
    for K in (4, 2):
        llk, _ = gmm_llk_topc_device(ubm, models, x, off, top_c=K)
        without = torch.cat((x[:30], x[100:]))
        other, _ = gmm_llk_topc_device(ubm, models, without, [0, 30, 35], top_c=K)
        assert torch.equal(llk[:, [0, 2]], other) and bool(torch.isfinite(other).all()), "the other segments: the same bits as without the nan's segment"
        want, _ = gtn.llk(ref, models, numpy.delete(X, numpy.arange(30, 100), axis=0), [0, 30, 35], top_c=K)
        err = mxn.rel(_np(other), want)
        print(f"K = {K}: the clean segments vs the restatement {err:.2e}")
        assert err < TOL


# ---- 7. range -----------------------------------------------------------------------------------------------------------------------------
def test_range(gpu):
    """tests/test_gpu_gmm_scoring.py::test_range's case: per frame lp_m - lse_ubm is about + 900 for one model and - 2 700 for the other"""
    import torch
    from sidekit_amd.gmm_scoring import gmm_llk_topc_device, gmm_llr_topc_device
    rs = numpy.random.RandomState(24)
    C, D, lengths, K = 4, 8, [40, 1, 90], 2
    ref = mxn.model(numpy.full(C, 0.25), 15.0 + 0.01 * rs.randn(C, D), numpy.ones((C, D)))
    models = numpy.stack((0.01 * rs.randn(C, D), 30.0 + 0.01 * rs.randn(C, D))).reshape(2, C * D)
    X = 0.1 * rs.randn(sum(lengths), D)
    off = numpy.concatenate(([0], numpy.cumsum(lengths)))
    lo, hi = gsn.margin_range(ref, models, X)
    assert hi > 850 and lo < -2600, (lo, hi)
    _assert_gap(ref, X, K)
    want = gtn.llr(ref, models, X, off, top_c=K)
    assert numpy.isfinite(want).all() and want[0].min() > 850 and want[1].max() < -2600
    ubm = _mixture(ref)
    x = torch.as_tensor(X).to(gpu)
    llk, lens = gmm_llk_topc_device(ubm, numpy.concatenate((models, ref["mu"].reshape(1, -1))), x, off, top_c=K)
    assert bool(torch.isfinite(llk).all())
    _check_sums("range", llk, lens, ref, models, X, off, K)
    llr = _np(gmm_llr_topc_device(ubm, models, x, off, top_c=K))
    bound = TOL * numpy.abs(gtn.llk(ref, list(models) + [ref["mu"].flatten()], X, off, top_c=K)[0] / numpy.diff(off)).max()
    err = numpy.abs(llr - want).max()
    print(f"llr in [{llr.min():.1f}, {llr.max():.1f}], error {err:.2e}, bound {bound:.2e}")
    assert numpy.isfinite(llr).all() and err < bound


# ---- 8. gmm_scoring_topc ------------------------------------------------------------------------------------------------------------------
class _Features:
    """the one call gmm_scoring makes"""
    def __init__(self, rows):
        self.rows = rows

    def load(self, show, channel=0):
        return self.rows[show], numpy.ones(self.rows[show].shape[0], dtype=bool)


def _enroll(fx):
    from sidekit_amd.statserver import StatServer
    e = StatServer()
    e.modelset = fx["enroll_modelset"].astype("|O")
    e.segset = e.modelset.copy()
    e.start, e.stop = numpy.empty(5, dtype="|O"), numpy.empty(5, dtype="|O")
    e.stat0, e.stat1 = numpy.ones((5, 1)), fx["enroll_stat1"].copy()
    return e


def _ndx(fx, mask=None):
    from sidekit_amd.bosaris import Ndx
    n = Ndx(models=numpy.repeat(fx["score_modelset"].astype("|O"), 7), testsegs=numpy.tile(fx["score_segset"].astype("|O"), 5))
    if mask is not None:
        n.trialmask = mask.copy()
    return n


def test_fixture_scores(gpu, fx):
    import torch
    from sidekit_amd.gmm_scoring import gmm_llk_topc_device, gmm_llr_topc_device, gmm_scoring, gmm_scoring_topc
    ref = mxn.model(*(fx[f"mix_split4_{k}"] for k in KEYS))
    ubm, enroll = _mixture(ref), _enroll(fx)
    X, off = fx["mix_X"], fx["mix_seg_off"]
    shows = [f"show{i}" for i in range(8)]
    seg = [shows.index(s) for s in fx["score_segset"]]
    order = [list(fx["enroll_modelset"]).index(n) for n in fx["score_modelset"]]
    ubm_row = list(fx["score_modelset"]).index("ubm")
    sums, lens = gsn.llk(ref, fx["enroll_stat1"], X, off)
    bound = TOL * numpy.abs(sums[:, seg] / lens[seg]).max()
    feats = _Features({n: X[off[i]:off[i + 1]] for i, n in enumerate(shows)})
    dense = gmm_scoring(ubm, enroll, _ndx(fx), feats)
    full = gmm_scoring_topc(ubm, enroll, _ndx(fx), feats, top_c=8)
    assert full.validate() and list(full.modelset) == list(dense.modelset) == list(fx["score_modelset"])
    assert list(full.segset) == list(dense.segset) == list(fx["score_segset"]) and numpy.array_equal(full.scoremask, dense.scoremask)
    assert numpy.all(full.scoremat[ubm_row] == 0.0), "the UBM against itself: exactly 0"
    masked = gmm_scoring_topc(ubm, enroll, _ndx(fx, fx["masked_scoremask"]), feats, top_c=32, num_thread=3)
    assert numpy.array_equal(masked.scoremask, fx["masked_scoremask"]) and numpy.all(masked.scoremat[~fx["masked_scoremask"]] == 0.0)
    assert numpy.array_equal(masked.scoremat[fx["masked_scoremask"]], full.scoremat[fx["masked_scoremask"]]), "a trial's bits do not depend on the mask"
    _assert_gap(ref, X, 3)
    three = gmm_scoring_topc(ubm, enroll, _ndx(fx), feats, top_c=3)
    want3 = gtn.llr(ref, fx["enroll_stat1"][order], X, off, top_c=3)[:, seg]
    errs = {"top_c = 8 vs the reference": numpy.abs(full.scoremat - fx["scoremat"]).max(),
            "top_c = 32, masked, vs the reference": numpy.abs(masked.scoremat - fx["masked_scoremat"]).max(),
            "top_c = 8 vs gmm_scoring": numpy.abs(full.scoremat - dense.scoremat).max(),
            "top_c = 3 vs the restatement": numpy.abs(three.scoremat - want3).max()}
    print({k: f"{v:.2e}" for k, v in errs.items()}, f"bound {bound:.2e}")
    assert all(v < bound for v in errs.values()), (errs, bound)
    # the caller's lists: an entry outside [0, C) is refused before anything is launched
    x = torch.as_tensor(X).to(gpu)
    lists = gtn.lists(ref, X, 3)
    for bad in (-1, 8):
        broken = lists.copy()
        broken[700, 1] = bad
        for comp in (broken, torch.as_tensor(broken).to(gpu)):
            with pytest.raises(ValueError, match="components"):
                gmm_llk_topc_device(ubm, fx["enroll_stat1"], x, off, top_c=3, components=comp)
            with pytest.raises(ValueError, match="components"):
                gmm_llr_topc_device(ubm, fx["enroll_stat1"], x, off, top_c=3, components=comp)
    got = _np(gmm_llr_topc_device(ubm, fx["enroll_stat1"][order], x, off, top_c=3, components=torch.as_tensor(lists).to(gpu)))[:, seg]
    assert numpy.array_equal(got, three.scoremat), "resident frames and the caller's lists: gmm_scoring_topc's bits"


def test_argument_errors_launch_nothing(gpu):
    import torch
    from sidekit_amd import _lib
    lib = _lib.lib()
    N, D, C, M, S, K = 70, 8, 4, 2, 1, 2
    x = torch.zeros((N, D), dtype=torch.float64, device=gpu)
    mus, ic, B = torch.zeros((M, C, D), dtype=torch.float64, device=gpu), torch.ones((C, D), dtype=torch.float64, device=gpu), torch.zeros(C, dtype=torch.float64, device=gpu)
    off = torch.tensor([0, N], dtype=torch.int32, device=gpu)
    llk = torch.full((M, S), 7.0, dtype=torch.float64, device=gpu)
    idx = torch.full((N, K), 9, dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()

    def top(K=K, dt=_lib.XT_F64, D=D):
        return lib.sc_gmm_top_components(x.data_ptr(), dt, N, D, mus.data_ptr(), ic.data_ptr(), B.data_ptr(), C, K, idx.data_ptr(), None)

    def score(K=K, M=M, max_len=N):
        return lib.sc_gmm_score_models_topc(x.data_ptr(), _lib.XT_F64, N, D, mus.data_ptr(), M, ic.data_ptr(), B.data_ptr(), C, off.data_ptr(), S, max_len, None,
                                            idx.data_ptr(), K, llk.data_ptr(), None)

    cases = {"lists K = 0": top(K=0), "lists K > C": top(K=5), "lists bf16": top(dt=_lib.XT_BF16), "lists D = 129": top(D=129),
             "score K = 0": score(K=0), "score K > C": score(K=5), "score M = 0": score(M=0), "score max_len > N": score(max_len=N + 1)}
    assert all(rc == _lib.SK_EARG for rc in cases.values()), cases
    torch.cuda.synchronize()
    assert bool((llk == 7.0).all()) and bool((idx == 9).all()), "a refused call wrote nothing"
    assert score() == _lib.SK_OK   # every index is outside [0, C): nothing is read through it, every frame is -inf
    torch.cuda.synchronize()
    assert bool((llk == -float("inf")).all()), "an index outside [0, C) contributes nothing"
    assert top() == _lib.SK_OK and score() == _lib.SK_OK
    torch.cuda.synchronize()
    assert bool((idx == torch.tensor([0, 1], dtype=torch.int32, device=gpu)).all()), "equal log posteriors: the lower indices"
    assert bool((llk == llk[0, 0]).all()) and bool(torch.isfinite(llk).all()), "the accepted call wrote both (equal) models"
