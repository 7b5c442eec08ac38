"""GMM-UBM verification on the GPU (sidekit_amd/gmm_scoring.py, csrc/gmm_score.hip) against the reference's own scores
(tests/golden/gmm_scoring.npz, written by make_gmm_scoring_golden.py from the imported reference modules) and the float64 numpy
restatement (tests/tools/gmm_scoring_numpy.py, held to 1e-12 against that fixture by tests/test_gmm_scoring_cpu.py).

TOL = 1e-9 relative max-norm, this project's bound for float64 quantities, for the log-likelihood sums and means.  A log-likelihood
ratio is a difference of two such means, so its bound is absolute: TOL x the largest |mean llk| of the case.  Every comparison prints
the error it measured.  The bitwise tests are exact: no floating-point atomics, and every sum's order depends on the segment's own
length alone.
"""
import os
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gmm_scoring_numpy as gsn  # noqa: E402
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
    m._compute_all()
    return m


def _random_case(seed, C, D, lengths, M, spread=0.3):
    """a mixture, M models around it and frames drawn near its means -> (Mixture, restatement model, models (M, C D), X, seg_off)"""
    rs = numpy.random.RandomState(seed)
    w = rs.rand(C) + 0.5
    ref = mxn.model(w / w.sum(), 2.0 * rs.randn(C, D), 1.0 / (0.5 + rs.rand(C, D)))
    models = (ref["mu"][None] + spread * rs.randn(M, C, D)).reshape(M, C * D)
    n = int(sum(lengths))
    X = ref["mu"][rs.randint(0, C, n)] + 1.1 * rs.randn(n, D)
    return _mixture(ref), ref, models, X, numpy.concatenate(([0], numpy.cumsum(lengths)))


def _np(t):
    return t if isinstance(t, numpy.ndarray) else t.cpu().numpy()


def _check_sums(name, llk, lens, ref, models, X, off):
    """llk sums and means at TOL relative max-norm, the ratios at TOL x the largest |mean llk| -> the restatement's ratios"""
    want, want_lens = gsn.llk(ref, list(models) + [ref["mu"].flatten()], X, off)
    assert list(_np(lens)) == list(want_lens)
    got = _np(llk)
    some = want_lens > 0
    mean_got, mean_want = got[:, some] / want_lens[some], want[:, some] / want_lens[some]
    errs = {f"{name} llk": mxn.rel(got, want), f"{name} mean llk": mxn.rel(mean_got, mean_want),
            f"{name} llr over the largest mean": numpy.abs((mean_got[:-1] - mean_got[-1]) - (mean_want[:-1] - mean_want[-1])).max() / numpy.abs(mean_want).max()}
    print({k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < TOL, f"{k} differs by {v:.3e} (bound {TOL})"
    assert numpy.all(got[:, ~some] == 0), "an empty segment's sum is exactly 0"


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
    assert list(n.modelset) == list(fx["score_modelset"]) and list(n.segset) == list(fx["score_segset"])
    if mask is not None:
        n.trialmask = mask.copy()
    return n


def test_fixture_scores(gpu, fx, monkeypatch):
    import torch
    from sidekit_amd.gmm_scoring import gmm_llr_device, gmm_scoring
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
    full = gmm_scoring(ubm, enroll, _ndx(fx), feats)
    assert full.validate() and list(full.modelset) == list(fx["score_modelset"]) and list(full.segset) == list(fx["score_segset"])
    assert numpy.array_equal(full.scoremask, fx["scoremask"]) and numpy.all(full.scoremat[ubm_row] == 0.0), "the UBM against itself: exactly 0"
    masked = gmm_scoring(ubm, enroll, _ndx(fx, fx["masked_scoremask"]), feats, num_thread=3)
    assert numpy.array_equal(masked.scoremask, fx["masked_scoremask"]) and numpy.all(masked.scoremat[~fx["masked_scoremask"]] == 0.0)
    assert numpy.array_equal(masked.scoremat[fx["masked_scoremask"]], full.scoremat[fx["masked_scoremask"]]), "a trial's bits do not depend on the mask"
    from sidekit_amd import gmm_scoring as module
    monkeypatch.setattr(module, "SCORING_BYTES", 1)
    assert numpy.array_equal(gmm_scoring(ubm, enroll, _ndx(fx, fx["masked_scoremask"]), feats).scoremat, masked.scoremat), "one segment per batch: the same bits"
    monkeypatch.undo()
    # resident frames, all eight segments: the empty one gives nan
    x = torch.as_tensor(X).to(gpu)
    llr = gmm_llr_device(ubm, fx["enroll_stat1"][order], x, off)
    assert llr.is_cuda and llr.shape == (5, 8) and bool(torch.isnan(llr[:, 2]).all()) and bool((llr[ubm_row, seg] == 0.0).all())
    mask8 = numpy.zeros((5, 8), dtype=bool)
    mask8[:, seg] = fx["masked_scoremask"]
    llr_m = gmm_llr_device(ubm, fx["enroll_stat1"][order], x, off, mask8)
    errs = {"gmm_scoring vs the reference": numpy.abs(full.scoremat - fx["scoremat"]).max(),
            "gmm_scoring, masked, vs the reference": numpy.abs(masked.scoremat - fx["masked_scoremat"]).max(),
            "gmm_llr_device vs the reference": numpy.abs(_np(llr)[:, seg] - fx["scoremat"]).max(),
            "gmm_llr_device, masked, vs the reference": numpy.abs(_np(llr_m)[:, seg] - fx["masked_scoremat"]).max()}
    print({k: f"{v:.2e}" for k, v in errs.items()}, f"bound {bound:.2e}")
    assert all(v < bound for v in errs.values()), (errs, bound)
    assert bool((llr_m[:, 2] == 0.0).all()) and numpy.all(_np(llr_m)[~mask8] == 0.0), "entries without a trial are exactly 0"
    # float32 frames: the float64 result of the widened frames, bit for bit
    X32 = X.astype(numpy.float32)
    a = gmm_llr_device(ubm, fx["enroll_stat1"][order], torch.as_tensor(X32).to(gpu), off, mask8)
    b = gmm_llr_device(ubm, fx["enroll_stat1"][order], torch.as_tensor(X32.astype(numpy.float64)).to(gpu), off, mask8)
    assert torch.equal(a[:, seg], b[:, seg]) and bool((a[ubm_row, seg] == 0.0).all())
    want32 = gsn.llr(ref, fx["enroll_stat1"][order], X32.astype(numpy.float64), off, mask8)[:, seg]
    err32 = numpy.abs(_np(a)[:, seg] - want32).max()
    print(f"float32 frames vs the restatement on the widened frames: {err32:.2e}")
    assert err32 < bound
    host32 = gmm_scoring(ubm, enroll, _ndx(fx, fx["masked_scoremask"]), _Features({n: X32[off[i]:off[i + 1]] for i, n in enumerate(shows)}))
    assert numpy.array_equal(host32.scoremat, _np(a)[:, seg]), "gmm_scoring keeps float32 features float32"


@pytest.mark.parametrize("C,D,lengths,M", [(130, 23, [3, 64, 0, 133], 5), (65, 128, [70], 3), (130, 23, [3, 64, 0, 133], 1)],
                         ids=["three_component_tiles", "lds_above_64k", "one_model"])
def test_more_than_one_component_tile(gpu, C, D, lengths, M):
    import torch
    from sidekit_amd.gmm_scoring import gmm_llk_device
    ubm, ref, models, X, off = _random_case(21, C, D, lengths, M)
    stacked = numpy.concatenate((models, ref["mu"].reshape(1, -1)))
    llk, lens = gmm_llk_device(ubm, stacked, torch.as_tensor(X).to(gpu), off)
    assert llk.is_cuda and llk.shape == (M + 1, len(lengths))
    _check_sums("device", llk, lens, ref, models, X, off)
    host_llk, host_lens = gmm_llk_device(ubm, stacked.reshape(M + 1, C, D), X, off)
    assert isinstance(host_llk, numpy.ndarray) and numpy.array_equal(host_llk, _np(llk)) and list(host_lens) == list(lengths)


def test_slabs(gpu):
    """700 frames: two slabs; 33 000: the slab count at its cap of 64, slabs of 576 frames"""
    import torch
    from sidekit_amd import mixture
    from sidekit_amd.gmm_scoring import gmm_llk_device
    lengths = [700, 33000]
    assert mixture._slabs(700) == 2 and mixture._slabs(33000) == mixture.MAX_SLABS == 64 and -(-33000 // mixture.SLAB_FRAMES) > 64
    ubm, ref, models, X, off = _random_case(22, 8, 8, lengths, 2)
    stacked = numpy.concatenate((models, ref["mu"].reshape(1, -1)))
    x = torch.as_tensor(X).to(gpu)
    llk, lens = gmm_llk_device(ubm, stacked, x, off)
    _check_sums("slabs", llk, lens, ref, models, X, off)
    alone, _ = gmm_llk_device(ubm, stacked, x[:700].clone())
    assert torch.equal(alone[:, 0], llk[:, 0]), "two slabs through the workspace of a call with 64: the same bits as alone"


def test_bits(gpu):
    import torch
    from sidekit_amd.gmm_scoring import gmm_llk_device
    lengths = [3, 64, 0, 133]
    ubm, ref, models, X, off = _random_case(23, 130, 23, lengths, 7)
    x = torch.as_tensor(X).to(gpu)
    llk, _ = gmm_llk_device(ubm, models, x, off)
    assert bool(torch.isfinite(llk).all()) and bool((llk[:, 2] == 0).all()) and bool((llk[:, [0, 1, 3]] != 0).all())
    for k in range(7):
        assert torch.equal(gmm_llk_device(ubm, models[k:k + 1], x, off)[0][0], llk[k]), f"model {k} alone"
    perm = numpy.array([4, 0, 6, 2, 5, 1, 3])
    assert torch.equal(gmm_llk_device(ubm, models[perm], x, off)[0], llk[torch.as_tensor(perm).to(gpu)]), "any position in the stack"
    for k in (0, 3, 6):
        mask = numpy.zeros((7, 4), dtype=bool)
        mask[k] = True
        alone = gmm_llk_device(ubm, models, x, off, mask)[0]
        assert torch.equal(alone[k], llk[k]) and bool((alone[numpy.arange(7) != k] == 0).all()), f"the others masked out around model {k}"
    mask = numpy.random.RandomState(5).rand(7, 4) < 0.5
    part = gmm_llk_device(ubm, models, x, off, mask)[0]
    d_mask = torch.as_tensor(mask).to(gpu)
    assert torch.equal(part[d_mask], llk[d_mask]) and bool((part[~d_mask] == 0).all()), "a scattered mask"
    assert torch.equal(gmm_llk_device(ubm, models, x, off, None, max_workspace_bytes=1)[0], llk), "chunks of one model"
    # a segment alone, among others, and elsewhere in X (behind a long one that is cut into slabs)
    seg3 = x[off[3]:off[4]].clone()
    assert torch.equal(gmm_llk_device(ubm, models, seg3)[0][:, 0], llk[:, 3]), "the 133-frame segment alone"
    rs = numpy.random.RandomState(6)
    long = torch.as_tensor(ref["mu"][rs.randint(0, 130, 700)] + rs.randn(700, 23)).to(gpu)
    moved = gmm_llk_device(ubm, models, torch.cat((long, seg3, x[off[1]:off[2]])), [0, 700, 833, 897])[0]
    assert torch.equal(moved[:, 1], llk[:, 3]) and torch.equal(moved[:, 2], llk[:, 1]), "behind a 700-frame segment"
    assert torch.equal(gmm_llk_device(ubm, models, x, off)[0], llk), "the same call again"


def test_range(gpu):
    """A model that fits the frames far better than the UBM does, and one far worse: per frame lp_m - lse_ubm is about + 900 and - 2 700,
    so exp(lp_m - lse_ubm) would overflow; the running maximum per model keeps every exponent at or below 0."""
    import torch
    from sidekit_amd.gmm_scoring import gmm_llk_device, gmm_llr_device
    rs = numpy.random.RandomState(24)
    C, D, lengths = 4, 8, [40, 1, 90]
    ref = mxn.model(numpy.full(C, 0.25), 15.0 + 0.01 * rs.randn(C, D), numpy.ones((C, D)))
    models = numpy.stack((0.01 * rs.randn(C, D), 30.0 + 0.01 * rs.randn(C, D))).reshape(2, C * D)
    X = 0.1 * rs.randn(sum(lengths), D)
    off = numpy.concatenate(([0], numpy.cumsum(lengths)))
    lo, hi = gsn.margin_range(ref, models, X)
    with numpy.errstate(over="ignore"):
        assert hi > 850 and lo < -2600 and not numpy.isfinite(numpy.exp(hi)), (lo, hi)
    want = gsn.llr(ref, models, X, off)
    assert numpy.isfinite(want).all() and want[0].min() > 850 and want[1].max() < -2600
    ubm = _mixture(ref)
    x = torch.as_tensor(X).to(gpu)
    llk, lens = gmm_llk_device(ubm, numpy.concatenate((models, ref["mu"].reshape(1, -1))), x, off)
    assert bool(torch.isfinite(llk).all())
    _check_sums("range", llk, lens, ref, models, X, off)
    llr = _np(gmm_llr_device(ubm, models, x, off))
    bound = TOL * numpy.abs(gsn.llk(ref, list(models) + [ref["mu"].flatten()], X, off)[0] / numpy.diff(off)).max()
    err = numpy.abs(llr - want).max()
    print(f"llr in [{llr.min():.1f}, {llr.max():.1f}], error {err:.2e}, bound {bound:.2e}")
    assert numpy.isfinite(llr).all() and err < bound


def test_device_route_equals_host_route(gpu, fx):
    """statistics -> adapted models -> scores without leaving the device, against StatServer.adapt_mean_map_multisession and gmm_scoring"""
    import torch
    from sidekit_amd.gmm_scoring import gmm_llr_device, gmm_scoring, map_adapt_device
    from sidekit_amd.mixture import gmm_stats_device
    from sidekit_amd.statserver import StatServer
    ref = mxn.model(*(fx[f"mix_split4_{k}"] for k in KEYS))
    ubm = _mixture(ref)
    X, off = fx["mix_X"], fx["mix_seg_off"]
    x = torch.as_tensor(X).to(gpu)
    stat0, stat1, _, _ = gmm_stats_device(ubm, x, off, order=1)
    models = map_adapt_device(stat0, stat1, ubm, 16, fx["modelset"])
    single = map_adapt_device(stat0, stat1, ubm, 0.5)
    llr = gmm_llr_device(ubm, models, x, off)
    assert stat0.is_cuda and stat1.is_cuda and models.is_cuda and single.is_cuda and llr.is_cuda and models.shape == (4, 8, 23) and single.shape == (8, 8, 23)
    server = StatServer()
    server.modelset, server.segset = fx["modelset"].astype("|O"), fx["segset"].astype("|O")
    server.start, server.stop = numpy.empty(8, dtype="|O"), numpy.empty(8, dtype="|O")
    server.accumulate_stat_device(ubm, x, off)
    enroll = server.adapt_mean_map_multisession(ubm, 16)
    shows = [f"show{i}" for i in range(8)]
    scores = gmm_scoring(ubm, enroll, _ndx_of(enroll.modelset, fx["score_segset"]), _Features({n: X[off[i]:off[i + 1]] for i, n in enumerate(shows)}))
    seg = [shows.index(s) for s in scores.segset]
    sums, lens = gsn.llk(ref, fx["multi_stat1"], X, off)
    bound = TOL * numpy.abs(sums[:, seg] / lens[seg]).max()
    errs = {"adapted means, device vs host": mxn.rel(_np(models).reshape(4, -1), enroll.stat1),
            "adapted means vs the reference": mxn.rel(_np(models).reshape(4, -1), fx["multi_stat1"]),
            "single-session means vs the reference": mxn.rel(_np(single).reshape(8, -1), fx["map_r0p5_plain"])}
    err = numpy.abs(_np(llr)[:, seg] - scores.scoremat).max()
    print({k: f"{v:.2e}" for k, v in errs.items()}, f"llr device vs host {err:.2e}, bound {bound:.2e}")
    assert all(v < TOL for v in errs.values()) and err < bound
    assert numpy.abs(scores.scoremat - fx["scoremat"][:4]).max() < bound, "and both are the reference's scores"


def _ndx_of(models, segs):
    from sidekit_amd.bosaris import Ndx
    return Ndx(models=numpy.repeat(numpy.asarray(models, dtype="|O"), len(segs)), testsegs=numpy.tile(numpy.asarray(segs).astype("|O"), len(models)))


def test_argument_errors_launch_nothing(gpu):
    import torch
    from sidekit_amd import _lib
    lib = _lib.lib()
    N, D, C, M, S = 70, 8, 4, 2, 1
    x = torch.zeros((N, D), dtype=torch.float64, device=gpu)
    mus, ic, B = torch.zeros((M, C, D), dtype=torch.float64, device=gpu), torch.ones((C, D), dtype=torch.float64, device=gpu), torch.zeros(C, dtype=torch.float64, device=gpu)
    off = torch.tensor([0, N], dtype=torch.int32, device=gpu)
    llk = torch.full((M, S), 7.0, dtype=torch.float64, device=gpu)
    torch.cuda.synchronize()

    def score(X=x.data_ptr(), dt=_lib.XT_F64, N=N, D=D, mus=mus.data_ptr(), M=M, max_len=N):
        return lib.sc_gmm_score_models(X, dt, N, D, mus, M, ic.data_ptr(), B.data_ptr(), C, off.data_ptr(), S, max_len, None, llk.data_ptr(), None)

    cases = {"M = 0": score(M=0), "D = 129": score(D=129), "mus null": score(mus=None), "bf16": score(dt=_lib.XT_BF16), "i64": score(dt=_lib.XT_I64),
             "max_len > N": score(max_len=N + 1)}
    assert all(rc == _lib.SK_EARG for rc in cases.values()), cases
    torch.cuda.synchronize()
    assert bool((llk == 7.0).all()), "a refused call wrote nothing"
    assert score() == _lib.SK_OK
    torch.cuda.synchronize()
    assert bool((llk == llk[0, 0]).all()) and bool(torch.isfinite(llk).all()) and float(llk[0, 0]) != 7.0, "the accepted call wrote both (equal) models"
