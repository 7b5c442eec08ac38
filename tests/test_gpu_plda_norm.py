"""Cohort normalisation of PLDA log-likelihood ratios on the device (sc_plda_cohort_moments, sc_topk_stats_f64, sc_norm_apply_f64,
sc_plda_hist_norm and the Python layer over them), float64 throughout.

Small, odd shapes: tests/golden/plda_train.npz cut to D = 45 (an odd k, a partial k-tile, the scalar-load path), enrolment rows [57, 187),
test rows [0, 257), cohort rows [257, 376) (M = 119).  On the host: cohort stds >= 2.23 on both sides, top-7 unbiased stds >= 0.247, the
smallest gap between a row's 7th and 8th best cohort score 8.7e-4 (no ties), cohort scores in [-26.8, 8.8].

Large corpus: the one of tests/test_gpu_plda_hist.py (RandomState(11), 40 speakers, N = 1000, D = 256, noise 1.7, unit rows, as float64) with
the cohort of tests/test_gpu_hist_norm.py (RandomState(12), 60 speakers, M = 200) and the reference-trained (mu, F, Sigma) of
tests/golden/config5.npz, scored against itself.  Host facts (float64, 8192 bins over the widened range): exact EER z 8.2935 %, t 8.2935 %,
s 8.1103 %, adaptive s (top-50) 8.1404 %; the binned EERs are within 5.5e-5 of them; no score in an end bin; cohort stds >= 4.15 (top-50: 1.46).

The statistics are held to the host's two-pass float64 statistics of the device's own materialised cohort matrix at 1e-9 of the largest
cohort score (the bound tests/test_gpu_plda_hist.py puts on a PLDA score: mean and std are 1-Lipschitz in a per-score perturbation, and
the one-pass cancellation adds about eps * mean^2 / var <= 4 eps here)."""
import ctypes
import json
import os
import sys

import numpy
import pytest
import torch

from oracle import scoring as osc
from sidekit_amd import _lib, iv_scoring
from sidekit_amd import score_normalization as sn
from sidekit_amd.bosaris import eer_from_histograms

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import second_trips as st  # noqa: E402

pytestmark = pytest.mark.gpu
NB = iv_scoring.HIST_BINS
KINDS = ("z", "t", "s", "as")


def _range(z):
    """min / max widened by a quarter of the range, moved outward to multiples of 1/8."""
    zmin, zmax = float(z.min()), float(z.max())
    pad = 0.25 * (zmax - zmin)
    return float(numpy.floor((zmin - pad) * 8) / 8), float(numpy.ceil((zmax + pad) * 8) / 8)


def _bins(z, lo, hi, nb=NB):
    """The bin of every entry of a float64 matrix, with the kernel's float64 operations (tests/test_gpu_plda_hist.py)."""
    return numpy.clip(numpy.floor((z - lo) * (nb / (hi - lo))), 0, nb - 1).astype(numpy.int64)


def _count(bins, sel, nb=NB):
    return numpy.bincount(bins[sel], minlength=nb).astype(numpy.uint64)


def _same(got, bins, tar, keep, nb=NB):
    ht, hn = got
    assert ht.dtype == hn.dtype == numpy.uint64 and ht.shape == hn.shape == (nb,)
    assert int(ht.sum() + hn.sum()) == int(keep.sum())
    assert numpy.array_equal(ht, _count(bins, tar & keep, nb)) and numpy.array_equal(hn, _count(bins, ~tar & keep, nb))


def _topk_host(s, k):
    top = numpy.sort(s, axis=1)[:, -k:]
    return top.mean(axis=1), top.std(axis=1, ddof=1)


def _host_norm(kind, s, ec, ct, k):
    """The normalised scores in float64 numpy: s (Ne, Nt), ec = s(e, cohort) (Ne, M), ct = s(cohort, t) (M, Nt)."""
    if kind == "as":
        (me, se), (mt, st) = _topk_host(ec, k), _topk_host(ct.T, k)
    else:
        (me, se), (mt, st) = (ec.mean(1), ec.std(1)), (ct.mean(0), ct.std(0))
    if kind == "z":
        return (s - me[:, None]) / se[:, None]
    if kind == "t":
        return (s - mt[None, :]) / st[None, :]
    return 0.5 * ((s - me[:, None]) / se[:, None]) + 0.5 * ((s - mt[None, :]) / st[None, :])


def _device_norm(kind, mat, e, t, c, model, k):
    """The materialised path: plda_matrix_device's matrix (a copy) through plda_{z,t,s}norm_device."""
    z = mat.clone()
    if kind == "z":
        return sn.plda_znorm_device(z, e, c, *model)
    if kind == "t":
        return sn.plda_tnorm_device(z, t, c, *model)
    return sn.plda_snorm_device(z, e, t, c, *model, topk=k if kind == "as" else None)


def _hist_kw(kind, k):
    return dict(kind="s" if kind == "as" else kind, topk=k if kind == "as" else None)


# ---- small, odd shapes --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def odd(gpu, golden_dir):
    z = numpy.load(os.path.join(golden_dir, "plda_train.npz"))
    Xh = numpy.ascontiguousarray(z["X"][:, :45])
    X = torch.as_tensor(Xh).to(gpu)
    model = (z["mean_0"][:45], z["F_0"][:45], z["Sigma_0"][:45, :45])
    lab = numpy.unique(z["modelset"], return_inverse=True)[1].astype(numpy.int32)
    Phi, Psi, cst = iv_scoring.plda_parameters(*model)
    mu_d = torch.as_tensor(model[0]).to(gpu)
    Xc = (X - mu_d).contiguous()
    e, t, c = X[57:187], X[:257], X[257:]
    mat = iv_scoring.plda_matrix_device(Xc[57:187], Xc[:257], Phi, Psi, cst)
    ec = iv_scoring.plda_matrix_device(Xc[57:187], Xc[257:], Phi, Psi, cst)          # s(e_i, c_j): 130 x 119
    ct = iv_scoring.plda_matrix_device(Xc[257:], Xc[:257], Phi, Psi, cst)            # s(c_j, t_i): 119 x 257
    keep = numpy.ones((130, 257), dtype=bool)
    keep[numpy.arange(130), numpy.arange(130) + 57] = False
    return {"Xh": Xh, "X": X, "Xc": Xc, "e": e, "t": t, "c": c, "le": lab[57:187], "lt": lab[:257], "model": model, "params": (Phi, Psi, cst),
            "mat": mat, "ec": ec.cpu().numpy(), "ct": ct.cpu().numpy(), "ec_d": ec, "tar": lab[57:187, None] == lab[None, :257],
            "all": numpy.ones((130, 257), dtype=bool), "keep": keep}


def test_moments_on_both_sides(odd):
    mu, F, Sigma = odd["model"]
    ref_ec = osc.fast_plda_scores(odd["Xh"][57:187], odd["Xh"][257:], mu, F, Sigma)
    ref_ct = osc.fast_plda_scores(odd["Xh"][257:], odd["Xh"][:257], mu, F, Sigma)
    for side, x, own, ref in (("enrol", odd["e"], odd["ec"], ref_ec), ("test", odd["t"], odd["ct"].T, ref_ct.T)):
        mean, std = sn.plda_cohort_stats_device(x, odd["c"], *odd["model"], side=side)
        assert mean.dtype == std.dtype == torch.float64 and mean.is_cuda and mean.shape == std.shape == (x.shape[0],)
        mean, std = mean.cpu().numpy(), std.cpu().numpy()
        assert float(own.std(1).min()) >= 2.23
        for name, s in (("the device's own matrix", own), ("the oracle", ref)):
            bound = 1e-9 * float(numpy.abs(s).max())
            em, es = float(numpy.abs(mean - s.mean(1)).max()), float(numpy.abs(std - s.std(1)).max())
            print(f"{side} side against {name}: mean off by {em:.2e}, std by {es:.2e} (bound {bound:.2e})")
            assert em <= bound and es <= bound


def test_self_offset(odd):
    Phi, Psi, cst = odd["params"]
    full = iv_scoring.plda_matrix_device(odd["Xc"][57:187], odd["Xc"], Phi, Psi, cst).cpu().numpy()      # 130 x 376: three cohort tiles
    keep = numpy.ones(full.shape, dtype=bool)
    keep[numpy.arange(130), numpy.arange(130) + 57] = False
    rows = full[keep].reshape(130, 375)
    assert float(rows.std(1).min()) >= 2.33
    mean, std = (v.cpu().numpy() for v in sn.plda_cohort_stats_device(odd["e"], odd["X"], *odd["model"], self_offset=57))
    bound = 1e-9 * float(numpy.abs(full).max())
    assert float(numpy.abs(mean - rows.mean(1)).max()) <= bound and float(numpy.abs(std - rows.std(1)).max()) <= bound
    mean_all, std_all = (v.cpu().numpy() for v in sn.plda_cohort_stats_device(odd["e"], odd["X"], *odd["model"], self_offset=None))
    assert float(numpy.abs(mean_all - full.mean(1)).max()) <= bound and float(numpy.abs(std_all - full.std(1)).max()) <= bound
    assert not numpy.array_equal(mean, mean_all) and not numpy.array_equal(std, std_all)


def test_statistics_do_not_depend_on_the_launch(gpu, odd):
    many = sn.plda_cohort_stats_device(odd["e"], odd["c"], *odd["model"])
    few = sn.plda_cohort_stats_device(odd["X"][57:60], odd["c"], *odd["model"])
    assert torch.equal(few[0], many[0][:3]) and torch.equal(few[1], many[1][:3])
    # another stream, after a larger call grew that stream's workspace
    lib = _lib.lib()
    Phi, Psi, cst = odd["params"]
    phi, psi = torch.as_tensor(Phi).to(gpu).contiguous(), torch.as_tensor(Psi).to(gpu).contiguous()
    Xc, C = odd["Xc"], odd["Xc"][257:].contiguous()

    def moments(x, stream):
        mean, std = torch.full((x.shape[0],), -7.0, dtype=torch.float64, device=gpu), torch.full((x.shape[0],), -7.0, dtype=torch.float64, device=gpu)
        rc = lib.sc_plda_cohort_moments(x.data_ptr(), x.shape[0], C.data_ptr(), 119, 45, phi.data_ptr(), psi.data_ptr(), float(cst), 1.0, -1,
                                        mean.data_ptr(), std.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
        assert rc == _lib.SK_OK, _lib.last_error()
        return mean, std

    torch.cuda.synchronize(gpu)
    s2 = torch.cuda.Stream(gpu)
    with torch.cuda.stream(s2):
        small = moments(Xc[57:60].contiguous(), s2)
        big = moments(Xc, s2)                                  # 376 rows: the stream's workspace grows
        again = moments(Xc[57:60].contiguous(), s2)
    torch.cuda.synchronize(gpu)
    for got in (small, again):
        assert torch.equal(got[0], many[0][:3]) and torch.equal(got[1], many[1][:3])
    assert torch.equal(big[0][57:187], many[0]) and torch.equal(big[1][57:187], many[1])
    # N == 0 does nothing; a row that keeps no pair is refused before anything is enqueued
    cur = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    assert lib.sc_plda_cohort_moments(None, 0, C.data_ptr(), 119, 45, phi.data_ptr(), psi.data_ptr(), float(cst), 1.0, -1, None, None, cur) == _lib.SK_OK
    keepsake = torch.full((1,), -7.0, dtype=torch.float64, device=gpu)
    assert lib.sc_plda_cohort_moments(Xc.data_ptr(), 1, C.data_ptr(), 1, 45, phi.data_ptr(), psi.data_ptr(), float(cst), 1.0, 0, keepsake.data_ptr(),
                                      keepsake.data_ptr(), cur) == _lib.SK_EARG
    torch.cuda.synchronize(gpu)
    assert float(keepsake[0]) == -7.0


_LONG = {}


def _long_cohort(gpu, golden_dir, d):
    """33 000 rows drawn from the fixture's model cut to ``d`` dimensions (tests/tools/second_trips.py), raw and centred, on the device."""
    if d not in _LONG:
        model = st.plda_model(golden_dir, d)
        C = torch.as_tensor(st.plda_corpus(model, st.COHORT_M, seed=25 + d)[0]).to(gpu)
        Phi, Psi, cst = iv_scoring.plda_parameters(*model)
        _LONG[d] = {"model": model, "C": C, "Cc": (C - torch.as_tensor(model[0]).to(gpu)).contiguous(), "params": (Phi, Psi, cst),
                    "phi": torch.as_tensor(Phi).to(gpu).contiguous(), "psi": torch.as_tensor(Psi).to(gpu).contiguous()}
    return _LONG[d]


def _moments_direct(gpu, k, x, c, self_offset):
    """sc_plda_cohort_moments itself on centred rows; the outputs start at -7."""
    mean = torch.full((x.shape[0],), -7.0, dtype=torch.float64, device=gpu)
    std = torch.full((x.shape[0],), -7.0, dtype=torch.float64, device=gpu)
    rc = _lib.lib().sc_plda_cohort_moments(x.data_ptr(), x.shape[0], c.data_ptr(), c.shape[0], x.shape[1], k["phi"].data_ptr(), k["psi"].data_ptr(),
                                           float(k["params"][2]), 1.0, self_offset, mean.data_ptr(), std.data_ptr(),
                                           ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
    assert rc == _lib.SK_OK, _lib.last_error()
    return mean, std


def _host_moments_of_own_matrix(k, x, c, drop):
    """The module's yardstick: two-pass float64 statistics of the device's own materialised scores, and 1e-9 of the largest of them."""
    s = iv_scoring.plda_matrix_device(x, c, *k["params"]).cpu().numpy()
    return st.kept_moments(s, drop) + (1e-9 * float(numpy.abs(s).max()),)


@pytest.mark.parametrize("d", [4, 5])
def test_moments_past_the_row_block(gpu, golden_dir, d, monkeypatch):
    """sc_plda_cohort_moments launches ROWS = 32 768 rows of X at a time and gives a slab more than two cohort tiles once M > 16 384
    (``tiles_m > 128``).  X = C[r : r + N] with N = 32 768 + 130, M = 33 000 and self_offset = r crosses both in one call: the second
    launch reads ``w.epsi + r0 * D`` and ``w.qe + r0`` (with ``x_stride = N``), drops the pair ``i + self_offset + r0``, writes
    ``d_mean + r0`` and reuses the first launch's partials; a slab holds 5 tiles, 52 partials are joined.  D = 4 (16-byte loads) and D = 5
    (the scalar-load path).  (a) Rows [32 766, N) against the host's statistics of the device's own matrix of those rows at this module's
    1e-9 of the largest score.  (b) The same rows, and four ranges of the first block, against calls of their own on those rows alone:
    bit for bit (a row's additions do not depend on N or on the launch)."""
    k = _long_cohort(gpu, golden_dir, d)
    M, r, N = st.COHORT_M, st.COHORT_R, st.ROWS + st.COHORT_EXTRA
    tiles_m, per, slabs = st.slab_rule(M)
    assert N > st.ROWS and M > st.SLAB_TILES * st.COHORT_TILE and tiles_m > st.SLAB_TILES and per > st.MIN_PER and r + N <= M
    c = k["Cc"]
    x = c[r:r + N].contiguous()
    mean, std = _moments_direct(gpu, k, x, c, r)
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(std).all()) and float(std.min()) > 0.0
    reached, lib = [], _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: _Spy(lib, reached))
    m2, s2 = sn.plda_cohort_stats_device(k["C"][r:r + N], k["C"], *k["model"], self_offset=r)   # the Python entry: ONE call carries the whole N
    monkeypatch.undo()
    assert reached.count("sc_plda_cohort_moments") == 1 and m2.shape == (N,) and torch.equal(m2, mean) and torch.equal(s2, std)
    a = st.ROWS - 2
    want_mean, want_std, bound = _host_moments_of_own_matrix(k, x[a:].contiguous(), c, numpy.arange(a, N) + r)
    em, es = float(numpy.abs(mean[a:].cpu().numpy() - want_mean).max()), float(numpy.abs(std[a:].cpu().numpy() - want_std).max())
    print(f"D = {d}: mean off by {em:.2e}, std by {es:.2e} (bound {bound:.2e})")
    assert em <= bound and es <= bound
    for a0, a1 in st.first_block_samples() + [(st.ROWS - 128, N)]:
        part = _moments_direct(gpu, k, x[a0:a1].contiguous(), c, r + a0)
        assert torch.equal(part[0], mean[a0:a1]) and torch.equal(part[1], std[a0:a1]), (a0, a1)


@pytest.mark.parametrize("M", st.SLAB_M)
def test_moments_at_and_past_the_slab_limit(gpu, golden_dir, M):
    """M = 16 384: the last cohort whose slabs hold two tiles (64 slabs of 2); M = 16 385 + 100: 129 tiles, 3 to a slab, 43 partials.
    N = 130 rows, X = C[100 : 230] with its self-pairs dropped, D = 6: the module's bound, and the bits of a call on the last 53 rows."""
    k = _long_cohort(gpu, golden_dir, 6)
    tiles_m, per, slabs = st.slab_rule(M)
    assert (tiles_m, per, slabs) == ((128, 2, 64) if M == st.SLAB_TILES * st.COHORT_TILE else (129, 3, 43))
    r, n = st.COHORT_R, st.COHORT_EXTRA
    c = k["Cc"][:M].contiguous()
    x = c[r:r + n].contiguous()
    mean, std = _moments_direct(gpu, k, x, c, r)
    want_mean, want_std, bound = _host_moments_of_own_matrix(k, x, c, numpy.arange(n) + r)
    assert float(numpy.abs(mean.cpu().numpy() - want_mean).max()) <= bound and float(numpy.abs(std.cpu().numpy() - want_std).max()) <= bound
    part = _moments_direct(gpu, k, x[77:].contiguous(), c, r + 77)
    assert torch.equal(part[0], mean[77:]) and torch.equal(part[1], std[77:])


def test_scaling_factor_and_channel_subspace(gpu, golden_dir):
    """The model arguments of plda_histograms: a scaling factor, and with G both sides projected by B (the route of full_PLDA_scoring)."""
    fx = numpy.load(os.path.join(golden_dir, "scoring.npz"))
    mu, F, G, Sigma, E, C = (fx[k].astype(numpy.float64) for k in ("mu", "F", "G", "Sigma", "E", "T"))
    for g, scaling in ((None, 0.7), (G, 0.5)):
        if g is None:
            B, (Phi, Psi, cst) = None, iv_scoring.plda_parameters(mu, F, Sigma, scaling)
        else:
            B, Phi, Psi, cst = iv_scoring.full_plda_parameters(F, g, Sigma, scaling)
        proj = lambda x: (x - mu) if B is None else (x - mu) @ B.T
        for side, own in (("enrol", iv_scoring.plda_matrix_device(proj(E), proj(C), Phi, Psi, cst, scaling, gpu).cpu().numpy()),
                          ("test", iv_scoring.plda_matrix_device(proj(C), proj(E), Phi, Psi, cst, scaling, gpu).cpu().numpy().T)):
            mean, std = (v.cpu().numpy() for v in sn.plda_cohort_stats_device(torch.as_tensor(E).to(gpu), C, mu, F, Sigma, g, scaling, side=side))
            bound = 1e-9 * float(numpy.abs(own).max())
            assert own.shape == (32, 40) and float(numpy.abs(mean - own.mean(1)).max()) <= bound and float(numpy.abs(std - own.std(1)).max()) <= bound


def _topk_device(gpu, scores, k):
    lib = _lib.lib()
    scores = scores.contiguous()
    mean = torch.empty(scores.shape[0], dtype=torch.float64, device=gpu)
    std = torch.empty_like(mean)
    rc = lib.sc_topk_stats_f64(scores.data_ptr(), scores.shape[0], scores.shape[1], k, mean.data_ptr(), std.data_ptr(),
                               ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
    return rc, mean.cpu().numpy(), std.cpu().numpy()


def test_topk_stats_f64(gpu, odd):
    ec = odd["ec"]
    srt = numpy.sort(ec, axis=1)
    assert float((srt[:, -7] - srt[:, -8]).min()) >= 8.7e-4 and float(srt[:, -7:].std(axis=1, ddof=1).min()) >= 0.247
    for k in (7, 119):
        rc, mean, std = _topk_device(gpu, odd["ec_d"], k)
        assert rc == _lib.SK_OK, _lib.last_error()
        wm, ws = _topk_host(ec, k)
        rel = max(float(numpy.abs(mean / wm - 1).max()), float(numpy.abs(std / ws - 1).max()))
        print(f"k = {k}: largest relative difference {rel:.2e}")
        assert rel <= 1e-9
    # an exact tie at the threshold: column 118 repeats every row's 7th best score, so two copies straddle the cut
    tied = ec.copy()
    tied[:, 118] = srt[:, -7]
    rc, mean, std = _topk_device(gpu, torch.as_tensor(tied).to(gpu), 7)
    wm, ws = _topk_host(tied, 7)
    assert rc == _lib.SK_OK and float(numpy.abs(mean / wm - 1).max()) <= 1e-9 and float(numpy.abs(std / ws - 1).max()) <= 1e-9
    assert int((numpy.sort(tied, axis=1)[:, -7] == numpy.sort(tied, axis=1)[:, -8]).sum()) >= 100   # the tie does sit on the threshold
    for k in (1, 120):
        assert _topk_device(gpu, odd["ec_d"], k)[0] == _lib.SK_EARG
    # the Python route: row blocks of sc_plda_fast that fit the workspace, then the same kernel
    wm, ws = _topk_host(ec, 7)
    for budget in (1 << 30, 8 * 119 * 50):
        mean, std = sn.plda_cohort_stats_device(odd["e"], odd["c"], *odd["model"], topk=7, max_workspace_bytes=budget)
        assert float(numpy.abs(mean.cpu().numpy() / wm - 1).max()) <= 1e-9 and float(numpy.abs(std.cpu().numpy() / ws - 1).max()) <= 1e-9


def test_norm_apply_f64_is_the_numpy_expression(gpu, odd):
    lib = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    me, se = sn.plda_cohort_stats_device(odd["e"], odd["c"], *odd["model"], side="enrol")
    mt, sd = sn.plda_cohort_stats_device(odd["t"], odd["c"], *odd["model"], side="test")
    v = odd["mat"].cpu().numpy()
    a, b, c, d = (x.cpu().numpy() for x in (me, se, mt, sd))
    want = {"z": (v - a[:, None]) / b[:, None], "t": (v - c[None, :]) / d[None, :],
            "s": 0.5 * ((v - a[:, None]) / b[:, None]) + 0.5 * ((v - c[None, :]) / d[None, :])}
    ptr = lambda x: None if x is None else x.data_ptr()
    for kind, (e_pair, t_pair) in (("z", ((me, se), (None, None))), ("t", ((None, None), (mt, sd))), ("s", ((me, se), (mt, sd)))):
        z = odd["mat"].clone()
        assert lib.sc_norm_apply_f64(z.data_ptr(), 130, 257, ptr(e_pair[0]), ptr(e_pair[1]), ptr(t_pair[0]), ptr(t_pair[1]), st) == _lib.SK_OK
        assert numpy.array_equal(z.cpu().numpy(), want[kind]), kind
        assert torch.equal(_device_norm(kind, odd["mat"], odd["e"], odd["t"], odd["c"], odd["model"], None), z), kind
    # a zero std gives what IEEE division gives: +-inf, and NaN where the score equals the mean
    se0, me0 = se.clone(), me.clone()
    se0[3] = 0.0
    me0[3] = odd["mat"][3, 5]
    z = odd["mat"].clone()
    assert lib.sc_norm_apply_f64(z.data_ptr(), 130, 257, me0.data_ptr(), se0.data_ptr(), None, None, st) == _lib.SK_OK
    with numpy.errstate(divide="ignore", invalid="ignore"):
        w = (v - me0.cpu().numpy()[:, None]) / se0.cpu().numpy()[:, None]
    got = z.cpu().numpy()
    assert numpy.array_equal(got, w, equal_nan=True) and numpy.isnan(got[3, 5]) and numpy.isinf(got[3]).sum() == 256
    assert lib.sc_norm_apply_f64(z.data_ptr(), 130, 257, me.data_ptr(), None, None, None, st) == _lib.SK_EARG
    assert lib.sc_norm_apply_f64(z.data_ptr(), 130, 257, None, None, None, None, st) == _lib.SK_EARG


@pytest.mark.parametrize("kind", KINDS)
def test_odd_counts_are_those_of_the_materialised_path(odd, kind):
    e, t, c, model = odd["e"], odd["t"], odd["c"], odd["model"]
    z = _device_norm(kind, odd["mat"], e, t, c, model, 7).cpu().numpy()
    lo, hi = _range(z)
    bins = _bins(z, lo, hi)
    kw = _hist_kw(kind, 7)
    got = sn.plda_normalised_histograms(e, t, odd["le"], odd["lt"], c, *model, self_offset=None, lo=lo, hi=hi, **kw)
    _same(got, bins, odd["tar"], odd["all"])
    assert int(got[0].sum() + got[1].sum()) == 130 * 257
    got = sn.plda_normalised_histograms(e, t, odd["le"], odd["lt"], c, *model, self_offset=57, lo=lo, hi=hi, **kw)
    _same(got, bins, odd["tar"], odd["keep"])
    assert int(got[0].sum() + got[1].sum()) == 130 * 257 - 130
    if kind == "s":                                                                     # two passes of finer bins
        ft, fn = sn.plda_normalised_histograms(e, t, odd["le"], odd["lt"], c, *model, lo=lo, hi=hi, bins=2 * 8190, **kw)
        assert ft.shape == fn.shape == (16380,) and int(ft.sum() + fn.sum()) == 130 * 257
        coarse = _bins(z, lo, hi, 8190)
        assert numpy.array_equal(ft.reshape(8190, 2).sum(axis=1), _count(coarse, odd["tar"], 8190))
        assert numpy.array_equal(fn.reshape(8190, 2).sum(axis=1), _count(coarse, ~odd["tar"], 8190))
        # both pairs None: plda_histograms itself
        raw = odd["mat"].cpu().numpy()
        rlo, rhi = _range(raw)
        _same(iv_scoring.plda_norm_histograms(e, t, odd["le"], odd["lt"], *model, lo=rlo, hi=rhi), _bins(raw, rlo, rhi), odd["tar"], odd["all"])


@pytest.fixture(scope="module")
def walk(gpu, golden_dir):
    """A set whose 128 x 128 tiles outnumber the compute units (tests/tools/second_trips.py: D = 10, the fixture's model cut to 10
    dimensions, 40 speakers), a cohort of 300 from the same model, and the device's own raw matrix."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    n, t = st.hist_side(cus, st.PT)
    model = st.plda_model(golden_dir, 10)
    x, lab = st.plda_corpus(model, n)
    X, C = torch.as_tensor(x).to(gpu), torch.as_tensor(st.plda_corpus(model, 300, seed=27, n_spk=60)[0]).to(gpu)
    Xc = (X - torch.as_tensor(model[0]).to(gpu)).contiguous()
    mat = iv_scoring.plda_matrix_device(Xc, Xc, *iv_scoring.plda_parameters(*model))
    return {"cus": cus, "n": n, "t": t, "X": X, "C": C, "lab": lab, "model": model, "mat": mat, "off": ~torch.eye(n, dtype=torch.bool, device=gpu)}


@pytest.mark.parametrize("kind", KINDS)
def test_counts_when_the_tiles_outnumber_the_compute_units(walk, kind):
    """plda_hist_kernel<HN_ENROL | HN_TEST | HN_BOTH> walks ``tile += gridDim.x`` with one workgroup per compute unit; past CU-count
    tiles a workgroup takes a second one and rewrites ``term`` and ``stat`` for it behind dgemm_tile's barriers.  N = (t - 1) 128 + 3
    with t x t > CUs (2051 at 256 CUs: 289 tiles), both edges ragged, D = 10, the set against itself, every kind: the counts are those of
    the materialised path (plda_matrix_device, plda_{z,t,s}norm_device, then ``_bins`` -- evaluated on the device, every 97th row also
    by ``_bins`` itself)."""
    X, C, lab, model, n, t = walk["X"], walk["C"], walk["lab"], walk["model"], walk["n"], walk["t"]
    assert ((n + st.PT - 1) // st.PT) ** 2 == t * t > walk["cus"]
    z = _device_norm(kind, walk["mat"], X, X, C, model, K)
    assert bool(torch.isfinite(z).all())
    lo, hi = _range(z[walk["off"]])
    want_t, want_n, bins = st.device_counts(z, lo, hi, NB, lab, lab, 0)
    rows = slice(None, None, 97)
    assert numpy.array_equal(bins[rows].cpu().numpy(), _bins(z[rows].cpu().numpy(), lo, hi))
    ht, hn = sn.plda_normalised_histograms(X, X, lab, lab, C, *model, self_offset=0, lo=lo, hi=hi, **_hist_kw(kind, K))
    assert ht.dtype == hn.dtype == numpy.uint64 and int(ht.sum() + hn.sum()) == n * n - n
    assert numpy.array_equal(ht, want_t) and numpy.array_equal(hn, want_n)
    assert int(ht[0] + hn[0] + ht[-1] + hn[-1]) == 0 and int((ht + hn > 0).sum()) > 1000   # every score inside the range, spread over it


class _Spy:
    """The library with the names of the entry points that were reached."""
    def __init__(self, lib, seen):
        self._lib, self._seen = lib, seen

    def __getattr__(self, name):
        self._seen.append(name)
        return getattr(self._lib, name)


def test_guards(gpu, odd, monkeypatch):
    e, t, model = odd["e"], odd["t"], odd["model"]
    me, se = sn.plda_cohort_stats_device(e, odd["c"], *model, side="enrol")
    mt, sd = sn.plda_cohort_stats_device(t, odd["c"], *model, side="test")
    z = _device_norm("z", odd["mat"], e, t, odd["c"], model, None).cpu().numpy()
    lo, hi = _range(z)
    reached, lib = [], _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: _Spy(lib, reached))
    for bad in (0.0, float("nan"), float("inf")):
        for side in ("enroll", "test"):
            std = (se if side == "enroll" else sd).clone()
            std[17] = bad
            pairs = {"enroll_norm": (me, std)} if side == "enroll" else {"test_norm": (mt, std)}
            del reached[:]
            with pytest.raises(ValueError, match="finite and > 0"):
                iv_scoring.plda_norm_histograms(e, t, odd["le"], odd["lt"], *model, lo=lo, hi=hi, **pairs)
            assert not any(name.startswith("sc_plda_hist") for name in reached), reached
    monkeypatch.undo()
    # the entry point itself: a zero std gives row 17's trials no bin; the total is short by exactly those and nothing else moves
    Phi, Psi, cst = odd["params"]
    phi, psi = torch.as_tensor(Phi).to(gpu).contiguous(), torch.as_tensor(Psi).to(gpu).contiguous()
    Ec, Tc = odd["Xc"][57:187].contiguous(), odd["Xc"][:257].contiguous()
    le, lt = torch.as_tensor(odd["le"]).to(gpu), torch.as_tensor(odd["lt"]).to(gpu)
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def direct(std):
        ht, hn = torch.empty(NB, dtype=torch.int64, device=gpu), torch.empty(NB, dtype=torch.int64, device=gpu)
        rc = lib.sc_plda_hist_norm(Ec.data_ptr(), 130, Tc.data_ptr(), 257, 45, phi.data_ptr(), psi.data_ptr(), float(cst), 1.0, le.data_ptr(), lt.data_ptr(), -1,
                                   me.data_ptr(), std.data_ptr(), None, None, lo, hi, NB, ht.data_ptr(), hn.data_ptr(), st)
        assert rc == _lib.SK_OK, _lib.last_error()
        return ht.cpu().numpy().astype(numpy.uint64), hn.cpu().numpy().astype(numpy.uint64)

    bins = _bins(z, lo, hi)
    _same(direct(se), bins, odd["tar"], odd["all"])
    se0 = se.clone()
    se0[17] = 0.0
    without = odd["all"].copy()
    without[17] = False
    got = direct(se0)
    _same(got, bins, odd["tar"], without)
    assert int(got[0].sum() + got[1].sum()) == 130 * 257 - 257


def test_one_object_on_both_sides_does_not_share_statistics(gpu, odd, monkeypatch):
    """``test_xv is enroll_xv``: the enrolment side scores ``s(x, c)`` with ``Psi``, the test side ``s(c, x)`` with ``Psi'``; both are computed."""
    x, c, model = odd["X"][:65], odd["c"], odd["model"]
    Phi, Psi, cst = odd["params"]
    mat = iv_scoring.plda_matrix_device(odd["Xc"][:65], odd["Xc"][:65], Phi, Psi, cst)
    reached, lib = [], _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    for topk, want in ((None, {"sc_plda_cohort_moments": 2}), (7, {"sc_plda_fast": 2, "sc_topk_stats_f64": 2})):   # 65 rows: one row block per side
        (me, se), (mt, sd) = (sn.plda_cohort_stats_device(x, c, *model, side=side, topk=topk) for side in ("enrol", "test"))
        by_hand = mat.clone()
        assert lib.sc_norm_apply_f64(by_hand.data_ptr(), 65, 65, me.data_ptr(), se.data_ptr(), mt.data_ptr(), sd.data_ptr(), st) == _lib.SK_OK
        del reached[:]
        monkeypatch.setattr(_lib, "lib", lambda: _Spy(lib, reached))
        got = sn.plda_snorm_device(mat.clone(), x, x, c, *model, topk=topk)
        monkeypatch.undo()
        for name, count in want.items():
            assert reached.count(name) == count, (topk, reached)
        assert got.shape == (65, 65) and torch.equal(got, by_hand), topk


# ---- the corpus of the neighbouring tests -------------------------------------------------------------------------------------------
N, M, K = 1000, 200, 50
TABLE = {"z": ((-7.75, 8.625), 0.082935), "t": ((-7.75, 8.625), 0.082935), "s": ((-7.375, 8.25), 0.081103), "as": ((-20.5, 16.75), 0.081404)}


def _unit(seed, n_spk, n):
    rs = numpy.random.RandomState(seed)
    lab = rs.randint(0, n_spk, n).astype(numpy.int32)
    c = rs.randn(n_spk, 256)
    x = c[lab] + 1.7 * rs.randn(n, 256)
    return torch.nn.functional.normalize(torch.as_tensor(x, dtype=torch.float32), dim=1).double().numpy(), lab


@pytest.fixture(scope="module")
def big(gpu, golden_dir):
    """The corpus, its float64 host scores against itself and against the cohort, and the device's own raw matrix, computed once."""
    x, lab = _unit(11, 40, N)
    c, _ = _unit(12, 60, M)
    z = numpy.load(os.path.join(golden_dir, "config5.npz"))
    model = (z["mu"], z["F"], z["Sigma"])
    host = {"s": osc.fast_plda_scores(x, x, *model), "ec": osc.fast_plda_scores(x, c, *model), "ct": osc.fast_plda_scores(c, x, *model)}
    X, C = torch.as_tensor(x).to(gpu), torch.as_tensor(c).to(gpu)
    Phi, Psi, cst = iv_scoring.plda_parameters(*model)
    Xc = (X - torch.as_tensor(model[0]).to(gpu)).contiguous()
    mat = iv_scoring.plda_matrix_device(Xc, Xc, Phi, Psi, cst)
    return {"X": X, "C": C, "lab": lab, "model": model, "host": host, "mat": mat, "tar": lab[:, None] == lab[None, :], "off": ~numpy.eye(N, dtype=bool)}


@pytest.mark.parametrize("kind", KINDS)
def test_corpus_counts_eer_and_matrix(big, kind):
    X, C, lab, model, host, tar, off = big["X"], big["C"], big["lab"], big["model"], big["host"], big["tar"], big["off"]
    ref = _host_norm(kind, host["s"], host["ec"], host["ct"], K)
    lo, hi = _range(ref[off])
    assert (lo, hi) == TABLE[kind][0]
    z = _device_norm(kind, big["mat"], X, X, C, model, K).cpu().numpy()
    err = float(numpy.abs(z - ref)[off].max())
    print(f"{kind}: materialised device matrix against the float64 restatement: {err:.2e}")
    assert err <= 1e-6
    ht, hn = sn.plda_normalised_histograms(X, X, lab, lab, C, *model, self_offset=0, lo=lo, hi=hi, **_hist_kw(kind, K))
    _same((ht, hn), _bins(z, lo, hi), tar, off)
    assert int(ht.sum() + hn.sum()) == N * N - N
    assert int(ht[0] + hn[0] + ht[-1] + hn[-1]) == 0                                    # the cap of the end bins hides nothing
    eer_h = eer_from_histograms(ht, hn)
    eer_x = osc.eer(ref[tar & off], ref[~tar])
    print(f"{kind}: binned EER {eer_h:.6f}, exact EER {eer_x:.6f}, difference {abs(eer_h - eer_x):.2e}")
    assert abs(eer_x - TABLE[kind][1]) < 1e-5 and abs(eer_h - eer_x) < 5e-4, (eer_h, eer_x)


def test_range_from_sample(big):
    X, C, model = big["X"][:300], big["C"], big["model"]
    z = _device_norm("s", big["mat"][:300, :300].contiguous(), X, X, C, model, None).cpu().numpy()[~numpy.eye(300, dtype=bool)]
    lo, hi = sn.plda_normalised_range_from_sample(X, X, C, *model, kind="s")
    assert lo == float(z.min()) - 0.25 * float(z.max() - z.min()) and hi == float(z.max()) + 0.25 * float(z.max() - z.min())


# ---- pin to the reference -----------------------------------------------------------------------------------------------------------
def test_reference_tnorm_of_reference_plda_scores(gpu, golden_dir):
    fx = numpy.load(os.path.join(golden_dir, "plda_norm.npz"))
    model = (fx["mu"], fx["F"], fx["Sigma"])
    assert float(fx["min_cohort_std"]) > 1e-3
    e, t, c = (torch.as_tensor(fx[k]).to(gpu) for k in ("enrol", "test", "cohort"))
    Phi, Psi, cst = iv_scoring.plda_parameters(*model)
    mu_d = torch.as_tensor(model[0]).to(gpu)
    mat = iv_scoring.plda_matrix_device(e - mu_d, t - mu_d, Phi, Psi, cst)
    assert float(numpy.abs(mat.cpu().numpy() - fx["scores"]).max()) <= 1e-9 * float(numpy.abs(fx["scores"]).max())
    want = {"z": fx["znorm"], "t": fx["tnorm"], "s": 0.5 * (fx["znorm"] + fx["tnorm"])}
    for kind in ("z", "t", "s"):
        got = _device_norm(kind, mat, e, t, c, model, None).cpu().numpy()
        err = float(numpy.abs(got - want[kind]).max())
        print(f"{kind}-norm against the reference: {err:.2e}")
        assert got.shape == (37, 53) and err <= 1e-6, kind


# ---- the driver -----------------------------------------------------------------------------------------------------------------------
def test_sharded_driver_reports_the_normalised_plda_all_pairs_eer(gpu, capsys):
    from sidekit_amd.bin import shard_extract_score
    base = ["--utterances", "640", "--trials", "100", "--speakers", "40", "--batch", "64", "--seconds", "1", "--all-pairs-plda"]
    shard_extract_score.main(base)
    plain = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    shard_extract_score.main(base + ["--all-pairs-plda-norm", "as", "--norm-cohort", "200", "--norm-topk", "40"])
    d = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    assert d["plda_all_pairs_norm"] == 440 * 439 and d["plda_all_pairs_norm_kind"] == "as" and d["plda_all_pairs_norm_cohort"] == 200
    lo, hi = d["plda_all_pairs_norm_hist_range"]
    assert lo < hi and numpy.isfinite(d["plda_all_pairs_norm_eer"]) and 0.0 <= d["plda_all_pairs_norm_eer"] <= 0.5 and d["plda_all_pairs_norm_s"] > 0.0
    new = {"plda_all_pairs_norm", "plda_all_pairs_norm_kind", "plda_all_pairs_norm_cohort", "plda_all_pairs_norm_hist_range", "plda_all_pairs_norm_s",
           "plda_all_pairs_norm_eer"}
    assert set(d) - set(plain) == new and set(plain) - set(d) == set()
    assert list(plain) == [k for k in d if k not in new]                                # without the flag: the keys of today, in their order
    assert d["plda_all_pairs"] == plain["plda_all_pairs"] == 640 * 639 and d["plda_all_pairs_eer"] == plain["plda_all_pairs_eer"]
