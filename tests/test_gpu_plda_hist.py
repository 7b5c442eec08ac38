"""All-pairs PLDA histograms (sc_plda_hist, iv_scoring.plda_histograms): the counts are, bin for bin, those of binning the float64 matrix
sc_plda_fast writes (plda_matrix_device) on the host with the kernel's expression, and the EER of the counts is the exact EER of a float64
host restatement of the scores within the project's +-0.05 % absolute.

The large corpus is the one of tests/test_gpu_hist_norm.py (RandomState(11), 40 speakers, N = 1000, D = 256, noise 1.7, unit rows) as
float64, scored with the reference-trained (mu, F, Sigma) of tests/golden/config5.npz.  On the host, in float64: the scores range over
[-42.4, 18.9], the histogram range is [-57.75, 34.25], the exact EER is 8.3126 %, the float64-binned EER 8.3171 % (4.5e-5 apart), and no
score lies in an end bin."""
import ctypes
import json
import os
import sys

import numpy
import pytest
import torch

from oracle import scoring as osc
from sidekit_amd import _lib, iv_scoring
from sidekit_amd.bosaris import Ndx, eer_from_histograms
from sidekit_amd.statserver import StatServer

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import second_trips as st  # noqa: E402

pytestmark = pytest.mark.gpu
NB = iv_scoring.HIST_BINS
N = 1000


def _range(z):
    """min / max widened by a quarter of the range, moved outward to multiples of 1/8."""
    zmin, zmax = float(z.min()), float(z.max())
    pad = 0.25 * (zmax - zmin)
    return float(numpy.floor((zmin - pad) * 8) / 8), float(numpy.ceil((zmax + pad) * 8) / 8)


def _bins(z, lo, hi, nb=NB):
    """The bin of every entry of a float64 matrix, with the kernel's float64 operations."""
    return numpy.clip(numpy.floor((z - lo) * (nb / (hi - lo))), 0, nb - 1).astype(numpy.int64)


def _count(bins, sel, nb=NB):
    return numpy.bincount(bins[sel], minlength=nb).astype(numpy.uint64)


def _same(got, bins, tar, keep, nb=NB):
    ht, hn = got
    assert ht.dtype == hn.dtype == numpy.uint64 and ht.shape == hn.shape == (nb,)
    assert int(ht.sum() + hn.sum()) == int(keep.sum())
    assert numpy.array_equal(ht, _count(bins, tar & keep, nb)) and numpy.array_equal(hn, _count(bins, ~tar & keep, nb))


@pytest.fixture(scope="module")
def big(gpu, golden_dir):
    """The N = 1000 corpus, its float64 host scores, the device's own materialised matrix and the histograms, computed once."""
    rs = numpy.random.RandomState(11)
    lab = rs.randint(0, 40, N).astype(numpy.int32)
    c = rs.randn(40, 256)
    x = c[lab] + 1.7 * rs.randn(N, 256)
    x = torch.nn.functional.normalize(torch.as_tensor(x, dtype=torch.float32), dim=1).double().numpy()
    z = numpy.load(os.path.join(golden_dir, "config5.npz"))
    mu, F, Sigma = z["mu"], z["F"], z["Sigma"]
    ref = osc.fast_plda_scores(x, x, mu, F, Sigma)
    tar, off = lab[:, None] == lab[None, :], ~numpy.eye(N, dtype=bool)
    lo, hi = _range(ref[off])
    X = torch.as_tensor(x).to(gpu)
    Phi, Psi, cst = iv_scoring.plda_parameters(mu, F, Sigma)
    mat = iv_scoring.plda_matrix_device(X - torch.as_tensor(mu).to(gpu), X - torch.as_tensor(mu).to(gpu), Phi, Psi, cst).cpu().numpy()
    assert float(numpy.abs(mat - ref).max()) < 1e-9 * float(numpy.abs(ref).max())     # the materialised path is the score it says
    hist = iv_scoring.plda_histograms(X, X, lab, lab, mu, F, Sigma, self_offset=0, lo=lo, hi=hi)
    return {"ref": ref, "tar": tar, "off": off, "lo": lo, "hi": hi, "mat": mat, "hist": hist}


def test_counts_are_those_of_the_materialised_path(big):
    assert (big["lo"], big["hi"]) == (-57.75, 34.25)
    _same(big["hist"], _bins(big["mat"], big["lo"], big["hi"]), big["tar"], big["off"])
    assert int(big["hist"][0].sum() + big["hist"][1].sum()) == N * N - N


def test_eer_of_the_counts_is_the_exact_eer(big):
    ht, hn = big["hist"]
    assert int(ht[0] + hn[0] + ht[-1] + hn[-1]) == 0                                   # the cap of the end bins hides nothing
    eer_h = eer_from_histograms(ht, hn)
    eer_x = osc.eer(big["ref"][big["tar"] & big["off"]], big["ref"][~big["tar"]])
    print(f"binned EER {eer_h:.6f}, exact EER {eer_x:.6f}, difference {abs(eer_h - eer_x):.2e}")
    assert abs(eer_x - 0.083126) < 1e-5 and abs(eer_h - eer_x) < 5e-4, (eer_h, eer_x)


@pytest.fixture(scope="module")
def odd(gpu, golden_dir):
    """D = 45 (odd k, a partial k-tile, the scalar-load path), Ne = 130 rows [57, 187) against Nt = 257 rows [0, 257)."""
    z = numpy.load(os.path.join(golden_dir, "plda_train.npz"))
    X = torch.as_tensor(numpy.ascontiguousarray(z["X"][:, :45])).to(gpu)
    mu, F, Sigma = z["mean_0"][:45], z["F_0"][:45], z["Sigma_0"][:45, :45]
    lab = numpy.unique(z["modelset"], return_inverse=True)[1].astype(numpy.int32)
    e, t, le, lt = X[57:187], X[:257], lab[57:187], lab[:257]
    Phi, Psi, cst = iv_scoring.plda_parameters(mu, F, Sigma)
    mu_d = torch.as_tensor(mu).to(gpu)
    mat = iv_scoring.plda_matrix_device(e - mu_d, t - mu_d, Phi, Psi, cst).cpu().numpy()
    ref = osc.fast_plda_scores(z["X"][57:187, :45], z["X"][:257, :45], mu, F, Sigma)
    assert float(numpy.abs(mat - ref).max()) < 1e-9 * float(numpy.abs(ref).max())
    lo, hi = _range(mat)
    keep = numpy.ones((130, 257), dtype=bool)
    keep[numpy.arange(130), numpy.arange(130) + 57] = False
    return {"e": e, "t": t, "le": le, "lt": lt, "model": (mu, F, Sigma), "params": (Phi, Psi, cst), "mat": mat, "lo": lo, "hi": hi,
            "tar": le[:, None] == lt[None, :], "all": numpy.ones((130, 257), dtype=bool), "keep": keep}


def test_odd_shapes(odd):
    bins = _bins(odd["mat"], odd["lo"], odd["hi"])
    args = (odd["e"], odd["t"], odd["le"], odd["lt"]) + odd["model"]
    got = iv_scoring.plda_histograms(*args, self_offset=None, lo=odd["lo"], hi=odd["hi"])
    _same(got, bins, odd["tar"], odd["all"])
    assert int(got[0].sum() + got[1].sum()) == 130 * 257
    got = iv_scoring.plda_histograms(*args, self_offset=57, lo=odd["lo"], hi=odd["hi"])
    _same(got, bins, odd["tar"], odd["keep"])
    assert int(got[0].sum() + got[1].sum()) == 130 * 257 - 130


def test_counts_when_the_tiles_outnumber_the_compute_units(gpu, golden_dir):
    """plda_hist_kernel<HN_NONE> walks ``tile += gridDim.x`` with one workgroup per compute unit; past CU-count tiles a workgroup takes a
    second one and writes that tile's row and column terms into ``term`` behind dgemm_tile's barriers, over the ones the first tile's
    epilogue read.  N = (t - 1) 128 + 3 with t x t > CUs (2051 at 256 CUs: 289 tiles), both edges ragged, D = 10 (a partial k-tile of 16),
    the model of the ``odd`` fixture cut to 10 dimensions, 40 speakers, the set against itself: the counts are those of binning
    plda_matrix_device's matrix with ``_bins`` (on the device; every 97th row also by ``_bins`` itself).  A row shard of 16 x 17 tiles
    -- still more than CUs -- starts on another row of the tile."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    n, t = st.hist_side(cus, st.PT)
    assert ((n + st.PT - 1) // st.PT) ** 2 == t * t > cus
    model = st.plda_model(golden_dir, 10)
    x, lab = st.plda_corpus(model, n)
    X = torch.as_tensor(x).to(gpu)
    Xc = (X - torch.as_tensor(model[0]).to(gpu)).contiguous()
    mat = iv_scoring.plda_matrix_device(Xc, Xc, *iv_scoring.plda_parameters(*model))
    lo, hi = _range(mat[~torch.eye(n, dtype=torch.bool, device=gpu)])               # without the self-trials, as the ``big`` fixture's
    want_t, want_n, bins = st.device_counts(mat, lo, hi, NB, lab, lab, 0)
    rows = slice(None, None, 97)
    assert numpy.array_equal(bins[rows].cpu().numpy(), _bins(mat[rows].cpu().numpy(), lo, hi))
    ht, hn = iv_scoring.plda_histograms(X, X, lab, lab, *model, self_offset=0, lo=lo, hi=hi)
    assert ht.dtype == hn.dtype == numpy.uint64 and int(ht.sum() + hn.sum()) == n * n - n
    assert numpy.array_equal(ht, want_t) and numpy.array_equal(hn, want_n)
    assert int(ht[0] + hn[0] + ht[-1] + hn[-1]) == 0 and int((ht + hn > 0).sum()) > 1000   # every score inside the range, spread over it
    a = 67
    assert ((n - a + st.PT - 1) // st.PT) * t > cus
    want_t, want_n, _ = st.device_counts(mat[a:], lo, hi, NB, lab[a:], lab, a)
    ht, hn = iv_scoring.plda_histograms(X[a:], X, lab[a:], lab, *model, self_offset=a, lo=lo, hi=hi)
    assert int(ht.sum() + hn.sum()) == (n - a) * (n - 1)
    assert numpy.array_equal(ht, want_t) and numpy.array_equal(hn, want_n)


def _obj(a):
    return numpy.array([str(x) for x in a], dtype=object)


def test_scaling_and_the_channel_subspace(gpu, golden_dir):
    fx = numpy.load(os.path.join(golden_dir, "scoring.npz"))
    mu, F, G, Sigma = fx["mu"], fx["F"], fx["G"], fx["Sigma"]
    enroll = StatServer.from_arrays(_obj(fx["enr_ids"]), _obj(fx["enr_ids"]), fx["E"])
    test = StatServer.from_arrays(_obj(fx["tst_ids"]), _obj(fx["tst_ids"]), fx["T"])
    ndx = Ndx()
    ndx.modelset, ndx.segset, ndx.trialmask = enroll.modelset, test.segset, numpy.ones((32, 40), dtype=bool)
    le, lt = numpy.unique(fx["enr_ids"], return_inverse=True)[1].astype(numpy.int32) % 7, numpy.arange(40, dtype=numpy.int32) % 7
    tar, every = le[:, None] == lt[None, :], numpy.ones((32, 40), dtype=bool)
    # the golden matrices are the reference's, in the order its Ndx alignment leaves (scaling 0.7 for the two-covariance form, 1 with the
    # channel sub-space): the device matrix is checked against them as tests/test_gpu_scoring.py does, and the all-trials matrix in
    # file order that the histograms are compared with is that matrix with its rows and columns permuted
    gndx = Ndx(models=_obj(fx["trial_models"]), testsegs=_obj(fx["trial_segs"]))
    def same_scores(aligned, golden, tol, mat):
        err = float(numpy.abs(aligned.scoremat - golden).max() / numpy.abs(golden).max())
        print(f"device matrix against the golden one: largest difference {err:.2e} of the largest score")
        numpy.testing.assert_allclose(aligned.scoremat, golden, rtol=tol, atol=tol)
        rows = [list(fx["enr_ids"]).index(m) for m in aligned.modelset]
        cols = [list(fx["tst_ids"]).index(s) for s in aligned.segset]
        numpy.testing.assert_allclose(mat[numpy.ix_(rows, cols)], aligned.scoremat, rtol=1e-12, atol=1e-12)
    for scaling in (0.5, 0.7):
        mat = iv_scoring.fast_PLDA_scoring(enroll, test, ndx, mu, F, Sigma, scaling_factor=scaling, check_missing=False).scoremat
        if scaling == 0.7:
            same_scores(iv_scoring.fast_PLDA_scoring(enroll, test, gndx, mu, F, Sigma, scaling_factor=0.7), fx["plda_scaled_scoremat"], 1e-9, mat)
        lo, hi = _range(mat)
        _same(iv_scoring.plda_histograms(fx["E"], fx["T"], le, lt, mu, F, Sigma, scaling_factor=scaling, lo=lo, hi=hi, device=gpu),
              _bins(mat, lo, hi), tar, every)
    mat = iv_scoring.full_PLDA_scoring(enroll, test, ndx, mu, F, G, Sigma, check_missing=False).scoremat
    same_scores(iv_scoring.full_PLDA_scoring(enroll, test, gndx, mu, F, G, Sigma), fx["plda_full_scoremat"], 1e-9, mat)
    lo, hi = _range(mat)
    _same(iv_scoring.plda_histograms(fx["E"], fx["T"], le, lt, mu, F, Sigma, G, lo=lo, hi=hi, device=gpu), _bins(mat, lo, hi), tar, every)


def test_range_and_bins(odd):
    args = (odd["e"], odd["t"], odd["le"], odd["lt"]) + odd["model"]
    mat, tar, every = odd["mat"], odd["tar"], odd["all"]
    # a range narrower than the scores: the end bins hold what fell outside, the total is unchanged
    lo, hi = float(numpy.percentile(mat, 20)), float(numpy.percentile(mat, 70))
    ht, hn = iv_scoring.plda_histograms(*args, lo=lo, hi=hi)
    _same((ht, hn), _bins(mat, lo, hi), tar, every)
    assert int(ht[0] + hn[0]) >= int((mat < lo).sum()) > 1000 and int(ht[-1] + hn[-1]) >= int((mat >= hi).sum()) > 1000
    # two passes of finer bins over the full range
    lo, hi = odd["lo"], odd["hi"]
    ft, fn = iv_scoring.plda_histograms(*args, lo=lo, hi=hi, bins=2 * 8190)
    assert ft.shape == fn.shape == (16380,) and int(ft.sum() + fn.sum()) == 130 * 257
    coarse = _bins(mat, lo, hi, 8190)
    assert numpy.array_equal(ft.reshape(8190, 2).sum(axis=1), _count(coarse, tar, 8190))
    assert numpy.array_equal(fn.reshape(8190, 2).sum(axis=1), _count(coarse, ~tar, 8190))


def test_streams_reuse_and_the_shared_workspace(gpu, odd):
    lib = _lib.lib()
    Phi, Psi, cst = odd["params"]
    phi, psi = torch.as_tensor(Phi).to(gpu).contiguous(), torch.as_tensor(Psi).to(gpu).contiguous()
    mu_d = torch.as_tensor(odd["model"][0]).to(gpu)
    e, t = (odd["e"] - mu_d).contiguous(), (odd["t"] - mu_d).contiguous()
    le, lt = torch.as_tensor(odd["le"]).to(gpu), torch.as_tensor(odd["lt"]).to(gpu)
    lo, hi = odd["lo"], odd["hi"]
    bins = _bins(odd["mat"], lo, hi)
    want = {None: (odd["all"], -1), 57: (odd["keep"], 57)}

    def hist(a, la, b, lb, self_offset, stream):
        ht = torch.full((NB,), -7, dtype=torch.int64, device=gpu)
        hn = torch.full((NB,), -7, dtype=torch.int64, device=gpu)
        rc = lib.sc_plda_hist(a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], 45, phi.data_ptr(), psi.data_ptr(), float(cst), 1.0, la.data_ptr(),
                              lb.data_ptr(), self_offset, lo, hi, NB, ht.data_ptr(), hn.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
        assert rc == _lib.SK_OK, _lib.last_error()
        return ht, hn

    def fast(stream):
        out = torch.empty((130, 257), dtype=torch.float64, device=gpu)
        rc = lib.sc_plda_fast(e.data_ptr(), 130, t.data_ptr(), 257, 45, phi.data_ptr(), psi.data_ptr(), float(cst), 1.0, out.data_ptr(),
                              ctypes.c_void_p(stream.cuda_stream))
        assert rc == _lib.SK_OK, _lib.last_error()
        return out

    torch.cuda.synchronize(gpu)
    s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
    with torch.cuda.stream(s1):
        before = fast(s1)
        h1 = hist(e, le, t, lt, 57, s1)                       # 130 x 257 on one stream ...
        after = fast(s1)
    with torch.cuda.stream(s2):
        h2 = hist(t, lt, t, lt, 0, s2)                        # ... 257 x 257 on another, each with a workspace of its own
    torch.cuda.synchronize(gpu)
    assert torch.equal(before, after) and numpy.array_equal(before.cpu().numpy(), odd["mat"])       # the shared workspace is not corrupted
    _same(tuple(h.cpu().numpy().astype(numpy.uint64) for h in h1), bins, odd["tar"], odd["keep"])
    assert int(h2[0].sum() + h2[1].sum()) == 257 * 256
    assert lib.sc_release_workspace() == _lib.SK_OK
    with torch.cuda.stream(s1):
        h3 = hist(e, le, t, lt, -1, s1)
    torch.cuda.synchronize(gpu)
    _same(tuple(h.cpu().numpy().astype(numpy.uint64) for h in h3), bins, odd["tar"], odd["all"])
    # argument errors launch nothing
    ht = torch.full((NB,), -7, dtype=torch.int64, device=gpu)
    cur = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    head = (e.data_ptr(), 130, t.data_ptr(), 257, 45, phi.data_ptr(), psi.data_ptr(), float(cst), 1.0, le.data_ptr(), lt.data_ptr(), -1)
    assert lib.sc_plda_hist(*head, lo, lo, NB, ht.data_ptr(), ht.data_ptr(), cur) == _lib.SK_EARG
    assert lib.sc_plda_hist(*head, lo, float("inf"), NB, ht.data_ptr(), ht.data_ptr(), cur) == _lib.SK_EARG
    assert lib.sc_plda_hist(*head, lo, hi, 4096, ht.data_ptr(), ht.data_ptr(), cur) == _lib.SK_EARG
    torch.cuda.synchronize(gpu)
    assert bool((ht == -7).all())


def test_infinite_and_nan_scores(gpu, odd):
    """+-inf lands in an end bin (the clamp precedes the conversion to int); a NaN score is in no bin and is missing from the total."""
    mu, F, Sigma = odd["model"]
    e, t = odd["e"][:3].clone(), odd["t"][:5]
    le, lt = odd["le"][:3], odd["lt"][:5]
    lib = _lib.lib()
    Phi, Psi, cst = odd["params"]
    phi, psi = torch.as_tensor(Phi).to(gpu).contiguous(), torch.as_tensor(Psi).to(gpu).contiguous()
    ht, hn = torch.empty(NB, dtype=torch.int64, device=gpu), torch.empty(NB, dtype=torch.int64, device=gpu)
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    tc = (t - torch.as_tensor(mu).to(gpu)).contiguous()
    for cst_in, end_bin, total in ((float("inf"), NB - 1, 15), (-float("inf"), 0, 15), (float("nan"), None, 0)):
        ec = (e - torch.as_tensor(mu).to(gpu)).contiguous()
        assert lib.sc_plda_hist(ec.data_ptr(), 3, tc.data_ptr(), 5, 45, phi.data_ptr(), psi.data_ptr(), cst_in, 1.0, torch.as_tensor(le).to(gpu).data_ptr(),
                                torch.as_tensor(lt).to(gpu).data_ptr(), -1, odd["lo"], odd["hi"], NB, ht.data_ptr(), hn.data_ptr(), st) == _lib.SK_OK
        assert int(ht.sum() + hn.sum()) == total
        if end_bin is not None:
            assert int(ht[end_bin] + hn[end_bin]) == 15
    bad = odd["e"].clone()
    bad[4, 7] = float("nan")
    with pytest.raises(ValueError, match="centred vectors are not finite"):
        iv_scoring.plda_histograms(bad, odd["t"], odd["le"], odd["lt"], mu, F, Sigma, lo=odd["lo"], hi=odd["hi"])


def test_range_from_sample(gpu, odd):
    mu, F, Sigma = odd["model"]
    lo, hi = iv_scoring.plda_range_from_sample(odd["e"], odd["t"], mu, F, Sigma)
    zmin, zmax = float(odd["mat"].min()), float(odd["mat"].max())
    assert lo == zmin - 0.25 * (zmax - zmin) and hi == zmax + 0.25 * (zmax - zmin)
    t = odd["t"]
    lo, hi = iv_scoring.plda_range_from_sample(t, t, mu, F, Sigma)                      # one object: the self-trials are left out
    Phi, Psi, cst = odd["params"]
    tc = t - torch.as_tensor(mu).to(gpu)
    z = iv_scoring.plda_matrix_device(tc, tc, Phi, Psi, cst).cpu().numpy()[~numpy.eye(257, dtype=bool)]
    assert lo == float(z.min()) - 0.25 * float(z.max() - z.min()) and hi == float(z.max()) + 0.25 * float(z.max() - z.min())


def test_sharded_driver_reports_the_plda_all_pairs_eer(gpu, capsys):
    from sidekit_amd.bin import shard_extract_score
    base = ["--utterances", "1600", "--trials", "250", "--batch", "64", "--seconds", "1"]
    shard_extract_score.main(base + ["--all-pairs-plda"])
    d = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    assert d["plda_all_pairs"] == 1600 * 1599 and d["plda_all_pairs_hist_bins"] == NB
    lo, hi = d["plda_all_pairs_hist_range"]
    assert lo < hi and 0.0 <= d["plda_all_pairs_eer"] < 0.5 and d["plda_all_pairs_s"] > 0.0
    assert "all_pairs_eer" not in d                                                    # the flag implies no other
