"""All-pairs histograms of cohort-normalised scores (sc_cosine_hist_norm, iv_scoring.cosine_histograms(enroll_norm=, test_norm=),
score_normalization.normalised_histograms): the counts are, bin for bin, those of the materialised path -- sc_cosine, then
znorm_device / tnorm_device / snorm_device, then binning the matrix -- and the EER of the counts is the exact EER of a float64 numpy
restatement of the normalised scores within the project's +-0.05 % absolute.

The corpus is the one of tests/test_gpu_scoring.py::test_cosine_histograms_match_the_score_matrix (RandomState(11), 40 speakers, N = 1000,
D = 256, noise 1.7, unit rows) with a cohort built the same way (RandomState(12), 60 speakers, M = 200).  On the host, in float64, with
8192 bins over the widened range: exact EER of the whole-cohort s-normalised scores 1.67 %, binned 1.9e-5 away; top-50 adaptive s-norm
1.74 %, binned 1.7e-5 away; no score in an end bin.  sc_cosine, whose products the counts are held to, is itself judged against float64
in tests/test_gpu_scoring_kernels.py (off D = 256 too: k-tails, the padding branch, both tile forms)."""
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
N, M, TOPK = 1000, 200, 50
KINDS = {"z": ("z", None), "t": ("t", None), "s": ("s", None), "as": ("s", TOPK)}


def _st(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _speakers(seed, n_spk, n):
    rs = numpy.random.RandomState(seed)
    lab = rs.randint(0, n_spk, n).astype(numpy.int32)
    c = rs.randn(n_spk, 256)
    x = c[lab] + 1.7 * rs.randn(n, 256)
    return torch.nn.functional.normalize(torch.as_tensor(x, dtype=torch.float32), dim=1), lab


def _restated(x, c, kind, topk):
    """The normalised scores of a set against itself in float64 numpy, from the host x-vectors alone."""
    x, c = x.numpy().astype(numpy.float64), c.numpy().astype(numpy.float64)
    s, cs = x @ x.T, x @ c.T
    if topk is None:
        m, sd = cs.mean(axis=1), cs.std(axis=1)                       # population std (score_normalization.py:69,90)
    else:
        best = numpy.sort(cs, axis=1)[:, -topk:]
        m, sd = best.mean(axis=1), best.std(axis=1, ddof=1)           # torch's unbiased std (:133-136)
    z, t = (s - m[:, None]) / sd[:, None], (s - m[None, :]) / sd[None, :]
    return {"z": z, "t": t, "s": 0.5 * z + 0.5 * t}[kind]


def _range(z):
    """min / max widened by a quarter of the range, moved outward to multiples of 1/8: hi - lo is then exact in float32 too."""
    zmin, zmax = float(z.min()), float(z.max())
    pad = 0.25 * (zmax - zmin)
    return float(numpy.floor((zmin - pad) * 8) / 8), float(numpy.ceil((zmax + pad) * 8) / 8)


def _bins(z, lo, hi):
    """The bin of every entry of a float32 matrix, with the kernel's float32 operations."""
    scale = numpy.float32(NB / (hi - lo))
    assert scale == numpy.float32(NB) / (numpy.float32(hi) - numpy.float32(lo))      # the test's own edges: one rounding either way
    return numpy.clip(numpy.floor((z - numpy.float32(lo)) * scale).astype(numpy.int64), 0, NB - 1)


def _count(bins, sel):
    return numpy.bincount(bins[sel], minlength=NB).astype(numpy.uint64)


@pytest.fixture(scope="module")
def corpus(gpu):
    """Everything the cases share, computed once: the x-vectors, per kind the histogram range (from the float64 restatement), the
    device's own materialised normalised matrix and its bins."""
    x, lab = _speakers(11, 40, N)
    c, _ = _speakers(12, 60, M)
    tar = lab[:, None] == lab[None, :]
    off = ~numpy.eye(N, dtype=bool)
    d = {"X": x.to(gpu), "C": c.to(gpu), "lab": lab, "tar": tar, "off": off}
    for name, (kind, topk) in KINDS.items():
        ref = _restated(x, c, kind, topk)
        lo, hi = _range(ref[off])
        z = iv_scoring.cosine_matrix_device(d["X"], d["X"])
        if kind == "z":
            sn.znorm_device(z, d["X"], d["C"])
        elif kind == "t":
            sn.tnorm_device(z, d["X"], d["C"])
        else:
            sn.snorm_device(z, d["X"], d["X"], d["C"], topk=topk)
        z = z.cpu().numpy()
        assert numpy.isfinite(z).all() and float(numpy.abs(z - ref).max()) < 1e-3     # the materialised path is the normalisation it says
        d[name] = {"ref": ref, "lo": lo, "hi": hi, "bins": _bins(z, lo, hi)}
    return d


def _exact_eer(corpus, name):
    k = corpus[name]
    if "eer" not in k:
        k["eer"] = osc.eer(k["ref"][corpus["tar"] & corpus["off"]], k["ref"][~corpus["tar"]])
    return k["eer"]


@pytest.mark.parametrize("name", list(KINDS))
def test_counts_are_those_of_the_materialised_path(corpus, name):
    kind, topk = KINDS[name]
    k, tar, off = corpus[name], corpus["tar"], corpus["off"]
    ht, hn = sn.normalised_histograms(corpus["X"], corpus["X"], corpus["lab"], corpus["lab"], corpus["C"], kind=kind, topk=topk, self_offset=0,
                                      lo=k["lo"], hi=k["hi"])
    assert ht.dtype == hn.dtype == numpy.uint64 and ht.shape == hn.shape == (NB,)
    assert int(ht.sum() + hn.sum()) == N * N - N
    assert numpy.array_equal(ht, _count(k["bins"], tar & off)) and numpy.array_equal(hn, _count(k["bins"], ~tar))
    assert int(ht[0] + hn[0] + ht[-1] + hn[-1]) == 0                                   # the widened range holds every score


@pytest.mark.parametrize("ne,nt,dim", [(300, 333, 64), (257, 1, 36), (64, 700, 256)])
def test_ragged_and_small_shapes(gpu, ne, nt, dim):
    """2 x 2 tiles with both edges ragged and two k-tiles; one column, one row past a tile edge and a k-tail (D % 32 != 0); a single
    partial row tile -- s-mode, bit for bit the materialised path."""
    rs = numpy.random.RandomState(ne + nt)
    unit = lambda n: torch.nn.functional.normalize(torch.as_tensor(rs.randn(n, dim), dtype=torch.float32), dim=1).to(gpu)
    e, t, c = unit(ne), unit(nt), unit(90)
    le, lt = rs.randint(0, 5, ne).astype(numpy.int32), rs.randint(0, 5, nt).astype(numpy.int32)
    z = sn.snorm_device(iv_scoring.cosine_matrix_device(e, t), e, t, c).cpu().numpy()
    lo, hi = _range(z)
    ht, hn = sn.normalised_histograms(e, t, le, lt, c, kind="s", lo=lo, hi=hi)
    bins, tar = _bins(z, lo, hi), le[:, None] == lt[None, :]
    assert int(ht.sum() + hn.sum()) == ne * nt
    assert numpy.array_equal(ht, _count(bins, tar)) and numpy.array_equal(hn, _count(bins, ~tar))


@pytest.fixture(scope="module")
def walk(gpu):
    """A set whose 256 x 256 tiles outnumber the compute units (tests/tools/second_trips.py: D = 8, 40 speakers), and a cohort of 300."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    n, t = st.hist_side(cus, st.HT)
    x, lab = st.cosine_corpus(n)
    c, _ = st.cosine_corpus(300, seed=26)
    return {"cus": cus, "n": n, "t": t, "X": torch.from_numpy(x).to(gpu), "C": torch.from_numpy(c).to(gpu), "lab": lab}


@pytest.mark.parametrize("name", list(KINDS))
def test_counts_when_the_tiles_outnumber_the_compute_units(walk, name):
    """cosine_hist_kernel<HN_ENROL | HN_TEST | HN_BOTH> walks ``tile += gridDim.x`` with one workgroup per compute unit; past CU-count
    tiles a workgroup takes a second one and stages that tile's 512 (mean, std) in ``stat`` behind the k loop's barriers, over the ones
    the first tile's epilogue read.  N = (t - 1) 256 + 3 with t x t > CUs (4099 at 256 CUs: 289 tiles), both edges ragged, the set
    against itself, every kind: the counts are those of the materialised path (sc_cosine, the normalisation, then this module's
    ``_bins`` -- evaluated on the device, every 97th row also by ``_bins`` itself)."""
    kind, topk = KINDS[name]
    X, C, lab, n, t = walk["X"], walk["C"], walk["lab"], walk["n"], walk["t"]
    assert ((n + st.HT - 1) // st.HT) ** 2 == t * t > walk["cus"]
    z = iv_scoring.cosine_matrix_device(X, X)
    if kind == "z":
        sn.znorm_device(z, X, C)
    elif kind == "t":
        sn.tnorm_device(z, X, C)
    else:
        sn.snorm_device(z, X, X, C, topk=topk)
    assert bool(torch.isfinite(z).all())
    lo, hi = _range(z)
    want_t, want_n, bins = st.device_counts(z, lo, hi, NB, lab, lab, 0)
    rows = slice(None, None, 97)
    assert numpy.array_equal(bins[rows].cpu().numpy(), _bins(z[rows].cpu().numpy(), lo, hi))
    ht, hn = sn.normalised_histograms(X, X, lab, lab, C, kind=kind, topk=topk, self_offset=0, lo=lo, hi=hi)
    assert ht.dtype == hn.dtype == numpy.uint64 and int(ht.sum() + hn.sum()) == n * n - n
    assert numpy.array_equal(ht, want_t) and numpy.array_equal(hn, want_n)
    assert int(ht[0] + hn[0] + ht[-1] + hn[-1]) == 0 and int((ht + hn > 0).sum()) > 1000   # every score inside the range, spread over it


def test_disjoint_sets_drop_nothing(corpus):
    k, lab = corpus["s"], corpus["lab"]
    ht, hn = sn.normalised_histograms(corpus["X"][:77], corpus["X"][100:], lab[:77], lab[100:], corpus["C"], kind="s", lo=k["lo"], hi=k["hi"])
    assert int(ht.sum() + hn.sum()) == 77 * 900
    bins, tar = k["bins"][:77, 100:], corpus["tar"][:77, 100:]
    assert numpy.array_equal(ht, _count(bins, tar)) and numpy.array_equal(hn, _count(bins, ~tar))


def test_row_shard(corpus):
    """Rows [300, 650) against everything, self-trials at j == i + 300, the enrolment statistics sliced to the shard."""
    a, b = 300, 650
    k, lab, tar, off = corpus["s"], corpus["lab"], corpus["tar"], corpus["off"]
    me, se = sn.cohort_stats_device(corpus["X"], corpus["C"])
    ht, hn = iv_scoring.cosine_histograms(corpus["X"][a:b], corpus["X"], lab[a:b], lab, self_offset=a, lo=k["lo"], hi=k["hi"],
                                          enroll_norm=(me[a:b], se[a:b]), test_norm=(me, se))
    assert numpy.array_equal(ht, _count(k["bins"][a:b], (tar & off)[a:b])) and numpy.array_equal(hn, _count(k["bins"][a:b], ~tar[a:b]))


def test_one_sided_calls_through_the_c_symbol(gpu, corpus):
    """The enrolment pair alone and the test pair alone against sc_norm_apply on sc_cosine's matrix; the argument rules of sc_norm_apply."""
    lib = _lib.lib()
    e, t = corpus["X"][:300].contiguous(), corpus["X"][300:633].contiguous()
    le = torch.as_tensor(corpus["lab"][:300]).to(gpu)
    lt = torch.as_tensor(corpus["lab"][300:633]).to(gpu)
    (me, se), (mt, sd) = sn.cohort_stats_device(e, corpus["C"]), sn.cohort_stats_device(t, corpus["C"])
    tar = corpus["tar"][:300, 300:633]
    ht = torch.full((NB,), -7, dtype=torch.int64, device=gpu)
    hn = torch.full((NB,), -7, dtype=torch.int64, device=gpu)

    def call(a, b, c, d, lo, hi):
        p = lambda v: None if v is None else v.data_ptr()
        return lib.sc_cosine_hist_norm(e.data_ptr(), 300, t.data_ptr(), 333, 256, le.data_ptr(), lt.data_ptr(), -1, p(a), p(b), p(c), p(d), lo, hi, NB,
                                       ht.data_ptr(), hn.data_ptr(), _st(gpu))

    for pairs in ((me, se, None, None), (None, None, mt, sd)):
        z = iv_scoring.cosine_matrix_device(e, t)
        _lib.check(lib.sc_norm_apply(z.data_ptr(), 300, 333, *(None if v is None else v.data_ptr() for v in pairs), _st(gpu)))
        z = z.cpu().numpy()
        lo, hi = _range(z)
        assert call(*pairs, lo, hi) == _lib.SK_OK
        bins = _bins(z, lo, hi)
        assert numpy.array_equal(ht.cpu().numpy().astype(numpy.uint64), _count(bins, tar))
        assert numpy.array_equal(hn.cpu().numpy().astype(numpy.uint64), _count(bins, ~tar))
    ht.fill_(-7), hn.fill_(-7)
    assert call(me, None, None, None, -1.0, 1.0) == _lib.SK_EARG and "together" in _lib.last_error()      # a mean without its std
    assert call(None, None, mt, None, -1.0, 1.0) == _lib.SK_EARG
    assert call(None, None, None, None, -1.0, 1.0) == _lib.SK_EARG and "at least one" in _lib.last_error()  # no pair at all
    torch.cuda.synchronize(gpu)
    assert bool((ht == -7).all()) and bool((hn == -7).all())                                                 # nothing was launched


@pytest.mark.parametrize("name", ["s", "as"])
def test_eer_of_the_counts_is_the_exact_eer(corpus, name):
    kind, topk = KINDS[name]
    k = corpus[name]
    ht, hn = sn.normalised_histograms(corpus["X"], corpus["X"], corpus["lab"], corpus["lab"], corpus["C"], kind=kind, topk=topk, self_offset=0,
                                      lo=k["lo"], hi=k["hi"])
    eer_h, eer_x = eer_from_histograms(ht, hn), _exact_eer(corpus, name)
    print(f"{name}: binned EER {eer_h:.6f}, exact EER {eer_x:.6f}, difference {abs(eer_h - eer_x):.2e}")
    assert 0.01 < eer_x < 0.4 and abs(eer_h - eer_x) < 5e-4, (eer_h, eer_x)


def test_multi_pass_bins(corpus):
    k, nf = corpus["s"], 2 * (NB - 2)
    ht, hn = sn.normalised_histograms(corpus["X"], corpus["X"], corpus["lab"], corpus["lab"], corpus["C"], kind="s", self_offset=0,
                                      lo=k["lo"], hi=k["hi"], bins=nf)
    assert ht.shape == hn.shape == (16380,)
    total, eer_h, eer_x = int(ht.sum() + hn.sum()), eer_from_histograms(ht, hn), _exact_eer(corpus, "s")
    print(f"two passes: {total} of {N * N - N} pairs, binned EER {eer_h:.6f}, exact EER {eer_x:.6f}")
    assert total == N * N - N                                      # the passes are joined on cumulative counts: a slice boundary loses nothing
    assert abs(eer_h - eer_x) < 5e-4, (eer_h, eer_x)


class _Spy:
    """Stands where ``_lib.lib()`` stands and notes every entry point that is asked for."""

    def __init__(self, lib, seen):
        self._lib, self._seen = lib, seen

    def __getattr__(self, name):
        self._seen.append(name)
        return getattr(self._lib, name)


def test_rejected_inputs_raise_before_any_launch(gpu, corpus, monkeypatch):
    x, lab = corpus["X"][:64], corpus["lab"][:64]
    mean, ones = torch.zeros(64, device=gpu), torch.ones(64, device=gpu)
    reached, lib = [], _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: _Spy(lib, reached))
    for bad in (0.0, float("inf")):
        std = ones.clone()
        std[17] = bad
        with pytest.raises(ValueError, match="finite and > 0"):
            iv_scoring.cosine_histograms(x, x, lab, lab, self_offset=0, lo=-8.0, hi=8.0, enroll_norm=(mean, std))
        with pytest.raises(ValueError, match="finite and > 0"):
            iv_scoring.cosine_histograms(x, x, lab, lab, self_offset=0, lo=-8.0, hi=8.0, enroll_norm=(mean, ones), test_norm=(mean, std))
    with pytest.raises(ValueError, match="64 rows"):
        iv_scoring.cosine_histograms(x, x, lab, lab, self_offset=0, lo=-8.0, hi=8.0, test_norm=(mean[:63], ones[:63]))
    assert reached == []                                             # no entry point of the library: nothing was launched, nothing written


def _driver(capsys, extra):
    from sidekit_amd.bin import shard_extract_score
    shard_extract_score.main(["--utterances", "1600", "--trials", "250", "--batch", "64", "--seconds", "1", "--all-pairs"] + extra)
    return json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])


def test_sharded_driver_reports_the_normalised_eer(gpu, capsys):
    plain = _driver(capsys, [])
    d = _driver(capsys, ["--all-pairs-norm", "as", "--norm-cohort", "300", "--norm-topk", "50"])
    assert d["all_pairs_norm"] == 1300 * 1299 and d["all_pairs_norm_kind"] == "as" and d["all_pairs_norm_cohort"] == 300
    assert 0.0 <= d["all_pairs_norm_eer"] < 0.3, d["all_pairs_norm_eer"]
    lo, hi = d["all_pairs_norm_hist_range"]
    assert lo < hi and d["all_pairs_norm_s"] > 0.0
    for key in ("all_pairs", "all_pairs_eer", "all_pairs_hist_range"):
        assert d[key] == plain[key], key
    assert not any(key.startswith("all_pairs_norm") for key in plain)
