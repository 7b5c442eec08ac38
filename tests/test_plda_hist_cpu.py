"""All-pairs PLDA histograms without a GPU: the declaration and the argument checks of sc_plda_hist, the checks of
iv_scoring.plda_histograms that run before any device is touched, the host algebra it hands to the device with a channel sub-space, and
the driver's --all-pairs-plda control flow on gloo ranks with a stand-in scoring module."""
import inspect
import json
import os
import re

import numpy
import pytest
import torch
import torch.multiprocessing as mp

import sidekit_amd
from sidekit_amd import _lib, iv_scoring

from test_sharding_cpu import _BandEnergyXtractor, _CpuScoring, _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_sc_plda_hist_is_declared_exported_and_bound():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "sidekit_amd.h")).read())
    want = ("int sc_plda_hist(const double* d_E, int32_t Ne, const double* d_T, int32_t Nt, int32_t D, const double* d_Phi, const double* d_Psi, "
            "double cst, double scaling, const int32_t* d_labels_e, const int32_t* d_labels_t, int32_t self_offset, double lo, double hi, "
            "int32_t nbins, uint64_t* d_hist_tar, uint64_t* d_hist_non, void* stream);")
    assert want in text
    assert "iv_scoring.py:448-462" in text[text.index("All-pairs PLDA scoring"):text.index("int sc_plda_hist(")]
    res, args = _lib.SIGNATURES["sc_plda_hist"]
    assert len(args) == 18 and [args[i] for i in (7, 8, 12, 13)] == [_lib._F64] * 4
    assert _lib.lib().sc_plda_hist.argtypes == args
    for name in ("plda_histograms", "plda_range_from_sample"):
        assert sidekit_amd._LAZY[name] == "iv_scoring" and getattr(sidekit_amd, name) is getattr(iv_scoring, name)
        assert name in iv_scoring.__doc__
    p = inspect.signature(iv_scoring.plda_histograms).parameters
    assert list(p) == ["enroll_vectors", "test_vectors", "enroll_labels", "test_labels", "mu", "F", "Sigma", "G", "scaling_factor", "self_offset",
                       "lo", "hi", "bins", "device"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is None for k in ("lo", "hi", "bins", "device"))
    assert list(inspect.signature(iv_scoring.plda_range_from_sample).parameters) == ["enroll_vectors", "test_vectors", "mu", "F", "Sigma", "G",
                                                                                      "scaling_factor", "device"]


def test_sc_plda_hist_argument_errors_return_before_any_device_call():
    lib, EARG = _lib.lib(), _lib.SK_EARG
    ok = [1, 4, 1, 4, 8, 1, 1, 0.0, 1.0, 1, 1, -1, -1.0, 1.0, 8192, 1, 1, None]          # non-null stand-ins: never dereferenced

    def call(**change):
        a = list(ok)
        for k, v in change.items():
            a[int(k[1:])] = v
        return lib.sc_plda_hist(*a)

    for pointer in (0, 2, 5, 6, 9, 10, 15, 16):
        assert call(**{f"a{pointer}": None}) == EARG and "sc_plda_hist" in _lib.last_error(), pointer
    for size in (1, 3, 4):
        assert call(**{f"a{size}": 0}) == EARG and call(**{f"a{size}": -3}) == EARG
    for nbins in (4096, 8190, 0):
        assert call(a14=nbins) == EARG and "nbins must be 8192" in _lib.last_error()
    assert call(a12=1.0, a13=1.0) == EARG and "hi > lo" in _lib.last_error()
    assert call(a12=2.0, a13=1.0) == EARG
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(a12=bad) == EARG and "finite" in _lib.last_error()
        assert call(a13=bad) == EARG


@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to pick a device fails the test: the checks under test come first."""
    def touched(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(iv_scoring, "_device", touched)


def _model(D=8, rank=3, grank=2, seed=0):
    rs = numpy.random.RandomState(seed)
    A = rs.randn(D, D)
    return rs.randn(D), rs.randn(D, rank), A @ A.T + D * numpy.eye(D), rs.randn(D, grank)


def test_plda_histograms_checks_fire_before_any_device_call(no_device):
    mu, F, Sigma, G = _model()
    x, t = numpy.zeros((5, 8)), numpy.zeros((6, 8))
    le, lt = numpy.zeros(5, dtype=numpy.int32), numpy.zeros(6, dtype=numpy.int32)
    rng = dict(lo=-30.0, hi=20.0)
    H = iv_scoring.plda_histograms
    for missing in ({}, {"lo": -30.0}, {"hi": 20.0}):
        with pytest.raises(ValueError, match="lo and hi are required"):
            H(x, t, le, lt, mu, F, Sigma, **missing)
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.0, float("inf"))):
        with pytest.raises(ValueError, match="hi must exceed lo"):
            H(x, t, le, lt, mu, F, Sigma, lo=lo, hi=hi)
    with pytest.raises(TypeError):
        H(x, t, le, lt, mu, F, Sigma, None, 1.0, None, -30.0, 20.0)                       # lo / hi are keywords
    with pytest.raises(ValueError, match="bins must be 8192 or a multiple of 8190"):
        H(x, t, le, lt, mu, F, Sigma, bins=4096, **rng)
    for e2, t2 in ((numpy.zeros(8), t), (x, numpy.zeros((6, 8, 1))), (x, numpy.zeros((6, 9)))):
        with pytest.raises(ValueError, match="matrices of one width"):
            H(e2, t2, le, lt, mu, F, Sigma, **rng)
    for m2, F2, S2, G2 in ((mu[:7], F, Sigma, None), (mu, F[:7], Sigma, None), (mu, F, Sigma[:7], None), (mu, F, Sigma[:, :7], None),
                           (mu, F, Sigma, G[:7])):
        with pytest.raises(ValueError, match="the vectors are 8 wide"):
            H(x, t, le, lt, m2, F2, S2, G2, **rng)
    with pytest.raises(ValueError, match="enrolment side has 5 rows"):
        H(x, t, lt, lt, mu, F, Sigma, **rng)
    with pytest.raises(ValueError, match="test side has 6 rows"):
        H(x, t, le, numpy.zeros((6, 1), dtype=numpy.int32), mu, F, Sigma, **rng)
    for k, name in enumerate(("mu", "F", "Sigma", "G")):
        for bad in (numpy.nan, numpy.inf):
            model = [v.copy() for v in (mu, F, Sigma, G)]
            model[k].flat[1] = bad
            with pytest.raises(ValueError, match=f"{name} is not finite"):
                H(x, t, le, lt, model[0], model[1], model[2], model[3], **rng)
    with pytest.raises(ValueError, match="matrices of one width"):
        iv_scoring.plda_range_from_sample(x, numpy.zeros((6, 9)), mu, F, Sigma)
    with pytest.raises(ValueError, match="Sigma is not finite"):
        iv_scoring.plda_range_from_sample(x, t, mu, F, Sigma * numpy.nan)


def test_without_a_gpu_the_error_is_the_usual_one_once_the_checks_pass():
    assert not torch.cuda.is_available()
    mu, F, Sigma, _ = _model()
    x, lab = numpy.zeros((5, 8)), numpy.zeros(5, dtype=numpy.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        iv_scoring.plda_histograms(x, x, lab, lab, mu, F, Sigma, lo=-1.0, hi=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        iv_scoring.plda_range_from_sample(x, x, mu, F, Sigma)


def test_channel_subspace_hands_on_the_algebra_of_full_plda_scoring(monkeypatch):
    """What reaches the device call with ``G`` given is what ``full_PLDA_scoring`` hands to ``plda_matrix``: both sides centred and
    projected by ``B``, ``(Phi, Psi, constant)`` of ``full_plda_parameters``, the scaling factor; without ``G``, ``fast_PLDA_scoring``'s."""
    from sidekit_amd import backend
    from sidekit_amd.bosaris import Ndx
    from sidekit_amd.statserver import StatServer
    z = numpy.load(os.path.join(GOLD, "scoring.npz"))
    enroll, test, mu, F, G, Sigma = (z[k].astype(numpy.float64) for k in ("E", "T", "mu", "F", "G", "Sigma"))
    ne, nt = enroll.shape[0], test.shape[0]
    le, lt = numpy.arange(ne, dtype=numpy.int32) % 5, numpy.arange(nt, dtype=numpy.int32) % 5
    ids = lambda prefix, n: numpy.array([f"{prefix}{i:03d}" for i in range(n)], dtype=object)
    e_srv, t_srv = StatServer.from_arrays(ids("m", ne), ids("m", ne), enroll), StatServer.from_arrays(ids("s", nt), ids("s", nt), test)
    ndx = Ndx()                                                      # check_missing=False: the Ndx is only passed through
    ndx.modelset, ndx.segset, ndx.trialmask = ids("m", ne), ids("s", nt), numpy.ones((ne, nt), dtype=bool)
    matrix_calls, hist_calls = [], []

    def fake_matrix(e, t, Phi, Psi, cst, scaling_factor=1., device=None):
        matrix_calls.append((numpy.array(e), numpy.array(t), numpy.array(Phi), numpy.array(Psi), float(cst), float(scaling_factor)))
        return numpy.zeros((e.shape[0], t.shape[0]))

    def fake_pass(e, t, le_d, lt_d, phi, psi, cst, scaling_factor, self_offset, lo, hi, device):
        hist_calls.append((e.numpy(), t.numpy(), phi.numpy(), psi.numpy(), float(cst), float(scaling_factor), le_d.numpy(), lt_d.numpy(), self_offset, lo, hi))
        h = numpy.zeros(iv_scoring.HIST_BINS, dtype=numpy.uint64)
        return h, h.copy()

    monkeypatch.setattr(iv_scoring, "plda_matrix", fake_matrix)
    monkeypatch.setattr(iv_scoring, "_plda_hist_pass", fake_pass)
    monkeypatch.setattr(iv_scoring, "_device", lambda device: torch.device("cpu"))
    monkeypatch.setattr(backend, "whiten_rows_device", lambda x, m, R: x @ torch.as_tensor(R))   # the device projection, restated
    for scaling, g in ((1.0, G), (0.5, G), (0.5, None)):
        del matrix_calls[:], hist_calls[:]
        if g is None:
            iv_scoring.fast_PLDA_scoring(e_srv, t_srv, ndx, mu, F, Sigma, scaling_factor=scaling, check_missing=False)
        else:
            iv_scoring.full_PLDA_scoring(e_srv, t_srv, ndx, mu, F, g, Sigma, scaling_factor=scaling, check_missing=False)
        ht, hn = iv_scoring.plda_histograms(enroll, test, le, lt, mu, F, Sigma, g, scaling, 7, lo=-3.0, hi=5.0)
        assert ht.dtype == hn.dtype == numpy.uint64 and ht.shape == hn.shape == (iv_scoring.HIST_BINS,)
        (want,), (got,) = matrix_calls, hist_calls
        assert want[0].shape[1] == got[0].shape[1] == (F.shape[1] if g is not None else F.shape[0])
        for a, b in zip(want[:2], got[:2]):                      # centred (and projected: one matrix product either way) vectors
            assert a.shape == b.shape and numpy.allclose(a, b, rtol=1e-12, atol=1e-12 * numpy.abs(a).max())
        for a, b in zip(want[2:4], got[2:4]):                    # Phi, Psi: the same host function, the same bits
            assert numpy.array_equal(a, b)
        assert want[4:6] == got[4:6] == (want[4], scaling)
        assert numpy.array_equal(got[6], le) and numpy.array_equal(got[7], lt) and got[6].dtype == numpy.int32
        assert got[8:] == (7, -3.0, 5.0)
    # finer bins: two passes over the slices cosine_histograms would use
    del hist_calls[:]
    ht, _ = iv_scoring.plda_histograms(enroll, test, le, lt, mu, F, Sigma, lo=-8.0, hi=8.0, bins=2 * 8190)
    w = 16.0 / 16380
    assert ht.shape == (16380,) and [(c[9], c[10]) for c in hist_calls] == [(-8.0 - w, -8.0 + 8191 * w), (-8.0 + 8190 * w - w, -8.0 + 8190 * w + 8191 * w)]
    bad = enroll.copy()
    bad[3, 2] = numpy.inf
    with pytest.raises(ValueError, match="centred vectors are not finite"):
        iv_scoring.plda_histograms(bad, test, le, lt, mu, F, Sigma, lo=-8.0, hi=8.0)


# ---- the driver's --all-pairs-plda on gloo ranks -------------------------------------------------------------------------------
class _PldaHistScoring(_CpuScoring):
    """``_CpuScoring`` plus CPU stand-ins for ``plda_histograms`` / ``plda_range_from_sample`` that note, per call, the row range they were
    given (``LOG``: one JSON line per call)."""
    LOG = None

    @staticmethod
    def _scores(e, t, mu, F, Sigma):
        Phi, Psi, cst = iv_scoring.plda_parameters(mu, F, Sigma)
        m = torch.as_tensor(mu)
        return _CpuScoring.plda_matrix_device(e.double() - m, t.double() - m, Phi, Psi, cst).numpy()

    @staticmethod
    def plda_range_from_sample(e, t, mu, F, Sigma, G=None, scaling_factor=1., device=None):
        s = _PldaHistScoring._scores(e, t, mu, F, Sigma)
        s = s[~numpy.eye(s.shape[0], dtype=bool)]
        pad = 0.25 * (s.max() - s.min())
        return float(s.min() - pad), float(s.max() + pad)

    @staticmethod
    def plda_histograms(e, t, le, lt, mu, F, Sigma, G=None, scaling_factor=1., self_offset=None, *, lo=None, hi=None, bins=None, device=None):
        NB = iv_scoring.HIST_BINS
        s = _PldaHistScoring._scores(e, t, mu, F, Sigma)
        keep = numpy.ones(s.shape, dtype=bool)
        i = numpy.arange(s.shape[0])
        keep[i, i + self_offset] = False
        tar = le.numpy()[:, None] == lt.numpy()[None, :]
        b = numpy.clip(numpy.floor((s - lo) * (NB / (hi - lo))), 0, NB - 1).astype(numpy.int64)
        ht, hn = (numpy.bincount(b[keep & m], minlength=NB).astype(numpy.uint64) for m in (tar, ~tar))
        with open(_PldaHistScoring.LOG, "a") as f:
            f.write(json.dumps({"self_offset": self_offset, "rows": e.shape[0], "against": t.shape[0], "lo": lo, "hi": hi,
                                "first_row_is_corpus_row": bool(torch.equal(e[0], t[self_offset])), "counted": int(ht.sum() + hn.sum())}) + "\n")
        return ht, hn


_ARGS = ["--utterances", "192", "--batch", "16", "--seconds", "0.2", "--trials", "48", "--speakers", "12", "--plda-rank", "6", "--noise", "0.1",
         "--backend", "gloo", "--device", "cpu"]


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from sidekit_amd.bin import shard_extract_score
    _PldaHistScoring.LOG = os.path.join(out_dir, "calls.jsonl")
    out = shard_extract_score.main(_ARGS + ["--all-pairs-plda"], model=_BandEnergyXtractor(), scoring=_PldaHistScoring)
    assert (out is not None) == (rank == 0)
    if rank == 0:
        with open(os.path.join(out_dir, "three_ranks.json"), "w") as f:
            json.dump(out, f)


def test_driver_all_pairs_plda(tmp_path, monkeypatch, capsys):
    from sidekit_amd.bin import shard_extract_score
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    # without the flag plda_histograms is never looked up: a stand-in that has none (the one of tests/test_sharding_cpu.py) keeps working
    assert not hasattr(_CpuScoring, "plda_histograms") and not hasattr(_CpuScoring, "plda_range_from_sample")
    plain = shard_extract_score.main(_ARGS, model=_BandEnergyXtractor(), scoring=_CpuScoring)
    assert not any(k.startswith("plda_all_pairs") for k in plain) and "all_pairs" not in plain
    with pytest.raises(AttributeError, match="plda_"):
        shard_extract_score.main(_ARGS + ["--all-pairs-plda"], model=_BandEnergyXtractor(), scoring=_CpuScoring)
    with pytest.raises(SystemExit):
        shard_extract_score.main(_ARGS + ["--all-pairs-plda", "--plda-hist-range", "3", "3"], model=_BandEnergyXtractor(), scoring=_CpuScoring)
    assert "HI must exceed LO" in capsys.readouterr().err
    # one rank: every pair i != j once, an EER on the result line, the flag alone (no --all-pairs)
    monkeypatch.setattr(_PldaHistScoring, "LOG", str(tmp_path / "one.jsonl"))
    one = shard_extract_score.main(_ARGS + ["--all-pairs-plda"], model=_BandEnergyXtractor(), scoring=_PldaHistScoring)
    line = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    assert line["plda_all_pairs_eer"] == one["plda_all_pairs_eer"] and line["plda_all_pairs"] == 192 * 191
    assert 0.0 < one["plda_all_pairs_eer"] < 0.5 and one["plda_all_pairs_hist_bins"] == 8192 and "all_pairs_eer" not in one
    for k in ("cosine_eer", "plda_eer", "trials"):
        assert one[k] == plain[k], k
    (call,) = [json.loads(l) for l in open(tmp_path / "one.jsonl")]
    assert call["self_offset"] == 0 and call["rows"] == call["against"] == 192 and [call["lo"], call["hi"]] == one["plda_all_pairs_hist_range"]
    # three ranks: the shards' row ranges and self_offsets cover the corpus once, the counts are summed, the edges are rank 0's
    mp.spawn(_worker, args=(3, _free_port(), str(tmp_path)), nprocs=3, join=True)
    three = json.load(open(tmp_path / "three_ranks.json"))
    calls = sorted((json.loads(l) for l in open(tmp_path / "calls.jsonl")), key=lambda c: c["self_offset"])
    assert [(c["self_offset"], c["rows"]) for c in calls] == [(0, 64), (64, 64), (128, 64)]
    assert all(c["against"] == 192 and c["first_row_is_corpus_row"] and [c["lo"], c["hi"]] == three["plda_all_pairs_hist_range"] for c in calls)
    assert three["ranks"] == 3 and three["plda_all_pairs"] == sum(c["counted"] for c in calls) == 192 * 191
    assert three["plda_all_pairs_hist_range"] == one["plda_all_pairs_hist_range"] and three["plda_all_pairs_eer"] == one["plda_all_pairs_eer"]
    fixed = shard_extract_score.main(_ARGS + ["--all-pairs-plda", "--plda-hist-range", "-200", "100"], model=_BandEnergyXtractor(), scoring=_PldaHistScoring)
    assert fixed["plda_all_pairs_hist_range"] == [-200.0, 100.0] and fixed["plda_all_pairs"] == 192 * 191
