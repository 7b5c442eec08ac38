"""The four all-pairs histogram kernels (sc_cosine_hist, sc_cosine_hist_norm, sc_plda_hist, sc_plda_hist_norm; the normalised ones as z-,
t- and s-norm with means 0 and stds 1) on scores designed to sit where binning goes wrong: slice boundaries of the several-pass form,
``lo``, ``hi``, bin edges, the far outside, both zeros, values that are not finite (tests/tools/hist_bins.py).  The operands are made so
that the scores ARE those values (enrolment rows ``[1, 0, 0, 0]``, test rows ``[s, 0, 0, 0]``; PLDA with ``Phi = 0``, ``Psi = I``), every
score twice as a target and twice as a non-target, and every bin of both histograms is compared with the numpy restatement of the
kernel's binning in its own precision.

Several passes (``iv_scoring._histogram_passes``), asserted exactly:
  P1  each histogram sums to the number of scores one pass counts;
  P2  the bins are those of one non-decreasing function of the score: the cumulative count at a slice boundary is one number;
  P3  every score lies within one fine bin of ``clamp(floor((v - lo) / w), 0, bins - 1)`` taken in float64."""
import os
import sys

import numpy
import pytest
import torch

from sidekit_amd import iv_scoring

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import hist_bins as hb  # noqa: E402

pytestmark = pytest.mark.gpu
FORMS = (None, "z", "t", "s")
RANGES = {"cosine": ((-1.0, 1.0), (-0.35, 0.93)), "plda": ((-12.5, 9.25), (-7.3, 11.9))}     # the second: lo, hi and the scale all round
DTYPE = {"cosine": numpy.float32, "plda": numpy.float64}
C = hb.COPIES                                                                                  # of every score in each histogram
LOSSY = ((-1.0, 1.0, 8), (-1.0, 1.0, 3), (-0.35, 0.93, 3), (-12.5, 9.25, 2))                   # float32 grids of tests/test_hist_bins_cpu.py


def _histograms(gpu, kind, form, test_values, lo, hi, bins, shard_at=None, drop_self=True, scaling=1.0, passes=iv_scoring._histogram_passes):
    """Both histograms of ``hb.operands(test_values)`` from the entry point of ``kind`` / ``form`` through ``passes``."""
    E, T, le, lt, offset = hb.operands(test_values, DTYPE[kind], shard_at)
    e, t, le, lt = (torch.from_numpy(x).to(gpu) for x in (E, T, le, lt))
    offset = offset if drop_self else None
    stats = None
    if form is not None:
        side = lambda n: (torch.zeros(n, dtype=e.dtype, device=gpu), torch.ones(n, dtype=e.dtype, device=gpu))
        stats = (side(len(E)) if form in "zs" else (None, None)) + (side(len(T)) if form in "ts" else (None, None))
    if kind == "cosine":
        one_pass = lambda a, b: iv_scoring._hist_pass(iv_scoring.CosineScorer, (), e, t, le, lt, offset, a, b, gpu, stats)
    else:
        phi, psi = torch.zeros(4, 4, dtype=torch.float64, device=gpu), torch.eye(4, dtype=torch.float64, device=gpu)
        one_pass = lambda a, b: iv_scoring._plda_hist_pass(e, t, le, lt, phi, psi, 0.0, scaling, offset, a, b, gpu, stats)
    return passes(one_pass, lo, hi, bins)


@pytest.mark.parametrize("kind,form,rng", [(k, f, r) for k in RANGES for f in FORMS for r in RANGES[k]], ids=str)
def test_one_pass(gpu, kind, form, rng):
    (lo, hi), dtype = rng, DTYPE[kind]
    v = hb.designed_scores(lo, hi, hb.HB, dtype)
    ht, hn = _histograms(gpu, kind, form, v, lo, hi, hb.HB)
    want = hb.expected_histogram(v, lo, hi, hb.HB, dtype, normalised=form is not None)
    assert ht.dtype == hn.dtype == numpy.uint64 and ht.shape == hn.shape == (hb.HB,)
    assert numpy.array_equal(ht, want) and numpy.array_equal(hn, want) and int(want.sum()) == C * len(v)
    w, v64 = (hi - lo) / hb.HB, v.astype(numpy.float64)
    assert 20 < int((v64 < lo + w / 2).sum()) <= int(ht[0]) // C <= int((v64 < lo + 1.5 * w).sum())  # lo, its neighbours and all that lies under it
    assert 20 < int((v64 > hi - w / 2).sum()) <= int(ht[-1]) // C <= int((v64 > hi - 1.5 * w).sum()) # hi, its neighbours and all that lies above it
    assert int(ht[hb.bin_one_pass([0.0], lo, hi, dtype)[0][0]]) >= 2 * C                              # both zeros, one bin


@pytest.mark.parametrize("kind,rng,p", [(k, r, p) for k in RANGES for r in RANGES[k] for p in (2, 3, 8)], ids=str)
def test_several_passes(gpu, kind, rng, p):
    (lo, hi), dtype, bins = rng, DTYPE[kind], p * hb.INNER
    v = hb.designed_scores(lo, hi, bins, dtype)
    s, boundaries = numpy.sort(v), hb.pass_geometry(lo, hi, bins)[2]
    fb, counted = hb.fine_bins(v, lo, hi, bins, dtype)
    assert counted.all() and (numpy.diff(fb[numpy.argsort(v, kind="stable")]) >= 0).all()          # the restated placement is monotone
    assert int(numpy.abs(fb - hb.float64_bins(v, lo, hi, bins)).max()) <= 1                        # and within one bin of float64's
    want = C * numpy.bincount(fb, minlength=bins).astype(numpy.uint64)
    for form in FORMS:
        ht, hn = _histograms(gpu, kind, form, v, lo, hi, bins)
        assert ht.shape == hn.shape == (bins,)
        assert int(ht.sum()) == int(hn.sum()) == C * len(v), (form, int(ht.sum()), int(hn.sum()), C * len(v)) # P1
        for k in range(1, len(boundaries) + 1):                                                    # P2 at the boundaries
            under = int(ht[:k * hb.INNER].sum())
            assert under == int(hn[:k * hb.INNER].sum()) and under % C == 0 and 0 < under // C < len(v) and s[under // C - 1] < s[under // C]
        assert numpy.array_equal(ht, want) and numpy.array_equal(hn, want), form                   # P2 and P3: the restatement's bins


@pytest.mark.parametrize("lo,hi,p", LOSSY, ids=str)
def test_inner_bins_side_by_side_lose_scores_on_the_device_too(gpu, lo, hi, p):
    """The kernel's own passes, joined as they used to be: scores at the slice boundaries are missing, as many as the restatement says."""
    bins = p * hb.INNER
    v = hb.designed_scores(lo, hi, bins, numpy.float32)
    disputes = hb.boundary_disputes(v, lo, hi, bins, numpy.float32)
    lost = sum(a for a, _ in disputes) - sum(b for _, b in disputes)
    ht, hn = _histograms(gpu, "cosine", None, v, lo, hi, bins, passes=hb.histogram_passes_today)
    print(f"lo {lo}, hi {hi}, bins {bins}: {len(v)} scores, the old composition counts {int(ht.sum())}; (dropped, doubled) per boundary {disputes}")
    assert lost != 0 and int(ht.sum()) == int(hn.sum()) == C * (len(v) - lost)


@pytest.mark.parametrize("kind,form", [(k, f) for k in RANGES for f in FORMS], ids=str)
def test_scores_that_are_not_finite(gpu, kind, form):
    """PLDA: a NaN score is in no bin; a raw +-inf is in an end bin; a normalised score that is not finite has no bin.  A score overflows
    (rows of +-1.5e308 under ``scaling = 2``: the library's callers hand over finite vectors) or comes from a NaN row.

    Cosine (the test rows hold the values): TODAY'S placement, pinned as it is -- +-inf in the end bins and a NaN in bin 0, normalised or
    not.  It rests on an undefined conversion (``(int)floorf(x)`` before the clamp; the hardware's saturates and makes 0 of a NaN), and it
    is not the rule of the PLDA kernel; the defined form cost more than the parent's run-to-run spread (profiles/hist_bins_bench.json).
    Whoever makes the cosine kernel follow the rule changes the three lines marked below.

    Either way the other scores' counts do not change, in one pass and in two."""
    (lo, hi), dtype = RANGES[kind][0], DTYPE[kind]
    scale = 1.0 if kind == "cosine" else 2.0
    for bins in (hb.HB, 2 * hb.INNER):
        v = hb.designed_scores(lo, hi, bins, dtype)
        rows = v / dtype(scale)
        extra = numpy.array(hb.NOT_FINITE if kind == "cosine" else (1.5e308, -1.5e308, numpy.nan), dtype=dtype)
        with numpy.errstate(over="ignore"):
            assert numpy.array_equal(rows * dtype(scale), v) and numpy.array_equal(extra * dtype(scale), numpy.array(hb.NOT_FINITE, dtype=dtype), equal_nan=True)
        plain = hb.expected_histogram(v, lo, hi, bins, dtype)
        without = _histograms(gpu, kind, form, rows, lo, hi, bins, scaling=scale)
        ht, hn = _histograms(gpu, kind, form, numpy.concatenate([rows[:100], extra, rows[100:]]), lo, hi, bins, scaling=scale)
        assert numpy.array_equal(without[0], plain) and numpy.array_equal(without[1], plain)
        want = plain.copy()
        if kind == "cosine":                                                          # today's placement (an undefined conversion):
            want[0] += 2 * C                                                          #   -inf and the NaN
            want[-1] += C                                                             #   +inf
        elif form is None:
            want[0] += C
            want[-1] += C
        assert numpy.array_equal(ht, want) and numpy.array_equal(hn, want), (bins, int(ht.sum()), int(want.sum()))
        both = numpy.concatenate([v, numpy.array(hb.NOT_FINITE, dtype=dtype)])
        assert numpy.array_equal(want, hb.expected_histogram(both, lo, hi, bins, dtype, normalised=form is not None))


@pytest.mark.parametrize("kind", list(RANGES))
def test_a_row_shard_drops_its_self_trials_and_nothing_else(gpu, kind):
    """The enrolment side is two rows in the middle of the test side (``self_offset = len(v) + 7``; in three passes they lie in a later tile
    of the test side than the first): the two self-trials, targets of score 1, are what ``self_offset`` takes away, and nothing else."""
    (lo, hi), dtype = RANGES[kind][1], DTYPE[kind]
    for bins in (hb.HB, 3 * hb.INNER):
        v = hb.designed_scores(lo, hi, bins, dtype)
        at = len(v) + 7
        plain = hb.expected_histogram(v, lo, hi, bins, dtype)
        ones = hb.expected_histogram(numpy.ones(1, dtype=dtype), lo, hi, bins, dtype)          # 2 in the bin of a score of 1
        for form in FORMS:
            ht, hn = _histograms(gpu, kind, form, v, lo, hi, bins, shard_at=at)
            assert numpy.array_equal(ht, plain) and numpy.array_equal(hn, plain + ones), form
            ht, hn = _histograms(gpu, kind, form, v, lo, hi, bins, shard_at=at, drop_self=False)
            assert numpy.array_equal(ht, plain + ones) and numpy.array_equal(hn, plain + ones), form
