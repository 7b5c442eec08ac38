"""Finer bins from several passes of the 8192-bin histogram kernels, without a GPU: the numpy restatement of the kernels' binning
(tests/tools/hist_bins.py) drives the composition of the passes on scores designed to sit on slice boundaries, ``lo``, ``hi`` and bin
edges.

The composition as it stood (every pass's inner bins copied side by side) loses scores at slice boundaries: two neighbouring passes bin
with their own ``lo`` and scale and so round "is this score below the boundary" differently.  The shipped ``_histogram_passes`` must

  P1  conserve: each histogram sums to what one pass counts;
  P2  be one monotone binning: a higher score is never in a lower bin (so the cumulative count at a slice boundary is ONE number);
  P3  place every score within one fine bin of ``clamp(floor((v - lo) / w), 0, bins - 1)`` taken in float64.

The restated expressions are tied to sidekit_amd/csrc/scoring.hip by regular expression: whoever changes one there is sent here."""
import os
import sys

import numpy
import pytest

from sidekit_amd import iv_scoring

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import hist_bins as hb  # noqa: E402

# (lo, hi, passes): the four grids on which the loss was first counted (float32), then the ranges of the GPU tests in both precisions
LOSSY_F32 = ((-1.0, 1.0, 8), (-1.0, 1.0, 3), (-0.35, 0.93, 3), (-12.5, 9.25, 2))
GRIDS = [(lo, hi, p, numpy.float32) for lo, hi in ((-1.0, 1.0), (-0.35, 0.93), (-12.5, 9.25)) for p in (2, 3, 8)] + \
        [(lo, hi, p, numpy.float64) for lo, hi in ((-12.5, 9.25), (-57.75, 34.25), (-1.0, 1.0)) for p in (2, 3, 8)]


def test_the_restatement_is_the_kernels_text():
    assert hb.HB == iv_scoring.HIST_BINS and hb.INNER == iv_scoring.HIST_BINS - 2
    for pattern, found, want in hb.kernel_text_counts():
        assert found == want, f"scoring.hip: {pattern!r} stands there {found} times, not {want}: restate tests/tools/hist_bins.py with the kernel"


def test_pass_geometry_is_what_the_passes_are_handed():
    for lo, hi, p in LOSSY_F32:
        seen = []
        z = numpy.zeros(hb.HB, dtype=numpy.uint64)
        iv_scoring._histogram_passes(lambda a, b: (seen.append((a, b)), (z, z.copy()))[1], lo, hi, p * hb.INNER)
        w, ranges, boundaries = hb.pass_geometry(lo, hi, p * hb.INNER)
        assert seen == ranges and len(boundaries) == p - 1 and w == (hi - lo) / (p * hb.INNER)
    seen = []
    iv_scoring._histogram_passes(lambda a, b: (seen.append((a, b)), (z, z.copy()))[1], -3.0, 5.0, hb.HB)
    assert seen == [(-3.0, 5.0)]                                                      # one pass: the range itself


def test_one_pass_restatement_on_its_edges():
    """lo in bin 0, hi and above in the last bin, both zeros in one bin, what is not finite by each kernel's rule: PLDA (float64) leaves a NaN
    and a normalised infinity out; cosine (float32) counts everything, a NaN in bin 0 (an undefined conversion, pinned as the hardware does it)."""
    for dtype, lo, hi in ((numpy.float32, -1.0, 1.0), (numpy.float32, -0.35, 0.93), (numpy.float64, -12.5, 9.25), (numpy.float64, -1.0, 1.0)):
        ft = numpy.dtype(dtype).type
        cosine = ft is numpy.float32
        b, counted = hb.bin_one_pass([lo, hi, numpy.nextafter(ft(hi), ft(numpy.inf)), 0.0, -0.0, numpy.inf, -numpy.inf, numpy.nan], lo, hi, dtype)
        assert b[0] == 0 and b[1] == b[2] == hb.HB - 1 and b[3] == b[4] and b[5] == hb.HB - 1 and b[6] == 0 and b[7] == 0
        assert counted.tolist() == [True] * 7 + [cosine]
        _, counted = hb.bin_one_pass([0.0, numpy.inf, -numpy.inf, numpy.nan], lo, hi, dtype, normalised=True)
        assert counted.tolist() == [True, cosine, cosine, cosine]
    assert hb.bin_one_pass([0.0], -1.0, 1.0, numpy.float32)[0][0] == 4096


def test_the_old_composition_loses_scores_at_slice_boundaries():
    """On the four grids of the first count, in float32, on the designed scores: the total of the old composition is not the number of
    scores.  (-s shows the count per boundary.)"""
    for lo, hi, p in LOSSY_F32:
        bins = p * hb.INNER
        v = hb.designed_scores(lo, hi, bins, numpy.float32)
        disputes = hb.boundary_disputes(v, lo, hi, bins, numpy.float32)
        old = hb.histogram_passes_today(hb.one_pass_histogram(v, numpy.float32), lo, hi, bins)[0]
        lost = sum(d for d, _ in disputes) - sum(d for _, d in disputes)
        print(f"lo {lo}, hi {hi}, bins {bins}: {len(v)} scores, old total {int(old.sum())}; (dropped, doubled) per boundary {disputes}")
        assert int(old.sum()) == len(v) - lost
        assert int(old.sum()) != len(v)


@pytest.mark.parametrize("lo,hi,p,dtype", GRIDS, ids=lambda x: getattr(x, "__name__", str(x)))
def test_the_shipped_composition_counts_every_score_once(lo, hi, p, dtype):
    bins = p * hb.INNER
    v = hb.designed_scores(lo, hi, bins, dtype)
    got_t, got_n = iv_scoring._histogram_passes(hb.one_pass_histogram(v, dtype), lo, hi, bins)
    assert got_t.dtype == got_n.dtype == numpy.uint64 and got_t.shape == got_n.shape == (bins,)
    assert int(got_t.sum()) == int(got_n.sum()) == len(v)                             # P1
    fb, counted = hb.fine_bins(v, lo, hi, bins, dtype)
    assert counted.all()
    order = numpy.argsort(v, kind="stable")
    assert (numpy.diff(fb[order]) >= 0).all()                                         # P2: the score-by-score placement is monotone ...
    assert numpy.array_equal(got_t, numpy.bincount(fb, minlength=bins)) and numpy.array_equal(got_n, got_t)   # ... and the shipped counts are its
    _, _, boundaries = hb.pass_geometry(lo, hi, bins)
    s = numpy.sort(v)
    for k in range(1, len(boundaries) + 1):                                           # one cumulative count per slice boundary:
        under = int(got_t[:k * hb.INNER].sum())
        assert 0 < under < len(v) and s[under - 1] < s[under]                         # the cut falls between two different scores
    assert int(numpy.abs(fb - hb.float64_bins(v, lo, hi, bins)).max()) <= 1           # P3
    assert fb[v.astype(numpy.float64) >= hi].min() == bins - 1 and fb[v.astype(numpy.float64) < lo].max() == 0
    assert len(set(fb[v == 0])) == 1                                                  # -0.0 and +0.0 share a bin


def test_scores_that_are_not_finite_change_nothing_else():
    """Through several passes: what a pass leaves out is missing from the fine bins too, what it has in an end bin (in bin 0: the cosine
    kernel's NaN) is in the fine end bin, and the other scores' bins are what they were."""
    for dtype, lo, hi, bins in ((numpy.float32, -1.0, 1.0, 3 * hb.INNER), (numpy.float64, -12.5, 9.25, 2 * hb.INNER)):
        v = hb.designed_scores(lo, hi, bins, dtype)
        more = numpy.concatenate([v, numpy.array(hb.NOT_FINITE, dtype=dtype)])
        plain = iv_scoring._histogram_passes(hb.one_pass_histogram(v, dtype), lo, hi, bins)[0]
        raw = iv_scoring._histogram_passes(hb.one_pass_histogram(more, dtype), lo, hi, bins)[0]
        norm = iv_scoring._histogram_passes(hb.one_pass_histogram(more, dtype, normalised=True), lo, hi, bins)[0]
        ends = numpy.zeros(bins, dtype=numpy.uint64)
        ends[0] = ends[-1] = 1                                                        # the two infinities
        if dtype is numpy.float32:
            ends[0] += 1                                                              # the cosine kernel's NaN
            assert numpy.array_equal(raw, plain + ends) and numpy.array_equal(norm, plain + ends)
        else:
            assert numpy.array_equal(raw, plain + ends) and numpy.array_equal(norm, plain)
        assert numpy.array_equal(hb.COPIES * raw, hb.expected_histogram(more, lo, hi, bins, dtype))
        assert numpy.array_equal(hb.COPIES * norm, hb.expected_histogram(more, lo, hi, bins, dtype, normalised=True))


def test_a_pass_that_disagrees_in_either_direction_is_absorbed():
    """Hand-made passes, two slices: the upper pass's lower guard holds 3 more than the lower pass has under the boundary (dropped: into the
    last inner bin of slice 0), or 3 fewer (doubled: out of the upper pass's lowest occupied inner bins, 2 from one and 1 from the next)."""
    def passes(first, second):
        it = iter((first, second))
        return lambda a, b: (lambda h: (h, h.copy()))(next(it))
    z = lambda: numpy.zeros(hb.HB, dtype=numpy.uint64)
    bins = 2 * hb.INNER
    lower, upper = z(), z()
    lower[0], lower[5], lower[hb.INNER], lower[-1] = 2, 4, 1, 10 + 3                  # 7 under the boundary; 3 + 10 claimed above it
    upper[0], upper[7], upper[9], upper[-1] = 7 + 3, 5, 4, 1                          # 10 under it
    got = iv_scoring._histogram_passes(passes(lower, upper), 0.0, 1.0, bins)[0]
    want = numpy.zeros(bins, dtype=numpy.uint64)
    want[0], want[4], want[hb.INNER - 1], want[hb.INNER + 6], want[hb.INNER + 8], want[-1] = 2, 4, 1 + 3, 5, 4, 1
    assert numpy.array_equal(got, want) and int(got.sum()) == 20
    lower, upper = z(), z()
    lower[0], lower[5], lower[hb.INNER], lower[-1] = 2, 4, 1 + 3, 7                   # 10 under the boundary
    upper[0], upper[7], upper[9], upper[-1] = 7, 2, 4 + 3, 1                          # 7 under it: 3 counted twice
    got = iv_scoring._histogram_passes(passes(lower, upper), 0.0, 1.0, bins)[0]
    want = numpy.zeros(bins, dtype=numpy.uint64)
    want[0], want[4], want[hb.INNER - 1], want[hb.INNER + 8], want[-1] = 2, 4, 4, 6, 1
    assert numpy.array_equal(got, want) and int(got.sum()) == 17
