"""What tests/test_hist_bins_cpu.py and tests/test_gpu_hist_bins.py share: the binning of the four all-pairs histogram kernels restated in
numpy in each kernel's own precision, the pass geometry of ``iv_scoring._histogram_passes``, score sets designed to sit on everything that
can go wrong (slice boundaries, ``lo``, ``hi``, bin edges, the far outside, signed zeros, values that are not finite), and operands whose
scores are exactly those values.

One pass (``scoring.hip``): ``x = (v - lo) * inv_width`` with ``inv_width = HB / (hi - lo)``, all in float32 for cosine scores
(``lo``, ``hi`` rounded to float32 by the C ABI) and in float64 for PLDA; bin 0 for ``x < 0``, bin ``HB - 1`` for ``x >= HB``, else
``floor(x)``.  Scores that are not finite: in the PLDA kernel a NaN has no bin, a raw infinity lands in an end bin and a normalised score
that is not finite has no bin.  The cosine kernel converts ``floorf(x)`` to ``int`` BEFORE it clamps, which C++ leaves undefined for a NaN,
an infinity or a value past the int range; the hardware conversion saturates and makes 0 of a NaN, so today an infinity lands in an end
bin and a NaN in bin 0, normalised or not.  ``bin_one_pass`` restates that as it is; the defined form was measured and cost too much.

Several passes: ``fine_bins`` places every score by itself, with no histogram in between -- the slice is the first whose upper boundary
the score lies under according to EITHER neighbouring pass, the bin is that pass's, held to its inner bins.  ``histogram_passes_today``
is the composition as it stood before (inner bins copied side by side), kept to show what it lost."""
import os
import re

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HB = 8192
INNER = HB - 2
NEIGHBOURS = 16
COPIES = 2                                                                            # of every score in each histogram of ``operands``

# the text of the kernels' binning in sidekit_amd/csrc/scoring.hip that bin_one_pass restates: (pattern, how often it stands there)
KERNEL_TEXT = (
    (r"constexpr int HB = 8192;", 1),
    (r"int bin = \(int\)floorf\(\(v - lo\) \* inv_width\);", 1),
    (r"bin = bin < 0 \? 0 : \(bin >= HB \? HB - 1 : bin\);", 1),
    (r"\(float\)HB / \(hi - lo\)", 1),
    (r"const double x = \(v - lo\) \* inv_width;", 1),
    (r"const int bin = x < 0\.0 \? 0 : \(x >= \(double\)HB \? HB - 1 : \(int\)x\);", 1),
    (r"\(double\)HB / \(hi - lo\)", 1),
    (r"if constexpr \(NORM == HN_NONE\) \{ if \(x != x\) continue; \}", 1),
    (r"else \{ if \(!\(x - x == 0\.0\)\) continue; \}", 1),
)


def kernel_text_counts():
    """How often each pattern of ``KERNEL_TEXT`` stands in scoring.hip, beside how often it should."""
    with open(os.path.join(ROOT, "sidekit_amd", "csrc", "scoring.hip")) as f:
        text = f.read()
    return [(pattern, len(re.findall(pattern, text)), count) for pattern, count in KERNEL_TEXT]


# ---- one pass -----------------------------------------------------------------------------------------------------------------------
def bin_one_pass(v, lo, hi, dtype, normalised=False):
    """``(bins, counted)`` of scores ``v`` in one ``HB``-bin pass over ``[lo, hi)`` in the kernel's precision ``dtype`` (float32: the cosine
    kernel, float64: the PLDA kernel).  ``counted`` is False where the kernel leaves the score out; its bin is then meaningless."""
    ft = numpy.dtype(dtype).type
    v = numpy.asarray(v, dtype=ft)
    lo, hi = ft(lo), ft(hi)                                                           # what the C ABI hands the launch
    with numpy.errstate(all="ignore"):
        inv_width = ft(HB) / (hi - lo)
        x = (v - lo) * inv_width
        assert x.dtype == ft and type(inv_width) is ft
        b = numpy.where(x < 0, 0.0, numpy.where(x >= HB, HB - 1.0, numpy.floor(x)))   # clamped in float or after a saturating conversion: the same bin
        if ft is numpy.float32:                                                       # the cosine kernel: (int)floorf(NaN) is 0 on this hardware
            counted = numpy.ones(x.shape, dtype=bool)
        else:
            counted = numpy.isfinite(x) if normalised else ~numpy.isnan(x)
    return numpy.where(numpy.isnan(x), 0, b).astype(numpy.int64), counted


def one_pass_histogram(v, dtype, normalised=False):
    """A numpy ``one_pass(a, b)`` for ``_histogram_passes``: both histograms are that of ``v``, every score counted once."""
    def one_pass(a, b):
        bins, counted = bin_one_pass(v, a, b, dtype, normalised)
        h = numpy.bincount(bins[counted], minlength=HB).astype(numpy.uint64)
        return h, h.copy()
    return one_pass


# ---- several passes -----------------------------------------------------------------------------------------------------------------
def pass_geometry(lo, hi, bins):
    """``(w, ranges, boundaries)``: the fine bin width, the ``(a - w, a + 8191 w)`` every pass is run over and the slice boundaries
    between neighbouring passes, in the float64 expressions of ``_histogram_passes``."""
    assert bins % INNER == 0
    w = (float(hi) - float(lo)) / bins
    starts = [float(lo) + k * INNER * w for k in range(bins // INNER)]
    return w, [(a - w, a + (INNER + 1) * w) for a in starts], starts[1:]


def histogram_passes_today(one_pass, lo, hi, bins):
    """The composition before the fix: every pass's inner bins side by side, the outer guards of the first and last pass added."""
    w, ranges, _ = pass_geometry(lo, hi, bins)
    out_t, out_n = numpy.zeros(bins, dtype=numpy.uint64), numpy.zeros(bins, dtype=numpy.uint64)
    for k, (a, b) in enumerate(ranges):
        ht, hn = one_pass(a, b)
        for full, part in ((out_t, ht), (out_n, hn)):
            full[k * INNER:(k + 1) * INNER] = part[1:-1]
            if k == 0:
                full[0] += part[0]
            if k == len(ranges) - 1:
                full[-1] += part[-1]
    return out_t, out_n


def pass_bins(v, lo, hi, bins, dtype, normalised=False):
    """``(P, n)`` bins of every score in every pass, and which scores are counted (the same in every pass for the designed sets)."""
    _, ranges, _ = pass_geometry(lo, hi, bins)
    per = [bin_one_pass(v, a, b, dtype, normalised) for a, b in ranges]
    counted = per[0][1]
    assert all(numpy.array_equal(c, counted) for _, c in per)
    return numpy.stack([b for b, _ in per]), counted


def fine_bins(v, lo, hi, bins, dtype, normalised=False):
    """``(fine bin, counted)`` of every score under the fixed composition, score by score.  ``bins == HB``: the one pass itself."""
    if bins == HB:
        return bin_one_pass(v, lo, hi, dtype, normalised)
    b, counted = pass_bins(v, lo, hi, bins, dtype, normalised)
    P, n = b.shape
    slice_of = numpy.full(n, P - 1)
    for k in range(P - 2, -1, -1):                                                    # under boundary k + 1 if either neighbour says so
        under = (b[k] <= INNER) | (b[k + 1] == 0)
        slice_of[under] = k
    own = b[slice_of, numpy.arange(n)]
    return slice_of * INNER + numpy.clip(own, 1, INNER) - 1, counted


def boundary_disputes(v, lo, hi, bins, dtype):
    """Per slice boundary ``(dropped, doubled)``: the scores of ``v`` that neither neighbouring pass has in an inner bin on its side of
    the boundary, and those that both have."""
    b, counted = pass_bins(v, lo, hi, bins, dtype)
    out = []
    for k in range(b.shape[0] - 1):
        out.append((int((counted & (b[k] == HB - 1) & (b[k + 1] == 0)).sum()), int((counted & (b[k] <= INNER) & (b[k + 1] >= 1)).sum())))
    return out


def float64_bins(v, lo, hi, bins):
    """``clamp(floor((v - lo) / w), 0, bins - 1)`` in float64: where a score belongs, to within the rounding of the kernel's precision."""
    v = numpy.asarray(v, dtype=numpy.float64)
    w = (float(hi) - float(lo)) / bins
    with numpy.errstate(all="ignore"):
        return numpy.clip(numpy.floor((v - float(lo)) / w), 0, bins - 1).astype(numpy.int64)


# ---- the designed scores ------------------------------------------------------------------------------------------------------------
def neighbours(x, dtype, n=NEIGHBOURS):
    """``x`` rounded to ``dtype`` with its ``n`` neighbours on either side, ascending."""
    ft = numpy.dtype(dtype).type
    c = ft(x)
    down, up = [c], [c]
    for _ in range(n):
        down.append(numpy.nextafter(down[-1], ft(-numpy.inf)))
        up.append(numpy.nextafter(up[-1], ft(numpy.inf)))
    return numpy.array(down[:0:-1] + up, dtype=ft)


def designed_scores(lo, hi, bins, dtype):
    """Finite scores for the grid ``(lo, hi, bins)``: every slice boundary, ``lo`` and ``hi`` with 16 neighbours either side; a few
    fine-bin edges inside slices with 4; values well outside on both sides; both zeros (an edge of the (-1, 1) grids); 1, which the row
    shard's two extra rows score.  Sorted; a value appears once."""
    ft = numpy.dtype(dtype).type
    w = (float(hi) - float(lo)) / bins
    span = float(hi) - float(lo)
    boundaries = pass_geometry(lo, hi, bins)[2] if bins != HB else []
    parts = [neighbours(x, dtype) for x in boundaries + [float(lo), float(hi)]]
    for k in range(min(bins // INNER if bins != HB else 1, 3)):                       # bin edges inside slices: near both ends and mid-way
        for j in (1, 2, 4097, INNER - 1):
            parts.append(neighbours(float(lo) + (k * INNER + j) * w, dtype, 4))
    far = 1e30 if ft is numpy.float32 else 1e300
    parts.append(numpy.array([lo - 3 * span, lo - 1e3 * span, -far, hi + 3 * span, hi + 1e3 * span, far, 0.0, 1.0, lo + 0.3 * span], dtype=ft))
    v = numpy.unique(numpy.concatenate(parts))
    assert numpy.isfinite(v).all()
    v[v == 0] = 0.0                                                                   # unique keeps one zero: make it +0.0, add -0.0
    return numpy.concatenate([v, numpy.array([-0.0], dtype=ft)])


NOT_FINITE = (numpy.inf, -numpy.inf, numpy.nan)


# ---- operands whose scores are those values -----------------------------------------------------------------------------------------
def operands(scores, dtype, shard_at=None):
    """``(E, T, le, lt, self_offset)`` with D = 4: enrolment rows ``[1, 0, 0, 0]`` labelled 0 and 1, test rows ``[s, 0, 0, 0]``, every
    score once under label 0 and once under label 1, so that each of the two histograms receives every score ``COPIES`` = 2 times (as a
    target of the enrolment row with its label, as a non-target of the other).  ``1 s + 0 + 0 + 0``
    is exact on the matrix cores in either precision; for PLDA take ``Phi = 0``, ``Psi = I``, ``cst = 0``.

    ``shard_at = k``: two more test rows ``[1, 0, 0, 0]`` (labels 0, 1) stand at rows ``k`` and ``k + 1``, the enrolment side is exactly
    those two rows and ``self_offset = k``.  Each meets the other as a non-target of score 1 and itself as the target that is dropped."""
    ft = numpy.dtype(dtype).type
    s = numpy.asarray(scores, dtype=ft)
    col = numpy.concatenate([s, s])
    lt = numpy.concatenate([numpy.zeros(len(s), dtype=numpy.int32), numpy.ones(len(s), dtype=numpy.int32)])
    if shard_at is not None:
        col = numpy.concatenate([col[:shard_at], numpy.ones(2, dtype=ft), col[shard_at:]])
        lt = numpy.concatenate([lt[:shard_at], numpy.array([0, 1], dtype=numpy.int32), lt[shard_at:]])
    T = numpy.zeros((len(col), 4), dtype=ft)
    T[:, 0] = col
    E = numpy.zeros((2, 4), dtype=ft)
    E[:, 0] = 1
    if shard_at is not None:
        assert numpy.array_equal(T[shard_at:shard_at + 2], E)
    return E, T, numpy.array([0, 1], dtype=numpy.int32), lt, shard_at


def expected_histogram(scores, lo, hi, bins, dtype, normalised=False):
    """What each of the two histograms of ``operands(scores)`` must be under the restatement: ``bins`` uint64 counts, ``COPIES`` per score."""
    fb, counted = fine_bins(scores, lo, hi, bins, dtype, normalised)
    return COPIES * numpy.bincount(fb[counted], minlength=bins).astype(numpy.uint64)
