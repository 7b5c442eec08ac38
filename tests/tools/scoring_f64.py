"""Float64 references of the trial-scoring entry points one kernel at a time, on the operands each kernel actually reads (CPU only; torch +
numpy), the operands themselves, and the criteria tests/test_gpu_scoring_kernels.py judges the kernels by.  tests/test_scoring_reference_cpu.py
shows on the same operands that float32 evaluations of the formulas pass the criteria and that wrong kernels do not.

Written from csrc/scoring.hip (sc_cosine: launch_gemm's f32 MFMA kernels over k-tiles of BK = 32, 64 x 64 tiles, 128 x 128 ones from
M >= 2048 and N >= 128; cosine_trials_kernel: one wave per trial, four trials per workgroup, float64 FMA chains per lane and a butterfly),
csrc/pool.hip (normalize_rows_kernel: 256 threads stride a row, x / max(||x||, eps)) and csrc/score_norm.hip (topk_stats_kernel: a radix
select of the k-th largest key over 256-thread strides, then the sums of the keys above it and of the copies of the threshold that belong
to the k).  Each function takes what ONE entry point reads and returns the float64 (numpy.longdouble where the kernel itself computes in
float64) value and, where a bound needs it, ``S``: the same formula on absolute values.

Operands are NOT unit vectors: a row is randn x 2^uniform(-6, 6), its own scale, cast to float32, so that no absolute tolerance can hide
an error in a small row beside a large one.

Criteria (u = 2^-24):
    sc_cosine           |got - r| <= 2 K u S per element with K = D (the unpadded D), the NaN pattern of the reference, and a norm-relative
                        error of at most 16 x that of torch's float32 product (tdnn_f64.check_gemm)
    sc_normalize_rows   r = x / max(||x||, 1e-12); |got - r| <= (D + 4) u |r| (D squares in any order, a square root, a division); a zero row
                        gives exact zeros.  Row magnitudes are 2^uniform(-20, 20): there the float32 squares neither overflow nor underflow
                        (|x| < 2^23, x^2 D < 2^56; |x| > 2^-40 for all but a negligible share of a row's norm), which is the range the
                        kernel's float32 sum of squares is meant for; beyond it the bound does not hold and is not claimed.
    sc_cosine_trials    float64 arithmetic on float32 operands: r in numpy.longdouble, |got - r| <= 2 (D + 6) 2^-53 S / (||e|| ||t||); a zero
                        vector gives NaN, as numpy does
    sc_topk_stats[_f64] r_mean, r_std (ddof = 1) in numpy.longdouble on the k largest values, A = mean |those values|, u_T = 2^-24 for
                        float32 output and 0 for float64 output:  |mean - r_mean| <= u_T |r_mean| + (k + 2) 2^-53 A  and
                        |std - r_std| <= (u_T + (k + 8) 2^-52) r_std.  The std bound is what a centred evaluation sum (v - m)^2 meets; it
                        carries no conditioning term (mean^2 / var) on purpose: a one-pass sum v^2 - k m^2 cancels and does not meet it.
                        k equal values: the std is exactly 0 in float32 (k v and (k v) / k are exact in double) and at most 4 2^-52 |v|,
                        finite and non-negative, in float64 (the mean of k equal doubles may be off by an ulp).
"""
import os
import re

import numpy
import torch

import tdnn_f64 as tf

U32 = tf.U32
U64 = 2.0 ** -53
LD = numpy.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# ---- thresholds the shapes below assume (read_sources() reads them out of the sources) --------------------------------------------------
BK = 32                # k-tile of gemm_kernel / gemm128_kernel
TILE = 64              # rows and columns of gemm_kernel's tile
BIG_M, BIG_N = 2048, 128   # launch_gemm: 128 x 128 tiles from M >= 2048 and N >= 128
D_MULTIPLE = 4         # sc_cosine takes D % 4 == 0 only (cosine_matrix_device pads)
TOPK_STRIDE = 256      # topk_stats_kernel: threads per row
NORM_STRIDE = 256      # normalize_rows_kernel: threads per row
TRIALS_PER_WG = 4      # cosine_trials_kernel: one wave per trial

COSINE_SHAPES = [(1, 1, 4), (64, 64, 32), (65, 63, 36), (33, 130, 28), (129, 257, 64), (70, 70, 512), (2048, 128, 4), (2049, 129, 36)]
PAD_D = (1, 2, 3, 5, 150)
PAD_SHAPES = ((7, 5), (100, 77))
NORM_D = (1, 3, 100, 256, 257, 512, 1000)
NORM_ROWS, NORM_ZERO_ROW, NORM_TINY_ROW = 40, 5, 9
TRIAL_D = (1, 63, 64, 65, 100, 256, 600)
TRIAL_N = (1, 3, 4, 5, 1001)
TRIAL_ROWS_E, TRIAL_ROWS_T, TRIAL_ZERO_ROW = 9, 11, 4
TOPK_NCOLS = (2, 119, 256, 257, 1000)
TOPK_FAMILIES = {"float32": ("a", "b"), "float64": ("a", "b", "c")}
HIST_D, HIST_N = (36, 132), 300
# The std bound of the top-k statistics has no conditioning term.  A centred sum leaves k d^2 behind, d the error of the mean it is centred
# on: a relative (d / std)^2 of the variance.  d is a few ulps of the mean (2^-52 |mean|), so the term stays below 2^-52 while
# std >= 2^-24 |mean|; under that floor NO evaluation in float64 can be held to (k + 8) 2^-52, and a row there (two nearly tied best values at
# k = 2, for instance) is drawn again.  Family (c) itself is at std / mean = 2^-20.
STD_FLOOR = 2.0 ** -24


def _body(text, start):
    """the text from ``start`` to the first line that is a closing brace alone"""
    i = text.index(start)
    return text[i:text.index("\n}\n", i)]


def read_sources():
    """the thresholds above as the sources state them"""
    def src(name):
        with open(os.path.join(ROOT, "sidekit_amd", "csrc", name)) as f:
            return f.read()
    gemm, scoring, norm, pool = src("gemm.hip"), src("scoring.hip"), src("score_norm.hip"), src("pool.hip")
    bm, bn, bk = (int(v) for v in re.search(r"constexpr int BM = (\d+), BN = (\d+), BK = (\d+)", gemm).groups())
    assert bm == bn
    big = re.search(r"g\.ksplit == 1 && g\.M >= (\d+) && g\.N >= (\d+) && !g\.a_bf16", gemm)
    cosine = _body(scoring, "int sc_cosine(")
    assert "launch_gemm(g, (hipStream_t)stream)" in cosine
    topk = _body(norm, "void topk_stats_kernel(")
    strides = {int(v) for v in re.findall(r"i \+= (\d+)\)", topk)}
    launches = {int(v) for v in re.findall(r"topk_stats_kernel<\w+>, dim3\(n_rows\), dim3\((\d+)\)", norm)}
    assert len(strides) == 1 and strides == launches
    nrm = _body(pool, "void normalize_rows_kernel(")
    nstr = {int(v) for v in re.findall(r"d \+= (\d+)\)", nrm)}
    nlaunch = {int(v) for v in re.findall(r"normalize_rows_kernel, dim3\(B\), dim3\((\d+)\)", pool)}
    assert len(nstr) == 1 and nstr == nlaunch
    per = int(re.search(r"blockIdx\.x \* (\d+)L \+ \(threadIdx\.x >> 6\)", _body(scoring, "void cosine_trials_kernel(")).group(1))
    grid = re.search(r"\(n_trials \+ (\d+)\) / (\d+)\)\), dim3\((\d+)\)", _body(scoring, "int sc_cosine_trials("))
    assert (int(grid.group(1)) + 1, int(grid.group(2)), int(grid.group(3))) == (per, per, 64 * per)
    return {"BK": bk, "TILE": bm, "BIG_M": int(big.group(1)), "BIG_N": int(big.group(2)),
            "D_MULTIPLE": int(re.search(r"D % (\d+) == 0", cosine).group(1)), "TOPK_STRIDE": strides.pop(), "NORM_STRIDE": nstr.pop(),
            "TRIALS_PER_WG": per}


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
def rows(n, d, seed, lo=-6.0, hi=6.0):
    """[n][d] float32: randn x 2^uniform(lo, hi), one scale per row"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=torch.float64)
    s = torch.rand(n, 1, generator=g, dtype=torch.float64) * (hi - lo) + lo
    return (x * torch.pow(torch.tensor(2.0, dtype=torch.float64), s)).float()


def cosine_operands(ne, nt, d):
    return rows(ne, d, 1000 * ne + d), rows(nt, d, 1000 * nt + d + 1)


def padded(x, multiple=D_MULTIPLE):
    """x with zero columns up to the next multiple"""
    pad = -x.shape[1] % multiple
    return torch.nn.functional.pad(x, (0, pad)).contiguous()


def normalize_operands(d):
    """40 rows of magnitude 2^uniform(-20, 20); row 5 is zero; row 9 has norm 1e-15, below eps = 1e-12: the result is x / 1e-12"""
    x = rows(NORM_ROWS, d, 77 + d, -20.0, 20.0)
    x[NORM_ZERO_ROW] = 0.0
    tiny = torch.randn(d, generator=torch.Generator().manual_seed(78 + d), dtype=torch.float64)
    x[NORM_TINY_ROW] = (tiny * (1e-15 / tiny.norm())).float()
    return x


def trials_operands(d, n):
    """E [9][d] with row 4 zero, T [11][d], and n index pairs: trial 0 is (0, 0), trial n - 1 (8, 10), trial 1 names the zero row of E (n >= 3);
    the others are drawn with repeats from the rows that are not zero.  n = 1: the one trial is (8, 0)."""
    E, T = rows(TRIAL_ROWS_E, d, 300 + d), rows(TRIAL_ROWS_T, d, 301 + d)
    E[TRIAL_ZERO_ROW] = 0.0
    rs = numpy.random.RandomState(1000 * d + n)
    ok = numpy.array([i for i in range(TRIAL_ROWS_E) if i != TRIAL_ZERO_ROW])
    ei, ti = ok[rs.randint(0, len(ok), n)].astype(numpy.int32), rs.randint(0, TRIAL_ROWS_T, n).astype(numpy.int32)
    if n == 1:
        ei[0], ti[0] = TRIAL_ROWS_E - 1, 0
    else:
        ei[0], ti[0], ei[n - 1], ti[n - 1], ei[1] = 0, 0, TRIAL_ROWS_E - 1, TRIAL_ROWS_T - 1, TRIAL_ZERO_ROW
    return E, T, ei, ti


def topk_ks(ncols):
    return sorted({k for k in (2, 7, ncols - 1, ncols) if 1 < k <= ncols})


def topk_cases():
    return [(n, k) for n in TOPK_NCOLS for k in topk_ks(n)]


def _family(rs, family, n, ncols):
    if family == "a":      # both signs: what cosine cohorts look like
        return 0.3 * rs.standard_normal((n, ncols)) + rs.uniform(-1.0, 1.0, (n, 1))
    if family == "b":      # the magnitude of real PLDA / Mahalanobis score matrices
        return -600.0 + rs.standard_normal((n, ncols))
    assert family == "c"
    return 1e4 + 1e-2 * rs.standard_normal((n, ncols))


def topk_rows(ncols, k, family, dtype):
    """(x [R][ncols] of ``dtype``, names [R]): five rows of the family and the constructed rows that exist at (ncols, k), each built on a
    fresh row of the family and rounded to ``dtype`` BEFORE the copies are placed:
      straddle  the (k + 1)-th largest value is a copy of the k-th: a tie at the threshold with one copy on either side of the cut (k < ncols)
      strides   columns 3 and 700 -- different 256-column strides -- hold the same value, k - 1 others lie above it (ncols > 700, k < ncols)
      equal     the k best values are all equal
      zeros     k - 1 positive values, then +0.0 inside the cut and -0.0 outside it, the rest negative (family a, k < ncols)
      negative  an all-negative row (family a; family b is all negative anyway)
    A row whose k best values have a std below STD_FLOOR x their mean magnitude (and not exactly 0) is drawn again: see STD_FLOOR."""
    rs = numpy.random.RandomState(7919 * ncols + 31 * k + ord(family))
    dt = numpy.dtype(dtype)
    fresh = lambda: _family(rs, family, 1, ncols)[0].astype(dt)

    def straddle():
        x = fresh()
        order = numpy.argsort(-x, kind="stable")
        x[order[k]] = x[order[k - 1]]
        return x

    def strides():
        x = fresh()
        others = numpy.sort(numpy.delete(x, [3, 700]))[::-1]
        below = float(others[k - 1]) if k - 1 < len(others) else float(others[-1]) - 0.25      # k = ncols - 1: every other value lies above
        x[3] = x[700] = dt.type(0.5 * (float(others[k - 2]) + below))
        return x

    def equal():
        x = fresh()
        order = numpy.argsort(-x, kind="stable")
        x[order[:k]] = x[order[0]]
        return x

    def zeros():
        x = fresh()
        order = numpy.argsort(-x, kind="stable")
        x[order[:k - 1]] = numpy.abs(x[order[:k - 1]]) + dt.type(0.125)
        x[order[k + 1:]] = -numpy.abs(x[order[k + 1:]]) - dt.type(0.125)
        x[order[k - 1]], x[order[k]] = 0.0, -0.0
        return x

    plan = [("random", fresh)] * 5 + [("straddle", straddle)] * (k < ncols) + [("strides", strides)] * (ncols > 700 and k < ncols) + [("equal", equal)]
    if family == "a":
        plan += [("zeros", zeros)] * (k < ncols) + [("negative", lambda: -numpy.abs(fresh()) - dt.type(0.125))]
    out = []
    for _, build in plan:
        for _ in range(100):
            x = build()
            _, s, A = topk_ref(x[None], k)
            if s[0] == 0 or s[0] >= STD_FLOOR * A[0]:
                break
        else:
            raise AssertionError("no row of the family with a top-k std above the floor")
        out.append(x)
    return numpy.ascontiguousarray(numpy.stack(out)), [name for name, _ in plan]


# ---- references -------------------------------------------------------------------------------------------------------------------------
def cosine_ref(E, T):
    """(E . T' in float64, the same on absolute values)"""
    e, t = E.double(), T.double()
    return e @ t.T, e.abs() @ t.abs().T


def fma_chain(E, T):
    """E . T' as one float32 FMA per k in ascending k from a zero accumulator: what one accumulator of the f32 matrix cores computes
    (the product of two float32 is exact in double; the double sum is rounded to float32)"""
    e, t = E.numpy(), T.numpy()
    acc = numpy.zeros((e.shape[0], t.shape[0]), dtype=numpy.float32)
    for k in range(e.shape[1]):
        acc = (e[:, k, None].astype(numpy.float64) * t[None, :, k].astype(numpy.float64) + acc.astype(numpy.float64)).astype(numpy.float32)
    return torch.from_numpy(acc)


def normalize_ref(x):
    x = x.double()
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)


def trials_ref(E, T, ei, ti):
    """(r, bound): uv / (sqrt(uu) sqrt(vv)) in numpy.longdouble and 2 (D + 6) 2^-53 S / (||e|| ||t||); a zero vector gives NaN in both"""
    e, t = E.numpy().astype(LD)[ei], T.numpy().astype(LD)[ti]
    with numpy.errstate(invalid="ignore", divide="ignore"):
        den = numpy.sqrt((e * e).sum(1)) * numpy.sqrt((t * t).sum(1))
        r = (e * t).sum(1) / den
        bound = 2 * (E.shape[1] + 6) * LD(U64) * numpy.abs(e * t).sum(1) / den
    return r, bound


def topk_ref(x, k):
    """(mean, unbiased std, mean |v|) of the k largest values of every row, in numpy.longdouble"""
    v = -numpy.sort(-x.astype(LD), axis=1)[:, :k]
    m = v.sum(1) / k
    return m, numpy.sqrt(((v - m[:, None]) ** 2).sum(1) / (k - 1)), numpy.abs(v).sum(1) / k


# ---- criteria ---------------------------------------------------------------------------------------------------------------------------
def check_cosine(name, got, E, T):
    """sc_cosine's criterion on the UNPADDED operands (K = D).  Returns (norm-relative error, torch float32's, largest share of 2 K u S)."""
    r, S = cosine_ref(E, T)
    return tf.check_gemm(name, got, r, S, E.shape[1], None, E @ T.T)


def check_normalize(name, got, x):
    """Returns the largest |got - r| as a share of (D + 4) u |r|."""
    r = normalize_ref(x)
    got = got.double()
    assert got.shape == r.shape, f"{name}: shape {tuple(got.shape)}"
    zero = (x == 0).all(dim=1)
    assert bool((got[zero] == 0).all()), f"{name}: a zero row does not give exact zeros"
    bound = (x.shape[1] + 4) * U32 * r.abs()
    diff = (got - r).abs()
    assert bool((diff <= bound).all()), f"{name}: off by {(diff / bound)[bound > 0].max().item():.2f} of (D + 4) 2^-24 |r|"
    live = bound > 0
    return (diff[live] / bound[live]).max().item() if bool(live.any()) else 0.0


def check_trials(name, got, E, T, ei, ti):
    """Returns the largest |got - r| as a share of its bound over the trials that are not NaN."""
    r, bound = trials_ref(E, T, ei, ti)
    got = numpy.asarray(got, dtype=numpy.float64)
    assert got.shape == r.shape, f"{name}: shape {got.shape}"
    nan = numpy.isnan(r)
    zero = (E.numpy()[ei] == 0).all(1) | (T.numpy()[ti] == 0).all(1)
    assert numpy.array_equal(nan, zero), f"{name}: the reference is NaN exactly where a trial names a zero vector"
    assert numpy.array_equal(numpy.isnan(got), nan), f"{name}: NaN at trials {numpy.nonzero(numpy.isnan(got))[0][:8]}, expected at {numpy.nonzero(nan)[0][:8]}"
    if nan.all():
        return 0.0
    diff = numpy.abs(got.astype(LD) - r)[~nan]
    share = numpy.where(bound[~nan] > 0, diff / numpy.where(bound[~nan] > 0, bound[~nan], 1), numpy.where(diff == 0, 0.0, numpy.inf))
    assert (share <= 1).all(), f"{name}: off by {float(share.max()):.2f} of 2 (D + 6) 2^-53 S / (|e| |t|)"
    return float(share.max())


def topk_shares(mean, std, x, k):
    """(share of the mean's bound, share of the std's bound) per row; inf where a value that has to be exact is not, or is not finite"""
    rm, rs, A = topk_ref(x, k)
    uT = LD(U32) if x.dtype == numpy.float32 else LD(0)
    mean, std = numpy.asarray(mean).astype(LD), numpy.asarray(std).astype(LD)

    def share(diff, bound):
        with numpy.errstate(invalid="ignore", divide="ignore"):
            s = numpy.where(bound > 0, diff / numpy.where(bound > 0, bound, 1), numpy.where(diff == 0, 0.0, numpy.inf))
        return numpy.where(numpy.isfinite(s), s, numpy.inf).astype(numpy.float64)

    ms = share(numpy.abs(mean - rm), uT * numpy.abs(rm) + (k + 2) * LD(U64) * A)
    ss = share(numpy.abs(std - rs), (uT + (k + 8) * LD(2.0 ** -52)) * rs)
    equal = rs == 0                                                # the k best values are all equal
    if x.dtype == numpy.float64:
        ss[equal] = share(std, 4 * LD(2.0 ** -52) * numpy.abs(rm))[equal]
    ss[~(std >= 0)] = numpy.inf                                    # negative or NaN
    return ms, ss


def check_topk(name, mean, std, x, k, names=None):
    """Returns (largest share of the mean's bound, of the std's)."""
    ms, ss = topk_shares(mean, std, x, k)
    bad = numpy.nonzero(~((ms <= 1) & (ss <= 1)))[0]
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"{name}: {len(bad)} of {len(ms)} rows outside their bounds; row {i}" + (f" ({names[i]})" if names else "")
                             + f": mean {float(ms[i]):.3g} of its bound, std {float(ss[i]):.3g} of its bound; largest {float(ms.max()):.3g}, {float(ss.max()):.3g}")
    return float(ms.max()), float(ss.max())


# ---- float64 evaluations of the top-k statistics (stand-ins for the kernel on the CPU) --------------------------------------------------
def topk_eval(x, k, centred, select="topk", ddof=1):
    """The statistics in float64 numpy, cast to x's type.  ``centred``: sum (v - m)^2; otherwise the one-pass (sum v^2 - k m^2) / (k - 1)
    clamped at 0.  ``select`` names what is summed: "topk"; "k-1" (one value too few); "ties" (every copy of the threshold); "magnitude"
    (the k largest |x|: the order of keys whose negative half is not inverted); "first256" (only the first 256 columns are seen)."""
    mean, std = numpy.zeros(len(x)), numpy.zeros(len(x))
    for i, row in enumerate(x.astype(numpy.float64)):
        if select == "first256":
            row = row[:256]
        srt = -numpy.sort(-row)
        if select == "k-1":
            v = srt[:k - 1]
        elif select == "ties":
            v = srt[srt >= srt[min(k, len(srt)) - 1]]
        elif select == "magnitude":
            v = row[numpy.argsort(-numpy.abs(row), kind="stable")[:k]]
        else:
            v = srt[:k]
        m = v.sum() / k
        var = ((v - m) ** 2).sum() if centred else (v * v).sum() - k * m * m
        var = var / (k - ddof)
        mean[i], std[i] = m, numpy.sqrt(var if var > 0 else 0.0)
    return mean.astype(x.dtype), std.astype(x.dtype)
