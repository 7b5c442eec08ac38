"""numpy.longdouble references of the float64 back end one entry point at a time: the TN, NN and gathered-centre forms of csrc/dgemm_tile.h
behind sc_gemm_tn, sc_scatter_within, sc_class_scatter, sc_tv_gram, sc_dgemm_nn and sc_gauss_loglik, and sc_whiten_rows' tile of its own
on the same loaders.  Operands, references, criteria, the shapes, float64 numpy stand-ins of the kernels (with the wrong kernels the criteria must
reject) -- CPU only, numpy only.  tests/test_gpu_f64_forms.py judges the kernels by this file; tests/test_f64_forms_reference_cpu.py shows
on the same operands that a float64 numpy evaluation passes every criterion and that the wrong kernels do not.

Operands.  Every column of a TN operand (A [K][M], B [K][N], X [N][D] of the two scatters, F_c [D][R] of the Gram) is randn x 2^uniform(-6, 6),
a scale of its own; so is every row of the left operand and every column of the right one of the NN-shaped entry points (sc_dgemm_nn,
sc_whiten_rows, sc_gauss_loglik).  One norm over the matrix cannot hide an error in a small row or column then.  Float32 cases hold float32
values; the references widen exactly the arrays the kernel is handed (ca, cb, w, Mc, mu, means, W stay the float64 the kernel reads).
Centres are the column mean plus uniform(-1, 1) x the column's own scale, weights are uniform(0.5, 12).  The gathered form has one class
that holds a single row whose mean IS that row (it contributes exact zeros), one class number -1 and one C + 5 (neither is read).

References: r in numpy.longdouble (64-bit mantissa) and S, the same sum over the absolute values of the operands after centring and
weighting.  u = 2^-53.

Criteria, per element:

  sc_gemm_tn, sc_scatter_within, sc_class_scatter, sc_tv_gram        |got - r| <= (K + 8) u S
      K is the number of rows summed (a class scatter: the class's count; the gathered form: the rows whose class number is in range).
      A term of the sum is w (a - ca) (b - cb): one rounding for each centred operand and one for the weight leave
      (1 + d1)(1 + d2)(1 + d3) on the exact term, 3 u |term| to first order; a chain of K additions in any order adds at most
      (K - 1) u S (every partial sum is bounded by S), the matrix cores' fused products add none; the join of the slabs is part of that
      chain but adds its partial tiles from a zero, one addition more per slab boundary, and second-order terms stay far below 1 u S at
      K <= 2^13: together (K + 8) u S with more than three roundings to spare.  The bound does not grow with the centres: S is taken
      after centring.  A term that is exactly zero (a row equal to its class mean) bounds itself to zero.
  sc_dgemm_nn, SC_EPI_RANK1                                          |got - r| <= (K + 4) u (|alpha| S + |rowv[m] colv[n]|)
      r = alpha (A B) - rowv colv: K - 1 for the chain, one each for alpha x, rowv x colv and the subtraction, whose result is at most
      |alpha| S + |rowv colv|.  The plain form (rowv = colv = null) is the same with the second term zero.
  sc_dgemm_nn, SC_EPI_POSTERIOR                                      |got - r| <= (K + 6) u |alpha| S / (1 + t),  t = rowv[m] colv[n] >= 0
      r = alpha (A B) / (1 + t): with t >= 0 (the E-step's eigenvalue products) 1 + t does not cancel, so the roundings of t, of 1 + t,
      of alpha x and of the division are relative ones on the quotient: K - 1 + 4 <= K + 6.
  sc_whiten_rows, normalize = 0                                      |got - v| <= (D + 4) u Sv =: dv,  v = (x - mu) R,  Sv = |x - mu| |R|
      one rounding for x - mu, D - 1 for the chain.  A row equal to mu has Sv = 0: exact zeros.
  sc_whiten_rows, normalize = 1                                      r = v / L,  L = max(n, 1e-8),  n = |v|
      The kernel divides ITS v' = v + e, |e_j| <= dv_j, by ITS length.  To first order n' - n = (v . e) / n, so |n' - n| <= dn :=
      sum_j |v_j| dv_j / n.  The sum of P squares in any order, the squares themselves and the square root add a relative
      ((P + 1) / 2 + 1) u to the length, the division one u to the result:
          |got_j - r_j| <= dv_j / L + |r_j| (dn / L + (P / 2 + 3) u)       where n > 1e-8
          |got_j - r_j| <= dv_j / 1e-8 + 2 u |r_j|                         where n < 1e-8 (the length is the constant)
      First order in dv plus a few u |r| (the P / 2 is the any-order budget of the sum of squares; at (66, 18, 257) it is 131 u |r|
      beside first-order terms of at least 2 (D + 4) u |r| = 44 u |r|).  No row of a case has n within a factor 2 of 1e-8.
      A float32 output is the float64 result rounded once: the GPU test compares bits with the float64 output, not a bound.
  sc_gauss_loglik                                                    r = cst_c - q / 2,  q = sum_j y_j^2,  y = (x - m_c) W_c
      The kernel forms x W - m W, so what it can promise about y_j is relative to |x| |W| + |m| |W|, not to y_j:
          dy_j = (D + 4) u (|x| |W| + |m| |W|)_j          (two chains of D, their difference)
          |got - r| <= sum_j |y_j| dy_j + (P + 4) u q / 2 + u (|cst| + |r|)      (P = D columns: squares, their sum, the half, the subtraction)
      The cancellation this formulation permits shows as a share of this bound instead of disappearing in a norm.

A share is |got - r| / bound; a value that is not finite, or not exactly r where the bound is 0, has share inf.
"""
import functools
import os
import re

import numpy

U = 2.0 ** -53
LD = numpy.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EPS_LEN = 1e-8            # sc_whiten_rows: v / max(|v|, 1e-8)
EPI_RANK1, EPI_POSTERIOR = 0, 1
SENTINEL = -1.5e30        # what the GPU tests fill their output frames with

# ---- thresholds the shapes below assume (read_sources() reads them out of the sources) --------------------------------------------------
DK = 16                   # k-tile of dgemm_tile and of whiten_rows_kernel
TILE, BIG_TILE = 64, 128  # workgroup tile edges of the TN product
BIG_M, BIG_N, BIG_K = 128, 128, 4096   # tn_cut: 128 x 128 tiles from M >= 128 && N >= 128 && K >= 4096
SLAB_K = 512              # tn_cut: (K + 511) / 512 slabs at most ...
WG_TARGET = 512           # ... until about 512 workgroups exist
NN_TILE = 64              # dgemm_nn_kernel
WHITEN_ROWS = 64          # whiten_rows_kernel: rows per workgroup
WHITEN_P = (64, 128, 256)  # launch_whiten: 64, 128, 256 columns per workgroup; beyond 256 a normalising call runs twice
LOGLIK_BIG = 512          # sc_gauss_loglik: 128-row tiles from cdiv(N, 128) * C >= 512
GRAM_TILE = 64            # tv_gram_kernel

# ---- the shapes: the smallest that reach each branch ----------------------------------------------------------------------------------
TN_SHAPES = [(1, 1, 1), (16, 64, 64), (17, 65, 63), (15, 66, 130), (513, 6, 5), (4096, 128, 128), (4095, 128, 128), (4096, 128, 127), (4097, 129, 130)]
TN_FORMS = ("plain", "w", "ca", "w+ca+cb")
GATHERED_SHAPES = [(1, 1), (16, 64), (17, 65), (513, 6), (4096, 128), (4097, 130)]
CLASS_SHAPES = [((1, 15, 16, 17, 600), 6), ((3, 1), 65), ((4096, 1), 128)]
NN_SHAPES = [(1, 1, 1), (64, 64, 16), (65, 63, 17), (33, 130, 28), (129, 66, 64)]
NN_EPILOGUES = ("plain", "rank1", "posterior")
WHITEN_SHAPES = [(1, 1, 1), (64, 16, 64), (65, 17, 65), (70, 36, 128), (70, 37, 129), (66, 40, 256), (66, 18, 257)]
WHITEN_ZERO_ROW, WHITEN_TINY_ROW = 5, 9     # in the cases of 64 rows and more
LOGLIK_SHAPES = [(1, 1, 1), (65, 65, 3), (64, 130, 2), (1, 5, 512), (129, 66, 512)]
GRAM_SHAPES = [(2, 1, 2), (2, 16, 64), (3, 17, 65), (2, 5, 130), (1, 33, 192)]
DTYPES = ("float32", "float64")

# what the relative max-norm criterion of the suite before these tests lets through (tests/test_f64_forms_reference_cpu.py asserts the list):
# "entry: mutant" for every mutant that passed max|got - want| / max|want| <= OLD_TOL in at least one case it can show in
OLD_TOL = {"tn": 1e-12, "gathered": 1e-12, "class": 1e-12, "whiten": 1e-12, "nn": 1e-12, "gram": 1e-9, "loglik": 1e-9}


def _body(text, start):
    i = text.index(start)
    return text[i:text.index("\n}\n", i)]


def read_sources():
    """the thresholds above as the sources state them"""
    def src(name):
        with open(os.path.join(ROOT, "sidekit_amd", "csrc", name)) as f:
            return f.read()
    tile, plda, backend, gauss, ivec = src("dgemm_tile.h"), src("plda_train.hip"), src("backend.hip"), src("gaussian_backend.hip"), src("ivector.hip")
    dk = int(re.search(r"constexpr int DK = (\d+), DLD = DK \+ 1;", tile).group(1))
    assert "constexpr int T = 32 * WT;" in tile
    cut = _body(plda, "TnCut tn_cut(")
    big = re.search(r"c\.big = M >= (\d+) && N >= (\d+) && K >= (\d+);", cut)
    tl = re.search(r"c\.TL = c\.big \? (\d+) : (\d+);", cut)
    slab = re.search(r"c\.nsplit = \(K \+ (\d+)\) / (\d+);", cut)
    want = re.search(r"const long want = tiles >= (\d+) \? 1 : (\d+) / tiles;", cut)
    assert int(slab.group(1)) + 1 == int(slab.group(2)) and want.group(1) == want.group(2)
    assert "c.slab = (c.slab + DK - 1) / DK * DK;" in cut
    assert "dgemm_tn_kernel<4, T>" in plda and "dgemm_tn_kernel<2, T>" in plda and "constexpr int TL = 32 * WT;" in plda
    nn = _body(plda, "void dgemm_nn_kernel(")
    nn_tl = int(re.search(r"constexpr int WT = 2, TL = (\d+);", nn).group(1))
    assert f"dim3(cdiv(N, {nn_tl}), cdiv(M, {nn_tl}))" in _body(plda, "int sc_dgemm_nn(")
    wr = int(re.search(r"constexpr int TR = (\d+), TC = (\d+) \* CT;", backend).group(1))
    lw = _body(backend, "static int launch_whiten(")
    ps = tuple(int(v) for v in re.findall(r"if \(P <= (\d+)(?: \|\| !normalize)?\) \{ launch_whiten_ct<(?:1|2|4)>", lw))
    assert "if (P <= 256 || !normalize)" in lw
    ll = int(re.search(r"const bool big = \(long\)cdiv\(\(int\)N, 128\) \* C >= (\d+);", _body(gauss, "int sc_gauss_loglik(")).group(1))
    gram = int(re.search(r"constexpr int WT = 2, TL = (\d+);", _body(ivec, "void tv_gram_kernel(")).group(1))
    assert f"const int nt = cdiv(R, {gram});" in _body(ivec, "int sc_tv_gram(")
    return {"DK": dk, "TILE": int(tl.group(2)), "BIG_TILE": int(tl.group(1)), "BIG_M": int(big.group(1)), "BIG_N": int(big.group(2)),
            "BIG_K": int(big.group(3)), "SLAB_K": int(slab.group(2)), "WG_TARGET": int(want.group(1)), "NN_TILE": nn_tl, "WHITEN_ROWS": wr,
            "WHITEN_P": ps, "LOGLIK_BIG": ll, "GRAM_TILE": gram}


def tn_cut(K, M, N, batch=1):
    """plda_train.hip's tn_cut: (big, tile edge, slabs, rows per slab)"""
    big = M >= BIG_M and N >= BIG_N and K >= BIG_K
    tl = BIG_TILE if big else TILE
    tiles = batch * (-(-M // tl)) * (-(-N // tl))
    nsplit = (K + SLAB_K - 1) // SLAB_K
    want = 1 if tiles >= WG_TARGET else WG_TARGET // tiles
    nsplit = min(nsplit, want)
    slab = -(-K // nsplit)
    slab = -(-slab // DK) * DK
    return big, tl, -(-K // slab), slab


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
def _rs(*key):
    h = 0
    for v in key:
        for ch in str(v):
            h = (h * 131 + ord(ch)) % (2 ** 31 - 1)
    return numpy.random.RandomState(h)


def _columns(rs, k, m):
    """([k][m] float64, the column scales): randn x 2^uniform(-6, 6), one scale per column"""
    s = 2.0 ** rs.uniform(-6.0, 6.0, m)
    return rs.standard_normal((k, m)) * s, s


def _rows(rs, n, d):
    s = 2.0 ** rs.uniform(-6.0, 6.0, n)
    return rs.standard_normal((n, d)) * s[:, None], s


def _typed(x, dtype):
    return numpy.ascontiguousarray(x.astype(dtype))


def _centre(rs, x, scale):
    """column mean of the (typed) operand plus an offset of the column's own scale"""
    return x.astype(numpy.float64).mean(0) + scale * rs.uniform(-1.0, 1.0, x.shape[1])


def tn_case(shape, form, dtype):
    """A [K][M], B [K][N] of ``dtype``; w [K], ca [M], cb [N] float64 or None as ``form`` says"""
    K, M, N = shape
    rs = _rs("tn", shape, form, dtype)
    (A, sa), (B, sb) = _columns(rs, K, M), _columns(rs, K, N)
    A, B = _typed(A, dtype), _typed(B, dtype)
    return {"A": A, "B": B, "w": rs.uniform(0.5, 12.0, K) if "w" in form else None, "ca": _centre(rs, A, sa) if "ca" in form else None,
            "cb": _centre(rs, B, sb) if "cb" in form else None}


def gathered_case(shape, weighted, dtype):
    """X [N][D], cls [N] int32, Mc [C][D], w [C] or None.  N > 1: C = 4, classes 0 .. 2 are drawn, row N // 2 alone is class 3 and is its
    mean; cls[1] = -1 and cls[N - 2] = C + 5 are out of range.  N = 1: the one row is the one class and its mean."""
    N, D = shape
    rs = _rs("gathered", shape, weighted, dtype)
    X, sx = _columns(rs, N, D)
    X = _typed(X, dtype)
    if N == 1:
        C, cls = 1, numpy.zeros(1, dtype=numpy.int32)
        Mc = X.astype(numpy.float64).copy()
    else:
        C = 4
        cls = rs.randint(0, C - 1, N).astype(numpy.int32)
        cls[N // 2], cls[1], cls[N - 2] = C - 1, -1, C + 5
        Mc = numpy.stack([_centre(rs, X[cls == c], sx) for c in range(C - 1)] + [X[N // 2].astype(numpy.float64)])
    return {"X": X, "cls": cls, "Mc": numpy.ascontiguousarray(Mc), "w": rs.uniform(0.5, 12.0, C) if weighted else None, "C": C}


def class_case(counts, D, dtype):
    """X [sum counts][D] grouped by class, off [C + 1] int32, Mc [C][D]"""
    rs = _rs("class", counts, D, dtype)
    X, sx = _columns(rs, sum(counts), D)
    X = _typed(X, dtype)
    off = numpy.concatenate([[0], numpy.cumsum(counts)]).astype(numpy.int32)
    Mc = numpy.stack([_centre(rs, X[off[c]:off[c + 1]], sx) for c in range(len(counts))])
    return {"X": X, "off": off, "Mc": numpy.ascontiguousarray(Mc), "counts": tuple(counts)}


def nn_case(shape, epilogue):
    """A [M][K] (a scale per row), B [K][N] (a scale per column), alpha, rowv [M], colv [N] (None in the plain form), the epilogue's number.
    Posterior: rowv, colv in [0, 3), so that t = rowv[m] colv[n] >= 0 as in the E-step."""
    M, N, K = shape
    rs = _rs("nn", shape, epilogue)
    (A, sa), (B, sb) = _rows(rs, M, K), _columns(rs, K, N)
    rowv = colv = None
    if epilogue == "rank1":
        rowv, colv = sa * rs.standard_normal(M), sb * rs.standard_normal(N)
    elif epilogue == "posterior":
        rowv, colv = rs.uniform(0.0, 3.0, M), rs.uniform(0.0, 3.0, N)
    return {"A": A, "B": B, "alpha": 0.7 if epilogue != "plain" else -1.3, "rowv": rowv, "colv": colv,
            "epi": EPI_POSTERIOR if epilogue == "posterior" else EPI_RANK1}


def whiten_case(shape, centred, dtype):
    """X [N][D] of ``dtype`` (a scale per row), mu [D] or None, R [D][P] (a scale per column).  mu holds values of ``dtype`` (widened), so
    that a row can equal it.  From 64 rows on: row 5 equals mu (a zero row without mu); row 9 gives |v| < 1e-8 -- a tiny row without mu,
    mu (1 + 2^-48) under float64 with mu (x - mu is then a few units in mu's last places), and an ordinary row under float32 with mu, where
    no float32 row is that close to mu."""
    N, D, P = shape
    rs = _rs("whiten", shape, centred, dtype)
    (X, _), (R, _) = _rows(rs, N, D), _columns(rs, D, P)
    X = _typed(X, dtype)
    mu = None
    if centred:
        wide = X.astype(numpy.float64)
        mu = (wide.mean(0) + numpy.sqrt((wide * wide).mean(0)) * rs.uniform(-1.0, 1.0, D)).astype(dtype).astype(numpy.float64)
    tiny = None
    if N >= WHITEN_ROWS:
        X[WHITEN_ZERO_ROW] = mu if centred else 0.0
        if not centred:
            t = rs.standard_normal(D)
            X[WHITEN_TINY_ROW] = t * (1e-10 / numpy.linalg.norm(t @ R))
            tiny = WHITEN_TINY_ROW
        elif dtype == "float64":
            X[WHITEN_TINY_ROW] = mu * (1.0 + 2.0 ** -48)
            tiny = WHITEN_TINY_ROW
    return {"X": X, "mu": mu, "R": numpy.ascontiguousarray(R), "tiny": tiny}


def loglik_case(shape):
    """X [N][D] (a scale per row), means [C][D], W [C][D][D] (a scale per column of every W_c), cst [C]"""
    N, D, C = shape
    rs = _rs("loglik", shape)
    X, _ = _rows(rs, N, D)
    rms = numpy.sqrt((X * X).mean(0))
    means = X.mean(0) + rms * rs.uniform(-1.0, 1.0, (C, D))
    W = numpy.stack([_columns(rs, D, D)[0] for _ in range(C)])
    return {"X": numpy.ascontiguousarray(X), "means": numpy.ascontiguousarray(means), "W": numpy.ascontiguousarray(W), "cst": 100.0 * rs.standard_normal(C)}


def gram_case(shape):
    """F [C][D][R], a scale per column of every F_c"""
    C, D, R = shape
    rs = _rs("gram", shape)
    return {"F": numpy.ascontiguousarray(numpy.stack([_columns(rs, D, R)[0] for _ in range(C)]))}


# ---- references (numpy.longdouble) --------------------------------------------------------------------------------------------------------
def _tn(a, b):
    """(a' b, |a|' |b|) of longdouble operands"""
    return numpy.einsum("km,kn->mn", a, b), numpy.einsum("km,kn->mn", numpy.abs(a), numpy.abs(b))


def tn_ref(A, B, w=None, ca=None, cb=None):
    """(r, bound) of G = sum_k w[k] (A[k] - ca)' (B[k] - cb)"""
    a, b = A.astype(LD), B.astype(LD)
    if ca is not None:
        a = a - ca.astype(LD)
    if cb is not None:
        b = b - cb.astype(LD)
    if w is not None:
        a = a * w.astype(LD)[:, None]
    r, S = _tn(a, b)
    return r, (A.shape[0] + 8) * LD(U) * S


def gathered_ref(X, cls, Mc, w, C):
    valid = (cls >= 0) & (cls < C)
    a = X[valid].astype(LD) - Mc[cls[valid]].astype(LD)
    aw = a * w[cls[valid]].astype(LD)[:, None] if w is not None else a
    r, S = _tn(aw, a)
    return r, (int(valid.sum()) + 8) * LD(U) * S


def class_ref(X, off, Mc):
    """([C][D][D] r, bound): class c is rows [off[c], off[c + 1]), K = its count"""
    out = [tn_ref(X[off[c]:off[c + 1]], X[off[c]:off[c + 1]], None, Mc[c], Mc[c]) for c in range(len(Mc))]
    return numpy.stack([r for r, _ in out]), numpy.stack([b for _, b in out])


def gram_ref(F):
    """([C][R (R + 1) / 2] packed upper triangles in row-major order, bound)"""
    iu = numpy.triu_indices(F.shape[2])
    out = [tn_ref(Fc, Fc) for Fc in F]
    return numpy.stack([r[iu] for r, _ in out]), numpy.stack([b[iu] for _, b in out])


def nn_ref(A, B, alpha, rowv, colv, epi):
    a, b, K = A.astype(LD), B.astype(LD), A.shape[1]
    p, S = a @ b, numpy.abs(a) @ numpy.abs(b)
    al = LD(alpha)
    t = numpy.outer(rowv.astype(LD), colv.astype(LD)) if rowv is not None else numpy.zeros(p.shape, dtype=LD)
    if epi == EPI_POSTERIOR:
        assert (t >= 0).all()
        return al * p / (1 + t), (K + 6) * LD(U) * abs(al) * S / (1 + t)
    return al * p - t, (K + 4) * LD(U) * (abs(al) * S + numpy.abs(t))


def whiten_ref(X, mu, R, normalize):
    x = X.astype(LD)
    if mu is not None:
        x = x - mu.astype(LD)
    D, P = R.shape
    v, Sv = x @ R.astype(LD), numpy.abs(x) @ numpy.abs(R.astype(LD))
    dv = (D + 4) * LD(U) * Sv
    if not normalize:
        return v, dv
    n = numpy.sqrt((v * v).sum(1, keepdims=True))
    assert not ((n > EPS_LEN / 2) & (n < EPS_LEN * 2)).any(), "a row's length is within a factor 2 of 1e-8: change the case"
    L = numpy.maximum(n, LD(EPS_LEN))
    r = v / L
    dn = (numpy.abs(v) * dv).sum(1, keepdims=True) / numpy.where(n > 0, n, 1)
    live = numpy.abs(r) * (dn / L + (P / 2 + 3) * LD(U)) + dv / L
    return r, numpy.where(n > EPS_LEN, live, dv / LD(EPS_LEN) + 2 * LD(U) * numpy.abs(r))


def loglik_ref(X, means, W, cst):
    """([C][N] r, bound)"""
    x, (N, D) = X.astype(LD), X.shape
    rs, bs = [], []
    for c in range(len(means)):
        m, Wc = means[c].astype(LD), W[c].astype(LD)
        y = (x - m) @ Wc
        dy = (D + 4) * LD(U) * (numpy.abs(x) @ numpy.abs(Wc) + (numpy.abs(m) @ numpy.abs(Wc))[None])
        q = (y * y).sum(1)
        r = LD(cst[c]) - q / 2
        rs.append(r)
        bs.append((numpy.abs(y) * dy).sum(1) + (D + 4) * LD(U) * q / 2 + LD(U) * (abs(LD(cst[c])) + numpy.abs(r)))
    return numpy.stack(rs), numpy.stack(bs)


# one reference per case and process, shared by every test that needs it and never written to
@functools.lru_cache(maxsize=None)
def tn(shape, form, dtype):
    case = tn_case(shape, form, dtype)
    return (case,) + tn_ref(**case)


@functools.lru_cache(maxsize=None)
def gathered(shape, weighted, dtype):
    case = gathered_case(shape, weighted, dtype)
    return (case,) + gathered_ref(**case)


@functools.lru_cache(maxsize=None)
def classes(counts, D, dtype):
    case = class_case(counts, D, dtype)
    return (case,) + class_ref(case["X"], case["off"], case["Mc"])


@functools.lru_cache(maxsize=None)
def nn(shape, epilogue):
    case = nn_case(shape, epilogue)
    return (case,) + nn_ref(**case)


@functools.lru_cache(maxsize=None)
def whiten(shape, centred, dtype, normalize):
    case = whiten_case(shape, centred, dtype)
    return (case,) + whiten_ref(case["X"], case["mu"], case["R"], normalize)


@functools.lru_cache(maxsize=None)
def loglik(shape):
    case = loglik_case(shape)
    return (case,) + loglik_ref(**case)


@functools.lru_cache(maxsize=None)
def gram(shape):
    case = gram_case(shape)
    return (case,) + gram_ref(case["F"])


# ---- criteria ---------------------------------------------------------------------------------------------------------------------------
def shares(got, r, bound):
    """|got - r| / bound per element; inf where got is not finite, or not exactly r where the bound is 0"""
    got = numpy.asarray(got)
    assert got.shape == r.shape, f"shape {got.shape}, expected {r.shape}"
    diff = numpy.abs(got.astype(LD) - r)
    with numpy.errstate(invalid="ignore", divide="ignore"):
        s = numpy.where(bound > 0, diff / numpy.where(bound > 0, bound, 1), numpy.where(diff == 0, 0.0, numpy.inf))
    return numpy.where(numpy.isfinite(s), s, numpy.inf).astype(numpy.float64)


def check(name, got, r, bound):
    """Returns the largest share of the bound; raises AssertionError above 1."""
    s = shares(got, r, bound)
    worst = float(s.max())
    if not worst <= 1.0:
        i = numpy.unravel_index(int(numpy.argmax(s)), s.shape)
        raise AssertionError(f"{name}: {int((s > 1).sum())} of {s.size} elements outside their bounds; element {tuple(int(v) for v in i)} is "
                             f"{float(numpy.asarray(got)[i])!r} for {float(r[i])!r}, {worst:.3g} of its bound {float(bound[i]):.3g}")
    return worst


def old_criterion(got, want, tol):
    """the suite's criterion before these tests: one relative max-norm over the whole output against a float64 numpy evaluation"""
    got, want = numpy.asarray(got, dtype=numpy.float64), numpy.asarray(want, dtype=numpy.float64)
    if not numpy.isfinite(got).all():
        return False
    return float(numpy.abs(got - want).max()) <= tol * float(numpy.abs(want).max())


# ---- float64 numpy stand-ins of the kernels, and the wrong kernels ---------------------------------------------------------------------------
def _spill(a):
    """the last element of every row is taken from the next row's first (zero after the last row): a pair load one element over"""
    flat = numpy.append(a.ravel(), 0.0)
    out = a.copy()
    out[:, -1] = flat[(numpy.arange(a.shape[0]) + 1) * a.shape[1]]
    return out


def tn_eval(A, B, w=None, ca=None, cb=None, mutant=None, cut=None, same=False):
    """sum_k w[k] (A[k] - ca)' (B[k] - cb) in float64 numpy.  ``cut``: (slabs, rows per slab), tn_cut's by default; ``same``: B is A's
    buffer (a mutant of the loads hits both).  Mutants:
      drop_last_row  the last k-row is dropped          padding        rows past K up to the k-tile contribute (0 - ca)(0 - cb) with weight 1
      w_from_0       every slab reads w from index 0    join_early     the slab join stops one slab early
      swap_centres   ca and cb exchanged                odd_row_next   the last element of an (odd-length) row of A comes from the next row
      transposed     G' in G's memory"""
    a, b = A.astype(numpy.float64), B.astype(numpy.float64)
    K, M, N = a.shape[0], a.shape[1], b.shape[1]
    nsplit, slab = cut if cut is not None else tn_cut(K, M, N)[2:]
    wk = numpy.ones(K) if w is None else w
    ca = numpy.zeros(M) if ca is None else ca
    cb = numpy.zeros(N) if cb is None else cb
    if mutant == "swap_centres":
        ca, cb = numpy.resize(cb, M), numpy.resize(ca, N)
    if mutant == "odd_row_next":
        a = _spill(a)
        b = _spill(b) if same else b
    if mutant == "w_from_0":
        wk = wk[numpy.arange(K) % slab]
    ac, bc = (a - ca) * wk[:, None], b - cb
    if mutant == "drop_last_row":
        ac, bc = ac[:-1], bc[:-1]
    if mutant == "join_early":
        ac, bc = ac[:slab * (nsplit - 1)], bc[:slab * (nsplit - 1)]
    G = ac.T @ bc
    if mutant == "padding":
        G = G + (-K % DK) * numpy.outer(ca, cb)
    if mutant == "transposed":
        G = numpy.ascontiguousarray(G.T).reshape(M, N)
    return G


def gathered_eval(X, cls, Mc, w, C, mutant=None):
    """Mutants: drop_last_row, join_early, odd_row_next as above; clamp_class: an out-of-range class number is clamped, not skipped;
    w_k: w[k] for w[cls[k]] (w read cyclically)"""
    x, N = X.astype(numpy.float64), len(X)
    nsplit, slab = tn_cut(N, X.shape[1], X.shape[1])[2:]
    if mutant == "odd_row_next":
        x = _spill(x)
    c = numpy.clip(cls, 0, C - 1) if mutant == "clamp_class" else cls
    valid = (c >= 0) & (c < C)
    a, wk = numpy.zeros_like(x), numpy.zeros(N)
    a[valid] = x[valid] - Mc[c[valid]]
    wk[valid] = 1.0 if w is None else (numpy.resize(w, N)[valid] if mutant == "w_k" else w[c[valid]])
    if mutant == "drop_last_row":
        a, wk = a[:-1], wk[:-1]
    if mutant == "join_early":
        a, wk = a[:slab * (nsplit - 1)], wk[:slab * (nsplit - 1)]
    return (a * wk[:, None]).T @ a


def class_eval(X, off, Mc, counts, mutant=None):
    D = X.shape[1]
    cut = tn_cut(max(counts), D, D, len(counts))[2:]
    return numpy.stack([tn_eval(X[off[c]:off[c + 1]], X[off[c]:off[c + 1]], None, Mc[c], Mc[c], mutant, cut, same=True) for c in range(len(Mc))])


def pack_shifted(packed, R):
    """every row of the packed triangle after the first lands one element late; the element no row lands on keeps what the output held
    (the GPU test's sentinel)"""
    out = numpy.full_like(packed, SENTINEL)
    out[:, :R] = packed[:, :R]
    out[:, R + 1:] = packed[:, R:-1]
    return out


def gram_eval(F, mutant=None):
    iu = numpy.triu_indices(F.shape[2])
    packed = numpy.stack([tn_eval(Fc, Fc, mutant=None if mutant == "packed_shift" else mutant, cut=(1, 1 << 30), same=True)[iu] for Fc in F])
    return pack_shifted(packed, F.shape[2]) if mutant == "packed_shift" else packed


def _row64(out):
    out = out.copy()
    out[WHITEN_ROWS] = out[WHITEN_ROWS - 1]
    return out


def nn_eval(A, B, alpha, rowv, colv, epi, mutant=None):
    """Mutants: drop_last_row (the last k-term), odd_row_next (rows of A), swap_rowcol (rowv and colv exchanged), row64_is_63"""
    a, b = (_spill(A) if mutant == "odd_row_next" else A), B
    if mutant == "drop_last_row":
        a, b = a[:, :-1], b[:-1]
    p = alpha * (a @ b)
    if rowv is not None:
        t = numpy.outer(rowv, colv) if mutant != "swap_rowcol" else numpy.outer(numpy.resize(colv, len(rowv)), numpy.resize(rowv, len(colv)))
        p = p / (1.0 + t) if epi == EPI_POSTERIOR else p - t
    return _row64(p) if mutant == "row64_is_63" else p


def whiten_eval(X, mu, R, normalize, mutant=None):
    """Mutants: drop_last_row (the last k-term), odd_row_next (rows of X), len_plus_eps (len + 1e-8 for max(len, 1e-8)), len_block0 (the
    length from the first 256 columns alone), row64_is_63"""
    x = X.astype(numpy.float64)
    if mutant == "odd_row_next":
        x = _spill(x)
    if mu is not None:
        x = x - mu
    v = x[:, :-1] @ R[:-1] if mutant == "drop_last_row" else x @ R
    if normalize:
        n = numpy.sqrt((v[:, :WHITEN_P[-1]] ** 2).sum(1, keepdims=True)) if mutant == "len_block0" else numpy.sqrt((v * v).sum(1, keepdims=True))
        v = v / (n + EPS_LEN if mutant == "len_plus_eps" else numpy.maximum(n, EPS_LEN))
    return _row64(v) if mutant == "row64_is_63" else v


def loglik_eval(X, means, W, cst, mutant=None):
    """cst_c - 0.5 |x W_c - m_c W_c|^2, as the kernel forms it.  Mutants: drop_last_row (the last k-term of x W), row64_is_63,
    V_past_64 (m W is not subtracted past column 64), cst_prev (cst of class c - 1, cyclically)"""
    out = []
    for c in range(len(means)):
        V = means[c] @ W[c]
        if mutant == "V_past_64":
            V[TILE:] = 0.0
        y = (X[:, :-1] @ W[c][:-1] if mutant == "drop_last_row" else X @ W[c]) - V
        out.append(cst[c - 1 if mutant == "cst_prev" else c] - 0.5 * (y * y).sum(1))
    out = numpy.stack(out)
    return _row64(out.T).T if mutant == "row64_is_63" else out
