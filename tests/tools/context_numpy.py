"""The context features restated in numpy from their formulas (sidekit_amd/features_context.py's head): what the fixture
tests/golden/context.npz is reproduced with on the CPU and what the GPU tests evaluate in float64 on the kernels' own float32 operands.

A stream has n rows and cl(i) = min(max(i, 0), n - 1).  Every function takes one stream (n x D) and returns all n rows, or with
``rows=(start, stop)`` the rows start .. stop - 1 (which may lie beyond the stream: the clamp is at the stream's ends)."""
import numpy

# the cases of tests/golden/context.npz, shared by its generator and the tests
LENGTHS = (2, 3, 7, 40, 256, 257, 300)
SMALL = (2, 3, 7, 40)
DIMS = (5, 13)
SDC = ((1, 3, 7), (2, 2, 3), (3, 1, 2), (1, 4, 4))
WINDOWS = ((3, 2), (0, 2), (12, 12))
TRAPS_NB = (4, 16)
PCA_Q = (7, 40)
RANGES = ((None, None), (5, 30), (-3, 45), (0, 40), (38, 52))      # start / stop of get_context and get_traps on the 40-row stream


def cases():
    """name -> (kind, D, lengths, parameters): every array of the fixture but the inputs.  The long streams go with the cheap outputs."""
    out = {}
    for D in DIMS:
        for cfg in SDC:
            rows = LENGTHS if (D == 5 and cfg == (1, 3, 7)) else SMALL
            out["sdc_%d_%d_%d_D%d" % (cfg + (D,))] = ("sdc", D, rows, cfg)
        for win in WINDOWS:
            if win == (12, 12) and D == 13:
                continue
            out["ctx_%d_%d_D%d" % (win + (D,))] = ("ctx", D, SMALL + ((257,) if win == (3, 2) and D == 5 else ()), win)
            out["dct_%d_%d_D%d" % (win + (D,))] = ("dct", D, SMALL + ((257,) if win == (0, 2) and D == 5 else ()), win)
    out["pca_12_12_D5_Q7"] = ("pca", 5, LENGTHS, (12, 12, 7))
    out["pca_12_12_D5_Q40"] = ("pca", 5, SMALL + (257,), (12, 12, 40))
    out["pca_3_2_D13_Q7"] = ("pca", 13, SMALL, (3, 2, 7))
    out["pca_0_2_D13_Q40"] = ("pca", 13, SMALL, (0, 2, 40))
    out["traps_3_2_nb4_D5"] = ("traps", 5, SMALL, (3, 2, 4))
    out["traps_3_2_nb4_D13"] = ("traps", 13, SMALL, (3, 2, 4))
    out["traps_12_12_nb16_D5"] = ("traps", 5, SMALL, (12, 12, 16))
    out["traps_12_12_nb4_D5"] = ("traps", 5, (40,), (12, 12, 4))
    return out


def pca_name(left, right, D, Q):
    return "P_%d_%d_D%d_Q%d" % (left, right, D, Q)


def split(stacked, lengths):
    return numpy.split(stacked, numpy.cumsum(lengths)[:-1])


def dct_basis(nbasis, length):
    """The first rows of the orthonormal DCT-II basis: row j, column w = s_j cos(pi j (2 w + 1) / (2 length)), s_0 = sqrt(1 / length),
    s_j = sqrt(2 / length)"""
    j, w = numpy.arange(nbasis)[:, None], numpy.arange(length)[None, :]
    basis = numpy.sqrt(2.0 / length) * numpy.cos(numpy.pi * j * (2 * w + 1) / (2.0 * length))
    basis[0] *= numpy.sqrt(0.5)
    basis[length:] = 0.0
    return basis


def _rows(n, rows):
    start, stop = (0, n) if rows is None else (0 if rows[0] is None else rows[0], n if rows[1] is None else rows[1])
    return numpy.arange(start, stop)


def window_rows(n, left, W, rows=None):
    """(rows, W) indices cl(t + w - left)"""
    return numpy.clip(_rows(n, rows)[:, None] + numpy.arange(W)[None, :] - left, 0, n - 1)


def context(x, left, right, rows=None):
    """out[t, w D + c] = x[cl(t + w - left), c]"""
    idx = window_rows(x.shape[0], left, left + right + 1, rows)
    return x[idx].reshape(idx.shape[0], -1)


def sdc(x, d, p, k):
    """[x | x[cl(t + b p - d)] - x[cl(t + b p + d)]], in x's dtype"""
    n = x.shape[0]
    t, shift = numpy.arange(n)[:, None], (numpy.arange(k) * p)[None, :]
    early, late = numpy.clip(t + shift - d, 0, n - 1), numpy.clip(t + shift + d, 0, n - 1)
    return numpy.hstack((x, (x[early] - x[late]).reshape(n, -1)))


def dct_pca_basis(left, right):
    W = left + right + 1
    return dct_basis(W, W).T


def traps_basis(left, right, nb):
    W = left + right + 1
    return (dct_basis(nb, W) * numpy.hamming(W)).T


def basis_map(x, basis, left, rows=None):
    """out[t, c J + j] = sum_w x[cl(t + w - left), c] basis[w, j], float64"""
    idx = window_rows(x.shape[0], left, basis.shape[0], rows)
    win = x.astype(numpy.float64)[idx]                               # (rows, W, D)
    return numpy.einsum("twc,wj->tcj", win, basis).reshape(idx.shape[0], -1)


def pca_dct(x, left, right, p=None):
    z = basis_map(x, dct_pca_basis(left, right), left)
    return z if p is None else z @ numpy.asarray(p, dtype=numpy.float64)


def traps(x, left, right, nb, rows=None):
    return basis_map(x, traps_basis(left, right, nb), left, rows)


def composite(basis, p, D):
    """M[w D + c, q] = sum_j basis[w, j] p[c J + j, q], by loops"""
    W, J = basis.shape
    p = numpy.asarray(p, dtype=numpy.float64)
    M = numpy.zeros((W * D, p.shape[1]))
    for w in range(W):
        for c in range(D):
            M[w * D + c] = basis[w] @ p[c * J:(c + 1) * J]
    return M


def project(x, M, W, left, rows=None):
    """-> (ref64, S_abs): out[t, q] = sum_k a[t, k] M[k, q] with a[t, w D + c] = x[cl(t + w - left), c] in float64, and
    S_abs[t, q] = sum_k |a[t, k] M[k, q]|"""
    idx = window_rows(x.shape[0], left, W, rows)
    a = x.astype(numpy.float64)[idx].reshape(idx.shape[0], -1)
    return a @ M, numpy.abs(a) @ numpy.abs(M)


def basis_abs(x, basis, left):
    """S_abs of basis_map: sum_w |x[cl(t + w - left), c] basis[w, j]|"""
    return basis_map(numpy.abs(x), numpy.abs(basis), left)
