"""float64 numpy restatement of the total-variability arithmetic of ``sidekit/factor_analyser.py`` (``e_on_batch`` :51-91, the
accumulators and the M-step of ``total_variability_single`` :496-530, ``extract_ivectors_single`` :688-744) in the seven steps the
device code is cut into: Gram matrices, whitening, packed sums, projections, the posterior of every session, the accumulators, the
M-step.  The tests' reference: held to 1e-12 against what the reference's own module computed (tests/golden/ivector.npz,
make_ivector_golden.py).  Symmetric R x R matrices are packed upper triangles in the order of ``numpy.triu_indices(R)``."""
import numpy
import scipy.linalg


def packed_index(i, j, R):
    """position of (i, j), i <= j, in the packed upper triangle"""
    return i * R - i * (i - 1) // 2 + (j - i)


def unpack(p, R):
    """packed (..., P) -> symmetric (..., R, R)"""
    p = numpy.asarray(p)
    iu = numpy.triu_indices(R)
    full = numpy.zeros(p.shape[:-1] + (R, R))
    full[..., iu[0], iu[1]] = p
    full[..., iu[1], iu[0]] = p
    return full


def pack(full):
    R = full.shape[-1]
    iu = numpy.triu_indices(R)
    return full[..., iu[0], iu[1]]


def gram(F, C, D):
    """step 1: G[c] = F_c' F_c, packed (C, P)"""
    Fc = F.reshape(C, D, F.shape[1])
    return pack(numpy.einsum("cdi,cdj->cij", Fc, Fc))


def whiten(stat0, stat1, mu, invcov):
    """step 2: (stat1 - stat0[:, index_map] * mean_sv) * sqrt(invcov_sv); mu, invcov (C, D)"""
    C, D = mu.shape
    blocks = stat1.reshape(stat0.shape[0], C, D) - stat0[:, :, None] * mu[None]
    return (blocks * numpy.sqrt(invcov)[None]).reshape(stat1.shape)


def posterior(Lp, B):
    """step 5: Lambda = I + unpack(Lp) -> (e_h (N, R), E_hh packed (N, P))"""
    R = B.shape[1]
    inv_lambda = numpy.linalg.inv(numpy.eye(R)[None] + unpack(Lp, R))
    e_h = numpy.einsum("nij,nj->ni", inv_lambda, B)
    return e_h, pack(inv_lambda + e_h[:, :, None] * e_h[:, None, :])


def e_step(stat0, stat1_w, F, G=None):
    """steps 1, 3, 4, 5 on whitened statistics -> (e_h, E_hh packed)"""
    C = stat0.shape[1]
    if G is None:
        G = gram(F, C, F.shape[0] // C)
    return posterior(stat0.dot(G), stat1_w.dot(F))


def accumulate(stat0, stat1_w, e_h, e_hh):
    """step 6 for one batch -> (_A (C, P), _C (R, C D), _R (P,))"""
    return stat0.T.dot(e_hh), e_h.T.dot(stat1_w), e_hh.sum(axis=0)


def m_step(_A, _C, _R, n_sessions, min_div=True):
    """step 7: C solves, then F . cholesky(_R / N) when min_div -> F ((C D), R)"""
    C, R = _A.shape[0], _C.shape[0]
    D = _C.shape[1] // C
    F = numpy.empty((C * D, R))
    for c in range(C):
        F[c * D:(c + 1) * D] = scipy.linalg.solve(unpack(_A[c], R), _C[:, c * D:(c + 1) * D]).T
    if min_div:
        F = F.dot(scipy.linalg.cholesky(unpack(_R / n_sessions, R)))
    return F


def em_iteration(stat0, stat1, mu, invcov, F, batches, min_div=True):
    """one EM iteration over the sessions in ``batches`` (a list of index arrays), accumulators added in batch order
    -> (F, (_A, _C, _R before the division), e_h, e_hh of all sessions in batch order)"""
    C, D = mu.shape
    G = gram(F, C, D)
    acc, ehs, ehhs = None, [], []
    for idx in batches:
        s0, sw = stat0[idx], whiten(stat0[idx], stat1[idx], mu, invcov)
        e_h, e_hh = e_step(s0, sw, F, G)
        part = accumulate(s0, sw, e_h, e_hh)
        acc = part if acc is None else tuple(a + p for a, p in zip(acc, part))
        ehs.append(e_h)
        ehhs.append(e_hh)
    n = sum(len(idx) for idx in batches)
    return m_step(*acc, n, min_div), acc, numpy.concatenate(ehs), numpy.concatenate(ehhs)


def train(stat0, stat1, mu, invcov, F, nb_iter, batches, min_div=True):
    """-> the list of F after every iteration"""
    out = []
    for _ in range(nb_iter):
        F = em_iteration(stat0, stat1, mu, invcov, F, batches, min_div)[0]
        out.append(F)
    return out


def extract(stat0, stat1, mu, invcov, F):
    """-> (i-vectors (N, R), diagonal of E_hh (N, R))"""
    R = F.shape[1]
    e_h, e_hh = e_step(stat0, whiten(stat0, stat1, mu, invcov), F)
    return e_h, e_hh[:, [packed_index(i, i, R) for i in range(R)]]


def rel(a, b):
    """relative max-norm distance"""
    return numpy.abs(numpy.asarray(a) - numpy.asarray(b)).max() / numpy.abs(numpy.asarray(b)).max()
