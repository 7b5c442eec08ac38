"""float64 numpy restatement of the Gaussian back-end (sidekit/lid_utils.py) in the form the GPU code computes it: per-class scatters of
centred rows, log-likelihoods through one Cholesky factor per class (``inv(Sigma) = W W'``, ``W = inv(L)'``), closed-set LLRs through the
two largest values of a column.  tests/test_gaussian_backend_cpu.py pins it to the reference's own output
(tests/golden/gaussian_backend.npz); the GPU tests use it where the fixture has no case."""
import numpy
import scipy.linalg


def class_means(X, labels):
    """-> (sorted unique labels, class number per row, rows per class, class means)"""
    X = numpy.asarray(X, dtype=numpy.float64)
    ids, inv = numpy.unique(labels, return_inverse=True)
    counts = numpy.bincount(inv, minlength=ids.shape[0])
    return ids, inv, counts, numpy.stack([X[inv == c].mean(axis=0) for c in range(ids.shape[0])])


def class_scatters(X, labels):
    """-> (C, D, D): Z_c' Z_c of each class's rows less their mean"""
    X = numpy.asarray(X, dtype=numpy.float64)
    ids, inv, _, means = class_means(X, labels)
    return numpy.stack([(X[inv == c] - means[c]).T.dot(X[inv == c] - means[c]) for c in range(ids.shape[0])])


def constant(sigma):
    return -0.5 * (numpy.linalg.slogdet(sigma)[1] + sigma.shape[0] * numpy.log(2 * numpy.pi))


def train_tied(X, labels):
    """-> (class means, tied covariance, constant)"""
    means = class_means(X, labels)[3]
    sigma = class_scatters(X, labels).sum(axis=0) / numpy.shape(X)[0]
    return means, sigma, constant(sigma)


def train_hetero(X, labels, alpha=0.1):
    """-> (class means, (C, D, D) covariances alpha S_c / n_c + (1 - alpha) sum S_c / N, (C,) constants)"""
    _, _, counts, means = class_means(X, labels)
    S = class_scatters(X, labels)
    W = S.sum(axis=0) / numpy.shape(X)[0]
    sigmas = alpha * S / counts[:, None, None] + (1 - alpha) * W
    return means, sigmas, numpy.array([constant(s) for s in sigmas])


def precision_factor(sigma):
    """W with inv(sigma) = W W'"""
    return scipy.linalg.solve_triangular(scipy.linalg.cholesky(sigma, lower=True), numpy.eye(sigma.shape[0]), lower=True).T


def loglik(X, means, sigmas, csts):
    """(C, N): cst_c - 0.5 |(x_n - m_c) W_c|^2; one (D, D) sigma and a scalar constant serve every class (the tied model)"""
    X, sigmas = numpy.asarray(X, dtype=numpy.float64), numpy.asarray(sigmas, dtype=numpy.float64)
    C = means.shape[0]
    if sigmas.ndim == 2:
        sigmas, csts = numpy.broadcast_to(sigmas, (C,) + sigmas.shape), numpy.full(C, csts)
    out = numpy.empty((C, X.shape[0]))
    for c in range(C):
        Y = (X - means[c]).dot(precision_factor(sigmas[c]))
        out[c] = csts[c] - 0.5 * (Y * Y).sum(axis=1)
    return out


def closed_set_llr(M, p_tar=0.5):
    """log p_tar + M[c] - LSE_{j != c}(M[j] + log((1 - p_tar) / (C - 1))), the leave-one-out sums about the two largest values"""
    M = numpy.asarray(M, dtype=numpy.float64)
    C, cols = M.shape[0], numpy.arange(M.shape[1])
    a = M.argmax(axis=0)                         # first index on ties
    m1 = M[a, cols]
    others = M.copy()
    others[a, cols] = -numpy.inf
    m2 = others.max(axis=0)
    S1 = numpy.exp(M - m1).sum(axis=0)
    S2 = numpy.exp(others - m2).sum(axis=0)
    with numpy.errstate(divide="ignore", invalid="ignore"):   # the arg-max class's own entry of the general form is log(<= 0): replaced below
        lse = m1 + numpy.log(S1 - numpy.exp(M - m1))
    lse[a, cols] = m2 + numpy.log(S2)
    return numpy.log(p_tar) + M - (lse + numpy.log((1 - p_tar) / (C - 1)))
