"""Float64 numpy restatement of the back-end normalisations (within / between / total covariance, LDA, WCCN, Mahalanobis, spectral
normalisation: sidekit/statserver.py:797-1054, 1279-1333), written from their published definitions: the tests' yardstick.
tests/test_backend_cpu.py pins it to the reference's own output (tests/golden/backend.npz).

Classes are grouped once (``numpy.unique``) instead of one scan of all labels per class; every function takes the rows ``X`` (N, D)
and one label per row.
"""
import numpy
import scipy.linalg


def moments(X, labels):
    """-> (mean, class number per row, rows per class, class means)"""
    X = numpy.asarray(X, dtype=numpy.float64)
    ids, inv = numpy.unique(labels, return_inverse=True)
    counts = numpy.bincount(inv, minlength=ids.shape[0]).astype(numpy.float64)
    S = numpy.zeros((ids.shape[0], X.shape[1]))
    numpy.add.at(S, inv, X)
    return X.mean(axis=0), inv, counts, S / counts[:, None]


def scatter_within(X, cls, class_means, weights=None):
    """sum_k w[cls[k]] (x_k - m_cls[k])' (x_k - m_cls[k]), centred before it is squared"""
    X = numpy.asarray(X, dtype=numpy.float64)
    Z = X - class_means[cls]
    return (Z if weights is None else Z * numpy.asarray(weights)[cls][:, None]).T.dot(Z)


def covariances(X, labels):
    """-> (mean, within, between, total), each over N"""
    X = numpy.asarray(X, dtype=numpy.float64)
    mu, cls, counts, Mc = moments(X, labels)
    N = X.shape[0]
    Zc = Mc - mu
    return mu, scatter_within(X, cls, Mc) / N, (Zc * counts[:, None]).T.dot(Zc) / N, (X - mu).T.dot(X - mu) / N


def lda_spectrum(X, labels):
    """eigenvalues (ascending) and eigenvectors of the matrix the reference's LDA diagonalises: ``scipy.linalg.eigh`` of
    ``(Sb . inv(Sw))'`` -- not symmetric, LAPACK reads its lower triangle; Sb unweighted, Sw weighted by 1 / n_c"""
    X = numpy.asarray(X, dtype=numpy.float64)
    mu, cls, counts, Mc = moments(X, labels)
    Sw = scatter_within(X, cls, Mc, 1.0 / counts)
    Sb = (Mc - mu).T.dot(Mc - mu)
    return scipy.linalg.eigh(Sb.dot(scipy.linalg.inv(Sw)).T)


def lda(X, labels, rank):
    ev, evec = lda_spectrum(X, labels)
    return evec[:, ev.argsort()[-rank:][::-1]]


def wccn(X, labels):
    """lower Cholesky factor of the inverse of the class-averaged within-class covariance"""
    X = numpy.asarray(X, dtype=numpy.float64)
    _, cls, counts, Mc = moments(X, labels)
    W = scatter_within(X, cls, Mc, 1.0 / counts) / counts.shape[0]
    return scipy.linalg.cholesky(scipy.linalg.inv(W)).T


def mahalanobis(X, labels):
    return scipy.linalg.inv(covariances(X, labels)[1])


def whitening_transform(sigma):
    """V diag(lambda^-1/2), eigenvalues descending (not the symmetric inverse square root); a 1-D sigma is a diagonal covariance"""
    sigma = numpy.asarray(sigma, dtype=numpy.float64)
    if sigma.ndim == 1:
        return numpy.diag(1.0 / numpy.sqrt(sigma))
    lam, V = scipy.linalg.eigh(sigma)
    order = lam.argsort()[::-1]
    return V[:, order] * (1.0 / numpy.sqrt(lam[order]))


def cholesky_transform(sigma):
    """what whiten_cholesky_stat1 multiplies by: the lower Cholesky factor of inv(sigma), or 1 / sqrt of a diagonal covariance (1-D)"""
    sigma = numpy.asarray(sigma, dtype=numpy.float64)
    if sigma.ndim == 1:
        return numpy.diag(1.0 / numpy.sqrt(sigma))
    return scipy.linalg.cholesky(scipy.linalg.inv(sigma)).T


def whiten_rows(X, mu, R, normalize):
    """f((X - mu) . R), f = identity or v / max(|v|, 1e-8)"""
    Y = numpy.asarray(X, dtype=numpy.float64)
    if mu is not None:
        Y = Y - mu
    Y = Y.dot(R)
    if normalize:
        Y = Y / numpy.maximum(numpy.sqrt((Y * Y).sum(axis=1)), 1e-8)[:, None]
    return Y


def spectral_norm_estimate(X, labels, it=1, mode="efr"):
    """-> (means, covs, transformed rows)"""
    cur = numpy.asarray(X, dtype=numpy.float64)
    means, covs = [], []
    for _ in range(it):
        mu, within, _, total = covariances(cur, labels)
        means.append(mu)
        covs.append(total if mode == "efr" else within)
        cur = whiten_rows(cur, mu, whitening_transform(covs[-1]), True)
    return means, covs, cur


def spectral_norm_apply(X, means, covs, is_sqr_inv_sigma=False):
    cur = numpy.asarray(X, dtype=numpy.float64)
    for mu, cov in zip(means, covs):
        cur = whiten_rows(cur, mu, cov if is_sqr_inv_sigma else whitening_transform(cov), True)
    return cur


def sorted_eigenvalues(cov):
    return numpy.sort(scipy.linalg.eigvalsh(cov))


def top_gap(eigenvalues, rank):
    """smallest gap among the top rank + 1 eigenvalues over the largest one: what an eigenvector comparison is conditioned on"""
    top = numpy.sort(eigenvalues)[::-1][:rank + 1]
    return numpy.abs(numpy.diff(top)).min() / top[0]
