"""Float64 numpy restatement of PLDA training (``FactorAnalyser.plda``, sidekit/factor_analyser.py:830-932): the tests' yardstick.

``em(X, labels, rank, ...)`` -> ``(mu, F, Sigma)``.  Two forms of the E-step: ``eigen_form=False`` inverts ``I + n F'F`` once per
distinct session count, as the reference does; ``eigen_form=True`` diagonalises ``F'F`` once per iteration and scales in its
eigenbasis, as the device code does.  Both are pinned against the reference's own output (tests/test_plda_train_cpu.py).
"""
import numpy
import scipy.linalg


def class_sums(X, labels):
    """-> (sorted unique labels, class number per row, rows per class, per-class sums of X in float64)"""
    X = numpy.asarray(X, dtype=numpy.float64)
    ids, inv = numpy.unique(labels, return_inverse=True)
    S = numpy.zeros((ids.shape[0], X.shape[1]))
    numpy.add.at(S, inv, X)
    return ids, inv, numpy.bincount(inv, minlength=ids.shape[0]), S


def em(X, labels, rank, nb_iter=10, scaling_factor=1.0, eigen_form=True):
    X = numpy.asarray(X, dtype=numpy.float64)
    N = X.shape[0]
    mu = X.mean(axis=0)
    centred = X - mu
    sigma_obs = centred.T.dot(centred) / N
    ids, _, counts, S = class_sums(X, labels)
    C = ids.shape[0]
    n, S = counts * scaling_factor, S * scaling_factor
    ev, evec = scipy.linalg.eigh(sigma_obs)
    F = evec[:, numpy.argsort(ev)[::-1][:rank]]
    Sigma = sigma_obs.copy()
    for _ in range(nb_iter):
        lam, V = scipy.linalg.eigh(Sigma)
        order = lam.argsort()[::-1]
        W = V[:, order] * (1.0 / numpy.sqrt(lam[order]))          # whitening transform
        Sw = (S - n[:, None] * mu).dot(W)
        Fw = W.T.dot(F)
        A = Fw.T.dot(Fw)
        P = Sw.dot(Fw)                                            # row i: F_w' s_i
        if eigen_form:
            a, U = numpy.linalg.eigh(A)
            g = 1.0 / (1.0 + n[:, None] * a[None, :])
            Eh = (P.dot(U) * g).dot(U.T)
            sum_inv = (U * g.sum(axis=0)).dot(U.T)
            sum_ninv = (U * (n[:, None] * g).sum(axis=0)).dot(U.T)
        else:
            Eh, sum_inv, sum_ninv, cache = numpy.zeros((C, rank)), numpy.zeros((rank, rank)), numpy.zeros((rank, rank)), {}
            for i in range(C):
                if n[i] not in cache:
                    cache[n[i]] = scipy.linalg.inv(n[i] * A + numpy.eye(rank))
                L = cache[n[i]]
                Eh[i] = P[i].dot(L)
                sum_inv += L
                sum_ninv += n[i] * L
        R = (sum_inv + Eh.T.dot(Eh)) / C
        Am = sum_ninv + (Eh * n[:, None]).T.dot(Eh)
        Cm = Eh.T.dot(Sw).dot(scipy.linalg.inv(W))
        F = scipy.linalg.solve(Am, Cm).T
        Sigma = sigma_obs - F.dot(Cm) / n.sum()
        F = F.dot(scipy.linalg.cholesky(R))
    return mu, F, Sigma


def sign_align(F, F_ref):
    """F with each column's sign set to agree with F_ref's (F is defined up to those signs)."""
    return F * numpy.sign((F * F_ref).sum(axis=0))


def rel(a, b):
    """relative max-norm distance"""
    return numpy.abs(numpy.asarray(a) - numpy.asarray(b)).max() / numpy.abs(b).max()


def ragged_set(seed=5, classes=60, max_sessions=12, dim=48):
    """The ragged training set of tests/golden/plda_train.npz: `classes` classes of 1..max_sessions unit-length sessions, rows
    shuffled, string model ids.  -> X (N, dim) float64, ids (N,) object"""
    rs = numpy.random.RandomState(seed)
    cnt = rs.randint(1, max_sessions + 1, classes)
    lab = numpy.repeat(numpy.arange(classes), cnt)
    centres = rs.randn(classes, dim)
    X = centres[lab] + 1.5 * rs.randn(lab.shape[0], dim)
    X /= numpy.linalg.norm(X, axis=1, keepdims=True)
    p = rs.permutation(X.shape[0])
    return X[p], numpy.array([f"m{l:03d}" for l in lab[p]], dtype="|O")
