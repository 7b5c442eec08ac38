"""float64 numpy restatement of the full-covariance half of ``sidekit/mixture.py`` (``init_from_diag`` :263-283, ``_compute_all``
:435-445, posteriors :490-508, E-step :586-617, M-step :673-686, ``EM_diag2full`` :926-1009) and of ``StatServer.accumulate_stat`` for a
full-covariance mixture (statserver.py:731-739), with both factors: ``reference_factor=True`` multiplies by ``invchol`` as the reference
does, ``False`` by its transpose, the factor under which ``lp`` is a log density.  The tests' reference: held to 1e-12 against what the
reference's own module computed (tests/golden/mixture_full.npz, make_mixture_full_golden.py).  A model is a dict of ``w, mu, invcov,
invchol, cov_var_ctl, cst, det, A``.  Nothing here builds an ``N x D x D`` array: the second order statistic is ``X' diag(pp) X``."""
import numpy

from mixture_numpy import rel, sum_log_probabilities  # noqa: F401


def compute_all(m):
    C, D = m["mu"].shape
    m["det"] = numpy.array([1.0 / numpy.linalg.det(m["invcov"][c]) for c in range(C)])
    m["invchol"] = numpy.stack([numpy.linalg.cholesky(m["invcov"][c]) for c in range(C)])
    m["cst"] = 1.0 / (numpy.sqrt(m["det"]) * (2.0 * numpy.pi) ** (D / 2.0))
    m["A"] = numpy.zeros(C)
    return m


def model(w, mu, invcov):
    """A full-covariance model from its weights, means and (C, D, D) inverse covariances"""
    m = {"w": numpy.array(w, dtype=numpy.float64), "mu": numpy.array(mu, dtype=numpy.float64), "invcov": numpy.array(invcov, dtype=numpy.float64),
         "cov_var_ctl": numpy.array([])}
    return compute_all(m)


def init_from_diag(d):
    """``d``: a diagonal model (mixture_numpy.model).  ``det`` and ``cst`` are the diagonal model's own, as in the reference."""
    C = d["w"].shape[0]
    invcov = numpy.stack([numpy.diag(d["invcov"][c]) for c in range(C)])
    return {"w": d["w"].copy(), "mu": d["mu"].copy(), "cst": d["cst"].copy(), "det": d["det"].copy(), "invcov": invcov,
            "invchol": numpy.stack([numpy.linalg.cholesky(invcov[c]) for c in range(C)]), "cov_var_ctl": numpy.diag(d["cov_var_ctl"]).copy(),
            "A": numpy.zeros(C)}


def factor(m, reference_factor):
    return m["invchol"] if reference_factor else m["invchol"].transpose(0, 2, 1)


def log_posteriors(m, X, reference_factor=False, mu=None, M=None):
    """lp (N, C) = log w + log cst - 0.5 |M (x - mu)|^2, component by component; ``M``: an explicit (C, D, D) factor"""
    mu = m["mu"] if mu is None else numpy.asarray(mu).reshape(m["mu"].shape)
    M = factor(m, reference_factor) if M is None else M
    lp = numpy.empty((X.shape[0], mu.shape[0]))
    with numpy.errstate(divide="ignore"):
        g = numpy.log(m["w"]) + numpy.log(m["cst"])
    for c in range(mu.shape[0]):
        y = numpy.dot(X - mu[c], M[c].T)
        lp[:, c] = g[c] - 0.5 * (y * y).sum(1)
    return lp


def stats(m, X, seg_off=None, reference_factor=False, M=None):
    """-> stat0 (S, C), stat1 (S, C, D), stat2 (S, C, D, D), llk (S,)"""
    off = [0, X.shape[0]] if seg_off is None else seg_off
    S, (C, D) = len(off) - 1, m["mu"].shape
    s0, s1, s2, llk = numpy.zeros((S, C)), numpy.zeros((S, C, D)), numpy.zeros((S, C, D, D)), numpy.zeros(S)
    for s in range(S):
        x = X[off[s]:off[s + 1]]
        if x.shape[0] == 0:
            continue
        pp, llk[s] = sum_log_probabilities(log_posteriors(m, x, reference_factor, M=M))
        s0[s], s1[s] = pp.sum(0), numpy.dot(x.T, pp).T
        for c in range(C):
            s2[s, c] = numpy.dot(x.T * pp[:, c], x)
    return s0, s1, s2, llk


def maximization(s0, s1, s2):
    mu = s1 / s0[:, None]
    cov = s2 / s0[:, None, None] - mu[:, :, None] * mu[:, None, :]
    out = {"w": s0 / numpy.sum(s0), "mu": mu, "invcov": numpy.stack([numpy.linalg.inv(cov[c]) for c in range(cov.shape[0])]),
           "cov_var_ctl": numpy.array([])}
    return compute_all(out)


def em_step(m, X, reference_factor=False):
    """One E and M step -> (model, llk per unit of occupation, (s0, s1, s2, total llk))"""
    s0, s1, s2, llk = stats(m, X, None, reference_factor)
    return maximization(s0[0], s1[0], s2[0]), llk[0] / numpy.sum(s0[0]), (s0[0], s1[0], s2[0], llk[0])


def em_diag2full(d, X, iterations=2, reference_factor=False):
    """-> the list of (model, llk) after every iteration, from the diagonal model ``d``"""
    m, trace = init_from_diag(d), []
    for _ in range(iterations):
        m, llk, _ = em_step(m, X, reference_factor)
        trace.append((m, llk))
    return trace
