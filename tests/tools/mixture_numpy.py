"""float64 numpy restatement of the diagonal-GMM arithmetic of ``sidekit/mixture.py`` (posteriors :510-536, ``sum_log_probabilities``
:52-64, E-step :586-617, M-step :665-686, split :566-584, ``_init`` :709-719, ``_init_uniform`` :896-924, ``EM_split`` :721-833,
``EM_uniform`` :835-894) and of ``StatServer.accumulate_stat`` (statserver.py:731-739).  The tests' reference: held to 1e-12 against what
the reference's own module computed (tests/golden/mixture.npz, make_mixture_golden.py).  A model is a dict of ``w, mu, invcov,
cov_var_ctl, cst, det, A``."""
import numpy


def compute_all(m):
    m["det"] = 1.0 / numpy.prod(m["invcov"], axis=1)
    m["cst"] = 1.0 / (numpy.sqrt(m["det"]) * (2.0 * numpy.pi) ** (m["mu"].shape[1] / 2.0))
    m["A"] = (numpy.square(m["mu"]) * m["invcov"]).sum(1) - 2.0 * (numpy.log(m["w"]) + numpy.log(m["cst"]))
    return m


def model(w, mu, invcov, cov_var_ctl=None):
    m = {"w": numpy.array(w, dtype=numpy.float64), "mu": numpy.array(mu, dtype=numpy.float64), "invcov": numpy.array(invcov, dtype=numpy.float64)}
    m["cov_var_ctl"] = 1.0 / m["invcov"] if cov_var_ctl is None else numpy.array(cov_var_ctl, dtype=numpy.float64)
    return compute_all(m)


def log_posteriors(m, X, mu=None):
    A = m["A"]
    if mu is None:
        mu = m["mu"]
    else:
        mu = numpy.asarray(mu).reshape(m["mu"].shape)
        A = (numpy.square(mu) * m["invcov"]).sum(1) - 2.0 * (numpy.log(m["w"]) + numpy.log(m["cst"]))
    B = numpy.dot(numpy.square(X), m["invcov"].T) - 2.0 * numpy.dot(X, numpy.transpose(mu * m["invcov"]))
    return -0.5 * (B + A)


def frame_lse(lp):
    top = numpy.max(lp, axis=1)
    return top + numpy.log(numpy.sum(numpy.exp((lp.T - top).T), axis=1))


def sum_log_probabilities(lp):
    lse = frame_lse(lp)
    return numpy.exp((lp.T - lse).T), lse.sum()


def stats(m, X, seg_off=None):
    """-> stat0 (S, C), stat1 (S, C, D), stat2 (S, C, D), llk (S,)"""
    off = [0, X.shape[0]] if seg_off is None else seg_off
    S, (C, D) = len(off) - 1, m["mu"].shape
    s0, s1, s2, llk = numpy.zeros((S, C)), numpy.zeros((S, C, D)), numpy.zeros((S, C, D)), numpy.zeros(S)
    for s in range(S):
        x = X[off[s]:off[s + 1]]
        if x.shape[0] == 0:
            continue
        pp, llk[s] = sum_log_probabilities(log_posteriors(m, x))
        s0[s], s1[s], s2[s] = pp.sum(0), numpy.dot(x.T, pp).T, numpy.dot(numpy.square(x.T), pp).T
    return s0, s1, s2, llk


def variance_control(cov, flooring, ceiling, cov_ctl):
    floor, ceil = flooring * cov_ctl, ceiling * cov_ctl
    lo, hi = cov <= floor, cov >= ceil
    cov = cov.copy()
    cov[lo] = floor[lo]
    cov[hi] = ceil[hi]
    return cov


def maximization(m, s0, s1, s2, ceil_cov=10, floor_cov=1e-2):
    out = {"w": s0 / numpy.sum(s0), "mu": s1 / s0[:, None], "cov_var_ctl": m["cov_var_ctl"]}
    cov = s2 / s0[:, None] - numpy.square(out["mu"])
    out["invcov"] = 1.0 / variance_control(cov, floor_cov, ceil_cov, m["cov_var_ctl"])
    return compute_all(out)


def split(m):
    sigma = 1.0 / m["invcov"]
    shift = numpy.zeros(m["mu"].shape)
    shift[numpy.arange(sigma.shape[0]), numpy.argmax(sigma, axis=1)] = numpy.sqrt(numpy.max(sigma, axis=1))
    return compute_all({"mu": numpy.vstack((m["mu"] - shift, m["mu"] + shift)), "invcov": numpy.vstack((m["invcov"], m["invcov"])),
                        "w": numpy.concatenate([m["w"], m["w"]]) * 0.5, "cov_var_ctl": numpy.vstack((m["cov_var_ctl"], m["cov_var_ctl"]))})


def init_single(X):
    return model([1.0], X.mean(0)[None], 1.0 / (X ** 2).mean(0)[None])


def init_uniform(X, distrib_nb):
    nb = X.shape[0]
    mu, invcov = [], []
    for i in range(distrib_nb):
        start = nb // distrib_nb * i
        end = max(start + 10, nb)
        mu.append(numpy.mean(X[start:end], axis=0))
        cov = (X[start:end] ** 2).mean(0)
        invcov.append(1.0 / cov if i == 0 else cov)
    return model(numpy.full(distrib_nb, 1.0 / distrib_nb), numpy.vstack(mu), numpy.vstack(invcov))


def em_step(m, X, seg_off=None, ceil_cov=10, floor_cov=1e-2, per_frame=False):
    """One E and M step -> (model, llk): llk = sum lse / sum stat0 (EM_split) or / N (EM_uniform, per_frame)"""
    s0, s1, s2, llk = stats(m, X, seg_off)
    s0, s1, s2 = s0.sum(0), s1.sum(0), s2.sum(0)
    return maximization(m, s0, s1, s2, ceil_cov, floor_cov), llk.sum() / (X.shape[0] if per_frame else numpy.sum(s0))


def em_split(X, distrib_nb, iterations, seg_off=None, init_frames=None):
    """-> the list of (model, llk) after every iteration"""
    m = init_single(X if init_frames is None else X[:init_frames])
    trace = []
    for it in iterations[:int(numpy.log2(distrib_nb))]:
        m = split(m)
        for _ in range(it):
            m, llk = em_step(m, X, seg_off)
            trace.append((m, llk))
    return trace


def em_uniform(m, X, iteration_min=3, iteration_max=10, llk_gain=0.01):
    trace = []
    for i in range(iteration_max):
        m, llk = em_step(m, X, per_frame=True)
        trace.append((m, llk))
        if i > 0 and trace[-1][1] - trace[-2][1] < llk_gain and i >= iteration_min:
            break
    return trace


def rel(a, b):
    """relative max-norm distance"""
    return numpy.abs(numpy.asarray(a) - numpy.asarray(b)).max() / numpy.abs(numpy.asarray(b)).max()
