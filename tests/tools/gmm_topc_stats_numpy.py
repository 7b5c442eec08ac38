"""float64 numpy restatement of top-C Baum-Welch statistics (include/sidekit_amd/gmm_topc_stats.h), on top of the top-C scoring
restatement (gmm_topc_numpy.py: the direct-form log posterior).  The lists are an input: the GPU tests evaluate it on the device's own
lists (exact operands), so a near-tie between two log posteriors cannot make a test flaky.  With every component listed it is
mixture_numpy.stats, which is held to 1e-12 against the reference's own module (tests/test_gmm_topc_stats_cpu.py)."""
import numpy

import gmm_topc_numpy as gtn


def posteriors(m, X, idx):
    """-> post (N, K), lse (N,): the posteriors renormalised over each frame's list and the log of the list's sum.  An entry outside
    [0, C) contributes nothing; an entry with lp = -inf gets 0; a frame with no finite entry has lse = -inf and posteriors 0."""
    C = m["mu"].shape[0]
    idx = numpy.asarray(idx).astype(numpy.int64)
    valid = (idx >= 0) & (idx < C)
    lp = numpy.take_along_axis(gtn.log_posteriors(m, X), numpy.where(valid, idx, 0), axis=1)
    lp = numpy.where(valid, lp, -numpy.inf)
    top = lp.max(axis=1)
    some = numpy.isfinite(top)
    lse = numpy.full(X.shape[0], -numpy.inf)
    lse[some] = top[some] + numpy.log(numpy.exp(lp[some] - top[some, None]).sum(1))
    post = numpy.zeros(lp.shape)
    post[some] = numpy.exp(lp[some] - lse[some, None])
    return post, lse


def stats(m, X, idx, seg_off=None):
    """-> stat0 (S, C), stat1 (S, C, D), stat2 (S, C, D), llk (S,), post (N, K), lse (N,)"""
    off = [0, X.shape[0]] if seg_off is None else seg_off
    S, (C, D) = len(off) - 1, m["mu"].shape
    idx = numpy.asarray(idx).astype(numpy.int64)
    post, lse = posteriors(m, X, idx)
    s0, s1, s2, llk = numpy.zeros((S, C)), numpy.zeros((S, C, D)), numpy.zeros((S, C, D)), numpy.zeros(S)
    K = idx.shape[1]
    for s in range(S):
        rows = slice(off[s], off[s + 1])
        c, p, x = idx[rows].ravel(), post[rows].ravel(), numpy.repeat(X[rows], K, axis=0)
        keep = (c >= 0) & (c < C) & (p != 0.0)      # what adds nothing is not multiplied either: 0 x nan
        c, p, x = c[keep], p[keep], x[keep]
        numpy.add.at(s0[s], c, p)
        numpy.add.at(s1[s], c, p[:, None] * x)
        numpy.add.at(s2[s], c, p[:, None] * numpy.square(x))
        llk[s] = lse[rows].sum()
    return s0, s1, s2, llk, post, lse
