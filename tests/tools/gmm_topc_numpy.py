"""float64 numpy restatement of top-C GMM-UBM scoring (include/sidekit_amd/gmm_topc.h), on top of the diagonal-GMM restatement
(mixture_numpy.py) and the dense scoring restatement (gmm_scoring_numpy.py): per frame the ``top_c`` components with the largest log
posterior under the UBM, and the log-likelihoods and ratios of mean-adapted models over those components alone.  The log posterior takes
the direct form, ``-0.5 (sum_d (x - mu)^2 invcov + B)``.  With ``top_c = C`` it is gmm_scoring_numpy's arithmetic, which is held to 1e-12
against the reference's own scores (tests/test_gmm_topc_cpu.py)."""
import numpy

import gmm_scoring_numpy as gsn  # noqa: F401  (the dense restatement this one is compared with)
import mixture_numpy as mxn


def log_posteriors(m, X, mu=None):
    """(N, C) direct-form log posteriors under the mixture with its means replaced by ``mu``"""
    mu = m["mu"] if mu is None else numpy.asarray(mu).reshape(m["mu"].shape)
    with numpy.errstate(divide="ignore"):
        B = -2.0 * (numpy.log(m["w"]) + numpy.log(m["cst"]))
    out = numpy.empty((X.shape[0], mu.shape[0]))
    for c in range(mu.shape[0]):
        out[:, c] = -0.5 * ((numpy.square(X - mu[c]) * m["invcov"][c]).sum(1) + B[c])
    return out


def lists(m, X, top_c, lp=None):
    """(N, K) int32, K = min(top_c, C): the components with the largest log posterior under the mixture (at equal values the lower
    index), stored ascending"""
    lp = log_posteriors(m, X) if lp is None else lp
    K = min(int(top_c), lp.shape[1])
    return numpy.sort(numpy.argsort(-lp, axis=1, kind="stable")[:, :K], axis=1).astype(numpy.int32)


def gap(m, X, top_c):
    """-> (the smallest gap over the frames between the K-th and the (K + 1)-th largest log posterior (inf for K = C), max |lp|)"""
    lp = log_posteriors(m, X)
    K = min(int(top_c), lp.shape[1])
    if K == lp.shape[1]:
        return numpy.inf, numpy.abs(lp).max()
    s = -numpy.sort(-lp, axis=1)
    return float((s[:, K - 1] - s[:, K]).min()), float(numpy.abs(lp).max())


def frame_loglik(m, X, idx, mu=None):
    """log sum_k exp lp[n][idx[n][k]] of every frame under the mixture with its means replaced by ``mu``"""
    if X.shape[0] == 0:
        return numpy.zeros(0)
    return mxn.frame_lse(numpy.take_along_axis(log_posteriors(m, X, mu), idx.astype(numpy.int64), axis=1))


def llk(m, models, X, seg_off, top_c=10, components=None):
    """-> (M, S) sums of the frame log-likelihoods over each frame's list per model and segment, (S,) lengths"""
    idx = lists(m, X, top_c) if components is None else components
    models = numpy.asarray(models).reshape(len(models), -1)
    S = len(seg_off) - 1
    out = numpy.zeros((models.shape[0], S))
    for i, sv in enumerate(models):
        lse = frame_loglik(m, X, idx, sv)
        for s in range(S):
            out[i, s] = lse[seg_off[s]:seg_off[s + 1]].sum()
    return out, numpy.diff(seg_off)


def llr(m, models, X, seg_off, mask=None, top_c=10, components=None):
    """mean frame log-likelihood under each model less the same under the UBM, both over the lists; 0 outside the mask, nan on an empty
    segment"""
    sums, lens = llk(m, list(numpy.asarray(models).reshape(len(models), -1)) + [m["mu"].flatten()], X, seg_off, top_c, components)
    with numpy.errstate(divide="ignore", invalid="ignore"):
        mean = sums / lens
    out = mean[:-1] - mean[-1]
    return out if mask is None else numpy.where(mask, out, 0.0)
