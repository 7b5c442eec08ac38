"""float64 numpy restatement of GMM-UBM verification: MAP adaptation of the means (``sidekit/statserver.py:1075-1157``) and the
log-likelihood ratios of ``sidekit/gmm_scoring.py:53-116``, on top of the diagonal-GMM restatement (mixture_numpy.py).  The tests'
reference: held to 1e-12 against what the reference's own modules computed (tests/golden/gmm_scoring.npz,
make_gmm_scoring_golden.py).  A model is mixture_numpy's dict; statistics are ``stat0`` (S, C) and ``stat1`` (S, C D)."""
import numpy

import mixture_numpy as mxn

EPS32 = numpy.finfo(numpy.float32).eps


def _adapt(m, stat0, stat1, alpha, norm):
    C, D = m["mu"].shape
    s1 = stat1.reshape(stat0.shape[0], C, D)
    with numpy.errstate(divide="ignore", invalid="ignore"):
        mean = s1 / stat0[:, :, None]
    mean = numpy.where(numpy.isnan(mean), 0.0, mean)
    out = alpha[:, :, None] * mean + (1.0 - alpha[:, :, None]) * m["mu"][None]
    if norm:
        out = out * numpy.sqrt(m["w"][None, :, None] * m["invcov"][None])
    return out.reshape(stat0.shape[0], C * D)


def adapt_mean_map(m, stat0, stat1, r=16, norm=False):
    """one model per session; float32 eps inside alpha only -> (S, C D)"""
    return _adapt(m, stat0, stat1, (stat0 + EPS32) / (stat0 + EPS32 + r), norm)


def sum_per_model(modelset, stat0, stat1):
    """-> sorted unique ids, summed stat0, summed stat1 (sessions of an id added in row order)"""
    ids = numpy.unique(modelset)
    s0 = numpy.stack([stat0[modelset == i].sum(0) for i in ids])
    s1 = numpy.stack([stat1[modelset == i].sum(0) for i in ids])
    return ids, s0, s1


def adapt_mean_map_multisession(m, modelset, stat0, stat1, r=16, norm=False):
    """one model per id from the summed statistics; no eps -> (ids, (K, C D))"""
    ids, s0, s1 = sum_per_model(modelset, stat0, stat1)
    return ids, _adapt(m, s0, s1, s0 / (s0 + r), norm)


def frame_loglik(m, X, mu=None):
    """log sum_c exp lp[n][c] of every frame under the mixture with its means replaced by ``mu``"""
    return mxn.frame_lse(mxn.log_posteriors(m, X, mu))


def llk(m, models, X, seg_off):
    """-> (M, S) sums of the frame log-likelihoods per model and segment, (S,) lengths"""
    models = numpy.asarray(models).reshape(len(models), -1)
    S = len(seg_off) - 1
    out = numpy.zeros((models.shape[0], S))
    for i, sv in enumerate(models):
        lse = frame_loglik(m, X, sv)
        for s in range(S):
            out[i, s] = lse[seg_off[s]:seg_off[s + 1]].sum()
    return out, numpy.diff(seg_off)


def llr(m, models, X, seg_off, mask=None):
    """mean frame log-likelihood under each model less the same under the UBM; 0 outside the mask, nan on an empty segment"""
    sums, lens = llk(m, list(numpy.asarray(models).reshape(len(models), -1)) + [m["mu"].flatten()], X, seg_off)
    with numpy.errstate(divide="ignore", invalid="ignore"):
        mean = sums / lens
    out = mean[:-1] - mean[-1]
    return out if mask is None else numpy.where(mask, out, 0.0)


def margin_range(m, models, X):
    """the smallest and largest per-frame, per-component ``lp_m - lse_ubm`` over the models"""
    base = frame_loglik(m, X)
    d = [mxn.log_posteriors(m, X, sv) - base[:, None] for sv in numpy.asarray(models).reshape(len(models), -1)]
    return float(min(x.min() for x in d)), float(max(x.max() for x in d))
