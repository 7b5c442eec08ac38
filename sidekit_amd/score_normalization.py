"""Score normalisation -- mirror of ``sidekit/score_normalization.py``: ``asnorm`` (:120-140, the normalisation behind the reference's
"norm EER", ``sidekit/nnet/xvector.py:261``), ``znorm`` (:44-72), ``tnorm`` (:75-93) and ``ztnorm`` (:96-117), plus the device-level forms a
real trial list needs: an enrolment x test matrix normalised against an impostor cohort without ever forming the cohort score matrix.

``asnorm``: all-vs-all cosine scores of the enrolment x-vectors, cohort scores against the L2-normalised cohort,
mean / std of each row's 200 best cohort scores, then the symmetric normalisation
``0.5 (s - m_i)/sd_i + 0.5 (s - m_j)/sd_j``.  On the GPU: two f32 MFMA GEMMs (``sc_cosine``), an exact
radix-select top-k statistics kernel (``sc_topk_stats``) and an elementwise pass (``sc_snorm_apply``).

Cohort statistics over the WHOLE cohort (z-, t-, zt-, plain s-norm) come from ``sc_cohort_moments``: per-row float64 sums taken from the
accumulators of the cosine GEMM.  The adaptive (top-k) statistics need the scores themselves; they run over row blocks whose score buffer
stays inside ``max_workspace_bytes``.  The ``Scores``-level functions receive host matrices: ``sc_matrix_moments`` + ``sc_norm_apply``.

Two stated deviations from the reference's ``znorm`` ("Score normalisation"): the per-model statistics are applied
along rows (the reference's line 70 broadcasts them along the segment axis: it raises unless the matrix is square, and then normalises
columns), and with ``sym=True`` the std is the square root of the variance of the ``n - 1`` off-diagonal values (lines 64-66 omit the
root and centre along the wrong axis).

PLDA log-likelihood ratios get the same in float64 (``plda_cohort_stats_device``, ``plda_znorm_device`` / ``plda_tnorm_device`` /
``plda_snorm_device``, ``plda_normalised_histograms``, ``plda_normalised_range_from_sample``): what this module's reference functions
applied to ``fast_PLDA_scoring`` output amount to, with the statistics from ``sc_plda_cohort_moments``.

``normalised_histograms`` is the form for trial sets whose (Ne, Nt) matrix does not fit: the z-, t-, s- or adaptive s-normalised scores of
every pair counted into target / non-target histograms (``iv_scoring.cosine_histograms`` with the statistics of ``cohort_stats_device``;
``sc_cosine_hist_norm`` normalises each score between the GEMM's accumulator and its bin, in ``sc_norm_apply``'s expressions, so the counts
are those of the materialised path).  ``normalised_range_from_sample`` proposes its ``lo`` / ``hi``.  zt-norm is not offered there: it is a
t-norm against a z-normalised cohort, a different chain of expressions from the three ``sc_norm_apply`` has.

Every rule of this module is written once, against a scorer (``iv_scoring.CosineScorer`` / ``iv_scoring.PldaScorer``: element type, entry
points, the arguments that follow ``D``, whether the two sides share statistics); the public functions run their own checks and call it.
"""
import copy

import numpy
import torch

from . import _lib, iv_scoring
from .iv_scoring import CosineScorer, PldaScorer, _to_device, normalize_rows_device


def asnorm(enrol_xv, cohort_xv, ndx=None, topk=200, device=None):
    """Same arguments as the reference (``ndx`` is unused there too); returns the (N, N) float32 numpy matrix."""
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    e = _to_device(enrol_xv, torch.float32, device)
    c = _cohort_on(device, cohort_xv, True)                                               # F.normalize of the cohort, on the device
    n, d = e.shape
    if d % 4 or c.shape[1] != d:
        raise ValueError("x-vector dimension must match and be a multiple of 4")
    scores = iv_scoring._matrix(CosineScorer.matrix, e, e, exc=ValueError)
    calib = iv_scoring._matrix(CosineScorer.matrix, e, c, exc=ValueError)
    mean = torch.empty(n, dtype=torch.float32, device=device)
    std = torch.empty(n, dtype=torch.float32, device=device)
    _lib.launch(CosineScorer.topk, device, calib, n, c.shape[0], int(topk), mean, std)
    _lib.launch("sc_snorm_apply", device, scores, n, n, mean, std, mean, std)
    return scores.cpu().numpy()


# ---- device level ----------------------------------------------------------------------------------------------------------------
_NO_GPU = "sidekit_amd computes on the GPU only (no CPU fallback) and no GPU is visible"


def _shape2(x, what):
    shape = tuple(x.shape)
    if len(shape) != 2:
        raise ValueError(f"{what} must be a matrix, got shape {shape}")
    return shape


def _check_xv(xv, cohort_xv, what="x-vectors"):
    """Shape checks that need no device: (N, D) against (M, D), D a multiple of 4 (the GEMM's k granularity), a non-empty cohort."""
    (n, d), (m, dc) = _shape2(xv, what), _shape2(cohort_xv, "cohort")
    if dc != d or d % 4:
        raise ValueError(f"x-vector dimension must match and be a multiple of 4 ({what}: {d}, cohort: {dc})")
    if m == 0:
        raise ValueError("the cohort is empty")
    return n, m, d


def _check_topk(topk, m):
    if not 1 < int(topk) <= m:
        raise ValueError(f"need 1 < topk <= cohort size (topk={topk}, cohort={m})")


def _check_kind(kind, topk, m):
    if kind not in ("z", "t", "s"):
        raise ValueError(f"kind is 'z', 't' or 's' (zt-norm has no histogram form), got {kind!r}")
    if topk is not None:
        if kind != "s":
            raise ValueError("topk (adaptive statistics) goes with kind='s' only")
        _check_topk(topk, m)


def _check_scores(scorer, scores, ne, nt):
    if not (torch.is_tensor(scores) and scores.is_cuda and scores.dtype == scorer.dtype and scores.is_contiguous()):
        raise ValueError(f"scores must be a contiguous {str(scorer.dtype).split('.')[1]} device tensor (it is normalised in place)")
    if scores.dim() != 2 or (ne is not None and scores.shape[0] != ne) or (nt is not None and scores.shape[1] != nt):
        raise ValueError(f"scores have shape {tuple(scores.shape)}, the x-vectors say ({ne if ne is not None else 'any'}, {nt if nt is not None else 'any'})")


def _device_of(*xs):
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


def _cohort_on(device, cohort_xv, normalize):
    if normalize:
        return normalize_rows_device(torch.as_tensor(cohort_xv, dtype=torch.float32), device)
    return _to_device(cohort_xv, torch.float32, device)


# ---- the rules, once: each takes a scorer and operands that passed the caller's checks ----------------------------------------------
def _cohort_stats(scorer, x, c, side="enrol", topk=None, self_offset=None, max_workspace_bytes=1 << 30):
    """``(mean, std)`` per row of ``x`` against the cohort ``c`` (both prepared by ``scorer.vectors``).  ``topk=None``: the moments of the
    whole cohort, the scores never stored; else the top-k statistics over row blocks whose (rows, M) score buffer fits in
    ``max_workspace_bytes``.  ``side="test"`` scores ``s(c, x)``."""
    (n, d), m = x.shape, c.shape[0]
    mean = torch.empty(n, dtype=scorer.dtype, device=x.device)
    std = torch.empty(n, dtype=scorer.dtype, device=x.device)
    if topk is None:
        _lib.launch(scorer.moments, x.device, x, n, c, m, d, *scorer.group(side, moments=True), -1 if self_offset is None else int(self_offset),
                    mean, std)
    elif n:
        rows = max(1, min(n, int(max_workspace_bytes) // (mean.element_size() * m)))
        calib = torch.empty((rows, m), dtype=scorer.dtype, device=x.device)
        for r0 in range(0, n, rows):
            nr = min(rows, n - r0)
            _lib.launch(scorer.matrix, x.device, x[r0:], nr, c, m, d, *scorer.group(side), calib)
            _lib.launch(scorer.topk, x.device, calib, nr, m, int(topk), mean[r0:], std[r0:])
    return mean, std


def _side_stats(scorer, kind, enroll_xv, test_xv, cohort_xv, topk=None, max_workspace_bytes=1 << 30):
    """(enrolment pair, test pair) of ``kind``: the side a kind does not use is ``None``.  The cohort is prepared once; ``test_xv is
    enroll_xv`` prepares the vectors once and, where the scorer's two sides score alike, computes the statistics once."""
    e, c = scorer.vectors(enroll_xv, cohort_xv)
    en = _cohort_stats(scorer, e, c, "enrol", topk, None, max_workspace_bytes) if kind in ("z", "s") else None
    if kind == "z":
        return en, None
    if kind == "s" and test_xv is enroll_xv and scorer.shares_sides:
        return en, en
    t = e if test_xv is enroll_xv else scorer.vectors(test_xv, test_xv)[0]
    return en, _cohort_stats(scorer, t, c, "test", topk, None, max_workspace_bytes)


def _apply(scorer, scores, enrol=None, test=None):
    """``scorer.apply`` in place: ``enrol`` / ``test`` are (mean, std) pairs or None."""
    _lib.launch(scorer.apply, scores.device, scores, scores.shape[0], scores.shape[1], *(enrol or (None, None)), *(test or (None, None)))
    return scores


def _norm_device(scorer, kind, scores, enroll_xv, test_xv, cohort_xv, topk=None, max_workspace_bytes=1 << 30):
    """z-, t- or s-norm of a resident score matrix, in place; z and t prepare and use their own side only."""
    if kind == "z":
        return _apply(scorer, scores, enrol=_cohort_stats(scorer, *scorer.vectors(enroll_xv, cohort_xv), "enrol"))
    if kind == "t":
        return _apply(scorer, scores, test=_cohort_stats(scorer, *scorer.vectors(test_xv, cohort_xv), "test"))
    return _apply(scorer, scores, *_side_stats(scorer, "s", enroll_xv, test_xv, cohort_xv, topk, max_workspace_bytes))


# ---- cosine scores ---------------------------------------------------------------------------------------------------------------
def cohort_stats_device(xv, cohort_xv, topk=None, self_offset=None, col_shift=None, col_scale=None, max_workspace_bytes=1 << 30,
                        normalize=False):
    """Per row of ``xv`` (N, D): ``(mean, std)`` of its cosine scores against the cohort (M, D), float32 **device tensors**; rows are used
    as given (``normalize=True`` L2-normalises the cohort first, as the reference's ``asnorm`` does).

    ``topk=None``: every cohort score counts, population std (``sc_cohort_moments``; the (N, M) scores are never stored).  ``self_offset``
    drops the pair ``j == i + self_offset`` (``xv`` is a row range of the cohort); ``col_shift`` / ``col_scale`` (M each, together) turn
    the scores into ``(s_ij - shift_j) * scale_j`` first: cohort scores that were themselves z-normalised, for zt-norm.
    ``topk=k``: mean and unbiased std of the k best cohort scores (``sc_topk_stats``), over row blocks whose (rows, M) float32 score
    buffer fits in ``max_workspace_bytes``."""
    n, m, d = _check_xv(xv, cohort_xv)
    if (col_shift is None) != (col_scale is None):
        raise ValueError("col_shift and col_scale come together")
    if topk is not None:
        if self_offset is not None or col_shift is not None:
            raise ValueError("self_offset / col_shift / col_scale apply to whole-cohort statistics (topk=None) only")
        _check_topk(topk, m)
    if col_shift is not None and (tuple(col_shift.shape) != (m,) or tuple(col_scale.shape) != (m,)):
        raise ValueError(f"col_shift and col_scale must have one entry per cohort row ({m})")
    device = _device_of(xv, cohort_xv)
    x = _to_device(xv, torch.float32, device)
    return _cohort_stats(CosineScorer(device, col_shift, col_scale), x, _cohort_on(device, cohort_xv, normalize), "enrol", topk, self_offset,
                         max_workspace_bytes)


def znorm_device(scores, enroll_xv, cohort_xv, normalize=False):
    """z-norm of a device (Ne, Nt) float32 score tensor, in place: ``(s_ij - m_i) / sd_i`` with the statistics of enrolment i's cohort scores."""
    _check_xv(enroll_xv, cohort_xv, "enrolment x-vectors")
    _check_scores(CosineScorer, scores, enroll_xv.shape[0], None)
    device = _device_of(enroll_xv, cohort_xv)
    return _norm_device(CosineScorer(device), "z", scores, enroll_xv, None, _cohort_on(device, cohort_xv, normalize))


def tnorm_device(scores, test_xv, cohort_xv, normalize=False):
    """t-norm, in place: ``(s_ij - m_j) / sd_j`` with the statistics of test segment j's cohort scores."""
    _check_xv(test_xv, cohort_xv, "test x-vectors")
    _check_scores(CosineScorer, scores, None, test_xv.shape[0])
    device = _device_of(test_xv, cohort_xv)
    return _norm_device(CosineScorer(device), "t", scores, None, test_xv, _cohort_on(device, cohort_xv, normalize))


def snorm_device(scores, enroll_xv, test_xv, cohort_xv, topk=None, normalize=False, max_workspace_bytes=1 << 30):
    """s-norm, in place: ``0.5 ((s - m_i)/sd_i + (s - m_j)/sd_j)``; ``topk=k`` makes it adaptive (statistics of each side's k best
    cohort scores, unbiased std, as ``asnorm``).  ``test_xv is enroll_xv`` computes the statistics once."""
    _, m, _ = _check_xv(enroll_xv, cohort_xv, "enrolment x-vectors")
    _check_xv(test_xv, cohort_xv, "test x-vectors")
    _check_scores(CosineScorer, scores, enroll_xv.shape[0], test_xv.shape[0])
    if normalize:
        cohort_xv = _cohort_on(scores.device, cohort_xv, True)
    if topk is not None:
        _check_topk(topk, m)
    scorer = CosineScorer(_device_of(enroll_xv, test_xv, cohort_xv))
    return _norm_device(scorer, "s", scores, enroll_xv, test_xv, cohort_xv, topk, max_workspace_bytes)


def ztnorm_device(scores, enroll_xv, test_xv, cohort_xv, normalize=False):
    """z-norm followed by t-norm against the z-normalised cohort (``ztnorm``, :96-117, with ``znorm`` as this module defines it), in place;
    neither the cohort x cohort nor the cohort x test matrix is formed."""
    _check_xv(enroll_xv, cohort_xv, "enrolment x-vectors")
    _check_xv(test_xv, cohort_xv, "test x-vectors")
    _check_scores(CosineScorer, scores, enroll_xv.shape[0], test_xv.shape[0])
    cohort = _cohort_on(scores.device, cohort_xv, normalize)
    m_c, sd_c = cohort_stats_device(cohort, cohort, self_offset=0)                         # znorm(imp_test, imp_imp, sym=True): per cohort model
    test = cohort_stats_device(test_xv, cohort, col_shift=m_c, col_scale=1.0 / sd_c)       # tnorm's statistics of the z-normalised imp_test
    _apply(CosineScorer, scores, enrol=cohort_stats_device(enroll_xv, cohort))             # znorm(enrol_test, enrol_imp)
    return _apply(CosineScorer, scores, test=test)


def asnorm_trials(enroll_xv, test_xv, cohort_xv, topk=200, normalize=True, max_workspace_bytes=1 << 30):
    """Adaptive s-norm of an enrolment x test trial set: the (Ne, Nt) normalised cosine matrix as a float32 **device tensor**.  With
    ``test_xv is enroll_xv`` this is ``asnorm``."""
    _, m, _ = _check_xv(enroll_xv, cohort_xv, "enrolment x-vectors")
    _check_xv(test_xv, cohort_xv, "test x-vectors")
    _check_topk(topk, m)
    e, t = CosineScorer(_device_of(enroll_xv, test_xv, cohort_xv)).vectors(enroll_xv, test_xv)
    scores = iv_scoring._matrix(CosineScorer.matrix, e, t, exc=ValueError)
    return snorm_device(scores, e, t, cohort_xv, topk=topk, normalize=normalize, max_workspace_bytes=max_workspace_bytes)


def normalised_histograms(enroll_xv, test_xv, enroll_labels, test_labels, cohort_xv, kind="s", topk=None, normalize=False, self_offset=None, *,
                          lo=None, hi=None, bins=None, max_workspace_bytes=1 << 30):
    """Target / non-target histograms ``(hist_tar, hist_non)`` of the cohort-normalised cosine scores of ALL (enrol, test) pairs; neither
    the (Ne, Nt) score matrix nor (with ``topk=None``) a cohort score matrix is formed.  ``kind``: ``"z"`` (``znorm_device``'s
    expression), ``"t"`` (``tnorm_device``'s) or ``"s"`` (``snorm_device``'s); ``topk=k``, with ``"s"`` only, is adaptive s-norm with
    ``asnorm``'s unbiased std.  ``normalize=True`` L2-normalises the cohort first.  ``test_xv is enroll_xv`` computes the statistics once.
    ``self_offset``, ``bins`` and the labels are ``iv_scoring.cosine_histograms``'s.  ``lo`` / ``hi`` are required keywords: normalised scores have
    no natural range (``normalised_range_from_sample`` estimates one).  zt-norm is not offered (see the module docstring)."""
    _, m, _ = _check_xv(enroll_xv, cohort_xv, "enrolment x-vectors")
    _check_xv(test_xv, cohort_xv, "test x-vectors")
    _check_kind(kind, topk, m)
    if lo is None or hi is None:
        raise ValueError("lo and hi are required keywords: normalised scores have no default range (normalised_range_from_sample estimates one)")
    if not float(hi) > float(lo):
        raise ValueError("histogram range: hi must exceed lo")
    device = _device_of(enroll_xv, test_xv, cohort_xv)
    scorer = CosineScorer(device)
    e, t = scorer.vectors(enroll_xv, test_xv)
    en, tn = _side_stats(scorer, kind, e, t, _cohort_on(device, cohort_xv, normalize), topk, max_workspace_bytes)
    return iv_scoring.cosine_histograms(e, t, enroll_labels, test_labels, self_offset=self_offset, lo=lo, hi=hi, device=device, bins=bins,
                                        enroll_norm=en, test_norm=tn)


def normalised_range_from_sample(enroll_xv, test_xv, cohort_xv, kind="s", topk=None, normalize=False):
    """``(lo, hi)`` for ``normalised_histograms``: a strided sample of at most 2 048 rows per side, its materialised score matrix
    normalised by ``znorm_device`` / ``tnorm_device`` / ``snorm_device`` against the whole cohort, and the sample's smallest and largest
    normalised score, each widened by a quarter of the sampled range (what still falls outside is counted in the end bins)."""
    _, m, _ = _check_xv(enroll_xv, cohort_xv, "enrolment x-vectors")
    _check_xv(test_xv, cohort_xv, "test x-vectors")
    _check_kind(kind, topk, m)
    device = _device_of(enroll_xv, test_xv, cohort_xv)
    scorer = CosineScorer(device)
    e, t = scorer.vectors(enroll_xv, test_xv)
    cohort = _cohort_on(device, cohort_xv, normalize)
    return iv_scoring._range_from_sample(scorer, e, t, lambda z, es, ts: _norm_device(scorer, kind, z, es, ts, cohort, topk))


# ---- PLDA log-likelihood ratios: the same normalisations in float64 -----------------------------------------------------------------
def _plda_model(xv, cohort_xv, mu, F, Sigma, G, what="x-vectors"):
    """Every check of ``xv`` against the cohort that needs no device (``iv_scoring._plda_checks``); the model ``PldaScorer`` takes."""
    _shape2(xv, what), _shape2(cohort_xv, "cohort")
    if cohort_xv.shape[0] == 0:
        raise ValueError("the cohort is empty")
    return iv_scoring._plda_checks(xv, cohort_xv, None, None, mu, F, Sigma, G)


def _check_plda_topk(topk, self_offset, m):
    if topk is not None:
        if self_offset is not None:
            raise ValueError("self_offset applies to whole-cohort statistics (topk=None) only")
        _check_topk(topk, m)


def plda_cohort_stats_device(xv, cohort_xv, mu, F, Sigma, G=None, scaling_factor=1., side="enrol", topk=None, self_offset=None,
                             max_workspace_bytes=1 << 30):
    """Per row of ``xv`` (N, D): ``(mean, std)`` of its PLDA log-likelihood ratios against the cohort (M, D), float64 **device tensors**.
    The vectors are raw: they are centred by ``mu`` and, with ``G``, projected, as ``iv_scoring.plda_histograms`` does.

    ``side="enrol"``: the scores ``s(x_i, c_j)`` of ``plda_matrix_device(x, cohort)``; ``side="test"``: ``s(c_j, x_i)``, the transposed
    problem, whose cross term is ``x_i' Psi' c_j`` -- ``plda_parameters``' ``Psi`` is symmetric only up to rounding, so the test side
    passes ``Psi.T``.  ``topk=None``: every cohort score counts, population std (``sc_plda_cohort_moments``; the (N, M) scores are never
    stored); ``self_offset`` drops the pair ``j == i + self_offset``.  ``topk=k``: mean and unbiased std of the k best cohort scores
    (``sc_plda_fast`` + ``sc_topk_stats_f64`` over row blocks whose (rows, M) float64 buffer fits in ``max_workspace_bytes``)."""
    if side not in ("enrol", "test"):
        raise ValueError(f"side is 'enrol' or 'test', got {side!r}")
    model = _plda_model(xv, cohort_xv, mu, F, Sigma, G)
    _check_plda_topk(topk, self_offset, cohort_xv.shape[0])
    scorer = PldaScorer(*model, scaling_factor).on(_device_of(xv, cohort_xv))
    return _cohort_stats(scorer, *scorer.vectors(xv, cohort_xv), side, topk, self_offset, max_workspace_bytes)


def plda_znorm_device(scores, enroll_xv, cohort_xv, mu, F, Sigma, G=None, scaling_factor=1.):
    """z-norm of a device (Ne, Nt) float64 PLDA score tensor (``iv_scoring.plda_matrix_device``'s), in place: ``(s_ij - m_i) / sd_i`` with
    the statistics of enrolment i's cohort scores ``s(e_i, c)``."""
    model = _plda_model(enroll_xv, cohort_xv, mu, F, Sigma, G, "enrolment x-vectors")
    _check_scores(PldaScorer, scores, enroll_xv.shape[0], None)
    scorer = PldaScorer(*model, scaling_factor).on(_device_of(enroll_xv, cohort_xv))
    return _norm_device(scorer, "z", scores, enroll_xv, None, cohort_xv)


def plda_tnorm_device(scores, test_xv, cohort_xv, mu, F, Sigma, G=None, scaling_factor=1.):
    """t-norm, in place: ``(s_ij - m_j) / sd_j`` with the statistics of the cohort's scores ``s(c, t_j)`` on test segment j."""
    model = _plda_model(test_xv, cohort_xv, mu, F, Sigma, G, "test x-vectors")
    _check_scores(PldaScorer, scores, None, test_xv.shape[0])
    scorer = PldaScorer(*model, scaling_factor).on(_device_of(test_xv, cohort_xv))
    return _norm_device(scorer, "t", scores, None, test_xv, cohort_xv)


def plda_snorm_device(scores, enroll_xv, test_xv, cohort_xv, mu, F, Sigma, G=None, scaling_factor=1., topk=None, max_workspace_bytes=1 << 30):
    """s-norm, in place: ``0.5 ((s - m_i)/sd_i + (s - m_j)/sd_j)``; ``topk=k`` makes it adaptive (each side's k best cohort scores, unbiased
    std).  ``test_xv is enroll_xv`` does NOT share statistics: the enrolment side's cohort scores are ``s(e, c)``, the test side's
    ``s(c, t)``, which differ by ``Psi`` against ``Psi'`` (equal only up to rounding); both are computed."""
    model = _plda_model(enroll_xv, cohort_xv, mu, F, Sigma, G, "enrolment x-vectors")
    _plda_model(test_xv, cohort_xv, mu, F, Sigma, G, "test x-vectors")
    _check_plda_topk(topk, None, cohort_xv.shape[0])
    _check_scores(PldaScorer, scores, enroll_xv.shape[0], test_xv.shape[0])
    scorer = PldaScorer(*model, scaling_factor).on(_device_of(enroll_xv, test_xv, cohort_xv))
    return _norm_device(scorer, "s", scores, enroll_xv, test_xv, cohort_xv, topk, max_workspace_bytes)


def _check_plda_hist_args(enroll_xv, test_xv, cohort_xv, mu, F, Sigma, G, kind, topk):
    model = _plda_model(enroll_xv, cohort_xv, mu, F, Sigma, G, "enrolment x-vectors")
    _plda_model(test_xv, cohort_xv, mu, F, Sigma, G, "test x-vectors")
    _check_kind(kind, topk, cohort_xv.shape[0])
    return model


def plda_normalised_histograms(enroll_xv, test_xv, enroll_labels, test_labels, cohort_xv, mu, F, Sigma, G=None, scaling_factor=1., kind="s",
                               topk=None, self_offset=None, *, lo=None, hi=None, bins=None, max_workspace_bytes=1 << 30):
    """Target / non-target histograms ``(hist_tar, hist_non)`` of the cohort-normalised PLDA log-likelihood ratios of ALL (enrol, test)
    pairs: ``normalised_histograms`` for PLDA.  Neither the (Ne, Nt) float64 score matrix nor (with ``topk=None``) a cohort score matrix is
    formed.  ``kind``: ``"z"`` (``plda_znorm_device``'s expression), ``"t"`` (``plda_tnorm_device``'s) or ``"s"`` (``plda_snorm_device``'s);
    ``topk=k``, with ``"s"`` only, is adaptive s-norm.  The vectors are raw and the model is ``(mu, F, Sigma, G, scaling_factor)`` as in
    ``iv_scoring.plda_histograms``; ``iv_scoring.plda_norm_histograms`` does the counting with the statistics of ``plda_cohort_stats_device`` (``sc_plda_hist_norm``: the
    counts are those of the materialised path).  ``self_offset`` (of the TRIALS: the cohort is a set of its own), ``bins`` and the labels are
    ``plda_histograms``'.  ``lo`` / ``hi`` are required keywords (``plda_normalised_range_from_sample`` estimates them).  zt-norm is not offered."""
    model = _check_plda_hist_args(enroll_xv, test_xv, cohort_xv, mu, F, Sigma, G, kind, topk)
    if lo is None or hi is None:
        raise ValueError("lo and hi are required keywords: normalised scores have no default range (plda_normalised_range_from_sample estimates one)")
    if not float(hi) > float(lo):
        raise ValueError("histogram range: hi must exceed lo")
    scorer = PldaScorer(*model, scaling_factor).on(_device_of(enroll_xv, test_xv, cohort_xv))
    en, tn = _side_stats(scorer, kind, enroll_xv, test_xv, cohort_xv, topk, max_workspace_bytes)
    _, le, lt, bins = iv_scoring._plda_hist_checks(enroll_xv, test_xv, enroll_labels, test_labels, mu, F, Sigma, G, lo, hi, bins)   # plda_norm_histograms' own
    e, t = scorer.vectors(enroll_xv, test_xv)
    return iv_scoring._histograms(scorer, e, t, le, lt, self_offset, lo, hi, bins, en, tn)


def plda_normalised_range_from_sample(enroll_xv, test_xv, cohort_xv, mu, F, Sigma, G=None, scaling_factor=1., kind="s", topk=None):
    """``(lo, hi)`` for ``plda_normalised_histograms``, as ``normalised_range_from_sample`` finds it: a strided sample of at most 2 048 rows
    per side, its materialised PLDA score matrix normalised by ``plda_znorm_device`` / ``plda_tnorm_device`` / ``plda_snorm_device`` against
    the whole cohort (without the self-trials when the two sides are the same object), and the sample's smallest and largest normalised
    score, each widened by a quarter of the sampled range."""
    model = _check_plda_hist_args(enroll_xv, test_xv, cohort_xv, mu, F, Sigma, G, kind, topk)
    scorer = PldaScorer(*model, scaling_factor).on(_device_of(enroll_xv, test_xv, cohort_xv))
    return iv_scoring._range_from_sample(scorer, enroll_xv, test_xv, lambda z, es, ts: _norm_device(scorer, kind, z, es, ts, cohort_xv, topk))


def matrix_moments_device(scoremat, axis, skip_diag=False):
    """``(mean, std)`` (population std, float32 device tensors) of the rows (``axis=1``) or columns (``axis=0``) of a score matrix;
    ``skip_diag`` (square matrices only) leaves the diagonal out and divides by ``n - 1``."""
    rows, cols = _shape2(scoremat, "scoremat")
    if axis not in (0, 1):
        raise ValueError("axis is 0 or 1")
    if skip_diag and (rows != cols or rows < 2):
        raise ValueError(f"skip_diag needs a square matrix of at least 2 x 2, got {rows} x {cols}")
    if rows == 0 or cols == 0:
        raise ValueError("empty score matrix")
    device = _device_of(scoremat)
    s = _to_device(scoremat, torch.float32, device)
    n = rows if axis == 1 else cols
    mean = torch.empty(n, dtype=torch.float32, device=device)
    std = torch.empty(n, dtype=torch.float32, device=device)
    _lib.launch("sc_matrix_moments", device, s, rows, cols, int(axis), int(bool(skip_diag)), mean, std)
    return mean, std


# ---- Scores level: the reference's signatures ------------------------------------------------------------------------------------
def _same_ids(a, b, what):
    if a.shape != b.shape or not bool((a == b).all()):
        raise ValueError(f"the two Scores objects do not share their {what}")


def _normalised(scores, mat):
    """``scores.scoremat`` <- the device result, in the matrix's own float type (the arithmetic was float32 on the GPU)."""
    dtype = scores.scoremat.dtype if scores.scoremat.dtype.kind == "f" else numpy.float64
    scores.scoremat = mat.cpu().numpy().astype(dtype)
    return scores


def znorm(enrol_test_scores, enrol_imp_scores, sym=False):
    """``sidekit.score_normalization.znorm`` (:44-72): every model's scores minus the mean, over the std, of its impostor scores (rows of
    ``enrol_imp_scores``; ``sym=True``: the two model sets are the same cohort, the diagonal is left out).  See the module docstring for
    the two deviations from the reference's lines 64-70."""
    scores_znorm = copy.deepcopy(enrol_test_scores)
    scores_znorm.sort()
    enrol_imp_scores.sort()
    _same_ids(scores_znorm.modelset, enrol_imp_scores.modelset, "modelset")
    if sym and enrol_imp_scores.scoremat.shape[0] != enrol_imp_scores.scoremat.shape[1]:
        raise ValueError("sym=True needs a square impostor x impostor matrix")
    stats = matrix_moments_device(enrol_imp_scores.scoremat, 1, skip_diag=sym)
    return _normalised(scores_znorm, _apply(CosineScorer, _to_device(scores_znorm.scoremat, torch.float32, stats[0].device), enrol=stats))


def tnorm(enrol_test_scores, imp_test_scores):
    """``sidekit.score_normalization.tnorm`` (:75-93): every test segment's scores minus the mean, over the std, of the impostor models'
    scores on that segment (columns of ``imp_test_scores``)."""
    scores_tnorm = copy.deepcopy(enrol_test_scores)
    scores_tnorm.sort()
    imp_test_scores.sort()
    _same_ids(scores_tnorm.segset, imp_test_scores.segset, "segset")
    stats = matrix_moments_device(imp_test_scores.scoremat, 0)
    return _normalised(scores_tnorm, _apply(CosineScorer, _to_device(scores_tnorm.scoremat, torch.float32, stats[0].device), test=stats))


def ztnorm(enrol_test_scores, enrol_imp_scores, imp_test_scores, imp_imp_scores):
    """``sidekit.score_normalization.ztnorm`` (:96-117): z-norm of the trials and of the impostor x test scores, then t-norm."""
    z_enrol_test_scores = znorm(enrol_test_scores, enrol_imp_scores)
    z_imp_test_scores = znorm(imp_test_scores, imp_imp_scores, sym=True)
    return tnorm(z_enrol_test_scores, z_imp_test_scores)
