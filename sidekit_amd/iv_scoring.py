"""Trial scoring -- mirror of ``sidekit/iv_scoring.py``: ``cosine_scoring`` (:63-113), ``PLDA_scoring``
(:215-269), ``full_PLDA_scoring`` (:272-368), ``fast_PLDA_scoring`` (:370-477), ``plda_histograms`` / ``plda_range_from_sample`` (the scores of
:448-462 for every pair of a corpus, counted instead of stored; ``plda_norm_histograms``: cohort-normalised first), and -- beyond SURVEY 8's rows, because they are
the same device entry point with other matrices -- ``mahalanobis_scoring`` (:116-156) and ``two_covariance_scoring`` (:159-213).

The trial matrix is computed on the GPU through the C ABI (``sc_cosine``: f32 MFMA GEMM;
``sc_plda_fast``: float64 tiled GEMM with the quadratic terms and the constant fused in the
epilogue).  As in the reference the 256x256 float64 algebra (inverses, slogdet) stays on the host.
``full_PLDA_scoring`` maps onto the same device entry point: with e' = B e, t' = B t the reference's
per-model loop is  0.5 (e'+t')' K2 (e'+t') - 0.5 t' K1 t - 0.5 e' K1 e  =  0.5 e'(K2-K1)e' +
0.5 t'(K2-K1)t' + e' sym(K2) t'.  There is no CPU fallback.

``CosineScorer`` / ``PldaScorer`` describe how one kind of trial is scored on a device (element type, entry points, the arguments after
``D``, whether the two sides share cohort statistics, the preparation of raw vectors); the histogram functions here and
``score_normalization`` are written once against them.
"""
import copy
import logging

import numpy
import scipy.linalg
import torch

from . import _lib
from .bosaris import Ndx, Scores
from .statserver import StatServer


def _check_missing_model(enroll, test, ndx):
    """Drop trials whose model / segment has no vector, align both StatServers to the cleaned Ndx."""
    clean_ndx = ndx.filter(enroll.modelset, test.segset, True)
    enroll.align_models(clean_ndx.modelset)
    test.align_segments(clean_ndx.segset)
    return clean_ndx


def _device(device):
    if not torch.cuda.is_available():
        raise RuntimeError("sidekit_amd.iv_scoring computes on the GPU only (no CPU fallback) and no GPU is visible")
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"sidekit_amd.iv_scoring computes on the GPU only; got device={device}")
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


def _to_device(x, dtype, device):
    """numpy array or torch tensor (any device) -> contiguous tensor of `dtype` on `device`; a tensor already there is used as is, unless
    it starts off a 16-byte boundary (a view into a larger buffer): the kernels read rows with 16-byte loads, so that one is copied."""
    if torch.is_tensor(x):
        x = x.to(device=device, dtype=dtype).contiguous()
        return x.clone() if x.data_ptr() % 16 else x
    return torch.as_tensor(numpy.ascontiguousarray(x, dtype=numpy.float32 if dtype == torch.float32 else numpy.float64)).to(device)


def _matrix(symbol, e, t, group=(), exc=AssertionError):
    """The (Ne, Nt) scores of resident operands from ``symbol`` (``sc_cosine`` / ``sc_plda_fast``; ``group`` is what follows ``D``)."""
    out = torch.empty((e.shape[0], t.shape[0]), dtype=e.dtype, device=e.device)
    _lib.launch(symbol, e.device, e, e.shape[0], t, t.shape[0], e.shape[1], *group, out, exc=exc)
    return out


def cosine_matrix_device(enroll_vectors, test_vectors, device=None):
    """(Ne, D) x (Nt, D) already-normalised vectors -> (Ne, Nt) float32 **device tensor**: x-vectors that are already on the GPU
    (fresh from ``Xtractor.forward`` or an all-gather) are scored where they are, nothing crosses PCIe."""
    device = _device(device if device is not None else (enroll_vectors.device if torch.is_tensor(enroll_vectors) and enroll_vectors.is_cuda else None))
    e, t = _to_device(enroll_vectors, torch.float32, device), _to_device(test_vectors, torch.float32, device)
    if e.shape[1] % 4:  # the GEMM wants K % 4 == 0: zero columns do not change a dot product
        pad = 4 - e.shape[1] % 4
        e = torch.nn.functional.pad(e, (0, pad))
        t = torch.nn.functional.pad(t, (0, pad))
    return _matrix("sc_cosine", e, t)


def normalize_rows_device(vectors, device=None):
    """``torch.nn.functional.normalize(x, dim=1)`` on the GPU (``sc_normalize_rows``): (N, D) -> float32 **device tensor** of unit rows."""
    device = _device(device if device is not None else (vectors.device if torch.is_tensor(vectors) and vectors.is_cuda else None))
    x = _to_device(vectors, torch.float32, device)
    out = torch.empty_like(x)
    _lib.launch("sc_normalize_rows", device, x, x.shape[0], x.shape[1], out, exc=AssertionError)
    return out


def cosine_matrix(enroll_vectors, test_vectors, device=None):
    """(Ne, D) x (Nt, D) already-normalised float vectors -> (Ne, Nt) float32 numpy matrix (computed on the GPU)."""
    return cosine_matrix_device(enroll_vectors, test_vectors, device).cpu().numpy()


def plda_matrix_device(enroll_vectors, test_vectors, Phi, Psi, cst, scaling_factor=1., device=None):
    """scaling * (0.5 e'Phi e + 0.5 t'Phi t + cst + e'Psi t) for all pairs, float64 **device tensor** (f64 MFMA GEMM)."""
    device = _device(device if device is not None else (enroll_vectors.device if torch.is_tensor(enroll_vectors) and enroll_vectors.is_cuda else None))
    e, t = _to_device(enroll_vectors, torch.float64, device), _to_device(test_vectors, torch.float64, device)
    return _matrix("sc_plda_fast", e, t, (_to_device(Phi, torch.float64, device), _to_device(Psi, torch.float64, device), float(cst), float(scaling_factor)))


def plda_matrix(enroll_vectors, test_vectors, Phi, Psi, cst, scaling_factor=1., device=None):
    """Same, returned as a float64 numpy matrix."""
    return plda_matrix_device(enroll_vectors, test_vectors, Phi, Psi, cst, scaling_factor, device).cpu().numpy()


HIST_BINS = 8192


def _norm_pair(pair, n, side):
    """A ``(mean, std)`` pair of ``cosine_histograms``: ``None``, or two vectors of ``n`` entries (checked without a device)."""
    if pair is None:
        return None
    if not isinstance(pair, (tuple, list)) or len(pair) != 2 or pair[0] is None or pair[1] is None:
        raise ValueError(f"{side}_norm is a (mean, std) pair: a mean comes with its std")
    for name, v in zip(("mean", "std"), pair):
        if tuple(v.shape) != (n,):
            raise ValueError(f"{side}_norm: the {name} has shape {tuple(v.shape)}, the {side} side has {n} rows")
    return pair


def _histogram_passes(one_pass, lo, hi, bins):
    """``bins`` bins over ``[lo, hi)`` from ``one_pass(a, b)``, which counts every pair into ``HIST_BINS`` bins over ``[a, b)``: one pass for
    ``HIST_BINS`` itself, else ``bins / (HIST_BINS - 2)`` passes, each over a slice of the range with one guard bin either side (bins 0 and
    ``HIST_BINS - 1`` of a pass hold everything below / above its slice).

    Every pass bins with its own ``lo`` and scale, so two neighbouring passes round "is this score below the boundary between us"
    differently: copying the inner bins side by side would count a score within rounding of a boundary twice or not at all.  The passes
    are therefore joined on CUMULATIVE counts.  Pass ``k`` says how many scores lie below each of its edges (the running sum of its bins:
    its lower guard at its first edge, guard plus inner bins at its last); at a slice boundary, an edge of two passes, the larger of the
    two claims stands, and an edge inside a slice never claims less than the boundary under it.  A score that neither pass counted (the
    upper pass has it in its lower guard, the lower one in its upper guard) thus joins the last inner bin of the lower slice, and one
    that both counted stays where the lower pass put it and leaves the lowest occupied inner bins of the upper pass.  The fine histogram
    is the difference of one non-decreasing sequence that starts at 0 and ends at the count of one pass: every score is in exactly one
    bin, and the bin is a non-decreasing function of the score."""
    if bins == HIST_BINS:
        return one_pass(lo, hi)
    inner = HIST_BINS - 2
    w = (float(hi) - float(lo)) / bins
    below_t, below_n = numpy.zeros(bins + 1, dtype=numpy.int64), numpy.zeros(bins + 1, dtype=numpy.int64)   # scores under fine edge i
    passes = bins // inner
    for k in range(passes):
        a = float(lo) + k * inner * w
        for below, part in zip((below_t, below_n), one_pass(a - w, a + (inner + 1) * w)):
            claims = numpy.cumsum(part.astype(numpy.int64))                            # claims[j]: scores under the pass's edge j + 1
            edges = below[k * inner:(k + 1) * inner + 1]                               # a view: fine edges k * inner .. (k + 1) * inner
            numpy.maximum(edges, claims[:-1], out=edges)
            below[-1] = claims[-1]                                                     # every pass counts the same scores
    for below in (below_t, below_n):
        below[0] = 0                                                                   # what lies under lo is in the first bin
        numpy.minimum(numpy.maximum.accumulate(below), below[-1], out=below)
    return numpy.diff(below_t).astype(numpy.uint64), numpy.diff(below_n).astype(numpy.uint64)


def _check_bins(bins, exc):
    bins = HIST_BINS if bins is None else int(bins)
    if bins != HIST_BINS and (bins <= 0 or bins % (HIST_BINS - 2)):
        raise exc(f"bins must be {HIST_BINS} or a multiple of {HIST_BINS - 2}")
    return bins


def _labels(labels, device):
    return torch.as_tensor(labels).to(device=device, dtype=torch.int32).contiguous()


def _hist_device(device, *tensors):
    return _device(device if device is not None else next((x.device for x in tensors if torch.is_tensor(x) and x.is_cuda), None))


def _stat_pairs(scorer, enroll_norm, test_norm, device):
    """The ``(mean, std)`` pairs of a normalised histogram on the device, flat (``None`` twice for a side without one), or ``None`` without
    either; one reduction checks every std."""
    if enroll_norm is None and test_norm is None:
        return None
    stats = [(None, None) if pair is None else tuple(_to_device(v, scorer.dtype, device) for v in pair) for pair in (enroll_norm, test_norm)]
    stds = torch.cat([std for _, std in stats if std is not None])
    if not bool((torch.isfinite(stds) & (stds > 0)).all()):                         # one reduction, one scalar back
        raise ValueError(f"{scorer.histograms}: every std of enroll_norm / test_norm must be finite and > 0")
    return stats[0] + stats[1]


def _hist_pass(scorer, group, e, t, le, lt, self_offset, lo, hi, device, stats=None):
    """One ``scorer.hist`` call on resident operands (``scorer.hist_norm`` with the four statistics vectors ``stats``); ``group`` is what
    follows ``D``.  The two ``HIST_BINS``-bin uint64 histograms over ``[lo, hi)``."""
    ht = torch.empty(HIST_BINS, dtype=torch.int64, device=device)
    hn = torch.empty(HIST_BINS, dtype=torch.int64, device=device)
    head = (e, e.shape[0], t, t.shape[0], e.shape[1], *group, le, lt, -1 if self_offset is None else int(self_offset))
    tail = (float(lo), float(hi), HIST_BINS, ht, hn)
    if stats is None:
        _lib.launch(scorer.hist, device, *head, *tail, exc=scorer.hist_exc)
    else:
        _lib.launch(scorer.hist_norm, device, *head, *stats, *tail, exc=scorer.hist_exc)
    return ht.cpu().numpy().astype(numpy.uint64), hn.cpu().numpy().astype(numpy.uint64)


def _plda_hist_pass(e, t, le, lt, phi, psi, cst, scaling_factor, self_offset, lo, hi, device, norm_ptrs=None):
    """``_hist_pass`` of PLDA operands, spelled out: the seam at which ``tests/test_plda_hist_cpu.py`` reads what reaches the device."""
    return _hist_pass(PldaScorer, (phi, psi, cst, scaling_factor), e, t, le, lt, self_offset, lo, hi, device, norm_ptrs)


def _histograms(scorer, e, t, le, lt, self_offset, lo, hi, bins, enroll_norm=None, test_norm=None):
    """Prepared vectors, checked labels and ``bins``: labels and statistics pairs onto the device, then the passes."""
    le, lt = _labels(le, e.device), _labels(lt, e.device)
    stats = _stat_pairs(scorer, enroll_norm, test_norm, e.device)
    return _histogram_passes(lambda a, b: scorer.hist_pass(e, t, le, lt, self_offset, a, b, stats), lo, hi, bins)


def cosine_histograms(enroll_vectors, test_vectors, enroll_labels, test_labels, self_offset=None, lo=-1.0, hi=1.0, device=None, bins=None,
                      enroll_norm=None, test_norm=None):
    """Target / non-target score histograms of ALL (enrol, test) pairs without materialising the (Ne, Nt) score matrix
    (100k x 100k cosine trials are 40 GB).  A trial is a target when the two integer labels are equal;
    ``self_offset=k`` drops the self-trials ``j == i + k`` when the enrolment side is rows ``[k, k + Ne)`` of the test side (``0`` for
    a set scored against itself, a shard's first row for one rank's block of it); ``None`` keeps every pair.  Returns two uint64 arrays of
    ``bins`` equal bins over ``[lo, hi)`` (scores outside land in the end bins); ``bosaris.detplot.eer_from_histograms`` turns them into the
    ROCCH EER.  ``bins``: ``HIST_BINS`` (8192, the kernel's LDS histograms: one pass over the pairs) or a multiple of ``HIST_BINS - 2``: that
    many finer bins from ``bins / (HIST_BINS - 2)`` passes, each over a slice of the range with one guard bin either side, joined so that
    every trial is in exactly one bin (``_histogram_passes``).  Scores that are not finite: the rule of the histogram kernels is that a NaN
    score is in no bin, a raw ``+-inf`` lands in an end bin and a normalised score that is not finite has no bin, and ``plda_histograms``
    keeps it.  The cosine kernel does NOT yet: it counts ``+-inf`` in the end bins and a NaN in the FIRST bin, normalised or not (a NaN
    x-vector is a row or column of trials with the lowest possible score) -- through a conversion C++ leaves undefined, kept because the
    defined one measured slower; ``tests/test_gpu_hist_bins.py`` pins what happens.  Hand over finite vectors.

    ``enroll_norm`` / ``test_norm``: ``(mean, std)`` float32 vectors, one entry per enrolment / test row (device tensors are used as
    given; ``score_normalization.cohort_stats_device`` makes them).  The scores are then normalised before they are binned
    (``sc_cosine_hist_norm``): ``enroll_norm`` alone is z-norm, ``test_norm`` alone t-norm, both s-norm -- the bits of ``sc_cosine``
    followed by ``sc_norm_apply``.  A pair of the wrong length, a mean without its std, or a std that is not finite and positive (a NaN
    score has no bin, and counting it somewhere would hide a broken cohort) raise ``ValueError`` before any launch; ``lo`` / ``hi`` are then
    the range of the NORMALISED scores (``score_normalization.normalised_range_from_sample``).  Both ``None``: the raw scores, as before."""
    if enroll_norm is not None or test_norm is not None:                              # what needs no device is said before one is touched
        if len(enroll_vectors.shape) != 2 or len(test_vectors.shape) != 2 or enroll_vectors.shape[1] != test_vectors.shape[1] or enroll_vectors.shape[1] % 4:
            raise ValueError("x-vector dimensions must match and be a multiple of 4")
        enroll_norm = _norm_pair(enroll_norm, enroll_vectors.shape[0], "enroll")
        test_norm = _norm_pair(test_norm, test_vectors.shape[0], "test")
    scorer = CosineScorer(_hist_device(device, enroll_vectors))
    e, t = scorer.vectors(enroll_vectors, test_vectors)
    if e.shape[1] % 4 or e.shape[1] != t.shape[1]:
        raise AssertionError("x-vector dimensions must match and be a multiple of 4")
    le, lt = _labels(enroll_labels, e.device), _labels(test_labels, e.device)
    assert le.shape == (e.shape[0],) and lt.shape == (t.shape[0],), "one label per vector"
    bins = _check_bins(bins, AssertionError)
    if not float(hi) > float(lo):
        raise AssertionError("histogram range: hi must exceed lo")
    return _histograms(scorer, e, t, le, lt, self_offset, lo, hi, bins, enroll_norm, test_norm)


def _speaker_posterior_terms(K):
    """For ``K`` = speaker-subspace precision gained from ONE observation: the posterior covariances after one and after two observations
    of a speaker, ``(I + K)^-1`` and ``(I + 2K)^-1``, and the constant of the log-likelihood ratio they leave,
    ``log|I + K| - 0.5 log|I + 2K|``."""
    eye = numpy.eye(K.shape[0])
    one, two = eye + K, eye + 2.0 * K
    return numpy.linalg.inv(one), numpy.linalg.inv(two), numpy.linalg.slogdet(one)[1] - 0.5 * numpy.linalg.slogdet(two)[1]


def plda_parameters(mu, F, Sigma, scaling_factor=1.):
    """The D x D float64 algebra of two-covariance PLDA scoring, kept on the host as the reference keeps it (``iv_scoring.py:428-446``):
    ``(Phi, Psi, plda_cst)`` such that ``score(e, t) = scaling * (0.5 e'Phi e + 0.5 t'Phi t + plda_cst + e'Psi t)`` for centred vectors.

    A same-speaker pair ``(e, t)`` is jointly Gaussian with covariance ``[[T, A], [A, T]]`` (``A = F F'`` across speakers, ``T = A + Sigma``
    total), a different-speaker pair with ``[[T, 0], [0, T]]``; the log-likelihood ratio's quadratic form is the difference of the two
    precisions, whose blocks follow from the Schur complement ``S = T - A T^-1 A``: diagonal ``T^-1 - S^-1``, off-diagonal ``T^-1 A S^-1``."""
    F = numpy.asarray(F, dtype=numpy.float64)
    within = numpy.asarray(Sigma, dtype=numpy.float64)
    across = F @ F.T
    total = across + within
    total_inv = numpy.linalg.inv(total)
    schur_inv = numpy.linalg.inv(total - across @ total_inv @ across)
    Phi = total_inv - schur_inv
    Psi = total_inv @ across @ schur_inv
    _, _, plda_cst = _speaker_posterior_terms(scaling_factor * (F.T @ numpy.linalg.solve(within, F)))
    return Phi, Psi, plda_cst


def full_plda_parameters(F, G, Sigma, scaling_factor=1.):
    """Host algebra of PLDA with a channel sub-space (``iv_scoring.py:299-330``): ``(B, Phi, Psi, constant)`` with which the reference's
    per-model loop becomes the two-covariance kernel's form on projected vectors ``e' = B e``, ``t' = B t`` (module docstring).

    Precision of an observation once the channel factor is integrated out (Woodbury on ``Sigma + G G'``), then everything lives in the
    speaker sub-space: ``B`` projects a centred vector there and ``B F`` is what one observation adds to the speaker's posterior precision."""
    F, G = numpy.asarray(F, dtype=numpy.float64), numpy.asarray(G, dtype=numpy.float64)
    prec = scaling_factor * numpy.linalg.inv(numpy.asarray(Sigma, dtype=numpy.float64))
    PG = prec @ G
    prec_marg = prec - PG @ numpy.linalg.inv(numpy.eye(G.shape[1]) + G.T @ PG) @ PG.T
    B = F.T @ prec_marg
    K1, K2, constant = _speaker_posterior_terms(B @ F)
    return B, K2 - K1, 0.5 * (K2 + K2.T), constant


def _plda_checks(enroll_vectors, test_vectors, enroll_labels, test_labels, mu, F, Sigma, G):
    """Every check of a PLDA call that needs no device.  Returns the model as float64 arrays ``(mu, F, Sigma, G)``: what ``PldaScorer`` takes."""
    if len(enroll_vectors.shape) != 2 or len(test_vectors.shape) != 2 or enroll_vectors.shape[1] != test_vectors.shape[1]:
        raise ValueError("enrolment and test vectors are matrices of one width")
    if enroll_vectors.shape[0] == 0 or test_vectors.shape[0] == 0:
        raise ValueError("empty enrolment or test side")
    D = enroll_vectors.shape[1]
    mu, F, Sigma = (numpy.asarray(v, dtype=numpy.float64) for v in (mu, F, Sigma))
    G = None if G is None else numpy.asarray(G, dtype=numpy.float64)
    if mu.shape != (D,) or F.ndim != 2 or F.shape[0] != D or Sigma.shape != (D, D) or (G is not None and (G.ndim != 2 or G.shape[0] != D)):
        raise ValueError(f"the vectors are {D} wide: mu must be ({D},), F ({D}, rank), Sigma ({D}, {D}) and G ({D}, rank); got "
                         f"{mu.shape}, {F.shape}, {Sigma.shape}" + ("" if G is None else f", {G.shape}"))
    for side, labels, n in (("enrolment", enroll_labels, enroll_vectors.shape[0]), ("test", test_labels, test_vectors.shape[0])):
        if labels is not None and tuple(labels.shape) != (n,):
            raise ValueError(f"one label per row: the {side} side has {n} rows and labels of shape {tuple(labels.shape)}")
    for name, v in (("mu", mu), ("F", F), ("Sigma", Sigma), ("G", G)):
        if v is not None and not numpy.isfinite(v).all():
            raise ValueError(f"{name} is not finite")
    return mu, F, Sigma, G


# ---- scorers: how one kind of trial is scored on a device ---------------------------------------------------------------------------
# A scorer holds the element type, the names of its entry points, the arguments that follow ``D`` in them (``group``), whether the two
# sides of a trial share cohort statistics, and the preparation of raw vectors (``vectors``).  The histogram functions of this module and
# every rule of ``score_normalization`` are written once, against a scorer.  There are two.  The element type and the names are class
# attributes: a rule that needs nothing else (``_check_scores``, ``_apply``, ``_hist_pass``) takes the class as well as an instance.
class CosineScorer:
    """Cosine scores of float32 rows.  Nothing follows ``D`` but, in the cohort moments, ``col_shift`` / ``col_scale``."""
    dtype = torch.float32
    matrix, moments, topk, apply = "sc_cosine", "sc_cohort_moments", "sc_topk_stats", "sc_norm_apply"
    hist, hist_norm, hist_exc, histograms = "sc_cosine_hist", "sc_cosine_hist_norm", AssertionError, "cosine_histograms"
    shares_sides = True                                     # s(x, c) is s(c, x): one object on both sides needs its statistics once

    def __init__(self, device, col_shift=None, col_scale=None):
        self.device = device
        self.columns = (None, None) if col_shift is None else (_to_device(col_shift, self.dtype, device), _to_device(col_scale, self.dtype, device))

    def group(self, side="enrol", moments=False):
        return self.columns if moments else ()

    def vectors(self, enroll_vectors, test_vectors):
        """Both sides on the device in float32, used as given; one object for both sides when the caller passed one."""
        e = _to_device(enroll_vectors, self.dtype, self.device)
        return e, (e if test_vectors is enroll_vectors else _to_device(test_vectors, self.dtype, self.device))

    def hist_pass(self, e, t, le, lt, self_offset, lo, hi, stats):                       # PldaScorer's goes through a seam of its own
        return _hist_pass(self, (), e, t, le, lt, self_offset, lo, hi, self.device, stats)


class PldaScorer:
    """PLDA log-likelihood ratios in float64.  ``(phi, psi, cst, scaling)`` follow ``D``, resident on the device and built once from the
    host algebra of ``plda_parameters`` (``G is None``) or ``full_plda_parameters``; the ``"test"`` side of the cohort statistics scores
    ``s(c, x)``, whose cross term is ``x' Psi' c``, so it gets ``Psi'`` (``Psi`` is symmetric only up to rounding)."""
    dtype = torch.float64
    matrix, moments, topk, apply = "sc_plda_fast", "sc_plda_cohort_moments", "sc_topk_stats_f64", "sc_norm_apply_f64"
    hist, hist_norm, hist_exc, histograms = "sc_plda_hist", "sc_plda_hist_norm", ValueError, "plda_histograms"
    shares_sides = False                                    # Psi on one side, Psi' on the other

    def __init__(self, mu, F, Sigma, G, scaling_factor):
        """The host algebra, once; ``on(device)`` makes it resident."""
        if G is None:
            self.B, (Phi, Psi, cst) = None, plda_parameters(mu, F, Sigma, scaling_factor)
        else:
            self.B, Phi, Psi, cst = full_plda_parameters(F, G, Sigma, scaling_factor)
        self.host = (mu, Phi, Psi)
        self.cst, self.scaling = float(cst), float(scaling_factor)

    def on(self, device):
        mu, Phi, Psi = self.host
        self.device, self.mu, self.psi_t = device, torch.as_tensor(mu, device=device), None
        self.phi, self.psi = _to_device(Phi, self.dtype, device), _to_device(Psi, self.dtype, device)
        return self

    def group(self, side="enrol", moments=False):
        if side == "test" and self.psi_t is None:
            self.psi_t = _to_device(numpy.ascontiguousarray(self.host[2].T), self.dtype, self.device)
        return self.phi, (self.psi_t if side == "test" else self.psi), self.cst, self.scaling

    def hist_pass(self, e, t, le, lt, self_offset, lo, hi, stats):
        return _plda_hist_pass(e, t, le, lt, *self.group(), self_offset, lo, hi, self.device, *(() if stats is None else (stats,)))

    def vectors(self, enroll_vectors, test_vectors):
        """Both sides on the device in float64, centred by ``mu`` and, with a channel sub-space, projected by ``B`` (the route of
        ``full_PLDA_scoring``); one object for both sides when the caller passed one.  One reduction checks that they are finite."""
        prep = lambda x: _to_device(x, self.dtype, self.device) - self.mu
        e = prep(enroll_vectors)
        t = e if test_vectors is enroll_vectors else prep(test_vectors)
        if not bool(torch.isfinite(e).all() & torch.isfinite(t).all()):                  # one scalar back
            raise ValueError("the centred vectors are not finite")
        if self.B is not None:
            from .backend import whiten_rows_device
            R = numpy.ascontiguousarray(self.B.T)
            pe = whiten_rows_device(e.contiguous(), None, R)
            e, t = pe, (pe if t is e else whiten_rows_device(t.contiguous(), None, R))
        return e.contiguous(), t.contiguous()


def plda_histograms(enroll_vectors, test_vectors, enroll_labels, test_labels, mu, F, Sigma, G=None, scaling_factor=1., self_offset=None, *,
                    lo=None, hi=None, bins=None, device=None):
    """Target / non-target histograms of the PLDA log-likelihood ratios of ALL (enrol, test) pairs without the (Ne, Nt) float64 score
    matrix (100k x 100k trials are 80 GB): what ``cosine_histograms`` is to ``cosine_scoring``, for ``fast_PLDA_scoring`` (``G is None``:
    ``plda_parameters``) and ``full_PLDA_scoring`` (``G`` given: ``full_plda_parameters``, both sides projected by ``B``, so the kernel sees
    rank-dimensional vectors).  The vectors are centred by ``mu`` on the device in float64; every score is the double ``plda_matrix_device``
    would have stored (``sc_plda_hist``), so the counts are those of binning that matrix.  Labels, ``self_offset`` and the two uint64 arrays
    returned are ``cosine_histograms``'; so is ``bins`` (``HIST_BINS`` or a multiple of ``HIST_BINS - 2``: that many finer bins from several
    passes).  Log-likelihood ratios have no natural range: ``lo`` / ``hi`` are required keywords (``plda_range_from_sample``).  Scores outside
    land in the end bins; a NaN score is in no bin.

    What needs no device raises ``ValueError`` before one is touched: missing ``lo`` / ``hi`` or ``hi <= lo``, vectors that are not matrices
    of one width, a width other than ``len(mu)``, ``F.shape[0]`` or ``Sigma.shape``, labels that are not one per row, ``bins``, and non-finite
    ``mu`` / ``F`` / ``Sigma`` / ``G``; centred vectors that are not finite raise it after one device reduction."""
    return _plda_histograms(enroll_vectors, test_vectors, enroll_labels, test_labels, mu, F, Sigma, G, scaling_factor, self_offset, lo, hi, bins,
                            device, None, None)


def plda_norm_histograms(enroll_vectors, test_vectors, enroll_labels, test_labels, mu, F, Sigma, G=None, scaling_factor=1., self_offset=None, *,
                         enroll_norm=None, test_norm=None, lo=None, hi=None, bins=None, device=None):
    """``plda_histograms`` of cohort-normalised scores: what ``cosine_histograms(enroll_norm=, test_norm=)`` is to cosine scores.

    ``enroll_norm`` / ``test_norm``: ``(mean, std)`` float64 vectors, one entry per enrolment / test row (device tensors are used as given;
    ``score_normalization.plda_cohort_stats_device`` makes them).  The scores are normalised before they are binned
    (``sc_plda_hist_norm``): ``enroll_norm`` alone is z-norm, ``test_norm`` alone t-norm, both s-norm -- the bits of ``sc_plda_fast`` followed
    by ``sc_norm_apply_f64``.  A pair of the wrong length, a mean without its std, or a std that is not finite and positive raise
    ``ValueError`` before any launch; ``lo`` / ``hi`` are the range of the NORMALISED scores
    (``score_normalization.plda_normalised_range_from_sample``).  Both ``None``: ``plda_histograms`` itself (``sc_plda_hist``).  Every other
    argument and check is ``plda_histograms``'.  (The two keywords live here and not on ``plda_histograms``, whose parameter list is fixed.)"""
    return _plda_histograms(enroll_vectors, test_vectors, enroll_labels, test_labels, mu, F, Sigma, G, scaling_factor, self_offset, lo, hi, bins,
                            device, enroll_norm, test_norm)


def _plda_hist_checks(enroll_vectors, test_vectors, enroll_labels, test_labels, mu, F, Sigma, G, lo, hi, bins):
    """The checks of ``plda_histograms`` that need no device.  Returns ``(model, enroll_labels, test_labels, bins)``: the model as
    ``PldaScorer`` takes it, the labels as arrays or tensors, ``bins`` as an int."""
    if lo is None or hi is None:
        raise ValueError("plda_histograms: lo and hi are required (log-likelihood ratios have no natural range: plda_range_from_sample)")
    if not (numpy.isfinite(lo) and numpy.isfinite(hi) and float(hi) > float(lo)):
        raise ValueError("plda_histograms: lo and hi must be finite and hi must exceed lo")
    bins = _check_bins(bins, ValueError)
    enroll_labels = enroll_labels if torch.is_tensor(enroll_labels) else numpy.asarray(enroll_labels)
    test_labels = test_labels if torch.is_tensor(test_labels) else numpy.asarray(test_labels)
    return _plda_checks(enroll_vectors, test_vectors, enroll_labels, test_labels, mu, F, Sigma, G), enroll_labels, test_labels, bins


def _plda_histograms(enroll_vectors, test_vectors, enroll_labels, test_labels, mu, F, Sigma, G, scaling_factor, self_offset, lo, hi, bins, device,
                     enroll_norm, test_norm):
    model, enroll_labels, test_labels, bins = _plda_hist_checks(enroll_vectors, test_vectors, enroll_labels, test_labels, mu, F, Sigma, G, lo, hi, bins)
    scorer = PldaScorer(*model, scaling_factor)
    enroll_norm = _norm_pair(enroll_norm, enroll_vectors.shape[0], "enroll")
    test_norm = _norm_pair(test_norm, test_vectors.shape[0], "test")
    e, t = scorer.on(_hist_device(device, enroll_vectors, test_vectors)).vectors(enroll_vectors, test_vectors)
    return _histograms(scorer, e, t, enroll_labels, test_labels, self_offset, lo, hi, bins, enroll_norm, test_norm)


def _range_from_sample(scorer, enroll_vectors, test_vectors, normalise=None):
    """``(lo, hi)`` from a strided sample of at most 2 048 rows per side: its materialised score matrix, normalised in place by
    ``normalise(z, enrol sample, test sample)`` if given, without the self-trials when the two sides are the same object; the smallest and
    largest entry, each widened by a quarter of the sampled range (what still falls outside is counted in the end bins)."""
    sample = lambda x: x[:: max(1, x.shape[0] // 2048)][:2048]
    gather = lambda x: x.contiguous() if torch.is_tensor(x) else x                  # once: the sample is prepared for the matrix and for each side
    es = gather(sample(enroll_vectors))
    ts = es if test_vectors is enroll_vectors else gather(sample(test_vectors))
    e, t = scorer.vectors(es, ts)
    z = _matrix(scorer.matrix, e, t, scorer.group())
    if normalise is not None:
        normalise(z, es, ts)
    if es is ts:
        z = z[~torch.eye(z.shape[0], dtype=torch.bool, device=z.device)]            # a set against itself: the self-trials are not trials
    zmin, zmax = float(z.min()), float(z.max())
    pad = 0.25 * (zmax - zmin)
    return zmin - pad, zmax + pad


def plda_range_from_sample(enroll_vectors, test_vectors, mu, F, Sigma, G=None, scaling_factor=1., device=None):
    """``(lo, hi)`` for ``plda_histograms``, as ``score_normalization.normalised_range_from_sample`` finds it: a strided sample of at most
    2 048 rows per side, its score matrix from ``plda_matrix_device`` (without the self-trials when the two sides are the same object), and
    the sample's smallest and largest score, each widened by a quarter of the sampled range."""
    model = _plda_checks(enroll_vectors, test_vectors, None, None, mu, F, Sigma, G)
    return _range_from_sample(PldaScorer(*model, scaling_factor).on(_hist_device(device, enroll_vectors, test_vectors)), enroll_vectors, test_vectors)


def _open_set(scoremat, p_known):
    """Open-set identification term (iv_scoring.py:467-475): impostor mass = mean of the other models' likelihoods."""
    N = scoremat.shape[0]
    tmp = numpy.exp(scoremat)
    others = tmp.sum(axis=0)[numpy.newaxis, :] - tmp
    return scoremat - numpy.log(p_known * others / (N - 1) + (1 - p_known))


def cosine_scoring(enroll, test, ndx, wccn=None, check_missing=True, device=None):
    """Cosine similarity of every (model, segment) pair of ``ndx``; returns a ``Scores`` (float32 matrix)."""
    assert isinstance(enroll, StatServer), 'First parameter should be a StatServer'
    assert isinstance(test, StatServer), 'Second parameter should be a StatServer'
    assert isinstance(ndx, Ndx), 'Third parameter should be an Ndx'
    enroll_copy = copy.deepcopy(enroll)
    test_copy = copy.deepcopy(test)
    clean_ndx = _check_missing_model(enroll_copy, test_copy, ndx) if check_missing else ndx
    if wccn is not None:
        enroll_copy.rotate_stat1(wccn)
        test_copy.rotate_stat1(wccn)
    enroll_copy.norm_stat1()
    test_copy.norm_stat1()
    score = Scores()
    score.scoremat = cosine_matrix(enroll_copy.stat1, test_copy.stat1, device)
    score.modelset = clean_ndx.modelset
    score.segset = clean_ndx.segset
    score.scoremask = clean_ndx.trialmask
    return score


def PLDA_scoring(enroll, test, ndx, mu, F, G, Sigma, test_uncertainty=None, Vtrans=None, p_known=0.0, scaling_factor=1.,
                 full_model=False):
    """PLDA log-likelihood ratios; dispatches to the two-covariance form unless ``full_model``."""
    assert isinstance(enroll, StatServer), 'First parameter should be a StatServer'
    assert isinstance(test, StatServer), 'Second parameter should be a StatServer'
    assert isinstance(ndx, Ndx), 'Third parameter should be an Ndx'
    assert enroll.stat1.shape[1] == test.stat1.shape[1], 'I-vectors dimension mismatch'
    assert enroll.stat1.shape[1] == F.shape[0], 'I-vectors and co-variance matrix dimension mismatch'
    assert enroll.stat1.shape[1] == G.shape[0], 'I-vectors and co-variance matrix dimension mismatch'
    if not full_model:
        return fast_PLDA_scoring(enroll, test, ndx, mu, F, Sigma, test_uncertainty, Vtrans, p_known=p_known,
                                 scaling_factor=scaling_factor, check_missing=True)
    return full_PLDA_scoring(enroll, test, ndx, mu, F, G, Sigma, p_known=p_known, scaling_factor=scaling_factor)


def full_PLDA_scoring(enroll, test, ndx, mu, F, G, Sigma, p_known=0.0, scaling_factor=1., check_missing=True, device=None):
    """PLDA with a channel sub-space G."""
    enroll_copy = copy.deepcopy(enroll)
    test_copy = copy.deepcopy(test)
    clean_ndx = _check_missing_model(enroll_copy, test_copy, ndx) if check_missing else ndx
    enroll_copy.center_stat1(mu)
    test_copy.center_stat1(mu)
    B, Phi, Psi, constant = full_plda_parameters(F, G, Sigma, scaling_factor)
    enroll_tmp = enroll_copy.stat1 @ B.T      # (Ne, rank): speaker-subspace projections
    test_tmp = test_copy.stat1 @ B.T
    score = Scores()
    score.scoremat = plda_matrix(enroll_tmp, test_tmp, Phi, Psi, constant, scaling_factor, device)
    score.modelset = clean_ndx.modelset
    score.segset = clean_ndx.segset
    score.scoremask = clean_ndx.trialmask
    if p_known != 0:
        score.scoremat = _open_set(score.scoremat, p_known)
    return score


def fast_PLDA_scoring(enroll, test, ndx, mu, F, Sigma, test_uncertainty=None, Vtrans=None, p_known=0.0, scaling_factor=1.,
                      check_missing=True, device=None):
    """Two-covariance PLDA scoring of all trials of ``ndx`` (float64)."""
    enroll_ctr = copy.deepcopy(enroll)
    test_ctr = copy.deepcopy(test)
    if not numpy.unique(enroll_ctr.modelset).shape == enroll_ctr.modelset.shape:
        logging.warning("Enrollment models are not unique, average i-vectors")
        enroll_ctr = enroll_ctr.mean_stat_per_model()
    clean_ndx = _check_missing_model(enroll_ctr, test_ctr, ndx) if check_missing else ndx
    enroll_ctr.center_stat1(mu)
    test_ctr.center_stat1(mu)
    Phi, Psi, plda_cst = plda_parameters(mu, F, Sigma, scaling_factor)
    score = Scores()
    score.modelset = clean_ndx.modelset
    score.segset = clean_ndx.segset
    score.scoremask = clean_ndx.trialmask
    score.scoremat = plda_matrix(enroll_ctr.stat1, test_ctr.stat1, Phi, Psi, plda_cst, scaling_factor, device)
    if p_known != 0:
        score.scoremat = _open_set(score.scoremat, p_known)
    return score


def _prepared(enroll, test, ndx, check_missing):
    """Shared head of the two functions below (iv_scoring.py:134-143,183-192): duplicate models averaged with a warning, missing
    models / segments dropped.  The reference works on the caller's objects (its alignment reorders them in place); here copies."""
    enroll, test = copy.deepcopy(enroll), copy.deepcopy(test)
    if not numpy.unique(enroll.modelset).shape == enroll.modelset.shape:
        logging.warning("Enrollment models are not unique, average i-vectors")
        enroll = enroll.mean_stat_per_model()
    clean_ndx = _check_missing_model(enroll, test, ndx) if check_missing else ndx
    return enroll, test, clean_ndx


def _scores(scoremat, clean_ndx):
    score = Scores()
    score.scoremat = scoremat
    score.modelset = clean_ndx.modelset
    score.segset = clean_ndx.segset
    score.scoremask = clean_ndx.trialmask
    return score


def mahalanobis_scoring(enroll, test, ndx, m, check_missing=True, device=None):
    """``-0.5 (e - t)' M (e - t)`` for every trial (iv_scoring.py:116-156; the reference loops over models on the host).  Expanded it is
    the PLDA kernel's form with ``Phi = -sym(M)``, ``Psi = sym(M)``, no constant: one ``sc_plda_fast`` call, float64."""
    assert isinstance(enroll, StatServer), 'First parameter should be a StatServer'
    assert isinstance(test, StatServer), 'Second parameter should be a StatServer'
    assert isinstance(ndx, Ndx), 'Third parameter should be an Ndx'
    assert enroll.stat1.shape[1] == test.stat1.shape[1], 'I-vectors dimension mismatch'
    assert enroll.stat1.shape[1] == m.shape[0], 'I-vectors and Mahalanobis matrix dimension mismatch'
    enroll, test, clean_ndx = _prepared(enroll, test, ndx, check_missing)
    ms = 0.5 * (numpy.asarray(m, dtype=numpy.float64) + numpy.asarray(m, dtype=numpy.float64).T)
    return _scores(plda_matrix(enroll.stat1, test.stat1, -ms, ms, 0.0, 1.0, device), clean_ndx)


def two_covariance_scoring(enroll, test, ndx, W, B, check_missing=True, device=None):
    """Two-covariance scores (iv_scoring.py:159-213): ``(e + t)' G (e + t) - t' H t - e' H e`` with ``G = iW (iB + 2 iW)^-1 iW``,
    ``H = iW (iB + iW)^-1 iW`` from the host's float64 algebra, i.e. ``Phi = 2 sym(G - H)``, ``Psi = G + G'`` in the PLDA kernel's form."""
    assert isinstance(enroll, StatServer), 'First parameter should be a directory'
    assert isinstance(test, StatServer), 'Second parameter should be a StatServer'
    assert isinstance(ndx, Ndx), 'Third parameter should be an Ndx'
    assert enroll.stat1.shape[1] == test.stat1.shape[1], 'I-vectors dimension mismatch'
    assert enroll.stat1.shape[1] == W.shape[0], 'I-vectors and co-variance matrix dimension mismatch'
    assert enroll.stat1.shape[1] == B.shape[0], 'I-vectors and co-variance matrix dimension mismatch'
    enroll, test, clean_ndx = _prepared(enroll, test, ndx, check_missing)
    iW, iB = scipy.linalg.inv(W), scipy.linalg.inv(B)
    G = iW.dot(scipy.linalg.inv(iB + 2 * iW)).dot(iW)
    H = iW.dot(scipy.linalg.inv(iB + iW)).dot(iW)
    GH = G - H
    return _scores(plda_matrix(enroll.stat1, test.stat1, GH + GH.T, G + G.T, 0.0, 1.0, device), clean_ndx)
