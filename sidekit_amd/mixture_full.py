"""Full-covariance Gaussian mixtures -- the full-covariance half of ``sidekit/mixture.py``: ``init_from_diag`` (:263-283),
``_compute_all`` (:435-445), ``compute_log_posterior_probabilities_full`` (:490-508), the E / M steps (:586-617, :673-686) and
``EM_diag2full`` (:926-1009), as a class of its own, ``FullMixture``.  ``mixture.Mixture`` stays diagonal and keeps refusing a 3-D
``invcov``; ``FullMixture`` is not a subclass of it, so nothing that asks for a ``Mixture`` (total variability, JFA, MAP adaptation, GMM
scoring, ``StatServer.accumulate_stat``) takes one by accident.  ``StatServer.accumulate_stat_full`` is the one door.

The split is ``mixture``'s: everything with a frame (N) dimension runs on the device in float64 through the C ABI
(``include/sidekit_amd/gmm_full.h``) -- ``sc_gmm_full_frame_loglik`` (the log-sum-exp of every frame over the components, and the
``N x C`` matrix of log posteriors only where the reference's method returns it) and ``sc_gmm_full_stats`` (zeroth and first order
statistics and the full ``D x D`` second order per segment, recomputing the posteriors tile by tile: no ``N x C`` and no ``N x D x D``
array exists) -- and the ``C x D x D`` algebra (M-step, ``_compute_all``) stays on the host in the reference's operation order.

**The factor.**  The kernels take one general matrix ``M[c]`` per component and compute ``lp = log w + log cst - 0.5 |M (x - mu)|^2``.
The reference's ``_compute_all`` stores ``invchol[c] = cholesky(invcov[c])``, the LOWER factor ``L`` with ``L L' = invcov``, and its
``compute_log_posterior_probabilities_full`` forms ``|L d|^2 = d' L' L d``, which is not ``d' invcov d`` unless the matrix is diagonal
(``_maximization`` stores the transposed factor, the right one, one line before ``_compute_all`` overwrites it).  On
``tests/golden/mixture.npz`` (1260 x 23), log-likelihood per frame over four iterations from the recorded diagonal states:

    start            reference's factor                 transposed factor (|L' d|^2)
    split0 (C = 2)   -45.41, -51.04, -52.35, -52.37     -45.41, -36.44, -36.19, -36.01
    split2 (C = 4)   -39.04, -40.77, -40.47, -40.47     -39.04, -33.82, -33.74, -33.60

With the reference's factor the likelihood FALLS after the first M-step (from ``split4``, C = 8, the run ends in nan); with the
transposed one EM is monotone.  So ``invchol`` always holds what the reference stores, and the operand is a choice:
``reference_factor=True`` gives ``M = invchol`` -- the reference's arithmetic number for number, for those who must match it -- and the
default ``False`` gives ``M = invchol`` transposed, under which ``lp`` is the log density of ``N(mu_c, invcov_c^-1)`` and EM is EM.

There is no CPU fallback; importing the module needs neither a GPU nor torch.  Variance control for full covariances, ``read_alize``,
``read_htk``, ``merge`` and top-C lists on full covariances are not built.
"""
import copy

import numpy

from . import _lib, mixture
from .mixture import _DATASETS, _device_f64, _frames, _offsets, _torch

MAX_SLABS, SLAB_FRAMES = mixture.MAX_SLABS, mixture.SLAB_FRAMES
SLAB_TARGET, MAX_D = _lib.SC_GMM_FULL_SLAB_TARGET, _lib.SC_GMM_FULL_MAX_D    # include/sidekit_amd/gmm_full.h


def _slabs(length, C):
    """slabs(L, C) of include/sidekit_amd/gmm_full.h"""
    return max(1, min(-(-int(length) // SLAB_FRAMES), max(1, min(MAX_SLABS, SLAB_TARGET // int(C)))))


def _segment_groups(lens, C, doubles_per_segment, budget_bytes):
    """Consecutive groups [a, b) of segments whose outputs and slab workspace, (1 + slabs of the longest) partials each, fit the budget"""
    groups, a, longest = [], 0, 0
    for i, n in enumerate(lens):
        top = max(longest, int(n))
        slabs = _slabs(top, C)
        if i > a and (i + 1 - a) * doubles_per_segment * 8 * (1 + (slabs if slabs > 1 else 0)) > budget_bytes:
            groups.append((a, i))
            a, top = i, int(n)
        longest = top
    groups.append((a, len(lens)))
    return groups


def _model(torch, ubm, dev, mu=None, factor=None):
    """The device operands of a full-covariance mixture: ``(mu, M, g)``, ``g = log w + log cst``"""
    if not isinstance(ubm, FullMixture):
        raise TypeError("expected a FullMixture (got {}): sidekit_amd.mixture_full computes full-covariance mixtures only".format(type(ubm).__name__))
    C, D = ubm.mu.shape
    assert ubm.invcov.shape == (C, D, D) and ubm.invchol.shape == (C, D, D), "a full-covariance mixture has (C, D, D) inverse covariances and factors"
    if D > MAX_D:
        raise ValueError("full-covariance mixtures of at most {:d} dimensions are built (got {:d})".format(MAX_D, D))
    if factor is None:
        factor = ubm.invchol if ubm.reference_factor else ubm.invchol.transpose(0, 2, 1)
    else:
        assert tuple(factor.shape) == (C, D, D), "factor: one (D, D) matrix per component"
    mu = ubm.mu if mu is None else numpy.asarray(mu, dtype=numpy.float64).reshape(ubm.mu.shape)
    with numpy.errstate(divide="ignore"):   # a zero weight: log 0, lp = -inf, posterior 0
        g = numpy.log(ubm.w) + numpy.log(ubm.cst)
    return _device_f64(torch, mu, dev), _device_f64(torch, factor, dev), _device_f64(torch, g, dev)


def _loglik(torch, ubm, x, dt, mu=None, factor=None, want_lp=False):
    N, D = x.shape
    assert D == ubm.dim(), 'dimension of ubm and features differ: {:d} / {:d}'.format(ubm.dim(), D)
    m, M, g = _model(torch, ubm, x.device, mu, factor)
    C = m.shape[0]
    lse = torch.empty(N, dtype=torch.float64, device=x.device)
    lp = torch.empty((N, C), dtype=torch.float64, device=x.device) if want_lp else None
    _lib.launch("sc_gmm_full_frame_loglik", x.device, x, dt, N, D, m, M, g, C, lse, lp)
    return lse, lp, (m, M, g)


def frame_loglik_full_device(ubm, frames, mu=None, factor=None):
    """``lse[n] = log sum_c w_c N(x_n; mu_c, Sigma_c)`` of every frame under a ``FullMixture`` (``sc_gmm_full_frame_loglik``).
    ``frames`` (N, D) CUDA tensor (float32 or float64) or host array; ``mu`` replaces the means; ``factor``: ``None`` for the model's own
    choice (``invchol`` transposed, or ``invchol`` itself with ``reference_factor``), or a (C, D, D) array used as ``M`` as it is."""
    torch = _torch()
    x, dt, host = _frames(torch, frames)
    lse = _loglik(torch, ubm, x, dt, mu, factor)[0]
    return lse.cpu().numpy() if host else lse


def gmm_stats_full_device(ubm, frames, seg_off=None, order=2, max_workspace_bytes=1 << 30, factor=None):
    """Baum-Welch statistics of ``frames`` under a ``FullMixture`` per segment (``sc_gmm_full_stats``; ``_expectation`` :586-617 with one
    segment and ``order=2``, ``StatServer.accumulate_stat_full`` with many and ``order=1``).  ``seg_off``: S + 1 ascending frame offsets
    (host), segment s is frames ``[seg_off[s], seg_off[s + 1])``; ``None``: one segment, all frames.  ``factor`` as
    ``frame_loglik_full_device`` takes it.  Returns ``(stat0 (S, C), stat1 (S, C, D), stat2 (S, C, D, D) or None, llk (S,))``, float64, on
    the device when the frames were there; ``stat2[s, c]`` is symmetric bit for bit.  Segments go to the kernel in consecutive groups whose
    outputs and slab workspace stay within ``max_workspace_bytes`` (one segment at least); the grouping does not change a bit."""
    assert order in (1, 2), "order: 1 (stat0, stat1) or 2 (and stat2)"
    torch = _torch()
    x, dt, host = _frames(torch, frames)
    N, D = x.shape
    dev = x.device
    off = _offsets(seg_off, N)
    S, lens = off.shape[0] - 1, numpy.diff(off)
    lse, _, (m, M, g) = _loglik(torch, ubm, x, dt, None, factor)
    C = m.shape[0]
    stat0 = torch.empty((S, C), dtype=torch.float64, device=dev)
    stat1 = torch.empty((S, C, D), dtype=torch.float64, device=dev)
    stat2 = torch.empty((S, C, D, D), dtype=torch.float64, device=dev) if order == 2 else None
    llk = torch.empty(S, dtype=torch.float64, device=dev)
    d_off = torch.as_tensor(off.astype(numpy.int32)).to(dev)
    for a, b in _segment_groups(lens, C, C * (1 + D + (D * D if order == 2 else 0)), max_workspace_bytes):
        _lib.launch("sc_gmm_full_stats", dev, x, dt, N, D, m, M, g, C, lse, d_off[a:], b - a, int(lens[a:b].max()), order, stat0[a:], stat1[a:],
                    None if stat2 is None else stat2[a:], llk[a:])
    out = (stat0, stat1, stat2, llk)
    return tuple(None if t is None else t.cpu().numpy() for t in out) if host else out


class FullMixture(object):
    """A full-covariance Gaussian mixture as the reference stores it: ``w`` (C,), ``mu`` (C, D), ``invcov`` (C, D, D), ``invchol``
    (C, D, D; the LOWER Cholesky factor of ``invcov``, always), ``cov_var_ctl``, ``cst`` (C,), ``det`` (C,), ``A`` (zeros) and ``name``.
    ``reference_factor``: which factor the E-step multiplies by (the module's docstring): ``False`` -- ``invchol`` transposed, the log
    density of ``N(mu, invcov^-1)``; ``True`` -- ``invchol`` as it is, the reference's numbers.  It is not stored in the file."""

    def __init__(self, mixture_file_name='', name='empty', reference_factor=False):
        for dataset in _DATASETS:
            setattr(self, dataset, numpy.array([]))
        self.A = 0
        self.name = name
        self.reference_factor = bool(reference_factor)
        if mixture_file_name != '':
            self.read(mixture_file_name)

    # ---- bookkeeping ------------------------------------------------------------------------------------------------------------------
    def get_distrib_nb(self):
        return self.w.shape[0]

    distrib_nb = get_distrib_nb

    def dim(self):
        return self.mu.shape[1]

    def sv_size(self):
        return self.mu.size

    read = mixture.Mixture.read        # the eight datasets, of any rank (hdf5_lite)
    write = mixture.Mixture.write

    def validate(self):
        """Whether the arrays have the shapes of one full-covariance mixture (:447-471)"""
        if self.w.ndim != 1 or self.mu.ndim != 2:
            return False
        C, D = self.mu.shape
        if self.w.shape != (C,) or self.cst.shape != (C,) or self.det.shape != (C,):
            return False
        return self.invcov.shape == (C, D, D)

    def get_mean_super_vector(self):
        return self.mu.flatten()

    def get_invcov_super_vector(self):
        assert self.invcov.ndim == 2, 'Must be diagonal co-variance.'
        return self.invcov.flatten()

    def init_from_diag(self, diag_mixture):
        """The diagonal mixture as a full one (:263-283): ``invcov[c] = diag(diag_mixture.invcov[c])`` and its Cholesky factor;
        ``cov_var_ctl = numpy.diag(diag_mixture.cov_var_ctl)`` as the reference has it (on a 2-D array that is its diagonal; it is never
        read: the full M-step has no variance control).  The arrays are copies: the diagonal mixture is not changed by what follows."""
        self.w = numpy.array(diag_mixture.w, dtype=numpy.float64)
        self.cst = numpy.array(diag_mixture.cst, dtype=numpy.float64)
        self.det = numpy.array(diag_mixture.det, dtype=numpy.float64)
        self.mu = numpy.array(diag_mixture.mu, dtype=numpy.float64)
        C, D = self.mu.shape
        self.invcov = numpy.empty((C, D, D))
        self.invchol = numpy.empty((C, D, D))
        for gg in range(C):
            self.invcov[gg] = numpy.diag(diag_mixture.invcov[gg, :])
            self.invchol[gg] = numpy.linalg.cholesky(self.invcov[gg])
        self.cov_var_ctl = numpy.array(numpy.diag(diag_mixture.cov_var_ctl), dtype=numpy.float64)
        self.name = diag_mixture.name
        self.A = numpy.zeros(self.cst.shape)

    def _compute_all(self):
        """What follows from ``w, mu, invcov`` (:435-445): ``det = 1 / det(invcov)``, ``invchol = cholesky(invcov)`` (lower),
        ``cst = 1 / (sqrt(det) (2 pi)^(D / 2))`` and ``A = 0``"""
        for gg in range(self.mu.shape[0]):
            self.det[gg] = 1. / numpy.linalg.det(self.invcov[gg])
            self.invchol[gg] = numpy.linalg.cholesky(self.invcov[gg])
        self.cst = 1.0 / (numpy.sqrt(self.det) * (2.0 * numpy.pi) ** (self.dim() / 2.0))
        self.A = numpy.zeros(self.cst.shape)

    def _reset(self):
        """An accumulator: zeros of the same shapes"""
        for name in ("w", "mu", "invcov", "cst", "det"):
            getattr(self, name).fill(0.0)
        self.A = 0.0

    # ---- estimation -------------------------------------------------------------------------------------------------------------------
    def compute_log_posterior_probabilities_full(self, cep, mu=None):
        """The (N, C) log posteriors ``log w_c + log cst_c - 0.5 |M_c (x_n - mu_c)|^2`` (:490-508; ``sc_gmm_full_frame_loglik`` with its
        optional output); a 1-D ``cep`` is frames of one coefficient.  Host in, host out; a CUDA tensor stays there."""
        torch = _torch()
        if cep.ndim == 1:
            cep = cep[:, None]
        x, dt, host = _frames(torch, cep)
        lp = _loglik(torch, self, x, dt, mu, want_lp=True)[1]
        return lp.cpu().numpy() if host else lp

    def _expectation(self, accum, cep):
        """E-step (:586-617): the statistics of ``cep`` (host array or CUDA tensor; 1-D: frames of one coefficient) are added to
        ``accum.w``, ``accum.mu``, ``accum.invcov`` (C, D, D); returns the log-likelihood of the frames.  One ``sc_gmm_full_stats`` call;
        the reference's ``N x D x D`` temporary does not exist."""
        if cep.ndim == 1:
            cep = cep[:, None]
        stat0, stat1, stat2, llk = gmm_stats_full_device(self, cep, None, 2)
        host = (lambda t: t[0]) if isinstance(stat0, numpy.ndarray) else (lambda t: t[0].cpu().numpy())
        accum.w += host(stat0)
        accum.mu += host(stat1)
        accum.invcov += host(stat2)
        return float(host(llk))

    def _maximization(self, accum, ceil_cov=10, floor_cov=1e-2):
        """M-step (:673-686) from the statistics ``accum`` holds: weights = occupation shares, means = first order / occupation,
        covariances = second order / occupation - mean mean', inverted.  ``ceil_cov`` and ``floor_cov`` are accepted and unused, as in
        the reference (no variance control for full covariances); a component with zero occupation is not guarded."""
        self.w = accum.w / numpy.sum(accum.w)
        self.mu = accum.mu / accum.w[:, numpy.newaxis]
        cov = accum.invcov / accum.w[:, numpy.newaxis, numpy.newaxis] \
            - numpy.einsum('ijk,ilk->ijl', self.mu[:, :, numpy.newaxis], self.mu[:, :, numpy.newaxis])
        for gg in range(self.w.shape[0]):
            self.invcov[gg] = numpy.linalg.inv(cov[gg])
        self._compute_all()

    def _em_steps(self, x, count, after_iteration=None):
        """``count`` E / M steps on resident frames -> their log-likelihoods per unit of occupation"""
        llk = []
        accum = copy.deepcopy(self)
        for _ in range(count):
            accum._reset()
            total = self._expectation(accum, x)
            llk.append(total / numpy.sum(accum.w))
            self._maximization(accum)
            if after_iteration is not None:
                after_iteration(self, llk[-1])
        return llk

    def EM_diag2full(self, diagonal_mixture, features_server, featureList, iterations=2, num_thread=1):
        """EM from a diagonal mixture to full covariances (:926-1009) -> the list of log-likelihoods per unit of occupation, one per
        iteration.  ``features_server``: any object with ``stack_features(list, start_list=, stop_list=)``; the sessions are stacked once,
        as ``Mixture.EM_split`` stacks them, and the frames stay on the device over all iterations (``em_diag2full_device``).
        ``num_thread`` is accepted and unused.  The diagonal mixture is not changed."""
        features, _ = mixture.Mixture._stack_for_split(features_server, featureList)
        self.init_from_diag(diagonal_mixture)
        return self._em_steps(_frames(_torch(), features)[0], iterations)


def em_diag2full_device(diagonal_mixture, frames, iterations=2, reference_factor=False, after_iteration=None):
    """``EM_diag2full`` on a resident frame matrix -> ``(FullMixture, llk list)``: ``init_from_diag``, then ``iterations`` E / M steps,
    each E-step one ``sc_gmm_full_frame_loglik`` and one ``sc_gmm_full_stats`` over all frames; ``llk = sum lse / sum stat0`` per
    iteration.  ``after_iteration(mixture, llk)`` is called after every M-step."""
    x = _frames(_torch(), frames)[0]
    full = FullMixture(reference_factor=reference_factor)
    full.init_from_diag(diagonal_mixture)
    return full, full._em_steps(x, iterations, after_iteration)
