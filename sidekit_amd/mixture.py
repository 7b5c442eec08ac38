"""Diagonal Gaussian mixtures -- mirror of ``sidekit/mixture.py``: ``Mixture`` with the reference's attributes, its HDF5 file, ``EM_split``
(:721-833), ``EM_uniform`` (:835-894), ``compute_log_posterior_probabilities`` (:510-536) and the E / M steps they are made of.

The split is ``backend``'s: everything with a frame (N) dimension runs on the device in float64 through the C ABI
(``include/sidekit_amd/mixture.h``) -- ``sc_gmm_frame_loglik`` (the log-sum-exp of every frame over the components, and the ``N x C``
matrix of log posteriors only where the reference's method returns it) and ``sc_gmm_stats`` (zeroth, first and second order statistics
per segment, recomputing the posteriors tile by tile: no ``N x C`` array exists) -- and the ``C x D`` algebra (M-step, variance
control, the split, ``_compute_all``) stays on the host in the reference's operation order.  The ``*_device`` functions work on
resident frames (float32 or float64, widened in the load) and copy nothing with an N dimension to the host.  Beside the reference's
surface stand the top-C forms (Gaussian selection; ``include/sidekit_amd/gmm_topc_stats.h``): ``gmm_topc_posteriors_device`` gives the
posteriors of every frame over its list of ``top_c`` components (``gmm_scoring.gmm_top_components_device``) and
``gmm_stats_topc_device`` the statistics accumulated from them, ``K D`` of gather work per frame after the lists; and top-C EM
(``include/sidekit_amd/gmm_topc_em.h``): ``em_split_topc_device`` and ``Mixture.EM_split_topc`` train with the lists handed down the split
tree (``split_candidates``) and refreshed before every E-step from those candidates alone (``gmm_topc_refine_device``).  Full covariances
(``invcov.ndim == 3``) raise ``NotImplementedError`` here (``mixture_full.FullMixture`` is their class); ``read_alize``, ``read_htk``, ``write_alize`` and ``merge`` are not built.  There is
no CPU fallback; importing the module needs neither a GPU nor torch.
"""
import copy
import os

import numpy

from . import _lib, hdf5_lite
from .bosaris import IdMap

MAX_SLABS, SLAB_FRAMES = 64, 512    # SC_GMM_MAX_SLABS, SC_GMM_SLAB_FRAMES (include/sidekit_amd/mixture.h): the workspace of one sc_gmm_stats call
_DATASETS = ("w", "mu", "invcov", "invchol", "cov_var_ctl", "cst", "det")


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("sidekit_amd.mixture computes on the GPU only (no CPU fallback) and no GPU is visible")
    return torch


def _full_covariance():
    return NotImplementedError("full-covariance mixtures (invcov.ndim == 3) are not built: sidekit_amd.mixture is diagonal only "
                               "(sidekit_amd.mixture_full.FullMixture is the full-covariance class)")


def _frames(torch, frames):
    """frames -> ((N, D) contiguous CUDA tensor, float32 or float64, its XT_* dtype, whether they came from the host)"""
    host = not torch.is_tensor(frames)
    if host:
        a = numpy.asarray(frames)
        if a.dtype != numpy.float32:
            a = a.astype(numpy.float64, copy=False)
        if not (a.flags.c_contiguous and a.flags.writeable):     # torch wraps writable memory only
            a = numpy.array(a, order='C')
        frames = torch.as_tensor(a).to(torch.device("cuda", torch.cuda.current_device()))
    assert frames.is_cuda and frames.dim() == 2 and frames.shape[0] > 0, "expected (N, D) frames, N > 0"
    if frames.dtype not in (torch.float32, torch.float64):
        frames = frames.double()
    return frames.contiguous(), (_lib.XT_F32 if frames.dtype == torch.float32 else _lib.XT_F64), host


def _device_f64(torch, a, dev):
    """A host array or a tensor -> a contiguous float64 tensor on ``dev``"""
    if torch.is_tensor(a):
        return a.to(device=dev, dtype=torch.float64).contiguous()
    return torch.as_tensor(numpy.array(a, dtype=numpy.float64, order='C')).to(dev)   # a copy: the source may be read-only


def _offsets(seg_off, N):
    """``seg_off`` (``None``: one segment, all frames) -> the S + 1 offsets as int64, checked"""
    off = numpy.array([0, N], dtype=numpy.int64) if seg_off is None else numpy.asarray(seg_off, dtype=numpy.int64)
    assert off.ndim == 1 and off.shape[0] >= 2 and numpy.all(numpy.diff(off) >= 0) and off[0] >= 0 and off[-1] <= N, \
        "seg_off: S + 1 ascending offsets within [0, N]"
    return off


def _model(torch, ubm, dev, mu=None):
    """The device operands of a diagonal mixture: ``(mu, invcov, A)``; a replaced ``mu`` comes with its own ``A`` (:526-528)"""
    if ubm.invcov.ndim == 3:
        raise _full_covariance()
    assert ubm.invcov.ndim == 2 and ubm.mu.shape == ubm.invcov.shape, "a diagonal mixture has (C, D) means and inverse covariances"
    A = ubm.A
    if mu is None:
        mu = ubm.mu
    else:
        mu = numpy.asarray(mu, dtype=numpy.float64).reshape(ubm.mu.shape)
        A = (numpy.square(mu) * ubm.invcov).sum(1) - 2.0 * (numpy.log(ubm.w) + numpy.log(ubm.cst))
    A = numpy.broadcast_to(numpy.asarray(A, dtype=numpy.float64), ubm.w.shape)
    return _device_f64(torch, mu, dev), _device_f64(torch, ubm.invcov, dev), _device_f64(torch, A, dev)


def _loglik(torch, ubm, x, dt, mu=None, want_lp=False):
    N, D = x.shape
    assert D == ubm.dim(), 'dimension of ubm and features differ: {:d} / {:d}'.format(ubm.dim(), D)
    m, ic, A = _model(torch, ubm, x.device, mu)
    C = m.shape[0]
    lse = torch.empty(N, dtype=torch.float64, device=x.device)
    lp = torch.empty((N, C), dtype=torch.float64, device=x.device) if want_lp else None
    _lib.launch("sc_gmm_frame_loglik", x.device, x, dt, N, D, m, ic, A, C, lse, lp)
    return lse, lp, (m, ic, A)


def frame_loglik_device(ubm, frames, mu=None):
    """``lse[n] = log sum_c w_c N(x_n; mu_c, Sigma_c)`` of every frame (``sc_gmm_frame_loglik``): the per-frame term of
    ``sum_log_probabilities`` (:52-64).  ``frames`` (N, D) CUDA tensor (float32 or float64) or host array; ``mu`` replaces the means."""
    torch = _torch()
    x, dt, host = _frames(torch, frames)
    lse = _loglik(torch, ubm, x, dt, mu)[0]
    return lse.cpu().numpy() if host else lse


def _slabs(length):
    return min(MAX_SLABS, max(1, -(-int(length) // SLAB_FRAMES)))


def _segment_groups(lens, doubles_per_segment, budget_bytes):
    """Consecutive groups [a, b) of segments whose outputs and slab workspace, (1 + slabs of the longest) partials each, fit the budget"""
    groups, a, longest = [], 0, 0
    for i, n in enumerate(lens):
        top = max(longest, int(n))
        slabs = _slabs(top)
        if i > a and (i + 1 - a) * doubles_per_segment * 8 * (1 + (slabs if slabs > 1 else 0)) > budget_bytes:
            groups.append((a, i))
            a, top = i, int(n)
        longest = top
    groups.append((a, len(lens)))
    return groups


def gmm_stats_device(ubm, frames, seg_off=None, order=2, max_workspace_bytes=1 << 30):
    """Baum-Welch statistics of ``frames`` under ``ubm`` per segment (``sc_gmm_stats``; ``_expectation`` :586-617 with one segment and
    ``order=2``, ``StatServer.accumulate_stat`` with many and ``order=1``).  ``seg_off``: S + 1 ascending frame offsets (host), segment s
    is frames ``[seg_off[s], seg_off[s + 1])``; ``None``: one segment, all frames.  Returns ``(stat0 (S, C), stat1 (S, C, D), stat2
    (S, C, D) or None, llk (S,))``, float64, on the device when the frames were there.  Segments go to the kernel in consecutive groups
    whose outputs and slab workspace stay within ``max_workspace_bytes`` (one segment at least); the grouping does not change a bit."""
    assert order in (1, 2), "order: 1 (stat0, stat1) or 2 (and stat2)"
    torch = _torch()
    x, dt, host = _frames(torch, frames)
    N, D = x.shape
    dev = x.device
    off = _offsets(seg_off, N)
    S, lens = off.shape[0] - 1, numpy.diff(off)
    lse, _, (m, ic, A) = _loglik(torch, ubm, x, dt)
    C = m.shape[0]
    stat0 = torch.empty((S, C), dtype=torch.float64, device=dev)
    stat1 = torch.empty((S, C, D), dtype=torch.float64, device=dev)
    stat2 = torch.empty((S, C, D), dtype=torch.float64, device=dev) if order == 2 else None
    llk = torch.empty(S, dtype=torch.float64, device=dev)
    d_off = torch.as_tensor(off.astype(numpy.int32)).to(dev)
    for a, b in _segment_groups(lens, C * (order * D + 1), max_workspace_bytes):
        _lib.launch("sc_gmm_stats", dev, x, dt, N, D, m, ic, A, C, lse, d_off[a:], b - a, int(lens[a:b].max()), order, stat0[a:], stat1[a:],
                    None if stat2 is None else stat2[a:], llk[a:])
    out = (stat0, stat1, stat2, llk)
    return tuple(None if t is None else t.cpu().numpy() for t in out) if host else out


def _topc_posteriors(torch, ubm, x, dt, K, components):
    """``(idx (N, K) int32, post (N, K), lse (N,))`` on the frames' device: the lists (``sc_gmm_top_components``, or the caller's as they
    are -- the kernels skip an entry outside [0, C)) and the posteriors over them (``sc_gmm_topc_posteriors``)"""
    from . import gmm_scoring
    N, D = x.shape
    dev = x.device
    assert D == ubm.dim(), 'dimension of ubm and features differ: {:d} / {:d}'.format(ubm.dim(), D)
    assert ubm.invcov.ndim == 2 and ubm.mu.shape == ubm.invcov.shape, "a diagonal mixture has (C, D) means and inverse covariances"
    if components is None:
        idx = gmm_scoring._lists(torch, ubm, x, dt, K)
    else:
        idx = (components if torch.is_tensor(components) else torch.as_tensor(numpy.ascontiguousarray(components))).to(dev).contiguous()
    C = ubm.mu.shape[0]
    post = torch.empty((N, K), dtype=torch.float64, device=dev)
    lse = torch.empty(N, dtype=torch.float64, device=dev)
    _lib.launch("sc_gmm_topc_posteriors", dev, x, dt, N, D, *_topc_model(torch, ubm, dev), C, idx, K, post, lse)
    return idx, post, lse


def _topc_model(torch, ubm, dev):
    """The device operands of the direct-form kernels: ``(mu, invcov, B)``, ``B = -2 (log w + log cst)``"""
    with numpy.errstate(divide="ignore"):   # a zero weight: log 0, B = inf, posterior 0
        B = -2.0 * (numpy.log(ubm.w) + numpy.log(ubm.cst))
    return _device_f64(torch, ubm.mu, dev), _device_f64(torch, ubm.invcov, dev), _device_f64(torch, B, dev)


def gmm_topc_posteriors_device(ubm, frames, top_c=10, components=None):
    """Sparse posteriors (``sc_gmm_topc_posteriors``, ``include/sidekit_amd/gmm_topc_stats.h``): per frame the ``K = min(top_c, C)``
    components of its list, their posteriors renormalised over the list (they sum to 1) and ``lse[n] = log sum_k w_c N(x_n; mu_c,
    Sigma_c)`` over the list.  ``components``: (N, K) int32, host array or CUDA tensor -- an entry outside [0, C) contributes nothing and
    gets posterior 0, a frame without a valid entry has ``lse = -inf``; ``None``: the lists of ``gmm_top_components_device(ubm, frames,
    top_c)``.  ``frames``: (N, D) CUDA tensor (float32 or float64) or host array.  Returns ``(idx (N, K) int32, post (N, K) float64, lse
    (N,) float64)``, on the device when the frames were there.  No ``N x C`` array exists."""
    from . import gmm_scoring
    K = gmm_scoring._top_c(ubm, top_c, frames, components)
    torch = _torch()
    x, dt, host = _frames(torch, frames)
    out = _topc_posteriors(torch, ubm, x, dt, K, components)
    return tuple(t.cpu().numpy() for t in out) if host else out


def gmm_stats_topc_device(ubm, frames, seg_off=None, order=2, top_c=10, components=None, max_workspace_bytes=1 << 30):
    """``gmm_stats_device`` with every frame's posteriors cut to its list of ``min(top_c, C)`` components and renormalised over it
    (Gaussian selection; ``sc_gmm_topc_posteriors`` then ``sc_gmm_topc_stats``): a component's statistics sum over the frames that list
    it, ``llk`` sums ``lse`` over the lists.  ``components`` as ``gmm_topc_posteriors_device`` takes them, computed once per call
    whatever the grouping when ``None``.  The other arguments, the shapes, dtypes and placement of ``(stat0, stat1, stat2 or None, llk)``
    as ``gmm_stats_device``; the grouping does not change a bit, and a segment's statistics depend on its own frames and lists alone."""
    from . import gmm_scoring
    assert order in (1, 2), "order: 1 (stat0, stat1) or 2 (and stat2)"
    K = gmm_scoring._top_c(ubm, top_c, frames, components)
    torch = _torch()
    x, dt, host = _frames(torch, frames)
    N, D = x.shape
    dev = x.device
    off = _offsets(seg_off, N)
    S, lens = off.shape[0] - 1, numpy.diff(off)
    idx, post, lse = _topc_posteriors(torch, ubm, x, dt, K, components)
    C = ubm.mu.shape[0]
    stat0 = torch.empty((S, C), dtype=torch.float64, device=dev)
    stat1 = torch.empty((S, C, D), dtype=torch.float64, device=dev)
    stat2 = torch.empty((S, C, D), dtype=torch.float64, device=dev) if order == 2 else None
    llk = torch.empty(S, dtype=torch.float64, device=dev)
    d_off = torch.as_tensor(off.astype(numpy.int32)).to(dev)
    for a, b in _segment_groups(lens, C * (order * D + 1), max_workspace_bytes):
        _lib.launch("sc_gmm_topc_stats", dev, x, dt, N, D, C, idx, post, K, lse, d_off[a:], b - a, int(lens[a:b].max()), order, stat0[a:], stat1[a:],
                    None if stat2 is None else stat2[a:], llk[a:])
    out = (stat0, stat1, stat2, llk)
    return tuple(None if t is None else t.cpu().numpy() for t in out) if host else out


def split_candidates(idx, c_old):
    """The candidates a split hands down: ``(N, K)`` lists over the ``c_old`` parents -> ``(N, 2 K)`` int32 ``[idx, idx + c_old]``, the
    children of every listed parent in ``_split_ditribution``'s layout (the lower halves first, then the upper ones); an entry of -1
    stays -1 in both halves.  A CUDA tensor gives a CUDA tensor, anything else a host array."""
    if type(idx).__module__.split(".")[0] == "torch":
        import torch
        idx = idx.to(torch.int32)
        return torch.cat((idx, torch.where(idx < 0, idx, idx + int(c_old))), dim=1).contiguous()
    idx = numpy.asarray(idx, dtype=numpy.int32)
    return numpy.concatenate((idx, numpy.where(idx < 0, idx, idx + numpy.int32(c_old))), axis=1)


def _refine(torch, ubm, x, dt, cand, K, posteriors):
    """``sc_gmm_topc_refine`` on resident operands -> ``(idx (N, K) int32, post (N, K) or None, lse (N,) or None)``"""
    N, D = x.shape
    dev = x.device
    assert D == ubm.dim(), 'dimension of ubm and features differ: {:d} / {:d}'.format(ubm.dim(), D)
    assert ubm.invcov.ndim == 2 and ubm.mu.shape == ubm.invcov.shape, "a diagonal mixture has (C, D) means and inverse covariances"
    idx = torch.empty((N, K), dtype=torch.int32, device=dev)
    post = torch.empty((N, K), dtype=torch.float64, device=dev) if posteriors else None
    lse = torch.empty(N, dtype=torch.float64, device=dev) if posteriors else None
    _lib.launch("sc_gmm_topc_refine", dev, x, dt, N, D, *_topc_model(torch, ubm, dev), ubm.mu.shape[0], cand, cand.shape[1], K, idx, post, lse)
    return idx, post, lse


def gmm_topc_refine_device(ubm, frames, candidates, top_c=10, posteriors=False):
    """Lists refreshed from candidates (``sc_gmm_topc_refine``, ``include/sidekit_amd/gmm_topc_em.h``): per frame the ``K = min(top_c, C)``
    entries of its row of ``candidates`` that score best under ``ubm`` (the larger log posterior, at equal values the lower index), in
    ascending component order, ``2 Kc D`` of work per frame whatever ``C`` is.  ``candidates``: (N, Kc) int32 with ``Kc <= 64``, host
    array or CUDA tensor; an entry outside [0, C) and the repeat of an earlier entry of its row are ignored, and a row with fewer than
    ``K`` valid entries gives a list padded with -1.  ``frames``: (N, D) CUDA tensor (float32 or float64) or host array.  Returns ``idx
    (N, K) int32``, or with ``posteriors`` ``(idx, post (N, K) float64, lse (N,) float64)`` where ``post`` and ``lse`` have the bits of
    ``gmm_topc_posteriors_device(ubm, frames, top_c, components=idx)``; on the device when the frames were there."""
    from . import gmm_scoring
    K = gmm_scoring._top_c(ubm, top_c)
    shape, dtype = tuple(getattr(candidates, "shape", ())), getattr(candidates, "dtype", type(candidates).__name__)
    if len(shape) != 2 or shape[0] != numpy.shape(frames)[0] or not 1 <= shape[1] <= _lib.SC_GMM_TOPC_CAND_MAX or str(dtype).split(".")[-1] != "int32":
        raise ValueError("candidates: ({:d}, Kc) int32 with between 1 and {:d} candidates per frame (got {} {})".format(
            numpy.shape(frames)[0], _lib.SC_GMM_TOPC_CAND_MAX, shape, dtype))
    torch = _torch()
    x, dt, host = _frames(torch, frames)
    cand = (candidates if torch.is_tensor(candidates) else torch.as_tensor(numpy.ascontiguousarray(candidates))).to(x.device).contiguous()
    out = _refine(torch, ubm, x, dt, cand, K, posteriors)[:3 if posteriors else 1]
    if host:
        out = tuple(t.cpu().numpy() for t in out)
    return out if posteriors else out[0]


class _TopCLevels(object):
    """The E-steps of ``em_split_topc_device``, one level (the EM steps between two splits) at a time.  It keeps the lists the last level
    ended with (``None``: every component, the host-side fact after a dense level and before the first split)."""

    def __init__(self, x, top_c, exact_lists_at):
        self.torch = _torch()
        self.x, self.dt = x, (_lib.XT_F32 if x.dtype == self.torch.float32 else _lib.XT_F64)
        self.top_c, self.exact = int(top_c), frozenset(int(c) for c in exact_lists_at)
        self.idx, self.parents = None, 1

    def _candidates(self, ubm):
        from . import gmm_scoring
        C = ubm.mu.shape[0]
        if C in self.exact:
            return gmm_scoring.gmm_top_components_device(ubm, self.x, min(2 * self.top_c, _lib.SC_GMM_TOPC_MAX, C))
        if self.idx is None:
            everyone = self.torch.arange(self.parents, dtype=self.torch.int32, device=self.x.device)
            self.idx = everyone.expand(self.x.shape[0], self.parents)
        return split_candidates(self.idx, self.parents)

    def _expectation(self, ubm, accum, cand):
        """``Mixture._expectation`` with the posteriors cut to the lists refined from ``cand``: ``sc_gmm_topc_refine``, then
        ``sc_gmm_topc_stats`` with one segment at order 2"""
        torch, x, dt = self.torch, self.x, self.dt
        N, D = x.shape
        C, dev = ubm.mu.shape[0], x.device
        idx, post, lse = _refine(torch, ubm, x, dt, cand, self.top_c, True)
        stat0 = torch.empty((1, C), dtype=torch.float64, device=dev)
        stat1 = torch.empty((1, C, D), dtype=torch.float64, device=dev)
        stat2 = torch.empty((1, C, D), dtype=torch.float64, device=dev)
        llk = torch.empty(1, dtype=torch.float64, device=dev)
        d_off = torch.as_tensor(numpy.array([0, N], dtype=numpy.int32)).to(dev)
        _lib.launch("sc_gmm_topc_stats", dev, x, dt, N, D, C, idx, post, self.top_c, lse, d_off, 1, N, 2, stat0, stat1, stat2, llk)
        accum.w += stat0[0].cpu().numpy()
        accum.mu += stat1[0].cpu().numpy()
        accum.invcov += stat2[0].cpu().numpy()
        return float(llk[0])

    def steps(self, ubm, count, ceil_cov, floor_cov, after_iteration):
        """``count`` E / M steps of the just-split ``ubm`` -> their log-likelihoods per unit of occupation"""
        C = ubm.mu.shape[0]
        if C <= self.top_c:   # dense: Mixture._expectation as it is; afterwards every frame lists 0 .. C - 1
            self.idx, self.parents = None, C
            return ubm._em_steps(self.x, count, False, ceil_cov=ceil_cov, floor_cov=floor_cov, after_iteration=after_iteration)
        cand = self._candidates(ubm)
        llk = ubm._em_steps(self.x, count, False, ceil_cov=ceil_cov, floor_cov=floor_cov, after_iteration=after_iteration,
                            expectation=lambda accum, _: self._expectation(ubm, accum, cand))
        self.idx, self.parents = _refine(self.torch, ubm, self.x, self.dt, cand, self.top_c, False)[0], C   # under the model that is split next
        return llk


class Mixture(object):
    """A Gaussian mixture as the reference stores it: ``w`` (C,), ``mu`` (C, D), ``invcov`` (C, D) for diagonal covariances, ``invchol``,
    ``cov_var_ctl`` (C, D), ``cst`` (C,), ``det`` (C,), ``A`` (C,) and ``name``."""

    def __init__(self, mixture_file_name='', name='empty'):
        for dataset in _DATASETS:
            setattr(self, dataset, numpy.array([]))
        self.A = 0
        self.name = name
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

    def read(self, mixture_file_name, prefix=''):
        """The eight datasets ``<prefix>w, mu, invcov, invchol, cov_var_ctl, cst, det, a`` (:329-344)"""
        with hdf5_lite.File(mixture_file_name) as f:
            for name in _DATASETS:
                setattr(self, name, f[prefix + name][()])
            self.w = self.w.reshape(numpy.max(self.w.shape))
            self.A = f[prefix + 'a'][()]

    def write(self, mixture_file_name, prefix='', mode='w'):
        """The same datasets as float64 (:374-408); ``mode='a'`` keeps what the file holds beside them"""
        w = hdf5_lite.Writer()
        if mode != 'w' and os.path.exists(mixture_file_name):
            for path, arr in hdf5_lite.read_all(mixture_file_name).items():
                w[path] = arr
        for name in _DATASETS:
            w[prefix + name] = numpy.asarray(getattr(self, name), dtype=numpy.float64)
        w[prefix + 'a'] = numpy.asarray(self.A, dtype=numpy.float64)
        w.save(mixture_file_name)

    def _compute_all(self):
        """What follows from ``w, mu, invcov`` (:431-445), in the reference's order of operations: ``det = 1 / prod invcov``,
        ``cst = 1 / (sqrt(det) (2 pi)^(D / 2))`` and the data-independent term ``A = sum_d mu^2 invcov - 2 (log w + log cst)``"""
        if self.invcov.ndim == 3:
            raise _full_covariance()
        precision_product = self.invcov.prod(axis=1)
        self.det = 1.0 / precision_product
        normaliser = numpy.sqrt(self.det) * (2.0 * numpy.pi) ** (self.dim() / 2.0)
        self.cst = 1.0 / normaliser
        quadratic = (self.mu * self.mu * self.invcov).sum(axis=1)
        self.A = quadratic - 2.0 * (numpy.log(self.w) + numpy.log(self.cst))

    def _set(self, w, mu, invcov, cov_var_ctl):
        """New parameters, and everything ``_compute_all`` derives from them"""
        self.w, self.mu, self.invcov, self.cov_var_ctl = w, mu, invcov, cov_var_ctl
        self.cst = numpy.zeros(w.shape)
        self.det = numpy.zeros(w.shape)
        self._compute_all()

    def validate(self):
        """Whether the arrays have the shapes of one mixture: C weights, constants and determinants, (C, D) means, and (C, D) diagonal
        or (C, D, D) full inverse covariances"""
        if self.w.ndim != 1 or self.mu.ndim != 2:
            return False
        C, D = self.mu.shape
        if self.w.shape != (C,) or self.cst.shape != (C,) or self.det.shape != (C,):
            return False
        return self.invcov.shape in ((C, D), (C, D, D))

    def get_mean_super_vector(self):
        return self.mu.flatten()

    def get_invcov_super_vector(self):
        assert self.invcov.ndim == 2, 'the super-vector of inverse covariances exists for diagonal covariances only'
        return self.invcov.flatten()

    # ---- full covariances: not built --------------------------------------------------------------------------------------------------
    def init_from_diag(self, diag_mixture):
        raise _full_covariance()

    def compute_log_posterior_probabilities_full(self, cep, mu=None):
        raise _full_covariance()

    def EM_diag2full(self, diagonal_mixture, features_server, featureList, iterations=2, num_thread=1):
        raise _full_covariance()

    # ---- estimation -------------------------------------------------------------------------------------------------------------------
    def compute_log_posterior_probabilities(self, cep, mu=None):
        """The (N, C) log posteriors ``log(w_c N(x_n; mu_c, Sigma_c))`` (:510-536), the one method that wants the ``N x C`` matrix
        (``sc_gmm_frame_loglik`` with its optional output); a 1-D ``cep`` is one frame.  Host in, host out; a CUDA tensor stays there."""
        if self.invcov.ndim == 3:
            raise _full_covariance()
        torch = _torch()
        if cep.ndim == 1:
            cep = cep[None, :]
        x, dt, host = _frames(torch, cep)
        lp = _loglik(torch, self, x, dt, mu, want_lp=True)[1]
        return lp.cpu().numpy() if host else lp

    @staticmethod
    def variance_control(cov, flooring, ceiling, cov_ctl):
        """``cov`` limited, in place, to ``[flooring cov_ctl, ceiling cov_ctl]`` element by element (:538-555) -> ``cov``"""
        return numpy.clip(cov, flooring * cov_ctl, ceiling * cov_ctl, out=cov)

    def _reset(self):
        """An accumulator: zeros of the same shapes"""
        for name in ("w", "mu", "invcov", "cst", "det"):
            getattr(self, name).fill(0.0)
        self.A = 0.0

    def _split_ditribution(self):
        """Each distribution becomes two (:566-584), one standard deviation to either side of its mean along the coefficient of largest
        variance; the lower halves first, then the upper ones, each with half the weight and the parent's covariance and control"""
        variance = 1.0 / self.invcov
        widest = variance.argmax(axis=1)
        rows = numpy.arange(variance.shape[0])
        step = numpy.zeros_like(self.mu)
        step[rows, widest] = numpy.sqrt(variance[rows, widest])
        twice = lambda a: numpy.concatenate((a, a))   # noqa: E731
        self._set(twice(self.w) * 0.5, numpy.concatenate((self.mu - step, self.mu + step)), twice(self.invcov), twice(self.cov_var_ctl))

    def _expectation(self, accum, cep):
        """E-step (:586-617): the statistics of ``cep`` (host array or CUDA tensor; 1-D: frames of one coefficient) are added to
        ``accum.w``, ``accum.mu``, ``accum.invcov``; returns the log-likelihood of the frames.  One ``sc_gmm_stats`` call."""
        if self.invcov.ndim == 3:
            raise _full_covariance()
        if cep.ndim == 1:
            cep = cep[:, None]
        stat0, stat1, stat2, llk = gmm_stats_device(self, cep, None, 2)
        host = (lambda t: t[0]) if isinstance(stat0, numpy.ndarray) else (lambda t: t[0].cpu().numpy())
        accum.w += host(stat0)
        accum.mu += host(stat1)
        accum.invcov += host(stat2)
        return float(host(llk))

    def _maximization(self, accum, ceil_cov=10, floor_cov=1e-2):
        """M-step (:665-686) from the statistics ``accum`` holds (``w``: occupations, ``mu``: first, ``invcov``: second order): weights
        = occupation shares, means = first order / occupation, variances = second order / occupation - mean^2 under variance control"""
        if accum.invcov.ndim == 3:
            raise _full_covariance()
        occupation = accum.w[:, None]
        mean = accum.mu / occupation
        variance = accum.invcov / occupation - mean * mean
        Mixture.variance_control(variance, floor_cov, ceil_cov, self.cov_var_ctl)
        self._set(accum.w / accum.w.sum(), mean, 1.0 / variance, self.cov_var_ctl)

    def _init_single(self, mean, second_moment):
        """One Gaussian from a mean and a SECOND MOMENT, which stands where a variance is meant, as in ``_init`` (:709-719); the variance
        control is taken from it"""
        precision = 1.0 / second_moment[None]
        self._set(numpy.ones(1), mean[None], precision, 1.0 / precision)

    def _init_uniform(self, cep, distrib_nb):
        """The reference's uniform initialisation with its own behaviour (:896-924), which the fixture pins: component i is taken from
        the frames from ``i (N // distrib_nb)`` TO THE END (its window never stops short of the last frame), and only component 0 has its
        second moment inverted -- the others keep the second moment itself as ``invcov``.  The variance control is ``1 / invcov``."""
        stride = cep.shape[0] // distrib_nb
        means, moments = [], []
        for i in range(distrib_nb):
            window = cep[stride * i:max(stride * i + 10, cep.shape[0])]
            means.append(window.mean(axis=0))
            moments.append((window ** 2).mean(axis=0))
        invcov = numpy.stack(moments)
        invcov[0] = 1.0 / invcov[0]
        self._set(numpy.full(distrib_nb, 1.0 / distrib_nb), numpy.stack(means), invcov, 1.0 / invcov)

    def _em_steps(self, x, count, per_frame, stop=None, ceil_cov=10, floor_cov=1e-2, after_iteration=None, expectation=None):
        """``count`` E / M steps on resident frames -> their log-likelihoods, per frame (``per_frame``) or per unit of occupation;
        ``stop(llk list)`` ends the loop after an M-step; ``expectation(accum, x)`` stands in for ``_expectation``"""
        llk = []
        accum = copy.deepcopy(self)
        if expectation is None:
            expectation = self._expectation
        for _ in range(count):
            accum._reset()
            total = expectation(accum, x)
            llk.append(total / (x.shape[0] if per_frame else accum.w.sum()))
            self._maximization(accum, ceil_cov=ceil_cov, floor_cov=floor_cov)
            if after_iteration is not None:
                after_iteration(self, llk[-1])
            if stop is not None and stop(llk):
                break
        return llk

    def EM_uniform(self, cep, distrib_nb, iteration_min=3, iteration_max=10, llk_gain=0.01, do_init=True):
        """EM from the uniform initialisation (:835-894) -> the list of per-frame log-likelihoods, one per iteration: at most
        ``iteration_max``, and once more than ``iteration_min`` are done it ends with the first whose gain is below ``llk_gain``.  The
        frames are uploaded once."""
        if do_init:
            self._init_uniform(cep.cpu().numpy() if hasattr(cep, "cpu") else cep, distrib_nb)
        converged = lambda llk: len(llk) > max(iteration_min, 1) and llk[-1] - llk[-2] < llk_gain   # noqa: E731
        return self._em_steps(_frames(_torch(), cep)[0], iteration_max, True, stop=converged)

    def _unit(self, D):
        """One standard Gaussian: under it every posterior is exactly 1, so its statistics are the column sums of the frames"""
        self._set(numpy.ones(1), numpy.zeros((1, D)), numpy.ones((1, D)), numpy.ones((1, D)))
        return self

    def _em_split(self, x, distrib_nb, iterations, init_frames, ceil_cov, floor_cov, before_split=None, after_iteration=None, top_c=None,
                  exact_lists_at=()):
        """-> the llk list; with ``top_c`` (``em_split_topc_device``) ``(llk list, the lists the last level ended with or None)``"""
        x = _frames(_torch(), x)[0]
        head = x if init_frames is None else x[:init_frames]
        count, first, second, _ = gmm_stats_device(Mixture()._unit(x.shape[1]), head, None, 2)    # sum 1, sum x, sum x^2: no float64 copy of the frames
        self._init_single((first[0, 0] / count[0, 0]).cpu().numpy(), (second[0, 0] / count[0, 0]).cpu().numpy())
        levels = None if top_c is None else _TopCLevels(x, top_c, exact_lists_at)
        llk = []
        for steps in iterations[:int(numpy.log2(distrib_nb))]:
            if before_split is not None:
                before_split(self)
            self._split_ditribution()
            if levels is None:
                llk += self._em_steps(x, steps, False, ceil_cov=ceil_cov, floor_cov=floor_cov, after_iteration=after_iteration)
            else:
                llk += levels.steps(self, steps, ceil_cov, floor_cov, after_iteration)
        return llk if levels is None else (llk, levels.idx)

    @staticmethod
    def _stack_for_split(features_server, feature_list):
        """What ``EM_split`` trains on -> ``(frames, init_frames)``: every session stacked once, the first 20 (from which the single
        Gaussian the splits start from is taken: ``init_frames`` rows, ``None`` when there are no more sessions) and then the rest"""
        HEAD = 20
        if isinstance(feature_list, IdMap):
            sessions, bounds = feature_list.rightids, (feature_list.start, feature_list.stop)
        else:
            sessions, bounds = feature_list, None

        def stack(part):
            start, stop = (None, None) if bounds is None else (bounds[0][part], bounds[1][part])
            return features_server.stack_features(sessions[part], start_list=start, stop_list=stop)

        features = stack(slice(0, HEAD))
        init_frames = None
        if len(sessions) > HEAD:
            init_frames = features.shape[0]
            features = numpy.concatenate((features, stack(slice(HEAD, None))))
        return features, init_frames

    @staticmethod
    def _save_partial(save_partial, output_file_name):
        """``before_split`` of ``_em_split``: ``<output_file_name>_<C>g.h5``, or nothing"""
        return (lambda m: m.write('{}_{}g.h5'.format(output_file_name, m.get_distrib_nb()), prefix='')) if save_partial else None

    def EM_split(self, features_server, feature_list, distrib_nb, iterations=(1, 2, 2, 4, 4, 4, 4, 8, 8, 8, 8, 8, 8), num_thread=1,
                 llk_gain=0.01, save_partial=False, output_file_name="ubm", ceil_cov=10, floor_cov=1e-2):
        """EM with binary splits (:721-833) -> the list of log-likelihoods per unit of occupation, one per iteration.
        ``features_server``: any object with ``stack_features(list, start_list=, stop_list=)``; every session is stacked once (the first
        20, from which the single Gaussian the splits start from is taken, then the rest) and the frames stay on the device over all
        iterations (``em_split_device``).  An ``IdMap`` feature list gives the sessions (``rightids``) with their starts and stops.
        ``save_partial`` writes ``<output_file_name>_<C>g.h5`` before every split; ``num_thread`` and ``llk_gain`` are accepted and, as in
        the reference, unused."""
        features, init_frames = self._stack_for_split(features_server, feature_list)
        return self._em_split(features, distrib_nb, iterations, init_frames, ceil_cov, floor_cov,
                              before_split=self._save_partial(save_partial, output_file_name))

    def EM_split_topc(self, features_server, feature_list, distrib_nb, iterations=(1, 2, 2, 4, 4, 4, 4, 8, 8, 8, 8, 8, 8), top_c=10, num_thread=1,
                      llk_gain=0.01, save_partial=False, output_file_name="ubm", ceil_cov=10, floor_cov=1e-2, exact_lists_at=()):
        """``EM_split`` with Gaussian selection carried down the split tree (``em_split_topc_device``): the same sessions, stacked and
        saved as ``EM_split`` does, the same start, splits and M-steps; the E-steps of a level with more than ``top_c`` components sum
        over each frame's ``top_c`` best of the children of the components it listed before the split.  Not in the reference."""
        _topc_em_arguments(top_c)
        features, init_frames = self._stack_for_split(features_server, feature_list)
        return self._em_split(features, distrib_nb, iterations, init_frames, ceil_cov, floor_cov,
                              before_split=self._save_partial(save_partial, output_file_name), top_c=top_c, exact_lists_at=exact_lists_at)[0]


def em_split_device(frames, distrib_nb, iterations=(1, 2, 2, 4, 4, 4, 4, 8, 8, 8, 8, 8, 8), init_frames=None, ceil_cov=10, floor_cov=1e-2,
                    after_iteration=None):
    """``EM_split`` on a resident frame matrix -> ``(Mixture, llk list)``.  Starts from one Gaussian with the mean and the second moment
    (as the reference: not the variance) of the first ``init_frames`` rows (all when ``None``), then per entry of ``iterations``: split,
    and that many E / M steps, each E-step one ``sc_gmm_frame_loglik`` and one ``sc_gmm_stats`` over all frames;
    ``llk = sum lse / sum stat0`` per iteration.  ``after_iteration(mixture, llk)`` is called after every M-step."""
    ubm = Mixture()
    llk = ubm._em_split(frames, distrib_nb, iterations, init_frames, ceil_cov, floor_cov, after_iteration=after_iteration)
    return ubm, llk


def _topc_em_arguments(top_c):
    if not 1 <= int(top_c) <= _lib.SC_GMM_TOPC_MAX:
        raise ValueError("top_c: between 1 and {:d} components per frame (got {})".format(_lib.SC_GMM_TOPC_MAX, top_c))


def em_split_topc_device(frames, distrib_nb, iterations=(1, 2, 2, 4, 4, 4, 4, 8, 8, 8, 8, 8, 8), top_c=10, init_frames=None, ceil_cov=10,
                         floor_cov=1e-2, exact_lists_at=(), after_iteration=None):
    """``em_split_device`` with Gaussian selection carried down the split tree -> ``(Mixture, llk list)``: the same start from one
    Gaussian, the same split, the same host M-step and ``llk = sum lse / sum stat0`` per iteration; only the E-step differs.

    A level (the E / M steps between two splits) with ``C <= top_c`` components runs the dense E-step, so ``top_c >= distrib_nb`` is
    ``em_split_device`` bit for bit; after it every frame lists all ``C`` components.  A level with ``C > top_c`` takes its candidates
    once, right after the split: ``split_candidates`` of the lists the previous level ended with -- a split turns component ``c`` into
    ``c`` and ``c + C / 2``, so the ``top_c`` parents a frame listed give ``2 top_c`` children.  Before every E-step
    ``sc_gmm_topc_refine`` picks the frame's ``top_c`` best candidates under the current model and forms their posteriors, then
    ``sc_gmm_topc_stats`` accumulates one segment at order 2: ``2 top_c D`` and ``top_c D`` of gather work per frame whatever ``C`` is,
    against ``12 C D`` FLOP.  After the level's last M-step the lists are refined once more, so the next split descends from lists made
    under the model that is split.  ``exact_lists_at``: component counts; at a level whose ``C`` is one of them (and above ``top_c``) the
    candidates are the ``min(2 top_c, 32, C)`` best of all components under the just-split mixture (``gmm_top_components_device``), not the
    parents' children: it repairs whatever the lists have drifted by, at the cost of one dense pass per chosen level.

    Nothing with an ``N x C`` footprint exists; resident beside the frames are the candidates (N x 2 top_c int32), the lists, their
    posteriors and ``lse``.  A component that no frame lists has zero occupation and, as in ``_maximization`` today, is not guarded: its
    mean and variance become nan.  ``top_c`` between 1 and 32; diagonal covariances.  Not in the reference."""
    _topc_em_arguments(top_c)
    ubm = Mixture()
    llk, _ = ubm._em_split(frames, distrib_nb, iterations, init_frames, ceil_cov, floor_cov, after_iteration=after_iteration, top_c=top_c,
                           exact_lists_at=exact_lists_at)
    return ubm, llk
