"""PLDA and total-variability training -- mirror of ``sidekit/factor_analyser.py``: ``FactorAnalyser`` with ``plda`` (:830-932),
``total_variability`` / ``total_variability_single`` (:433-686), ``extract_ivectors`` / ``extract_ivectors_single`` (:688-828), ``write`` /
``read`` (:265-324), ``plda_device`` for x-vectors and ``total_variability_device`` / ``extract_ivectors_device`` for Baum-Welch
statistics that are already on the GPU.

The producer of the ``(mean, F, Sigma)`` that ``iv_scoring.fast_PLDA_scoring`` consumes.  The split is the scoring side's: everything
with an utterance (N) or class (C) dimension runs on the device in float64 through the C ABI -- ``sc_class_sums`` (the sums
``StatServer.sum_stat_per_model`` forms with one Python pass over all model ids per class), ``sc_gemm_tn`` (total scatter and the
EM accumulators, f64 MFMA with fixed-order split-K), ``sc_dgemm_nn`` (whitening and the E-step) -- and the ``D x D`` / ``rank x rank``
algebra (``eigh``, ``solve``, ``cholesky``, one ``inv``) stays on the host.  x-vectors are read as float32 or float64 and widened in the
load: there is no float64 copy of the corpus and, in ``plda_device``, no host copy either.

The E-step is restated.  The reference inverts ``I + n F'F`` once per distinct session count (``fa_model_loop``, :188-205); with
``F_w'F_w = U diag(a) U'`` from one host ``eigh`` the posterior mean of class ``i`` is ``E_h[i] = ((F_w' s_i) U / (1 + n_i a)) U'``,
so the device forms ``Q = (S_w F_w U) / (1 + n a')`` in one GEMM with a per-element scale, the accumulators ``Q'Q``, ``Q' diag(n) Q``,
``Q' S_w`` are rotated back by ``U`` on the host, and the two sums of inverses become ``U diag(sum_i 1 / (1 + n_i a)) U'`` and
``U diag(sum_i n_i / (1 + n_i a)) U'``.  ``F`` is defined up to the sign of each column (the eigenvectors that initialise it have none).

Total variability follows the same split.  ``e_on_batch`` (:51-91) loops over the sessions in Python and inverts one ``R x R`` matrix built
from the whole ``C D x R`` loading matrix per session; here the four large products are GEMMs -- the packed sums ``stat0 . G`` with
``G[c] = F_c' F_c`` (``sc_tv_gram``, once per iteration), the projections ``S_w . F`` and the accumulators (``sc_dgemm_nn``, ``sc_gemm_tn``)
-- and the per-session step between them (``Lambda = I + sum``, its inverse, ``e_h``, ``E_hh``) is one kernel, ``sc_tv_posterior``
(``include/sidekit_amd/ivector.h``), a workgroup per session with the packed matrix in LDS.  The M-step (``C`` solves of ``R x R`` systems, one
Cholesky factor) stays on the host in the reference's operation order.  Ranks above ``TV_MAX_RANK`` are ``factor_analyser_wide``'s (a
blocked factorisation outside LDS, ``WideFactorAnalyser``); ``total_variability_raw``, full-covariance UBMs and
``weighted_likelihood_plda`` are not built.
There is no CPU fallback for training or extraction; importing the module, ``write`` and ``read`` work on any host.
"""
import copy
import ctypes
import logging
import os

import numpy
import scipy.linalg

from . import _lib, hdf5_lite
from .statserver import STAT_TYPE, StatServer

SLICE_ROWS = 256   # rows one workgroup of the class-sum kernel adds; longer classes are cut into slices joined in order
TV_MAX_RANK = 192  # SC_TV_MAX_RANK (include/sidekit_amd/ivector.h): one packed triangle of the rank in LDS


class ClassIndex:
    """The class index of N rows as the CSR ``sc_class_sums`` takes (host arrays): ``ids`` = sorted unique labels, ``inverse`` = class
    number per row, ``counts`` = rows per class, ``rows`` = row numbers grouped by class (ascending inside a class), ``slice_off`` /
    ``class_slice_off`` = the cut of ``rows`` into slices of at most ``SLICE_ROWS`` that never straddle a class."""

    def __init__(self, class_index):
        labels = numpy.asarray(class_index)
        assert labels.ndim == 1 and labels.shape[0] > 0, "one class label per row"
        self.ids, self.inverse = numpy.unique(labels, return_inverse=True)
        n_classes = self.ids.shape[0]
        self.counts = numpy.bincount(self.inverse, minlength=n_classes)
        self.rows = numpy.argsort(self.inverse, kind="stable").astype(numpy.int32)
        class_off = numpy.concatenate(([0], numpy.cumsum(self.counts)))
        slices = (self.counts + SLICE_ROWS - 1) // SLICE_ROWS
        self.class_slice_off = numpy.concatenate(([0], numpy.cumsum(slices))).astype(numpy.int32)
        owner = numpy.repeat(numpy.arange(n_classes), slices)
        within = numpy.arange(owner.shape[0]) - self.class_slice_off[owner]
        self.slice_off = numpy.concatenate((class_off[owner] + within * SLICE_ROWS, [labels.shape[0]])).astype(numpy.int32)


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("sidekit_amd.factor_analyser trains on the GPU only (no CPU fallback) and no GPU is visible")
    return torch


def _stream(torch, device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _f64(torch, x, device):
    """host array or tensor -> contiguous float64 tensor on `device`"""
    if torch.is_tensor(x):
        return x.to(device=device, dtype=torch.float64).contiguous()
    return torch.as_tensor(numpy.ascontiguousarray(x, dtype=numpy.float64)).to(device)


def _rows(torch, x):
    """(N, D) CUDA tensor, float32 or float64, used where it is"""
    assert torch.is_tensor(x) and x.is_cuda and x.dim() == 2, "expected an (N, D) CUDA tensor"
    assert x.dtype in (torch.float32, torch.float64), "x-vectors must be float32 or float64"
    return x.contiguous(), (_lib.XT_F32 if x.dtype == torch.float32 else _lib.XT_F64)


def _ptr(t):
    return None if t is None else t.data_ptr()


def class_sums_device(xv, index):
    """Per-class sums of the rows of ``xv`` ((N, D) CUDA tensor, float32 or float64): ``index`` is a ``ClassIndex`` (or the labels).
    Returns ``(S, colsum)``, float64 device tensors (C, D) and (D,); ``colsum / N`` is the mean."""
    torch = _torch()
    index = index if isinstance(index, ClassIndex) else ClassIndex(index)
    x, dt = _rows(torch, xv)
    N, D = x.shape
    assert index.rows.shape[0] == N, "one class label per row"
    dev = x.device
    rows, soff, coff = (torch.as_tensor(a).to(dev) for a in (index.rows, index.slice_off, index.class_slice_off))
    C = index.ids.shape[0]
    S = torch.empty((C, D), dtype=torch.float64, device=dev)
    colsum = torch.empty(D, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().sc_class_sums(x.data_ptr(), dt, N, D, rows.data_ptr(), soff.data_ptr(), soff.shape[0] - 1, coff.data_ptr(), C,
                                            S.data_ptr(), colsum.data_ptr(), _stream(torch, dev)))
    return S, colsum


def gemm_tn_device(A, B=None, w=None, a=None, b=None):
    """``G = sum_k w[k] (A[k] - a)' (B[k] - b)``: A (K, M) and B (K, Nn) CUDA tensors of one dtype (float32 or float64; ``B=None``: A),
    ``w`` (K,), ``a`` (M,), ``b`` (Nn,) optional float64.  Returns the (M, Nn) float64 device tensor."""
    torch = _torch()
    A, dt = _rows(torch, A)
    B = A if B is None else _rows(torch, B)[0]
    assert B.dtype == A.dtype and B.shape[0] == A.shape[0] and B.device == A.device, "A and B: same dtype, rows and device"
    dev = A.device
    w, a, b = (None if v is None else _f64(torch, v, dev) for v in (w, a, b))
    assert w is None or w.shape == (A.shape[0],)
    assert a is None or a.shape == (A.shape[1],)
    assert b is None or b.shape == (B.shape[1],)
    G = torch.empty((A.shape[1], B.shape[1]), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().sc_gemm_tn(A.data_ptr(), B.data_ptr(), dt, A.shape[0], A.shape[1], B.shape[1], _ptr(w), _ptr(a), _ptr(b),
                                         G.data_ptr(), _stream(torch, dev)))
    return G


def dgemm_nn_device(A, B, alpha=1., rowv=None, colv=None, epilogue=_lib.SC_EPI_RANK1):
    """``alpha * A . B`` (float64, A on the device) with ``- rowv colv'`` (``SC_EPI_RANK1``) or ``/ (1 + rowv colv')`` (``SC_EPI_POSTERIOR``)."""
    torch = _torch()
    dev = A.device
    A, B = _f64(torch, A, dev), _f64(torch, B, dev)
    assert A.shape[1] == B.shape[0]
    rowv, colv = (None if v is None else _f64(torch, v, dev) for v in (rowv, colv))
    assert rowv is None or (rowv.shape == (A.shape[0],) and colv.shape == (B.shape[1],))
    C = torch.empty((A.shape[0], B.shape[1]), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().sc_dgemm_nn(A.data_ptr(), B.data_ptr(), A.shape[0], B.shape[1], A.shape[1], float(alpha), _ptr(rowv), _ptr(colv),
                                          int(epilogue), C.data_ptr(), _stream(torch, dev)))
    return C


def _em(xv, index, rank_f, nb_iter, scaling_factor, stat0_sums=None, after_iteration=None):
    """The EM of ``FactorAnalyser.plda`` on device-resident rows.  ``stat0_sums``: per-class sums of the zero-order statistics (the
    session counts when None, as for x-vectors).  ``after_iteration(it, mean, F, Sigma)`` is called after every iteration."""
    torch = _torch()
    N, D = xv.shape
    assert 0 < rank_f <= D, "rank_f must be in [1, D]"
    dev = xv.device
    C = index.ids.shape[0]
    S, colsum = class_sums_device(xv, index)
    mean = colsum.cpu().numpy() / N
    mean_d = _f64(torch, mean, dev)
    sigma_obs = gemm_tn_device(xv, None, None, mean_d, mean_d).cpu().numpy() / N          # get_total_covariance_stat1
    sessions = index.counts.astype(STAT_TYPE) * scaling_factor                            # session_per_model (:863)
    n = sessions if stat0_sums is None else numpy.asarray(stat0_sums, dtype=STAT_TYPE) * scaling_factor   # model stat0 (:861)
    n_d = _f64(torch, n, dev)
    evals, evecs = scipy.linalg.eigh(sigma_obs)
    F = evecs.real[:, numpy.argsort(evals)[::-1][:rank_f]]
    Sigma = sigma_obs.copy()
    for it in range(nb_iter):
        logging.info('Estimate between class covariance, it %d / %d', it + 1, nb_iter)
        lam, vec = scipy.linalg.eigh(Sigma)
        order = lam.real.argsort()[::-1]
        W = vec.real[:, order] * (1 / numpy.sqrt(lam.real[order]))                        # sqr_inv_sigma (:886-891)
        # whitened, centred class sums (S - n mu') W = scaling * S_raw W - n (mu' W)
        Sw = dgemm_nn_device(S, W, scaling_factor, n_d, mean.dot(W), _lib.SC_EPI_RANK1)
        Fw = W.T.dot(F)
        a, U = numpy.linalg.eigh(Fw.T.dot(Fw))
        Q = dgemm_nn_device(Sw, Fw.dot(U), 1., n_d, a, _lib.SC_EPI_POSTERIOR)             # E_h U: posterior means in the eigenbasis
        QQ, QnQ, QS = gemm_tn_device(Q), gemm_tn_device(Q, None, n_d), gemm_tn_device(Q, Sw)
        QQ, QnQ, QS = QQ.cpu().numpy(), QnQ.cpu().numpy(), QS.cpu().numpy()
        g = 1.0 / (1.0 + n[:, None] * a[None, :])                                         # posterior covariances, diagonal in U
        R = (U * g.sum(axis=0)).dot(U.T) + U.dot(QQ).dot(U.T)                             # sum_i E[h h']
        A = (U * (n[:, None] * g).sum(axis=0)).dot(U.T) + U.dot(QnQ).dot(U.T)             # sum_i n_i E[h h']
        Cm = U.dot(QS).dot(scipy.linalg.inv(W))
        F = scipy.linalg.solve(A, Cm).T                                                   # M-step
        Sigma = sigma_obs - F.dot(Cm) / sessions.sum()
        F = F.dot(scipy.linalg.cholesky(R / C))                                           # minimum divergence
        if after_iteration is not None:
            after_iteration(it, mean, F, Sigma)
    return mean, F, Sigma


def plda_device(xv, class_index, rank_f, nb_iter=10, scaling_factor=1.):
    """Train PLDA on x-vectors that are on the GPU: ``xv`` (N, D) CUDA tensor, float32 or float64, ``class_index`` one integer label
    per row (tensor or array).  Returns ``(mean, F, Sigma)`` as float64 numpy arrays; ``xv`` is never copied to the host."""
    torch = _torch()
    if torch.is_tensor(class_index):
        class_index = class_index.cpu().numpy()
    return _em(xv, ClassIndex(class_index), rank_f, nb_iter, scaling_factor)


# ---- total variability ------------------------------------------------------------------------------------------------------------------

def packed_size(rank):
    """Doubles of a packed upper triangle; (i, j), i <= j, is at ``i R - i (i - 1) / 2 + (j - i)``, the order of ``numpy.triu_indices``"""
    return rank * (rank + 1) // 2


def _unpack(p, rank):
    full = numpy.zeros((rank, rank), dtype=STAT_TYPE)
    upper = numpy.triu_indices(rank)
    full[upper] = full.T[upper] = p
    return full


def _check_rank(tv_rank):
    if not 1 <= tv_rank <= TV_MAX_RANK:
        raise ValueError("tv_rank = {} is outside [1, {}]: sc_tv_posterior keeps one packed triangle of the rank in LDS "
                         "(SC_TV_MAX_RANK = {}); sidekit_amd.factor_analyser_wide (WideFactorAnalyser) takes ranks up to 1024"
                         .format(tv_rank, TV_MAX_RANK, TV_MAX_RANK))


def _check_ubm(ubm):
    """A diagonal mixture -> (C, D); a full-covariance one is refused like everywhere in ``sidekit_amd.mixture``"""
    from .mixture import Mixture, _full_covariance
    assert isinstance(ubm, Mixture) and ubm.validate(), "Second argument must be a proper Mixture"
    if ubm.invcov.ndim == 3:
        raise _full_covariance()
    return ubm.mu.shape


def _statistics(torch, stat0, stat1, C, D):
    """Resident statistics as ``gmm_stats_device`` returns them (stat1 (N, C, D) or (N, C D)) -> float64 (N, C) and (N, C D), used where they are"""
    assert torch.is_tensor(stat0) and torch.is_tensor(stat1) and stat0.is_cuda and stat1.is_cuda, "expected statistics on the device (CUDA tensors)"
    stat0, stat1 = _f64(torch, stat0, stat0.device), _f64(torch, stat1, stat0.device)
    assert stat0.dim() == 2 and stat0.shape[1] == C and stat0.shape[0] > 0, "stat0: (sessions, C)"
    assert stat1.shape[0] == stat0.shape[0] and stat1.numel() == stat0.shape[0] * C * D, "stat1: (sessions, C D)"
    return stat0, stat1.reshape(stat0.shape[0], C * D)


def _whitener(torch, ubm, dev):
    """(mean, sqrt(invcov)) as (C, D) device tensors"""
    return _f64(torch, ubm.mu, dev), torch.sqrt(_f64(torch, ubm.invcov, dev))


def _whiten(stat0, stat1, whitener):
    """``(stat1 - stat0[:, index_map] * mean_sv) * sqrt(invcov_sv)`` (:75-78) as a new tensor"""
    mean, scale = whitener
    N, C = stat0.shape
    return ((stat1.view(N, C, -1) - stat0[:, :, None] * mean) * scale).view(N, -1)


def _batch_rows(N, C, D, R, max_workspace_bytes):
    """Sessions per device batch: the packed triangle, the whitened statistics, the counts and two R-vectors per session within the budget"""
    return max(1, min(N, int(max_workspace_bytes) // (8 * (packed_size(R) + C * D + C + 2 * R))))


def tv_gram_device(F, C):
    """``G[c] = F_c' F_c`` packed, (C, P) (``sc_tv_gram``): F ((C D), R) float64 CUDA tensor"""
    torch = _torch()
    F = _f64(torch, F, F.device)
    R = F.shape[1]
    _check_rank(R)
    assert F.shape[0] % C == 0
    G = torch.empty((C, packed_size(R)), dtype=torch.float64, device=F.device)
    _lib.launch("sc_tv_gram", F.device, F, C, F.shape[0] // C, R, G)
    return G


def tv_posterior_device(stat0, stat1_w, F, G=None, want="packed"):
    """The posterior of every session given WHITENED first-order statistics (``e_on_batch`` :85-89): ``stat0`` (N, C), ``stat1_w``
    (N, C D), ``F`` ((C D), R) float64 CUDA tensors, ``G`` the packed Gram matrices of ``F`` (``tv_gram_device``; formed when None).
    Returns ``(e_h (N, R), E_hh)``: ``want="packed"``: the (N, P) packed upper triangles of ``inv_lambda + e_h e_h'``; ``"diag"``: their
    (N, R) diagonals only.  Two ``sc_dgemm_nn`` and one ``sc_tv_posterior``; the packed sums are overwritten by the packed output."""
    assert want in ("packed", "diag")
    torch = _torch()
    dev = stat0.device
    R = F.shape[1]
    _check_rank(R)
    if G is None:
        G = tv_gram_device(F, stat0.shape[1])
    Lp = dgemm_nn_device(stat0, G)
    B = dgemm_nn_device(stat1_w, F)
    e_h = torch.empty_like(B)
    diag = torch.empty_like(B) if want == "diag" else None
    _lib.launch("sc_tv_posterior", dev, Lp, B, Lp.shape[0], R, e_h, Lp if want == "packed" else None, diag)
    return e_h, (Lp if want == "packed" else diag)


def tv_m_step(_A, _C, _R, nb_sessions, min_div=True):
    """The host M-step (:516-530) from the accumulators ``_A`` (C, P), ``_C`` (R, C D), ``_R`` (P,) summed over ``nb_sessions``: per
    component ``F_c = solve(unpack(_A[c]), _C[:, c]).T``, then ``F . cholesky(unpack(_R / nb_sessions))`` when ``min_div``"""
    C, R = _A.shape[0], _C.shape[0]
    D = _C.shape[1] // C
    F = numpy.empty((C * D, R), dtype=STAT_TYPE)
    for c in range(C):
        F[c * D:(c + 1) * D, :] = scipy.linalg.solve(_unpack(_A[c], R), _C[:, c * D:(c + 1) * D]).T
    if min_div:
        F = F.dot(scipy.linalg.cholesky(_unpack(_R / nb_sessions, R)))
    return F


GEMM_TN_MAX_OUTPUT = 1 << 28  # sc_gemm_tn: M * Nn doubles at most in one call


def _count_weighted_sums(stat0, e_hh):
    """``stat0' . e_hh`` (C, P), the accumulator ``_A``.  One ``sc_gemm_tn`` while ``C P`` is within its bound, as ever; beyond it
    (C = 2 048 at rank 600 is 3.7e8) one call per block of components, each on a copy of the block's columns of ``stat0``."""
    C, P = stat0.shape[1], e_hh.shape[1]
    if C * P <= GEMM_TN_MAX_OUTPUT:
        return gemm_tn_device(stat0, e_hh)
    step = max(1, GEMM_TN_MAX_OUTPUT // P)
    return _torch().cat([gemm_tn_device(stat0[:, c:c + step], e_hh) for c in range(0, C, step)])


def _tv_e_step(torch, stat0, stat1, whitener, F_d, rows, posterior=tv_posterior_device, gram=tv_gram_device, to_host=True):
    """The accumulators of one E-step over all sessions, added in batch order -> host ``(_A, _C, _R)``; device tensors (``_R`` as
    (1, P)) when not ``to_host``.  ``posterior`` / ``gram``: the two calls of another rank range (``factor_analyser_wide``)."""
    N, C = stat0.shape
    G = gram(F_d, C)
    ones = torch.ones((rows, 1), dtype=torch.float64, device=stat0.device)
    acc = None
    for a in range(0, N, rows):
        s0 = stat0[a:a + rows]
        sw = _whiten(s0, stat1[a:a + rows], whitener)
        e_h, e_hh = posterior(s0, sw, F_d, G)
        part = (_count_weighted_sums(s0, e_hh), gemm_tn_device(e_h, sw), gemm_tn_device(ones[:s0.shape[0]], e_hh))
        acc = part if acc is None else tuple(t.add_(p) for t, p in zip(acc, part))
    if not to_host:
        return acc
    return acc[0].cpu().numpy(), acc[1].cpu().numpy(), acc[2].cpu().numpy()[0]


def total_variability_device(stat0, stat1, ubm, tv_rank, nb_iter=20, min_div=True, tv_init=None, max_workspace_bytes=1 << 30,
                             after_iteration=None):
    """Train a total variability matrix on Baum-Welch statistics that are on the GPU (the output of ``mixture.gmm_stats_device`` as it
    is): ``stat0`` (N, C), ``stat1`` (N, C, D) or (N, C D), not whitened and not modified.  ``tv_init=None`` draws
    ``numpy.random.randn(sv_size, tv_rank)`` as the reference does (:476), so ``numpy.random.seed`` gives the same start.  Sessions go
    through the E-step in batches cut from ``max_workspace_bytes`` (``P + C D + C + 2 R`` doubles per session, one session at least);
    the accumulators are added in batch order.  The M-step runs on the host.  ``after_iteration(it, F)`` is called after every
    iteration.  Returns ``F`` ((C D), R), a float64 numpy array; the statistics are never copied to the host."""
    C, D = _check_ubm(ubm)
    _check_rank(tv_rank)
    assert isinstance(nb_iter, int) and 0 < nb_iter, "nb_iter must be a positive integer"
    torch = _torch()
    stat0, stat1 = _statistics(torch, stat0, stat1, C, D)
    N, dev = stat0.shape[0], stat0.device
    F = numpy.random.randn(C * D, tv_rank) if tv_init is None else numpy.array(tv_init, dtype=STAT_TYPE)
    assert F.shape == (C * D, tv_rank), "tv_init: (C D, tv_rank)"
    whitener = _whitener(torch, ubm, dev)
    rows = _batch_rows(N, C, D, tv_rank, max_workspace_bytes)
    for it in range(nb_iter):
        logging.info('Total variability, it %d / %d', it + 1, nb_iter)
        _A, _C, _R = _tv_e_step(torch, stat0, stat1, whitener, _f64(torch, F, dev), rows)
        F = tv_m_step(_A, _C, _R, N, min_div)
        if after_iteration is not None:
            after_iteration(it, F)
    return F


def _extract(stat0, stat1, whitener, F, uncertainty, max_workspace_bytes, posterior=tv_posterior_device, gram=tv_gram_device,
             batch_rows=_batch_rows):
    """i-vectors (and the diagonal of ``E_hh``) of resident statistics; ``whitener=None``: ``stat1`` is whitened already.
    ``posterior`` / ``gram`` / ``batch_rows``: those of another rank range (``factor_analyser_wide``)."""
    torch = _torch()
    N, C = stat0.shape
    R = F.shape[1]
    F_d = _f64(torch, F, stat0.device)
    G = gram(F_d, C)
    iv = torch.empty((N, R), dtype=torch.float64, device=stat0.device)
    iv_sigma = torch.empty_like(iv)
    rows = batch_rows(N, C, stat1.shape[1] // C, R, max_workspace_bytes)
    for a in range(0, N, rows):
        s0, s1 = stat0[a:a + rows], stat1[a:a + rows]
        iv[a:a + rows], iv_sigma[a:a + rows] = posterior(s0, s1 if whitener is None else _whiten(s0, s1, whitener), F_d, G, want="diag")
    return (iv, iv_sigma) if uncertainty else iv


def extract_ivectors_device(stat0, stat1, ubm, F, uncertainty=False, max_workspace_bytes=1 << 30):
    """i-vectors of Baum-Welch statistics that are on the GPU (``stat0`` (N, C), ``stat1`` (N, C, D) or (N, C D), not whitened, not
    modified) under the loading matrix ``F`` ((C D), R): ``iv`` (N, R), or ``(iv, iv_sigma)`` with the diagonal of ``E_hh`` when
    ``uncertainty``; float64 CUDA tensors.  Batches as in ``total_variability_device``."""
    C, D = _check_ubm(ubm)
    _check_rank(F.shape[1])
    assert F.shape[0] == C * D, "F: (C D, R)"
    torch = _torch()
    stat0, stat1 = _statistics(torch, stat0, stat1, C, D)
    return _extract(stat0, stat1, _whitener(torch, ubm, stat0.device), F, uncertainty, max_workspace_bytes)


def _read_statistics(source, prefix=''):
    """A ``StatServer`` object, or the file of one (read with ``hdf5_lite``)"""
    return source if isinstance(source, StatServer) else StatServer.read(source, prefix)


def _ivector_server(stat_server, iv):
    """The reference's i-vector ``StatServer`` (:719-725): copies of the identifiers, ones as ``stat0``"""
    out = StatServer()
    out.modelset, out.segset = copy.deepcopy(stat_server.modelset), copy.deepcopy(stat_server.segset)
    out.start, out.stop = copy.deepcopy(stat_server.start), copy.deepcopy(stat_server.stop)
    out.stat0 = numpy.ones((stat_server.modelset.shape[0], 1), dtype=STAT_TYPE)
    out.stat1 = iv
    return out


class FactorAnalyser:
    """``sidekit.FactorAnalyser`` (factor_analyser.py:208-262) for PLDA and total variability: attributes ``mean, F, G, H, Sigma``."""

    def __init__(self, input_file_name=None, mean=None, F=None, G=None, H=None, Sigma=None):
        self.mean = self.F = self.G = self.H = self.Sigma = None
        if input_file_name is not None:
            fa = FactorAnalyser.read(input_file_name)
            self.mean, self.F, self.G, self.H, self.Sigma = fa.mean, fa.F, fa.G, fa.H, fa.Sigma
        for name, value in (("mean", mean), ("F", F), ("G", G), ("H", H), ("Sigma", Sigma)):
            if value is not None:
                setattr(self, name, value)

    _DATASETS = (("mean", "fa/mean"), ("F", "fa/f"), ("G", "fa/g"), ("H", "fa/h"), ("Sigma", "fa/sigma"))

    def write(self, output_file_name):
        """The reference's layout (:265-300): ``fa/mean, fa/f, fa/g, fa/h, fa/sigma`` for the fields that are set, ``fa/kind`` = int16[5]
        flags of which ones are."""
        folder = os.path.dirname(output_file_name)
        if folder:
            os.makedirs(folder, exist_ok=True)
        w = hdf5_lite.Writer()
        kind = numpy.zeros(5, dtype="int16")
        for i, (name, path) in enumerate(self._DATASETS):
            value = getattr(self, name)
            if value is not None:
                kind[i] = 1
                w[path] = numpy.asarray(value)
        w["fa/kind"] = kind
        w.save(output_file_name)

    @staticmethod
    def read(input_filename):
        fa = FactorAnalyser()
        with hdf5_lite.File(input_filename) as fh:
            kind = fh["fa/kind"][()]
            for i, (name, path) in enumerate(FactorAnalyser._DATASETS):
                if kind[i] != 0:
                    setattr(fa, name, fh[path][()])
        return fa

    def plda(self, stat_server, rank_f, nb_iter=10, scaling_factor=1., output_file_name=None, save_partial=False, save_final=True,
             num_thread=1):
        """Simplified PLDA (no within-class sub-space, full residual covariance), factor_analyser.py:830-932: classes are
        ``numpy.unique(stat_server.modelset)``, the statistics are scaled by ``scaling_factor``, ``F`` starts from the top ``rank_f``
        eigenvectors of the total covariance.  ``stat1`` is uploaded once; the rest is ``plda_device``'s code.  ``num_thread`` is
        accepted and ignored.  Saves ``<output_file_name>_it-<k>.h5`` / ``<output_file_name>.h5`` when the reference does."""
        torch = _torch()
        assert stat_server.stat0.shape[1] == 1, "PLDA training takes one zero-order statistic per session (x-vectors / i-vectors)"
        index = ClassIndex(stat_server.modelset)
        stat0_sums = numpy.bincount(index.inverse, weights=stat_server.stat0[:, 0], minlength=index.ids.shape[0])
        xv = torch.as_tensor(numpy.ascontiguousarray(stat_server.stat1, dtype=STAT_TYPE)).to(torch.device("cuda", torch.cuda.current_device()))
        if output_file_name is None:
            output_file_name = "plda"

        def save(it, mean, F, Sigma):
            self.mean, self.F, self.Sigma = mean, F, Sigma
            if save_partial and it < nb_iter - 1:
                self.write(output_file_name + "_it-{}.h5".format(it))
            elif it == nb_iter - 1 and save_final:
                self.write(output_file_name + ".h5")

        self.mean, self.F, self.Sigma = _em(xv, index, rank_f, nb_iter, scaling_factor, stat0_sums, save)

    # ---- total variability (sidekit_amd/csrc/ivector.hip): no CPU fallback ---------------------------------------------------------------

    # what depends on the rank range; factor_analyser_wide.WideFactorAnalyser replaces these four and inherits the methods
    _check_rank = staticmethod(_check_rank)
    _train_device = staticmethod(total_variability_device)
    _extract_whitened = staticmethod(_extract)
    _extract_device = staticmethod(extract_ivectors_device)

    def total_variability(self, stat_server_filename, ubm, tv_rank, nb_iter=20, min_div=True, tv_init=None, batch_size=300, save_init=False,
                          output_file_name=None, num_thread=1):
        """Train a total variability model (:539-686).  ``stat_server_filename``: the name of a ``StatServer`` file (read with
        ``hdf5_lite``), a list of names, or a ``StatServer`` object; with a list the sessions of all files accumulate into one E-step and
        ``_R`` is divided by their total, as in the reference.  The statistics are uploaded once and stay on the device over all
        iterations (``total_variability_device``); they are not modified.  ``batch_size`` and ``num_thread`` are accepted and ignored: the
        device batch is cut from a memory budget, not from a session count, and there are no worker processes.  Sets ``mean`` and
        ``Sigma`` to zeros of the supervector size and ``F``; with ``output_file_name`` saves ``<output_file_name>_it-<k>.h5`` after
        every iteration but the last and ``<output_file_name>.h5`` after the last; ``save_init`` writes ``<output_file_name>_init.h5``
        and needs ``output_file_name`` (the reference raises a ``TypeError`` without it)."""
        C, D = _check_ubm(ubm)
        self._check_rank(tv_rank)
        assert isinstance(nb_iter, int) and 0 < nb_iter, "nb_iter must be a positive integer"
        assert not save_init or output_file_name is not None, "save_init needs output_file_name"
        torch = _torch()
        sources = stat_server_filename if isinstance(stat_server_filename, list) else [stat_server_filename]
        servers = [_read_statistics(src) for src in sources]
        dev = torch.device("cuda", torch.cuda.current_device())
        stat0, stat1 = (torch.cat([torch.as_tensor(numpy.ascontiguousarray(getattr(sv, name), dtype=STAT_TYPE)).to(dev) for sv in servers])
                        for name in ("stat0", "stat1"))
        self.mean = numpy.zeros(ubm.get_mean_super_vector().shape, dtype=STAT_TYPE)
        self.Sigma = numpy.zeros(ubm.get_mean_super_vector().shape, dtype=STAT_TYPE)
        self.F = numpy.random.randn(C * D, tv_rank).astype(STAT_TYPE) if tv_init is None else tv_init
        if save_init:
            self.write(output_file_name + "_init.h5")

        def save(it, F):
            self.F = F
            if output_file_name is not None:
                self.write(output_file_name + ("_it-{}.h5".format(it) if it < nb_iter - 1 else ".h5"))

        self.F = self._train_device(stat0, stat1, ubm, tv_rank, nb_iter, min_div, self.F, after_iteration=save)

    def total_variability_single(self, stat_server_filename, ubm, tv_rank, nb_iter=20, min_div=True, tv_init=None, batch_size=300,
                                 save_init=False, output_file_name=None):
        """The reference's single-process variant (:433-537): here the same code as ``total_variability``"""
        self.total_variability(stat_server_filename, ubm, tv_rank, nb_iter, min_div, tv_init, batch_size, save_init, output_file_name)

    def extract_ivectors_single(self, ubm, stat_server, uncertainty=False):
        """i-vectors of a ``StatServer`` (:688-744) -> a ``StatServer`` with the i-vectors as ``stat1``, ones as ``stat0`` and copies of
        ``modelset``, ``segset``, ``start``, ``stop``; with ``uncertainty`` also ``iv_sigma``, the diagonal of ``E_hh``.  As in the
        reference the caller's ``stat_server`` is left whitened in place (``whiten_stat1``)."""
        assert isinstance(stat_server, StatServer) and stat_server.validate(), "First argument must be a proper StatServer"
        C, D = _check_ubm(ubm)
        self._check_rank(self.F.shape[1])
        torch = _torch()
        stat_server.whiten_stat1(ubm.get_mean_super_vector(), 1. / ubm.get_invcov_super_vector())
        dev = torch.device("cuda", torch.cuda.current_device())
        stat0, stat1 = _statistics(torch, *(torch.as_tensor(numpy.ascontiguousarray(x, dtype=STAT_TYPE)).to(dev)
                                            for x in (stat_server.stat0, stat_server.stat1)), C, D)
        iv, iv_sigma = self._extract_whitened(stat0, stat1, None, self.F, True, 1 << 30)
        out = _ivector_server(stat_server, iv.cpu().numpy())
        return (out, iv_sigma.cpu().numpy()) if uncertainty else out

    def extract_ivectors(self, ubm, stat_server_filename, prefix='', batch_size=300, uncertainty=False, num_thread=1):
        """i-vectors of the ``StatServer`` stored in a file (:746-828), or of a ``StatServer`` object, which is not modified -> as
        ``extract_ivectors_single``.  ``batch_size`` and ``num_thread`` are accepted and ignored (the device batch is cut from a memory
        budget).  One deviation on purpose: ``prefix`` applies to every dataset that is read; the reference forgets it on ``stat0`` /
        ``stat1`` (:808)."""
        C, D = _check_ubm(ubm)
        self._check_rank(self.F.shape[1])
        torch = _torch()
        server = _read_statistics(stat_server_filename, prefix)
        dev = torch.device("cuda", torch.cuda.current_device())
        stat0, stat1 = (torch.as_tensor(numpy.ascontiguousarray(x, dtype=STAT_TYPE)).to(dev) for x in (server.stat0, server.stat1))
        iv, iv_sigma = self._extract_device(stat0, stat1, ubm, self.F, uncertainty=True)
        out = _ivector_server(server, iv.cpu().numpy())
        return (out, iv_sigma.cpu().numpy()) if uncertainty else out
