"""Total variability at the ranks i-vector systems are trained at (400, 600; up to ``TVW_MAX_RANK`` = 1024): ``WideFactorAnalyser``,
``total_variability_wide_device`` and ``extract_ivectors_wide_device`` beside ``factor_analyser``'s, which keep their cap of 192, their
bits and their refusals -- as ``mixture_full`` stands beside ``mixture``.

``factor_analyser``'s per-session kernel holds one packed triangle of the rank in LDS.  ``sc_tvw_posterior``
(``include/sidekit_amd/ivector_wide.h``, ``csrc/ivector_wide.hip``) keeps the session's matrix in scratch that the caller owns,
``2 Rp^2`` doubles per session with ``Rp`` the rank rounded up to 64, and inverts it by a blocked Cholesky factorisation whose products
run on the f64 matrix cores.  It takes every rank from 1, so this module also runs the small ranks, with other bits than the narrow one.
Everything around the kernel is ``factor_analyser``'s own code (whitening, the GEMMs, the accumulators, the i-vector ``StatServer``),
called with this module's Gram and posterior functions; the batch size counts the kernel's scratch inside ``max_workspace_bytes``.

The M-step runs on the device by default (``tv_m_step_device``): the ``C`` matrices ``unpack(_A[c])`` are inverted by the same kernel
(``shift = 0``, no right-hand side), ``F_c = (inv(A_c) C_c)'`` is one batched float64 product, and only the single ``R x R`` Cholesky
factor of minimum divergence is formed on the host.  ``m_step="host"`` keeps ``factor_analyser.tv_m_step``, the reference's operation
order.

Joint factor analysis keeps its cap: ``jfa_scoring``, the ``sc_jfa_*`` entry points and ``TV_MAX_RANK`` there are not touched.  Ranks
above 1024, ``total_variability_raw``, ``weighted_likelihood_plda`` and full-covariance UBMs (refused as in ``FactorAnalyser``) are not
built.  There is no CPU fallback.
"""
import ctypes
import logging

import numpy
import scipy.linalg

from . import _lib
from . import factor_analyser as _fa
from .factor_analyser import FactorAnalyser, packed_size
from .statserver import STAT_TYPE

TVW_MAX_RANK = 1024            # SC_TVW_MAX_RANK (include/sidekit_amd/ivector_wide.h)
M_STEP_SCRATCH_BYTES = 1 << 30  # tv_m_step_device inverts the components in chunks whose kernel scratch stays within this


def _check_rank(tv_rank):
    if not 1 <= tv_rank <= TVW_MAX_RANK:
        raise ValueError("tv_rank = {} is outside [1, {}] (SC_TVW_MAX_RANK = {})".format(tv_rank, TVW_MAX_RANK, TVW_MAX_RANK))


def workspace_bytes(n_sessions, rank):
    """``sc_tvw_workspace``: the scratch ``sc_tvw_posterior`` needs for ``n_sessions`` matrices of ``rank``"""
    need = ctypes.c_int64(0)
    _lib.check(_lib.lib().sc_tvw_workspace(int(n_sessions), int(rank), ctypes.byref(need)))
    return need.value


def _session_bytes(C, D, R):
    """One session of a device batch: ``factor_analyser._batch_rows``' ``P + C D + C + 2 R`` doubles and the kernel's scratch"""
    Rp = (R + 63) // 64 * 64
    return 8 * (packed_size(R) + C * D + C + 2 * R + 2 * Rp * Rp)


def _batch_rows(N, C, D, R, max_workspace_bytes):
    return max(1, min(N, int(max_workspace_bytes) // _session_bytes(C, D, R)))


def tv_gram_wide_device(F, C):
    """``G[c] = F_c' F_c`` packed, (C, P) (``sc_tvw_gram``: the kernel of ``sc_tv_gram``): F ((C D), R) float64 CUDA tensor"""
    torch = _fa._torch()
    F = _fa._f64(torch, F, F.device)
    R = F.shape[1]
    _check_rank(R)
    assert F.shape[0] % C == 0
    G = torch.empty((C, packed_size(R)), dtype=torch.float64, device=F.device)
    _lib.launch("sc_tvw_gram", F.device, F, C, F.shape[0] // C, R, G)
    return G


def _posterior_launch(torch, Lp, B, shift, e_h, e_hh, diag):
    """One ``sc_tvw_posterior`` over the rows of ``Lp`` (N, P) with scratch of its own"""
    N, R = Lp.shape[0], (B.shape[1] if B is not None else int(round((numpy.sqrt(8 * Lp.shape[1] + 1) - 1) / 2)))
    assert packed_size(R) == Lp.shape[1]
    need = workspace_bytes(N, R)
    work = torch.empty(need // 8, dtype=torch.float64, device=Lp.device)
    _lib.launch("sc_tvw_posterior", Lp.device, Lp, B, N, R, float(shift), e_h, e_hh, diag, work, need)


def tv_posterior_wide_device(stat0, stat1_w, F, G=None, want="packed"):
    """``factor_analyser.tv_posterior_device`` for ranks up to ``TVW_MAX_RANK``: ``stat0`` (N, C), ``stat1_w`` (N, C D) WHITENED, ``F``
    ((C D), R) float64 CUDA tensors, ``G`` the packed Gram matrices of ``F`` (formed when None).  Returns ``(e_h (N, R), E_hh)``:
    ``want="packed"``: the (N, P) packed upper triangles of ``inv_lambda + e_h e_h'``; ``"diag"``: their (N, R) diagonals only.  Two
    ``sc_dgemm_nn`` and one ``sc_tvw_posterior``, whose scratch (``2 Rp^2`` doubles per session) is allocated here and released on return;
    the packed sums are overwritten by the packed output."""
    assert want in ("packed", "diag")
    torch = _fa._torch()
    R = F.shape[1]
    _check_rank(R)
    if G is None:
        G = tv_gram_wide_device(F, stat0.shape[1])
    Lp = _fa.dgemm_nn_device(stat0, G)
    B = _fa.dgemm_nn_device(stat1_w, F)
    e_h = torch.empty_like(B)
    diag = torch.empty_like(B) if want == "diag" else None
    _posterior_launch(torch, Lp, B, 1.0, e_h, Lp if want == "packed" else None, diag)
    return e_h, (Lp if want == "packed" else diag)


def tv_inverse_wide_device(Ap):
    """The inverses of the symmetric positive definite matrices ``unpack(Ap[c])``, packed like them: ``Ap`` (C, P) float64 CUDA tensor,
    not modified.  ``sc_tvw_posterior`` with ``shift = 0`` and no right-hand side, in chunks of ``M_STEP_SCRATCH_BYTES`` of scratch."""
    torch = _fa._torch()
    Ap = _fa._f64(torch, Ap, Ap.device)
    R = int(round((numpy.sqrt(8 * Ap.shape[1] + 1) - 1) / 2))
    _check_rank(R)
    out = torch.empty_like(Ap)
    rows = max(1, M_STEP_SCRATCH_BYTES // workspace_bytes(1, R))
    for a in range(0, Ap.shape[0], rows):
        _posterior_launch(torch, Ap[a:a + rows], None, 0.0, None, out[a:a + rows], None)
    return out


def _unpack(torch, p, R):
    """packed (C, P) -> symmetric (C, R, R), on the tensor's device"""
    iu = torch.triu_indices(R, R, device=p.device)
    full = torch.empty((p.shape[0], R, R), dtype=p.dtype, device=p.device)
    full[:, iu[0], iu[1]] = p
    full[:, iu[1], iu[0]] = p
    return full


def m_step_from_inverses(inv_A, _C, _R, nb_sessions, min_div=True):
    """The M-step given the packed inverses ``inv_A`` (C, P) of ``unpack(_A[c])``: ``F_c = (inv(A_c) C_c)'`` as one batched float64
    product, then ``F . cholesky(unpack(_R / nb_sessions))`` when ``min_div`` (that one factor on the host).  float64 torch tensors on
    any one device, ``_R`` a tensor or an array of P values; returns ``F`` ((C D), R) on that device.  Raises
    ``numpy.linalg.LinAlgError`` naming the components whose ``F_c`` is not finite (``A_c`` singular: a component nobody occupies,
    where the reference's ``scipy.linalg.solve`` raises)."""
    import torch
    C, R = inv_A.shape[0], _C.shape[0]
    D = _C.shape[1] // C
    F = torch.bmm(_unpack(torch, inv_A, R), _C.view(R, C, D).permute(1, 0, 2)).transpose(1, 2).reshape(C * D, R)
    bad = (~torch.isfinite(F)).view(C, -1).any(dim=1).nonzero().flatten().tolist()
    if bad:
        raise numpy.linalg.LinAlgError("total variability M-step: the matrix A_c of component(s) {} is singular or not positive definite "
                                       "(no session occupies them?)".format(bad))
    if min_div:
        r = _R.cpu().numpy() if torch.is_tensor(_R) else numpy.asarray(_R)
        ch = scipy.linalg.cholesky(_fa._unpack(r.reshape(-1) / nb_sessions, R))
        F = F.matmul(torch.as_tensor(ch).to(F.device))
    return F


def tv_m_step_device(_A, _C, _R, nb_sessions, min_div=True):
    """The M-step (factor_analyser.py:516-530 of the reference) with the accumulators on the card: ``_A`` (C, P), ``_C`` (R, C D) float64
    CUDA tensors, ``_R`` (P,) or (1, P), tensor or array.  The ``C`` matrices are inverted in ``sc_tvw_posterior`` calls
    (``tv_inverse_wide_device``), the rest is ``m_step_from_inverses``.  Returns ``F`` ((C D), R), a float64 CUDA tensor."""
    torch = _fa._torch()
    _C = _fa._f64(torch, _C, _A.device)
    return m_step_from_inverses(tv_inverse_wide_device(_A), _C, _R, nb_sessions, min_div)


def total_variability_wide_device(stat0, stat1, ubm, tv_rank, nb_iter=20, min_div=True, tv_init=None, max_workspace_bytes=1 << 30,
                                  after_iteration=None, m_step="device"):
    """``factor_analyser.total_variability_device`` for ranks up to ``TVW_MAX_RANK``: the same arguments, start and E-step code, with
    ``sc_tvw_posterior`` between the GEMMs.  Sessions go through the E-step in batches cut from ``max_workspace_bytes``
    (``P + C D + C + 2 R + 2 Rp^2`` doubles per session, one session at least).  ``m_step="device"``: the accumulators stay on the card
    (``tv_m_step_device``); ``"host"``: ``factor_analyser.tv_m_step``.  ``after_iteration(it, F)`` gets a numpy array.  Returns ``F``
    ((C D), R), a float64 numpy array."""
    assert m_step in ("device", "host")
    C, D = _fa._check_ubm(ubm)
    _check_rank(tv_rank)
    assert isinstance(nb_iter, int) and 0 < nb_iter, "nb_iter must be a positive integer"
    torch = _fa._torch()
    stat0, stat1 = _fa._statistics(torch, stat0, stat1, C, D)
    N, dev = stat0.shape[0], stat0.device
    F = numpy.random.randn(C * D, tv_rank) if tv_init is None else numpy.array(tv_init, dtype=STAT_TYPE)
    assert F.shape == (C * D, tv_rank), "tv_init: (C D, tv_rank)"
    whitener = _fa._whitener(torch, ubm, dev)
    rows = _batch_rows(N, C, D, tv_rank, max_workspace_bytes)
    F_d = _fa._f64(torch, F, dev)
    for it in range(nb_iter):
        logging.info('Total variability, it %d / %d', it + 1, nb_iter)
        acc = _fa._tv_e_step(torch, stat0, stat1, whitener, F_d, rows, tv_posterior_wide_device, tv_gram_wide_device, to_host=m_step == "host")
        if m_step == "host":
            F = _fa.tv_m_step(acc[0], acc[1], acc[2], N, min_div)
            F_d = _fa._f64(torch, F, dev)
        else:
            F_d = tv_m_step_device(acc[0], acc[1], acc[2], N, min_div)
            if after_iteration is not None or it == nb_iter - 1:
                F = F_d.cpu().numpy()
        if after_iteration is not None:
            after_iteration(it, F)
    return F


def _extract(stat0, stat1, whitener, F, uncertainty, max_workspace_bytes):
    return _fa._extract(stat0, stat1, whitener, F, uncertainty, max_workspace_bytes, tv_posterior_wide_device, tv_gram_wide_device, _batch_rows)


def extract_ivectors_wide_device(stat0, stat1, ubm, F, uncertainty=False, max_workspace_bytes=1 << 30):
    """``factor_analyser.extract_ivectors_device`` for ranks up to ``TVW_MAX_RANK``: ``iv`` (N, R), or ``(iv, iv_sigma)`` with the
    diagonal of ``E_hh`` when ``uncertainty``; float64 CUDA tensors.  Batches as in ``total_variability_wide_device``; a session's bits
    do not depend on the batch it falls into."""
    C, D = _fa._check_ubm(ubm)
    _check_rank(F.shape[1])
    assert F.shape[0] == C * D, "F: (C D, R)"
    torch = _fa._torch()
    stat0, stat1 = _fa._statistics(torch, stat0, stat1, C, D)
    return _extract(stat0, stat1, _fa._whitener(torch, ubm, stat0.device), F, uncertainty, max_workspace_bytes)


class WideFactorAnalyser(FactorAnalyser):
    """``FactorAnalyser`` whose ``total_variability``, ``total_variability_single``, ``extract_ivectors`` and
    ``extract_ivectors_single`` take ranks up to ``TVW_MAX_RANK``: the inherited methods (the reference's parameter lists, the same
    i-vector ``StatServer``) with this module's rank check, training and extraction.  ``plda``, ``read`` and ``write`` are inherited as
    they are."""
    _check_rank = staticmethod(_check_rank)
    _train_device = staticmethod(total_variability_wide_device)
    _extract_whitened = staticmethod(_extract)
    _extract_device = staticmethod(extract_ivectors_wide_device)
