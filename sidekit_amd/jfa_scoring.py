"""Joint factor analysis -- mirror of ``sidekit/jfa_scoring.py`` (``jfa_scoring`` :56-132) and the device side of the JFA training of
``sidekit/statserver.py`` (``factor_analysis`` :1798-1949 with ``estimate_between_class`` :1494, ``estimate_within_class`` :1569,
``estimate_map`` :1630 and ``estimate_hidden`` :1687), the model ``M = m + V y + U x + D z`` on Baum-Welch statistics.

The E-step of the two sub-space estimations is the total-variability posterior of ``sidekit_amd.factor_analyser`` (``tv_gram_device``,
``tv_posterior_device``, ``gemm_tn_device``).  What JFA adds are passes over the ``N x (C D)`` first-order statistics, which the reference
makes on whole copies of its ``StatServer`` (``duplicate_y.dot(F.T)``, ``copy.deepcopy(self)``, ``subtract_weighted_stat1``,
``whiten_stat1``, the per-model Python loop of ``estimate_map``).  Here they are two kernels (``include/sidekit_amd/jfa.h``):
``sc_jfa_shift`` subtracts the low-rank shift ``stat0 (mean + H[row] W')`` and whitens in one pass over a batch, the product on the f64
matrix cores; ``sc_jfa_map_acc`` forms the accumulators of a MAP E-step in one pass over the per-model statistics.  Sessions go
through the device in row batches cut from ``max_workspace_bytes``; per-model sums are ``sc_class_sums`` (fixed order, no atomic
scatter); the M-steps and the minimum-divergence step stay on the host (``tv_m_step``).  The ``*_device`` functions work on
statistics that are already on the GPU (the output of ``mixture.gmm_stats_device`` as it is) and never copy them to the host; the
``StatServer`` methods of the same names upload, call them and download.

The reference is reproduced as it is ("Joint factor analysis"), with one difference: the caller's ``StatServer``
objects are left unmodified.  Not built: the ``ubm=None`` route (PLDA with a full residual: ``FactorAnalyser.plda``), a 2-D ``sigma``,
``re_estimate_residual``, ``save_partial``, full-covariance UBMs and ranks above ``TV_MAX_RANK``.  There is no CPU fallback; importing
the module needs neither a GPU nor torch.
"""
import copy
import logging

import numpy

from . import _lib
from .bosaris import Ndx, Scores
from .factor_analyser import (TV_MAX_RANK, ClassIndex, _batch_rows, _check_ubm, _f64, _statistics, class_sums_device, dgemm_nn_device,
                              gemm_tn_device, tv_gram_device, tv_m_step, tv_posterior_device)
from .mixture import Mixture
from .statserver import STAT_TYPE, StatServer

SCORING_BYTES = 1 << 30   # bound of the workspace of jfa_score_device and of the StatServer methods: sessions per device batch are cut from it


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("sidekit_amd.jfa_scoring computes on the GPU only (no CPU fallback) and no GPU is visible")
    return torch


def _check_ranks(*ranks):
    """each rank within [0, TV_MAX_RANK]: the posterior keeps one packed triangle of the rank in LDS"""
    for r in ranks:
        if not 0 <= r <= TV_MAX_RANK:
            raise ValueError("rank {} is outside [0, {}]: sc_tv_posterior keeps one packed triangle of the rank in LDS "
                             "(SC_TV_MAX_RANK = {})".format(r, TV_MAX_RANK, TV_MAX_RANK))


def _no_ubm():
    return NotImplementedError("factor_analysis without a UBM (the deprecated PLDA route with a full residual covariance) is not built: "
                               "FactorAnalyser.plda trains that model")


def _check_sigma(sigma):
    if (sigma.ndim if hasattr(sigma, "ndim") else numpy.ndim(sigma)) != 1:
        raise NotImplementedError("a full residual covariance (sigma.ndim == 2, the PLDA route of factor_analysis) is not built: "
                                  "sidekit_amd.jfa_scoring takes the diagonal of a UBM's super-vector")


def _vector(torch, v, dev, size):
    """a (C D) vector, host or device, (C, D) or flat -> flat float64 device tensor; None stays None"""
    if v is None:
        return None
    v = _f64(torch, v, dev).reshape(-1)
    assert v.shape[0] == size, "expected a vector of C D = {} values".format(size)
    return v


def _loading(torch, W, dev, size):
    """a (C D, R) loading matrix -> float64 device tensor, or None when it is None or has no column"""
    if W is None or W.shape[1] == 0:
        return None
    assert W.shape[0] == size, "expected a (C D, R) matrix with C D = {}".format(size)
    return _f64(torch, W, dev)


# ---- sc_jfa_shift ---------------------------------------------------------------------------------------------------------------------

def jfa_shift_device(stat0, stat1, W=None, H=None, rows=None, mean=None, scale=None, out=None):
    """``out[i, k] = (stat1[i, k] - stat0[i, k // D] * (mean[k] + H[rows[i]] . W[k])) * scale[k]`` (``sc_jfa_shift``): the shift by the
    hidden variables, the centring and the whitening of a batch in one pass.  ``stat0`` (N, C), ``stat1`` (N, C D) contiguous float64
    CUDA tensors; ``W`` ((C D), R) and ``H`` (Nh, R) come together (both None, or R = 0: no shift); ``rows`` (N,) int32 row of ``H`` per
    session (None: session ``i`` takes row ``i``; a row outside ``[0, Nh)`` is a zero factor); ``mean`` and ``scale`` (C D) optional.
    ``out=None`` allocates; ``out`` may be ``stat1`` itself.  Returns ``out``."""
    torch = _torch()
    assert torch.is_tensor(stat0) and torch.is_tensor(stat1) and stat0.is_cuda and stat1.is_cuda, "expected statistics on the device (CUDA tensors)"
    assert stat0.dtype == stat1.dtype == torch.float64 and stat0.is_contiguous() and stat1.is_contiguous(), "contiguous float64 statistics"
    assert stat0.dim() == stat1.dim() == 2 and stat0.shape[0] == stat1.shape[0] > 0 and stat1.shape[1] % stat0.shape[1] == 0, \
        "stat0: (sessions, C), stat1: (sessions, C D)"
    dev = stat0.device
    (N, C), CD = stat0.shape, stat1.shape[1]
    assert (W is None) == (H is None), "W and H come together"
    R = 0 if W is None else W.shape[1]
    _check_ranks(R)
    Nh = 0
    if R == 0:
        W = H = rows = None
    else:
        W, H = _f64(torch, W, dev), _f64(torch, H, dev)
        assert W.shape == (CD, R) and H.dim() == 2 and H.shape[1] == R and H.shape[0] > 0, "W: (C D, R), H: (Nh, R)"
        Nh = H.shape[0]
        if rows is not None:
            rows = (rows if torch.is_tensor(rows) else torch.as_tensor(numpy.asarray(rows))).to(device=dev, dtype=torch.int32).contiguous()
            assert rows.shape == (N,), "rows: one row of H per session"
    mean, scale = _vector(torch, mean, dev, CD), _vector(torch, scale, dev, CD)
    if out is None:
        out = torch.empty_like(stat1)
    assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.shape == stat1.shape, "out: like stat1"
    _lib.launch("sc_jfa_shift", dev, stat1, stat0, N, C, CD // C, W, H, Nh, R, rows, mean, scale, out)
    return out


def jfa_map_acc_device(stat0, stat1, D, sigma):
    """The accumulators ``(_A, _C)`` of one MAP E-step (``sc_jfa_map_acc``, ``estimate_map`` :1670-1677) from per-model statistics that
    are centred and shifted but not whitened: ``stat0`` (M, C), ``stat1`` (M, C D), ``D`` and ``sigma`` (C D); float64 CUDA tensors."""
    torch = _torch()
    dev = stat0.device
    (M, C), CD = stat0.shape, stat1.shape[1]
    stat0, stat1 = _f64(torch, stat0, dev), _f64(torch, stat1, dev)
    D, sigma = _vector(torch, D, dev, CD), _vector(torch, sigma, dev, CD)
    A, Cacc = torch.empty(CD, dtype=torch.float64, device=dev), torch.empty(CD, dtype=torch.float64, device=dev)
    _lib.launch("sc_jfa_map_acc", dev, stat0, stat1, M, C, CD // C, D, sigma, A, Cacc)
    return A, Cacc


# ---- the hidden variables -------------------------------------------------------------------------------------------------------------

def estimate_hidden_device(stat0, stat1, mean, sigma, V=None, U=None, D=None, max_workspace_bytes=1 << 30):
    """Point estimates of the hidden variables of every session (``estimate_hidden`` :1687-1796) from statistics on the device that are
    not whitened and not modified: ``stat0`` (N, C), ``stat1`` (N, C D) or (N, C, D).  ``(y, x)`` are estimated jointly under
    ``W = [V U]`` from the statistics centred on ``mean`` and whitened by ``sigma`` (1-D); with ``D``, ``z = f D / (1 + n D^2)`` on the
    whitened statistics less ``n (W [y x])`` (``W`` not whitened, as in the reference).  Returns ``(y (N, rank V), x (N, rank U),
    z (N, C D) or None without D)`` as float64 CUDA tensors.  Sessions go in batches cut from ``max_workspace_bytes``; every quantity is
    per session, so the cut does not change a bit."""
    _check_sigma(sigma)
    rv, ru = (0 if m is None else m.shape[1] for m in (V, U))
    _check_ranks(rv, ru, rv + ru)
    torch = _torch()
    assert torch.is_tensor(stat0) and stat0.dim() == 2, "stat0: (sessions, C) on the device"
    C = stat0.shape[1]
    stat0, stat1 = _statistics(torch, stat0, stat1, C, stat1[0].numel() // C)
    dev, N, CD = stat0.device, stat0.shape[0], stat1.shape[1]
    Dd = CD // C
    mean_d = _vector(torch, mean, dev, CD)
    scale = 1.0 / torch.sqrt(_vector(torch, sigma, dev, CD))
    parts = [m for m in (_loading(torch, V, dev, CD), _loading(torch, U, dev, CD)) if m is not None]
    R = rv + ru
    W = W_white = G = None
    if R > 0:
        W = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
        W_white = (W * scale[:, None]).contiguous()
        G = tv_gram_device(W_white, C)
    e_h = torch.empty((N, R), dtype=torch.float64, device=dev)
    z = None
    if D is not None:
        Dm = _vector(torch, D, dev, CD).view(1, C, Dd)
        z = torch.empty((N, CD), dtype=torch.float64, device=dev)
    rows = _batch_rows(N, C, Dd, max(R, 1), max_workspace_bytes)
    for a in range(0, N, rows):
        s0 = stat0[a:a + rows]
        sw = jfa_shift_device(s0, stat1[a:a + rows], mean=mean_d, scale=scale)
        if R > 0:
            e_h[a:a + rows] = tv_posterior_device(s0, sw, W_white, G, want="diag")[0]
        if D is not None:
            if R > 0:
                jfa_shift_device(s0, sw, W, e_h[a:a + rows], out=sw)
            z[a:a + rows] = (sw.view(-1, C, Dd) * Dm / (1.0 + s0[:, :, None] * Dm ** 2)).view(-1, CD)
    return e_h[:, :rv], e_h[:, rv:], z


# ---- training -------------------------------------------------------------------------------------------------------------------------

def _e_step(torch, stat0, stat1, phi, mean, scale, rows, W=None, H=None, hrows=None):
    """The accumulators of one E-step of a sub-space estimation (``_expectation`` :1376-1467) over all sessions of ``stat0`` / ``stat1``
    (device, not whitened), added in batch order -> host ``(_A (C, P) packed, _C (R, C D) not whitened, _R (P,) packed, not divided)``.
    A batch is shifted by ``stat0 (H[hrows] W')`` (when given), centred on ``mean`` and whitened by ``scale`` in one ``sc_jfa_shift``."""
    dev, (N, C) = stat0.device, stat0.shape
    phi_w = (_f64(torch, phi, dev) * scale[:, None]).contiguous()
    G = tv_gram_device(phi_w, C)
    ones = torch.ones((min(rows, N), 1), dtype=torch.float64, device=dev)
    acc = None
    for a in range(0, N, rows):
        s0 = stat0[a:a + rows]
        if W is None:
            sw = jfa_shift_device(s0, stat1[a:a + rows], mean=mean, scale=scale)
        elif hrows is None:
            sw = jfa_shift_device(s0, stat1[a:a + rows], W, H[a:a + rows], None, mean, scale)
        else:
            sw = jfa_shift_device(s0, stat1[a:a + rows], W, H, hrows[a:a + rows], mean, scale)
        e_h, e_hh = tv_posterior_device(s0, sw, phi_w, G)
        part = (gemm_tn_device(s0, e_hh), gemm_tn_device(e_h, sw), gemm_tn_device(ones[:s0.shape[0]], e_hh))
        acc = part if acc is None else tuple(t.add_(p) for t, p in zip(acc, part))
    return acc[0].cpu().numpy(), (acc[1] / scale[None, :]).cpu().numpy(), acc[2].cpu().numpy()[0]


def _estimate_subspace(torch, stat0, stat1, phi, mean, scale, nb_iter, min_div, max_workspace_bytes, W=None, H=None, hrows=None):
    """``nb_iter`` EM iterations of a loading matrix (the loops of ``estimate_between_class`` and ``estimate_within_class``)"""
    N, C = stat0.shape
    phi = numpy.array(phi, dtype=STAT_TYPE)
    _check_ranks(phi.shape[1])
    rows = _batch_rows(N, C, stat1.shape[1] // C, phi.shape[1], max_workspace_bytes)
    for it in range(nb_iter):
        logging.info('Estimate a factor loading matrix, it %d / %d', it + 1, nb_iter)
        _A, _C, _R = _e_step(torch, stat0, stat1, phi, mean, scale, rows, W, H, hrows)
        phi = tv_m_step(_A, _C, _R, N, min_div)
    return phi


def _estimate_map(torch, stat0, stat1, D, sigma, nb_iter):
    """``nb_iter`` EM iterations of the diagonal MAP term on per-model statistics, centred and shifted (``estimate_map`` :1666-1680)"""
    D = _vector(torch, D, stat0.device, stat1.shape[1])
    for it in range(nb_iter):
        logging.info('Estimate MAP covariance, it %d / %d', it + 1, nb_iter)
        A, Cacc = jfa_map_acc_device(stat0, stat1, D, sigma)
        D = Cacc / A
    return D


def _map_statistics(torch, stat0, stat1, index, mean, scale, F, y, hrows, G, max_workspace_bytes):
    """What ``factor_analysis`` hands to ``estimate_map`` (:1918-1947, :1645-1656): ``x`` of every session under ``G`` from the
    statistics less ``n (F y)`` of the session's model, then the per-model sums of ``stat1 - n (mean + F y + G x)``.  Batches of
    sessions; a batch's class sums (``sc_class_sums``) are added to the models' rows in batch order."""
    dev, (N, C), CD = stat0.device, stat0.shape, stat1.shape[1]
    n_models = index.ids.shape[0]
    sums = torch.zeros((n_models, CD), dtype=torch.float64, device=dev)
    G_white = gram = None
    if G is not None:
        G_white = (G * scale[:, None]).contiguous()
        gram = tv_gram_device(G_white, C)
    rows = _batch_rows(N, C, CD // C, max(1, 0 if G is None else G.shape[1]), max_workspace_bytes)
    for a in range(0, N, rows):
        s0, s1 = stat0[a:a + rows], stat1[a:a + rows]
        hr = None if hrows is None else hrows[a:a + rows]
        shifted = jfa_shift_device(s0, s1, F, y, hr, mean, None)
        if G is not None:
            x = tv_posterior_device(s0, jfa_shift_device(s0, s1, F, y, hr, mean, scale), G_white, gram, want="diag")[0]
            jfa_shift_device(s0, shifted, G, x, out=shifted)
        batch = ClassIndex(index.inverse[a:a + rows])
        ids = torch.as_tensor(batch.ids).to(dev)
        sums[ids] = sums[ids] + class_sums_device(shifted, batch)[0]
    return sums


def factor_analysis_device(stat0, stat1, model_index, ubm, rank_f, rank_g=0, rank_h=None, it_nb=(10, 10, 10), min_div=True,
                           init_matrices=(None, None, None), max_workspace_bytes=1 << 30):
    """Train the JFA model on Baum-Welch statistics that are on the GPU (``factor_analysis`` :1798-1949): ``stat0`` (N, C), ``stat1``
    (N, C, D) or (N, C D), not whitened and not modified; ``model_index``: one model label per session (array, tensor or ``ClassIndex``).
    Eigenvoices ``F`` of rank ``rank_f`` from the per-model sums, eigenchannels ``G`` of rank ``rank_g`` from the sessions less their
    model's ``F y``, the diagonal ``H`` (``rank_h`` not None: full rank ``C D``) from the per-model sums less ``F y`` and ``G x``.  As the
    reference: ``it_nb[1]`` within-class iterations, skipped when ``it_nb[2] == 0``; missing ``init_matrices`` drawn with
    ``numpy.random.randn`` in the order ``F``, ``G``, ``H * Sigma_obs.mean()``; with ``rank_g == 0`` and no ``H`` every session is its
    own class.  Returns ``(mean, F, G, H, sigma)`` as float64 numpy arrays, ``sigma = 1 / invcov``; the statistics never go to the host."""
    if ubm is None:
        raise _no_ubm()
    C, D = _check_ubm(ubm)
    _check_ranks(rank_f, rank_g)
    vect_size = C * D
    mean = ubm.get_mean_super_vector().astype(STAT_TYPE)
    sigma_obs = 1. / ubm.get_invcov_super_vector()
    F_init, G_init, H_init = init_matrices
    if F_init is None:
        F_init = numpy.random.randn(vect_size, rank_f).astype(dtype=STAT_TYPE)
    if G_init is None:
        G_init = numpy.random.randn(vect_size, rank_g)
    rank_h = vect_size if rank_h is not None else 0
    if H_init is None:
        H_init = numpy.random.randn(rank_h).astype(dtype=STAT_TYPE) * sigma_obs.mean()
    F_init, G_init, H_init = (numpy.array(m, dtype=STAT_TYPE) for m in (F_init, G_init, H_init))
    assert F_init.shape == (vect_size, rank_f) and G_init.shape == (vect_size, rank_g) and H_init.shape == (rank_h,), \
        "init_matrices: (C D, rank_f), (C D, rank_g), (rank_h,)"
    torch = _torch()
    if torch.is_tensor(model_index):
        model_index = model_index.cpu().numpy()
    stat0, stat1 = _statistics(torch, stat0, stat1, C, D)
    N, dev = stat0.shape[0], stat0.device
    index = model_index if isinstance(model_index, ClassIndex) else ClassIndex(model_index)
    assert index.rows.shape[0] == N, "one model label per session"
    mean_d = _vector(torch, mean, dev, vect_size)
    sigma_d = _vector(torch, sigma_obs, dev, vect_size)
    scale = 1.0 / torch.sqrt(sigma_d)
    hrows = torch.as_tensor(index.inverse.astype(numpy.int32)).to(dev)
    model_sums = []

    def per_model():
        if not model_sums:
            model_sums.extend(class_sums_device(t, index)[0] for t in (stat0, stat1))
        return model_sums

    # eigenvoices, from the per-model sums (each session its own class when neither G nor H follows: total variability)
    if rank_f == 0 or it_nb[0] == 0:
        F = F_init
    else:
        m0, m1 = (stat0, stat1) if rank_g == rank_h == 0 else per_model()
        F = _estimate_subspace(torch, m0, m1, F_init, mean_d, scale, it_nb[0], min_div, max_workspace_bytes)
    F_d = _loading(torch, F, dev, vect_size)
    y = None
    if (rank_g != 0 or rank_h != 0) and it_nb[2] != 0 and F_d is not None:   # y per model (not per session)
        y = estimate_hidden_device(*per_model(), mean, sigma_obs, F, None, None, max_workspace_bytes)[0]

    # eigenchannels, from the sessions less n (F y) of their model
    if rank_g == 0 or it_nb[2] == 0:
        G = G_init
    else:
        G = _estimate_subspace(torch, stat0, stat1, G_init, mean_d, scale, it_nb[1], min_div, max_workspace_bytes, F_d, y, hrows)

    # the diagonal MAP term, from the per-model sums less n (F y) and n (G x)
    if rank_h == 0 or it_nb[2] == 0:
        H = H_init
    else:
        sums = _map_statistics(torch, stat0, stat1, index, mean_d, scale, F_d, y, hrows, _loading(torch, G, dev, vect_size), max_workspace_bytes)
        H = _estimate_map(torch, per_model()[0], sums, H_init, sigma_d, it_nb[2]).cpu().numpy()
    return mean, F, G, H, sigma_obs


# ---- scoring --------------------------------------------------------------------------------------------------------------------------

def jfa_score_device(ubm, enroll_stat0, enroll_stat1, test_stat0, test_stat1, mean, sigma, V, U, D):
    """The channel-point-estimate linear scores (:104-130) of every model against every segment from statistics on the device, not
    whitened and not modified; the enrolment statistics are already summed per model.  Both sides are first centred on the UBM's means
    and divided by the square roots of its INVERSE covariances (the reference passes ``get_invcov_super_vector()`` as the covariance);
    ``(y, z)`` of a model under ``(V, U, D)`` give ``M = V y + D z``, ``x`` of a segment under ``U`` alone gives its statistics less
    ``n (U x)``, and the score is ``M . (stat1 / sum(stat0))``.  Segments go in batches cut from ``SCORING_BYTES``; a score is a sum over
    ``C D`` in a fixed order, so the cut does not change a bit.  Returns the (models, segments) float64 matrix on the device."""
    _check_sigma(sigma)
    C, Dd = _check_ubm(ubm)
    rv, ru = (0 if m is None else m.shape[1] for m in (V, U))
    _check_ranks(rv, ru, rv + ru)
    torch = _torch()
    e0, e1 = _statistics(torch, enroll_stat0, enroll_stat1, C, Dd)
    t0, t1 = _statistics(torch, test_stat0, test_stat1, C, Dd)
    dev, CD = e0.device, C * Dd
    ubm_mean = _vector(torch, ubm.get_mean_super_vector(), dev, CD)
    ubm_scale = 1.0 / torch.sqrt(_vector(torch, ubm.get_invcov_super_vector(), dev, CD))
    mean, sigma, D = (_vector(torch, v, dev, CD) for v in (mean, sigma, D))   # the model goes to the device once
    V, U = _loading(torch, V, dev, CD), _loading(torch, U, dev, CD)
    Vt = None if V is None else V.t().contiguous()
    models = torch.zeros((e0.shape[0], CD), dtype=torch.float64, device=dev)
    rows = _batch_rows(max(e0.shape[0], t0.shape[0]), C, Dd, max(rv + ru, 1), SCORING_BYTES // 2)   # the batch and its transpose
    for a in range(0, e0.shape[0], rows):
        s0 = e0[a:a + rows]
        y, _, z = estimate_hidden_device(s0, jfa_shift_device(s0, e1[a:a + rows], mean=ubm_mean, scale=ubm_scale), mean, sigma, V, U, D, SCORING_BYTES)
        if Vt is not None:
            models[a:a + rows] = dgemm_nn_device(y, Vt)
        if z is not None:
            models[a:a + rows] += z * D
    scores = torch.empty((e0.shape[0], t0.shape[0]), dtype=torch.float64, device=dev)
    for a in range(0, t0.shape[0], rows):
        s0 = t0[a:a + rows]
        sw = jfa_shift_device(s0, t1[a:a + rows], mean=ubm_mean, scale=ubm_scale)
        if U is not None:
            x = estimate_hidden_device(s0, sw, mean, sigma, None, U, None, SCORING_BYTES)[1]
            jfa_shift_device(s0, sw, U, x, out=sw)
        scores[:, a:a + rows] = dgemm_nn_device(models, (sw / s0.sum(dim=1)[:, None]).t().contiguous())
    return scores


def _check_missing_model(enroll, test, ndx):
    """:45-53 -- missing models and segments dropped from the trials, both servers aligned with what is left (the caller passes copies)"""
    clean_ndx = ndx.filter(enroll.modelset, test.segset, True)
    enroll.align_models(clean_ndx.modelset)
    test.align_segments(clean_ndx.segset)
    return clean_ndx


def _to_device(torch, server):
    dev = torch.device("cuda", torch.cuda.current_device())
    return tuple(torch.as_tensor(numpy.ascontiguousarray(a, dtype=STAT_TYPE)).to(dev) for a in (server.stat0, server.stat1))


def jfa_scoring(ubm, enroll, test, ndx, mean, sigma, V, U, D, batch_size=100, num_thread=1, check_missing=True):
    """Channel-point-estimate linear scores of the trials of ``ndx`` under the JFA model ``(mean, sigma, V, U, D)`` (:56-132) ->
    ``Scores`` with the models of ``enroll`` (its statistics summed per model id, sorted) and the segments of ``test`` that ``ndx`` names,
    the trial mask copied.  The statistics are not whitened by the caller and, unlike in the reference, not modified here.
    ``batch_size`` and ``num_thread`` are accepted and unused: the device batches are cut from ``SCORING_BYTES``."""
    assert isinstance(ubm, Mixture), '1st parameter must be a Mixture'
    assert isinstance(enroll, StatServer), '2nd parameter must be a StatServer'
    assert isinstance(test, StatServer), '3rd parameter must be a StatServer'
    assert isinstance(ndx, Ndx), '4th parameter shomustuld be a Ndx'
    _check_sigma(sigma)
    _check_ubm(ubm)
    rv, ru = (0 if m is None else m.shape[1] for m in (V, U))
    _check_ranks(rv, ru, rv + ru)
    torch = _torch()
    enroll, test = copy.deepcopy(enroll), copy.deepcopy(test)
    clean_ndx = _check_missing_model(enroll, test, ndx) if check_missing else ndx
    enroll = enroll.sum_stat_per_model()[0]
    scores = Scores()
    scores.modelset = enroll.modelset
    scores.segset = test.segset
    scores.scoremask = clean_ndx.trialmask
    scores.scoremat = jfa_score_device(ubm, *_to_device(torch, enroll), *_to_device(torch, test), mean, sigma, V, U, D).cpu().numpy()
    return scores


# ---- the StatServer methods (sidekit_amd/statserver.py delegates here) ---------------------------------------------------------------------

def _refuse(save_partial=False, re_estimate_residual=False):
    if re_estimate_residual:
        raise NotImplementedError("re_estimate_residual=True (the residual of the PLDA route) is not built: FactorAnalyser.plda re-estimates it")
    if save_partial:
        raise NotImplementedError("save_partial is not built: write the returned matrices with sidekit_io.write_fa_hdf5")


def _hidden_server(server, stat1):
    out = StatServer()
    out.modelset, out.segset = copy.deepcopy(server.modelset), copy.deepcopy(server.segset)
    out.start, out.stop = copy.deepcopy(server.start), copy.deepcopy(server.stop)
    out.stat0 = numpy.ones((server.modelset.shape[0], 1), dtype=STAT_TYPE)
    out.stat1 = stat1
    return out


def server_estimate_hidden(server, mean, sigma, V=None, U=None, D=None):
    """``StatServer.estimate_hidden`` -> ``(y, x, z)`` as ``StatServer`` objects with ones as ``stat0``; ``z`` is empty without ``D``"""
    _check_sigma(sigma)
    rv, ru = (0 if m is None else m.shape[1] for m in (V, U))
    _check_ranks(rv, ru, rv + ru)
    torch = _torch()
    y, x, z = estimate_hidden_device(*_to_device(torch, server), mean, sigma, V, U, D, SCORING_BYTES)
    z_server = StatServer()
    if z is not None:
        z_server.modelset, z_server.segset = copy.deepcopy(server.modelset), copy.deepcopy(server.segset)
        z_server.stat0 = numpy.ones((server.modelset.shape[0], 1), dtype=STAT_TYPE)
        z_server.stat1 = z.cpu().numpy()
    return _hidden_server(server, y.cpu().numpy()), _hidden_server(server, x.cpu().numpy()), z_server


def server_estimate_subspace(server, nb_iter, phi, mean, sigma_obs, min_div, per_model):
    """``estimate_between_class`` (``per_model``: the statistics summed per model first) and ``estimate_within_class`` on a server whose
    statistics are shifted already -> the loading matrix"""
    _check_sigma(sigma_obs)
    _check_ranks(phi.shape[1])
    torch = _torch()
    stat0, stat1 = _to_device(torch, server)
    if per_model:
        index = ClassIndex(server.modelset)
        stat0, stat1 = class_sums_device(stat0, index)[0], class_sums_device(stat1, index)[0]
    dev, CD = stat0.device, stat1.shape[1]
    scale = 1.0 / torch.sqrt(_vector(torch, sigma_obs, dev, CD))
    return _estimate_subspace(torch, stat0, stat1, phi, _vector(torch, mean, dev, CD), scale, nb_iter, min_div, SCORING_BYTES)


def server_estimate_map(server, nb_iter, D, mean, sigma):
    """``estimate_map`` on a server whose statistics are shifted already (not centred) -> ``D``"""
    _check_sigma(sigma)
    torch = _torch()
    stat0, stat1 = _to_device(torch, server)
    dev, CD = stat0.device, stat1.shape[1]
    centred = jfa_shift_device(stat0, stat1, mean=_vector(torch, mean, dev, CD), out=stat1)
    index = ClassIndex(server.modelset)
    return _estimate_map(torch, class_sums_device(stat0, index)[0], class_sums_device(centred, index)[0], D,
                         _vector(torch, sigma, dev, CD), nb_iter).cpu().numpy()


def server_factor_analysis(server, rank_f, rank_g, rank_h, it_nb, min_div, ubm, init_matrices):
    """``StatServer.factor_analysis`` -> ``(mean, F, G, H, sigma)``"""
    if ubm is None:
        raise _no_ubm()
    _check_ubm(ubm)
    _check_ranks(rank_f, rank_g)
    torch = _torch()
    return factor_analysis_device(*_to_device(torch, server), server.modelset, ubm, rank_f, rank_g, rank_h, it_nb, min_div, init_matrices,
                                  SCORING_BYTES)
