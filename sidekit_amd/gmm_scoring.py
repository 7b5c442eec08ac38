"""GMM-UBM verification -- mirror of ``sidekit/gmm_scoring.py``: ``gmm_scoring`` and ``gmm_scoring_singleThread`` (:53-177), the
log-likelihood ratio between mean-adapted models of a diagonal ``Mixture`` and the mixture itself, averaged over a test segment's frames.

The reference loops over segments and models in Python and forms an ``N x C`` matrix of log posteriors per pair.  Here all models of a
batch of segments go through one kernel (``sc_gmm_score_models``, ``include/sidekit_amd/gmm_scoring.h``): float64 on the f64 matrix
cores, the model-independent half of the exponent computed once per group of models, and only the ``M x S`` segment sums leave it.
The ``*_device`` functions work on resident frames (float32 or float64, widened in the load) and resident models, and
``map_adapt_device`` adapts the means from resident statistics (``gmm_stats_device``), so the path from statistics to adapted models to
scores never leaves the device.  The UBM is scored as one more model by the same code, so a model equal to the UBM scores exactly 0.
Top-C (fast) scoring stands beside the reference's surface (Reynolds et al. 2000; ALIZE's ``topDistribsCount``;
``include/sidekit_amd/gmm_topc.h``): ``gmm_top_components_device`` lists per frame the ``top_c`` components that score best under the UBM
(``sc_gmm_top_components``), and ``gmm_llk_topc_device``, ``gmm_llr_topc_device`` and ``gmm_scoring_topc`` evaluate every model on those
alone (``sc_gmm_score_models_topc``): ``C / top_c`` times less work per model.
Full covariances raise ``NotImplementedError``; ``jfa_scoring`` is ``sidekit_amd.jfa_scoring``.  There is no CPU fallback;
importing the module needs neither a GPU nor torch.
"""
import logging

import numpy

from . import _lib, mixture
from .bosaris import Ndx, Scores
from .mixture import Mixture
from .statserver import StatServer

SCORING_BYTES = 1 << 30   # frames of the test segments that go to the device in one gmm_scoring batch, and the bound of its workspace
MAX_MODELS = 65535    # SC_GMM_SCORE_MAX_M (include/sidekit_amd/gmm_scoring.h): models of one sc_gmm_score_models call
MAX_TOP_C = _lib.SC_GMM_TOPC_MAX   # SC_GMM_TOPC_MAX (include/sidekit_amd/gmm_topc.h): components per frame of a list


def _device_mask(torch, mask, dev):
    """``mask`` (host array or tensor, ``None`` stays ``None``) -> booleans on ``dev``"""
    if mask is None:
        return None
    return (mask.to(dev) if torch.is_tensor(mask) else torch.as_tensor(numpy.ascontiguousarray(mask)).to(dev)).ne(0)


def gmm_llk_device(ubm, models, frames, seg_off=None, mask=None, max_workspace_bytes=1 << 30):
    """``llk[m, s] = sum_n log sum_c w_c N(x_n; models[m, c], Sigma_c)`` over the frames of segment ``s`` (``sc_gmm_score_models``).
    ``models``: (M, C D) or (M, C, D) means, host array or CUDA tensor; ``frames``: (N, D) CUDA tensor (float32 or float64) or host array;
    ``seg_off``: S + 1 ascending frame offsets (host), ``None``: one segment; ``mask``: (M, S) booleans, the trials to compute (``None``:
    all), the other entries are 0.  Returns ``(llk (M, S) float64, lengths (S,) int64)``, on the device when the frames were there.
    Models go to the kernel in consecutive chunks whose workspace stays within ``max_workspace_bytes`` (one model at least); the
    chunking does not change a bit."""
    return _llk(ubm, models, frames, seg_off, mask, max_workspace_bytes)


def _top_c(ubm, top_c, frames=None, components=None):
    """The refusals of the top-C functions that need no device -> K = min(top_c, C)"""
    if ubm.invcov.ndim == 3:
        raise mixture._full_covariance()
    if not 1 <= int(top_c) <= MAX_TOP_C:
        raise ValueError("top_c: between 1 and {:d} components per frame (got {})".format(MAX_TOP_C, top_c))
    K = min(int(top_c), ubm.mu.shape[0])
    if components is not None:
        shape, want = tuple(getattr(components, "shape", ())), (numpy.shape(frames)[0], K)
        dtype = getattr(components, "dtype", type(components).__name__)
        if shape != want or str(dtype).split(".")[-1] != "int32":
            raise ValueError("components: {} int32, one list of min(top_c, C) components per frame (got {} {})".format(want, shape, dtype))
    return K


def _lists(torch, ubm, x, dt, K, components=None):
    """(N, K) int32 lists on the frames' device: computed (``sc_gmm_top_components``), or the caller's once every entry is within [0, C)"""
    N, C = x.shape[0], ubm.mu.shape[0]
    if components is not None:
        idx = (components if torch.is_tensor(components) else torch.as_tensor(numpy.ascontiguousarray(components))).to(x.device).contiguous()
        lo, hi = (int(v) for v in torch.aminmax(idx))
        if lo < 0 or hi >= C:
            raise ValueError("components: entries within [0, {:d}) (got {:d} .. {:d})".format(C, lo, hi))
        return idx
    assert x.shape[1] == ubm.dim(), 'dimension of ubm and features differ: {:d} / {:d}'.format(ubm.dim(), x.shape[1])
    m, ic, A = mixture._model(torch, ubm, x.device)
    idx = torch.empty((N, K), dtype=torch.int32, device=x.device)
    _lib.launch("sc_gmm_top_components", x.device, x, dt, N, x.shape[1], m, ic, A, C, K, idx)
    return idx


def gmm_top_components_device(ubm, frames, top_c=10):
    """Per frame the ``K = min(top_c, C)`` components with the largest log posterior under ``ubm`` (``sc_gmm_top_components``): the larger
    value wins, at equal values the lower index; a frame's list is stored by ascending component and depends on that frame and the
    mixture alone.  ``frames``: (N, D) CUDA tensor (float32 or float64) or host array.  Returns (N, K) int32, on the device when the
    frames were there."""
    K = _top_c(ubm, top_c)
    torch = mixture._torch()
    x, dt, host = mixture._frames(torch, frames)
    idx = _lists(torch, ubm, x, dt, K)
    return idx.cpu().numpy() if host else idx


def gmm_llk_topc_device(ubm, models, frames, seg_off=None, mask=None, top_c=10, components=None, max_workspace_bytes=1 << 30):
    """``gmm_llk_device`` with the sum over the components cut to each frame's list (``sc_gmm_score_models_topc``):
    ``llk[m, s] = sum_n log sum_k w_c N(x_n; models[m, c], Sigma_c)``, ``c = components[n, k]``.  ``components``: (N, min(top_c, C)) int32,
    host array or CUDA tensor, entries within [0, C) (``ValueError`` otherwise, before any launch); ``None``: the lists of
    ``gmm_top_components_device(ubm, frames, top_c)``, computed once per call whatever the chunking.  The other arguments, the result and
    its placement as ``gmm_llk_device``; ``llk[m, s]`` depends on model ``m``, the segment's frames and their lists alone."""
    return _llk(ubm, models, frames, seg_off, mask, max_workspace_bytes, (_top_c(ubm, top_c, frames, components), components))


def _llk(ubm, models, frames, seg_off, mask, max_workspace_bytes, top=None):
    """What ``gmm_llk_device`` (``top=None``) and ``gmm_llk_topc_device`` (``top=(K, components)``) share: the operands, the chunks of
    models and the placement of the result"""
    if ubm.invcov.ndim == 3:
        raise mixture._full_covariance()
    torch = mixture._torch()
    x, dt, host = mixture._frames(torch, frames)
    N, D = x.shape
    dev = x.device
    assert ubm.invcov.ndim == 2 and ubm.mu.shape == ubm.invcov.shape, "a diagonal mixture has (C, D) means and inverse covariances"
    assert D == ubm.dim(), 'dimension of ubm and features differ: {:d} / {:d}'.format(ubm.dim(), D)
    C = ubm.mu.shape[0]
    mus = mixture._device_f64(torch, models, dev)
    assert mus.dim() in (2, 3) and mus.shape[0] > 0 and mus[0].numel() == C * D, "models: (M, C D) or (M, C, D) means of the mixture's shape"
    mus = mus.reshape(mus.shape[0], C, D)
    M = mus.shape[0]
    off = mixture._offsets(seg_off, N)
    S, lens = off.shape[0] - 1, numpy.diff(off)
    invcov = mixture._device_f64(torch, ubm.invcov, dev)
    B = mixture._device_f64(torch, -2.0 * (numpy.log(ubm.w) + numpy.log(ubm.cst)), dev)
    d_off = torch.as_tensor(off.astype(numpy.int32)).to(dev)
    d_mask = _device_mask(torch, mask, dev)
    if d_mask is not None:
        d_mask = d_mask.to(torch.uint8).contiguous()
        assert d_mask.shape == (M, S), "mask: one entry per model and segment"
    llk = torch.zeros((M, S), dtype=torch.float64, device=dev)
    longest = int(lens.max())
    slabs = mixture._slabs(longest)
    per_model = 8 * ((C if top is None else 0) + (slabs * S if slabs > 1 else 0))         # A (the dense kernel's) and the slab partials of one model
    step = int(min(MAX_MODELS, max(1, max_workspace_bytes // max(1, per_model))))
    idx = None if top is None else _lists(torch, ubm, x, dt, *top)
    for a in range(0, M, step):
        b = min(M, a + step)
        chunk_mask = None if d_mask is None else d_mask[a:b]
        if top is None:
            _lib.launch("sc_gmm_score_models", dev, x, dt, N, D, mus[a:b], b - a, invcov, B, C, d_off, S, longest, chunk_mask, llk[a:b])
        else:
            _lib.launch("sc_gmm_score_models_topc", dev, x, dt, N, D, mus[a:b], b - a, invcov, B, C, d_off, S, longest, chunk_mask, idx, top[0],
                        llk[a:b])
    d_lens = torch.as_tensor(lens).to(dev)
    return (llk.cpu().numpy(), lens) if host else (llk, d_lens)


def gmm_llr_device(ubm, models, frames, seg_off=None, mask=None, max_workspace_bytes=1 << 30):
    """``llr[m, s] = mean_n log p(x_n | model m) - mean_n log p(x_n | ubm)`` over the frames of segment ``s`` (:96-113).  The UBM's own
    means are stacked as one more model with every trial, so both terms come from the same code and a model equal to the UBM scores
    exactly 0.  Entries outside ``mask`` are 0; a trial on an empty segment is ``nan`` (the reference's mean of nothing).  Arguments and
    placement of the result as ``gmm_llk_device``."""
    return _llr(ubm, models, frames, seg_off, mask, max_workspace_bytes)


def gmm_llr_topc_device(ubm, models, frames, seg_off=None, mask=None, top_c=10, components=None, max_workspace_bytes=1 << 30):
    """``gmm_llr_device`` on the frames' lists (``gmm_llk_topc_device``): both terms of a ratio are sums over the same ``top_c``
    components per frame, chosen under the UBM -- the classical definition -- and come from the same code, so a model equal to the UBM
    scores exactly 0.  Arguments as ``gmm_llk_topc_device``, result as ``gmm_llr_device``."""
    return _llr(ubm, models, frames, seg_off, mask, max_workspace_bytes, (_top_c(ubm, top_c, frames, components), components))


def _llr(ubm, models, frames, seg_off, mask, max_workspace_bytes, top=None):
    """What ``gmm_llr_device`` and ``gmm_llr_topc_device`` share: the UBM stacked under the models, the means and their difference"""
    if ubm.invcov.ndim == 3:
        raise mixture._full_covariance()
    torch = mixture._torch()
    x, dt, host = mixture._frames(torch, frames)
    dev = x.device
    C, D = ubm.mu.shape
    mus = mixture._device_f64(torch, models, dev)
    mus = mus.reshape(mus.shape[0], C * D)
    M = mus.shape[0]
    stacked = torch.cat((mus, mixture._device_f64(torch, ubm.mu, dev).reshape(1, C * D)))
    d_mask = _device_mask(torch, mask, dev)
    if d_mask is not None:
        assert d_mask.dim() == 2 and d_mask.shape[0] == M, "mask: one entry per model and segment"
        stacked_mask = torch.cat((d_mask, torch.ones((1, d_mask.shape[1]), dtype=torch.bool, device=dev)))
    llk, lens = _llk(ubm, stacked, x, seg_off, None if mask is None else stacked_mask, max_workspace_bytes, top)
    mean = llk / lens.to(torch.float64)          # 0 / 0 = nan for an empty segment
    llr = mean[:M] - mean[M]
    if d_mask is not None:
        llr = torch.where(d_mask, llr, torch.zeros_like(llr))
    return llr.cpu().numpy() if host else llr


def map_adapt_device(stat0, stat1, ubm, r=16, multisession_index=None):
    """MAP adaptation of the UBM's means (``statserver.py:1075-1157``) from statistics that are on the device (``gmm_stats_device``):
    ``stat0`` (S, C), ``stat1`` (S, C, D) or (S, C D) float64 CUDA tensors.  ``multisession_index=None``: one model per row, the
    single-session form (float32 ``eps`` added to ``stat0`` inside ``alpha``); otherwise one label per row (or a ``ClassIndex``): the
    statistics of the rows of a label are added first (``sc_class_sums``: rows of a class in row order), one model per sorted unique
    label, the multi-session form (no ``eps``).  ``0 / 0`` is 0.  Returns the (models, C, D) float64 means on the device."""
    torch = mixture._torch()
    assert torch.is_tensor(stat0) and torch.is_tensor(stat1) and stat0.is_cuda and stat1.is_cuda, "statistics on the device"
    if ubm.invcov.ndim == 3:
        raise mixture._full_covariance()
    C, D = ubm.mu.shape
    dev = stat0.device
    s0 = stat0.to(torch.float64).reshape(-1, C)
    s1 = stat1.to(torch.float64).reshape(s0.shape[0], C * D)
    if multisession_index is None:
        eps = float(numpy.finfo(numpy.float32).eps)
        alpha = (s0 + eps) / (s0 + eps + r)
    else:
        from .factor_analyser import class_sums_device
        s0, s1 = class_sums_device(s0.contiguous(), multisession_index)[0], class_sums_device(s1.contiguous(), multisession_index)[0]
        alpha = s0 / (s0 + r)
    s1 = s1.reshape(-1, C, D)
    mean = s1 / s0[:, :, None]
    mean = torch.where(torch.isnan(mean), torch.zeros_like(mean), mean)
    alpha = alpha[:, :, None]
    return alpha * mean + (1 - alpha) * mixture._device_f64(torch, ubm.mu, dev)[None]


def _check_types(ubm, enroll, ndx):
    assert isinstance(ubm, Mixture), 'First parameter should be a Mixture'
    assert isinstance(enroll, StatServer), 'Second parameter should be a StatServer'
    assert isinstance(ndx, Ndx), 'Third parameter should be a Ndx'


def gmm_scoring_singleThread(ubm, enroll, ndx, feature_server, score_mat, seg_idx=None):
    """The trials of the test segments ``seg_idx`` of ``ndx`` (all when ``None``) into ``score_mat`` (models of ``ndx`` x segments of
    ``ndx``), :53-116.  ``enroll.stat1`` holds the mean super-vectors, ``feature_server`` is any object whose ``load(show)[0]`` is the
    (frames, D) array of a show.  Segments are loaded in batches of at most ``SCORING_BYTES`` of frames, stacked, and a batch is one
    ``gmm_llr_device`` call under the trial mask.  Scores are placed by model name (a name enrolled twice: its last row, as the
    reference's dictionary has it); a model of ``ndx`` that is not enrolled keeps what ``score_mat`` holds."""
    _score_trials(ubm, enroll, ndx, feature_server, score_mat, seg_idx, gmm_llr_device)


def _score_trials(ubm, enroll, ndx, feature_server, score_mat, seg_idx, llr_device):
    """``gmm_scoring_singleThread`` with the ratios of a batch from ``llr_device(ubm, models, frames, seg_off, mask, max_workspace_bytes)``:
    the batching and the placement that ``gmm_scoring`` and ``gmm_scoring_topc`` share"""
    _check_types(ubm, enroll, ndx)
    if ubm.invcov.ndim == 3:
        raise mixture._full_covariance()
    if seg_idx is None:
        seg_idx = range(ndx.segset.shape[0])
    seg_idx = [int(t) for t in seg_idx]
    enrolled = {name: i for i, name in enumerate(enroll.modelset)}
    rows = numpy.array([i for i, name in enumerate(ndx.modelset) if name in enrolled], dtype=numpy.int64)
    if rows.shape[0] == 0 or not seg_idx:
        return
    torch = mixture._torch()
    dev = torch.device("cuda", torch.cuda.current_device())
    models = mixture._device_f64(torch, enroll.stat1[[enrolled[name] for name in ndx.modelset[rows]], :], dev)

    def score(batch):
        cols = numpy.array([t for t, _ in batch], dtype=numpy.int64)
        off = numpy.concatenate(([0], numpy.cumsum([f.shape[0] for _, f in batch])))
        mask = ndx.trialmask[rows][:, cols]
        if off[-1] == 0:
            llr = numpy.full(mask.shape, numpy.nan)
        else:
            llr = llr_device(ubm, models, numpy.concatenate([f for _, f in batch]), off, mask, SCORING_BYTES)
        block = score_mat[numpy.ix_(rows, cols)]
        block[mask] = llr[mask]
        score_mat[numpy.ix_(rows, cols)] = block

    batch, held = [], 0
    for ts in seg_idx:
        logging.info('Compute trials involving test segment %d/%d', ts + 1, ndx.segset.shape[0])
        cep = numpy.asarray(feature_server.load(ndx.segset[ts])[0])
        batch.append((ts, cep))
        held += cep.nbytes
        if held >= SCORING_BYTES:
            score(batch)
            batch, held = [], 0
    if batch:
        score(batch)


def gmm_scoring(ubm, enroll, ndx, feature_server, num_thread=1):
    """Log-likelihood ratios of the trials of ``ndx`` between the models of ``enroll`` (``stat1``: mean super-vectors of models that
    differ from ``ubm`` in their means only) and ``ubm`` (:119-177) -> ``Scores`` with the models and segments of ``ndx`` that can be
    scored (models that are enrolled), ``scoremask`` = the trial mask and 0 where there is no trial.  ``feature_server``: any object
    whose ``load(show)[0]`` is the frames of a show; ``num_thread`` is accepted and unused."""
    return _scores(ubm, enroll, ndx, feature_server, gmm_llr_device)


def gmm_scoring_topc(ubm, enroll, ndx, feature_server, top_c=10, num_thread=1):
    """``gmm_scoring`` on the ``top_c`` components per frame that score best under ``ubm`` (``gmm_llr_topc_device``; between 1 and 32,
    at most the mixture's own): the same models, segments, mask, batches and placement, ``C / top_c`` times less work per model.
    ``num_thread`` is accepted and unused."""
    _check_types(ubm, enroll, ndx)
    _top_c(ubm, top_c)

    def llr_device(ubm, models, frames, seg_off, mask, max_workspace_bytes):
        return gmm_llr_topc_device(ubm, models, frames, seg_off, mask, top_c, None, max_workspace_bytes)

    return _scores(ubm, enroll, ndx, feature_server, llr_device)


def _scores(ubm, enroll, ndx, feature_server, llr_device):
    """``gmm_scoring`` with the ratios of a batch from ``llr_device`` (``_score_trials``)"""
    _check_types(ubm, enroll, ndx)
    if ubm.invcov.ndim == 3:
        raise mixture._full_covariance()
    clean_ndx = ndx.filter(enroll.modelset, ndx.segset, True)
    s = numpy.zeros(clean_ndx.trialmask.shape)
    _score_trials(ubm, enroll, clean_ndx, feature_server, s, None, llr_device)
    score = Scores()
    score.scoremat = s
    score.modelset = clean_ndx.modelset
    score.segset = clean_ndx.segset
    score.scoremask = clean_ndx.trialmask
    return score
