"""Feature post-processing -- mirror of ``sidekit/features_server.py``: ``FeaturesServer`` with the reference's constructor, ``load`` /
``stack_features`` and ``post_processing`` (:201-323): RASTA filtering, deltas and double deltas, the column mask, one of ``cms``,
``cmvn``, ``cms_sliding``, ``cmvn_sliding``, ``stg`` (``sidekit/frontend/normfeat.py``) and the selection of the speech frames.

The split is ``mixture``'s: everything with a frame dimension runs on the device through the C ABI (``include/sidekit_amd/features.h``:
``sc_feat_rasta``, ``sc_feat_delta``, ``sc_feat_moments``, ``sc_feat_norm``) on a stacked ragged batch -- float32 ``(N, D)`` rows and
``S + 1`` row offsets, float64 arithmetic, one rounding to float32 -- and torch does the plumbing only (compaction of the labelled rows,
the scatter back, the new offsets).  The ``*_device`` functions keep everything resident; ``post_process_device`` returns what
``em_split_device`` / ``accumulate_stat_device`` / ``gmm_llr_device`` take.  The numpy surface (``FeaturesServer``,
``sidekit_amd.frontend.normfeat``, ``sidekit_amd.frontend.features.compute_delta``) goes through the same kernels one utterance at a
time.  There is no CPU fallback; importing the module needs neither a GPU nor torch.

Where this differs from the reference, on purpose:
  * a stream without a single labelled frame is left as it is by every normalisation (the reference's ``cms`` returns NaN there and its
    ``stg`` raises);
  * feature warping of an even number ``n < win`` of frames: the reference duplicates the last frame, which then ties with the last real
    one, and the rank of that one frame depends on the tie order of numpy's unstable argsort (``c`` or ``c + 1`` frames below it);
    here it is always ``c``, the count of strictly smaller window values;
  * the labels are not smoothed: the reference's ``label_fusion(label)`` iterates over the scalars of a 1-D label and is the identity
    (but for a two-frame ``[True, True]``, which it turns into ``[False, False]``: mirrored by ``FeaturesServer.post_processing`` only);
  * the values are float32 device results, whatever the dtype they are returned in;
  * ``load`` always reads one source through ``get_features``; the reference does so only with a ``dataset_list`` and takes the tandem
    route (``sources``) without one, which is not built;
  * the HDF5 feature-file route, ``sources`` (tandem features), ``get_features_per_speaker`` and, for ``stack_features_device`` only,
    ``global_cmvn`` with the shows' own mean / std vectors (``stack_features`` applies them) are not built and raise
    ``NotImplementedError``;
  * ``dct_pca``, ``sdc``, ``context`` and TRAPs are built beside this class, not in it: ``FeaturesServer`` raises ``NotImplementedError``
    for them and names ``sidekit_amd.features_context.ContextFeaturesServer``, the same server with the temporal-context slot filled
    (``sc_ctx_gather``, ``sc_ctx_basis``, ``sc_ctx_project``).
"""
import logging
import re

import numpy

from . import _lib

TILE, COLS, MAX_WIN, MAX_TAPS = 256, 16, 1001, 15     # SC_FEAT_TILE, SC_FEAT_COLS, SC_FEAT_MAX_WIN, SC_FEAT_MAX_TAPS (include/sidekit_amd/features.h)
DEFAULT_DELTA_FILTER = (.25, .5, .25, 0, -.25, -.5, -.25)
MODES = {"cms": _lib.SC_FEAT_CENTER, "cmvn": _lib.SC_FEAT_CENTER_REDUCE, "cms_sliding": _lib.SC_FEAT_SLIDING_CENTER,
         "cmvn_sliding": _lib.SC_FEAT_SLIDING_CENTER_REDUCE, "stg": _lib.SC_FEAT_WARP}


def tile_lds_bytes(win):
    """LDS of one workgroup of the windowed modes of ``sc_feat_norm`` (csrc/featnorm.hip): ``TILE + win - 1`` staged rows, rounded up to
    a column stride of 2 mod 4 words, by ``COLS`` float32 columns, and the ``TILE x (COLS + 1)`` result tile."""
    stride = TILE + win - 1
    stride += 0 if stride % 4 == 2 else 2
    return (stride * COLS + TILE * (COLS + 1)) * 4


def parse_mask(mask):
    """``'[1-3,10,15-20]'`` -> ``[1, 2, 3, 10, 15, ..., 20]`` (``sidekit/sv_utils.py:377-394``)"""
    body = re.sub(r"\s", "", mask)[1:-1]
    if not set(body).issubset(set("0123456789-,")):
        raise Exception("Wrong mask format")
    indices = []
    for seg in (k.split('-') for k in body.split(',')):
        if len(seg) == 1:
            seg = seg + seg
        if len(seg) != 2:
            raise Exception("Wrong mask format")
        indices += list(range(int(seg[0]), int(seg[1]) + 1))
    return indices


# what repr(FeaturesServer) shows: the reference's layout, one field per attribute
_REPR = ("\t show: {show} \n\n\t input_feature_filename: {input_feature_filename} \n\n\t feature_filename_structure: {feature_filename_structure} \n"
         "\t  \n\t  \n\n\t Post processing options: \n\t\t mask: {mask}  \n\t\t feat_norm: {feat_norm} \n"
         "\t\t dct_pca: {dct_pca}, dct_pca_config: {dct_pca_config} \n\t\t sdc: {sdc}, sdc_config: {sdc_config} \n"
         "\t\t delta: {delta}, double_delta: {double_delta}, delta_filter: {delta_filter} \n\t\t rasta: {rasta} \n"
         "\t\t keep_all_features: {keep_all_features} \n")


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("sidekit_amd.features_server computes on the GPU only (no CPU fallback) and no GPU is visible")
    return torch


def _rows(torch, frames):
    """frames -> float32 CUDA matrix whose rows are contiguous (a column block of a wider matrix stays a view)"""
    if not torch.is_tensor(frames):
        a = numpy.array(frames, dtype=numpy.float32, order='C', ndmin=2)
        frames = torch.as_tensor(a).to(torch.device("cuda", torch.cuda.current_device()))
    assert frames.is_cuda and frames.dim() == 2 and frames.shape[1] > 0, "expected (N, D) frames, D > 0"
    if frames.dtype != torch.float32:
        frames = frames.float()
    if frames.shape[0] > 1 and (frames.stride(1) != 1 or frames.stride(0) < frames.shape[1]):
        frames = frames.contiguous()
    return frames


def _ld(x):
    return x.stride(0) if x.shape[0] > 1 else x.shape[1]


def _offsets(torch, seg_off, n_rows, dev):
    """S + 1 ascending int64 offsets from 0 to n_rows -> device tensor; ``None``: one segment, all rows.  The kernels take no row
    count, so the offsets are checked here (host offsets on the host; resident ones with one read-back of a flag), and they must cover
    every row: a row outside every segment would be written by no kernel."""
    if seg_off is None:
        seg_off = numpy.array([0, n_rows], dtype=numpy.int64)
    if torch.is_tensor(seg_off):
        off = seg_off.to(device=dev, dtype=torch.int64).contiguous()
        assert off.dim() == 1 and off.shape[0] >= 1, "seg_off: S + 1 ascending offsets"
        ok = (off[0] == 0) & (off[-1] == n_rows) & (off[1:] >= off[:-1]).all()
        assert bool(ok), "seg_off: S + 1 ascending offsets from 0 to N"
        return off
    host = numpy.asarray(seg_off, dtype=numpy.int64)
    assert host.ndim == 1 and host.shape[0] >= 1 and numpy.all(numpy.diff(host) >= 0) and host[0] == 0 and host[-1] == n_rows, \
        "seg_off: S + 1 ascending offsets from 0 to N"
    return torch.as_tensor(numpy.ascontiguousarray(host)).to(dev)


def _out(torch, x, out):
    if out is None:
        return torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.shape == x.shape and (out.shape[0] <= 1 or out.stride(1) == 1), \
        "out: a float32 matrix of the frames' shape with contiguous rows"
    return out


def rasta_device(frames, seg_off=None, out=None):
    """``rasta_filt`` of every segment (``sc_feat_rasta``): zeros for a segment's first four rows, then the FIR
    ``[.2, .1, 0, -.1, -.2]`` followed by the pole at 0.94.  Returns a new float32 matrix (``out`` must not be ``frames``)."""
    torch = _torch()
    x = _rows(torch, frames)
    off = _offsets(torch, seg_off, x.shape[0], x.device)
    y = _out(torch, x, out)
    if x.shape[0]:
        _lib.launch("sc_feat_rasta", x.device, x, _ld(x), off, off.shape[0] - 1, x.shape[1], y, _ld(y))
    return y


def delta_device(frames, seg_off=None, filt=None, out=None):
    """``compute_delta`` of every segment (``sc_feat_delta``): the 'same' convolution of each column with ``filt`` (odd length, at most
    ``MAX_TAPS``), zeros outside the segment.  ``frames`` and ``out`` may be different column blocks of one matrix."""
    torch = _torch()
    x = _rows(torch, frames)
    off = _offsets(torch, seg_off, x.shape[0], x.device)
    y = _out(torch, x, out)
    taps = numpy.array(DEFAULT_DELTA_FILTER if filt is None else filt, dtype=numpy.float64).reshape(-1)
    if x.shape[0]:
        _lib.launch("sc_feat_delta", x.device, x, _ld(x), off, off.shape[0] - 1, x.shape[1], torch.as_tensor(taps).to(x.device), taps.shape[0], y, _ld(y))
    return y


def segment_moments_device(frames, seg_off=None):
    """``(mean, std)``, float64 ``(S, D)``: the mean and the population standard deviation (``numpy.std``) of every segment's rows
    (``sc_feat_moments``); an empty segment gets mean 0 and std 1."""
    torch = _torch()
    x = _rows(torch, frames)
    off = _offsets(torch, seg_off, x.shape[0], x.device)
    S = off.shape[0] - 1
    mean = torch.empty((S, x.shape[1]), dtype=torch.float64, device=x.device)
    std = torch.empty((S, x.shape[1]), dtype=torch.float64, device=x.device)
    if x.shape[0] == 0:
        mean.zero_()
        std.fill_(1.0)
    elif S:
        _lib.launch("sc_feat_moments", x.device, x, _ld(x), off, S, x.shape[1], mean, std)
    return mean, std


def normalise_device(frames, seg_off=None, mode="cmvn", win=301, mean=None, std=None, out=None):
    """``sc_feat_norm`` on segments whose rows are the speech frames.  ``mode``: a key of ``MODES`` (or its ``SC_FEAT_*`` value);
    ``mean`` / ``std``: ``(S, D)`` float64 tables for the centring modes and the sliding modes' fallback, computed from the segments
    themselves when ``None``.  The two centring modes may work in place (``out=frames``); the windowed ones return a new matrix."""
    torch = _torch()
    x = _rows(torch, frames)
    off = _offsets(torch, seg_off, x.shape[0], x.device)
    mode = MODES[mode] if isinstance(mode, str) else int(mode)
    S, D = off.shape[0] - 1, x.shape[1]
    if mode != _lib.SC_FEAT_WARP:
        if mean is None:
            mean, std = segment_moments_device(x, off)
        mean = mean.to(device=x.device, dtype=torch.float64).contiguous()
        assert mean.shape == (S, D), "mean: (S, D)"
        if std is not None:
            std = std.to(device=x.device, dtype=torch.float64).contiguous()
            assert std.shape == (S, D), "std: (S, D)"
    else:
        mean = std = None
    y = _out(torch, x, out)
    if x.shape[0]:
        _lib.launch("sc_feat_norm", x.device, x, _ld(x), off, S, D, mode, int(win), mean, std, y, _ld(y))
    return y


def _table(torch, vec, S, D, dev):
    t = torch.as_tensor(numpy.array(vec, dtype=numpy.float64).reshape(-1)).to(dev) if not torch.is_tensor(vec) else vec.to(device=dev, dtype=torch.float64)
    assert t.shape == (D,), "a global mean / std has one entry per coefficient"
    return t.reshape(1, D).expand(S, D).contiguous()


def post_process_device(frames, seg_off, labels=None, *, rasta=False, delta=False, double_delta=False, delta_filter=None, mask=None, feat_norm=None,
                        win=301, global_mean=None, global_std=None, keep_all_features=True):
    """``FeaturesServer.post_processing`` (:201-245) of every segment of a stacked batch, resident:
    ``(frames (N, D), seg_off (S + 1), labels (N) bool or None = all speech) -> (out, labels, seg_off_out)``.

    In the reference's order: RASTA (then rows 0-1 of a segment become its row 2 and so do their labels; a segment of fewer than 3 rows
    gets zeros and keeps its labels), deltas and double deltas appended (``delta_filter``: 7 taps by default), the column ``mask`` (a
    list of indices), the normalisation ``feat_norm`` and, unless ``keep_all_features``, the selection of the labelled rows with the
    offsets recomputed.  ``cms`` / ``cmvn`` take their statistics from a segment's labelled rows (or ``global_mean`` / ``global_std``,
    one vector for the batch) and apply them to all its rows; ``cms_sliding`` / ``cmvn_sliding`` / ``stg`` (window ``win``) change the
    labelled rows only -- except the sliding modes' fallback for a segment of at most ``win`` labelled rows, which is ``cms`` / ``cmvn``
    and touches all rows.  A segment without a labelled row is left unchanged.  The labels are not smoothed."""
    torch = _torch()
    if feat_norm is not None and feat_norm not in MODES:
        raise ValueError(f"feat_norm must be one of {sorted(MODES)} or None (got {feat_norm!r})")
    x = _rows(torch, frames)
    N, dev = x.shape[0], x.device
    off = _offsets(torch, seg_off, N, dev)
    S = off.shape[0] - 1
    labels = torch.ones(N, dtype=torch.bool, device=dev) if labels is None else torch.as_tensor(labels).to(device=dev, dtype=torch.bool).clone()
    assert labels.shape == (N,), "labels: one per row"
    if rasta:
        x = rasta_device(x, off)
        first = off[:-1][(off[1:] - off[:-1]) >= 3]
        for k in (0, 1):
            x[first + k] = x[first + 2]
            labels[first + k] = labels[first + 2]
    elif x.data_ptr() == (frames.data_ptr() if torch.is_tensor(frames) else 0):
        x = x.clone()     # the caller's frames are never written
    if delta:
        D0 = x.shape[1]
        wide = torch.empty((N, D0 * (3 if double_delta else 2)), dtype=torch.float32, device=dev)
        wide[:, :D0] = x
        delta_device(wide[:, :D0], off, delta_filter, out=wide[:, D0:2 * D0])
        if double_delta:
            delta_device(wide[:, D0:2 * D0], off, delta_filter, out=wide[:, 2 * D0:])
        x = wide
    if mask is not None:
        if len(mask) == 0:
            raise Exception('filter list is empty')
        x = x[:, torch.as_tensor(list(mask), dtype=torch.int64, device=dev)].contiguous()
    D = x.shape[1]
    speech = soff = None

    def compact():
        idx = labels.nonzero().reshape(-1)
        count = torch.cat((torch.zeros(1, dtype=torch.int64, device=dev), labels.cumsum(0)))
        return idx, count[off].contiguous()

    if feat_norm in ("cms", "cmvn"):
        mode = MODES[feat_norm]
        if global_mean is not None and (feat_norm == "cms" or global_std is not None):
            mean = _table(torch, global_mean, S, D, dev)
            std = _table(torch, global_std, S, D, dev) if feat_norm == "cmvn" else None
        else:
            speech, soff = compact()
            mean, std = segment_moments_device(x[speech], soff)     # no labelled row: mean 0, std 1, which change nothing
        normalise_device(x, off, mode, win, mean, std, out=x)
    elif feat_norm is not None:
        mode = MODES[feat_norm]
        speech, soff = compact()
        xs = x[speech]
        if mode == _lib.SC_FEAT_WARP:
            ys = normalise_device(xs, soff, mode, win)
        else:
            mean, std = segment_moments_device(xs, soff)
            ys = normalise_device(xs, soff, mode, win, mean, std)
            # the fallback (at most win labelled rows) is cms / cmvn of ALL rows; elsewhere mean 0 and std 1 leave every bit as it is
            short = ((soff[1:] - soff[:-1]) <= win).reshape(S, 1)
            table_mode = _lib.SC_FEAT_CENTER_REDUCE if mode == _lib.SC_FEAT_SLIDING_CENTER_REDUCE else _lib.SC_FEAT_CENTER
            normalise_device(x, off, table_mode, win, torch.where(short, mean, torch.zeros_like(mean)), torch.where(short, std, torch.ones_like(std)), out=x)
        x[speech] = ys
    if keep_all_features:
        return x, labels, off
    if speech is None:
        speech, soff = compact()
    return x[speech], torch.ones(speech.shape[0], dtype=torch.bool, device=dev), soff


# ---- the numpy surface: one utterance at a time through the same kernels ------------------------------------------------------------------

def _host_labels(label, n):
    return numpy.ones(n, dtype=bool) if label is None else numpy.asarray(label).astype(bool).reshape(-1)


def normalise_host(features, label, feat_norm, win=301, global_mean=None, global_std=None):
    """``features`` (numpy, 2-D) normalised IN PLACE as the reference's ``cms`` / ``cmvn`` / ``stg`` / ``cep_sliding_norm`` do"""
    torch = _torch()
    out, _, _ = post_process_device(numpy.asarray(features, dtype=numpy.float32), None, torch.as_tensor(_host_labels(label, features.shape[0])),
                                    feat_norm=feat_norm, win=win, global_mean=global_mean, global_std=global_std)
    features[...] = out.cpu().numpy()


class FeaturesServer(object):
    """Management of features (``sidekit/features_server.py:53``): loads the frames of a show from ``features_extractor`` -- any object
    whose ``extract(show, channel, input_audio_filename=None)`` returns ``(feat, label)`` or ``(feat, label, global_mean, global_std)``,
    ``label=None`` meaning all speech -- and post-processes them on the GPU."""

    def __init__(self,
                 features_extractor=None,
                 feature_filename_structure=None,
                 sources=None,
                 dataset_list=None,
                 mask=None,
                 feat_norm=None,
                 global_cmvn=None,
                 dct_pca=False,
                 dct_pca_config=None,
                 sdc=False,
                 sdc_config=None,
                 delta=None,
                 double_delta=None,
                 delta_filter=None,
                 context=None,
                 traps_dct_nb=None,
                 rasta=None,
                 keep_all_features=True):
        self.features_extractor = features_extractor
        self.feature_filename_structure = '{}' if feature_filename_structure is None else feature_filename_structure
        self.sources = () if sources is None else sources
        self.dataset_list = dataset_list
        self.mask = None if mask is None else parse_mask(mask)
        self.feat_norm = feat_norm
        self.global_cmvn = global_cmvn
        self.dct_pca = False if dct_pca is None else dct_pca
        self.dct_pca_config = (12, 12, None) if dct_pca_config is None else dct_pca_config
        self.sdc = False if sdc is None else sdc
        self.sdc_config = (1, 3, 7) if sdc_config is None else sdc_config
        self.delta = False if delta is None else delta
        self.double_delta = False if double_delta is None else double_delta
        self.delta_filter = numpy.array(DEFAULT_DELTA_FILTER) if delta_filter is None else delta_filter
        self.context = (0, 0) if context is None else context
        self.traps_dct_nb = 0 if traps_dct_nb is None else traps_dct_nb
        self.rasta = False if rasta is None else rasta
        self.keep_all_features = True if keep_all_features is None else keep_all_features

        self.show = 'empty'
        self.input_feature_filename = 'empty'
        self.start_stop = (None, None)
        self.previous_load = None

    def __repr__(self):
        return _REPR.format(**vars(self))

    _BUILDS_CONTEXT = False     # features_context.ContextFeaturesServer: dct_pca, sdc, context and TRAPs

    def _unbuilt(self):
        """The options of the reference this server does not build"""
        if self.features_extractor is None:
            raise NotImplementedError("the HDF5 feature-file route (features_extractor=None; the 'none', 'htk' and 'percentile' storage "
                                      "formats) is not built: give a features_extractor whose extract() returns (feat, label)")
        if self.sources:
            raise NotImplementedError("sources (tandem features from several servers) are not built")
        for name, on in (("dct_pca", self.dct_pca), ("sdc", self.sdc), ("context", tuple(self.context) != (0, 0)),
                         ("traps_dct_nb (TRAPs)", self.traps_dct_nb)):
            if on and not self._BUILDS_CONTEXT:
                raise NotImplementedError(f"{name} is not built: sidekit_amd.features_server does RASTA, deltas, the mask and the normalisations "
                                          f"(sidekit_amd.features_context.ContextFeaturesServer builds it)")

    def _process(self, frames, seg_off, labels, **options):
        """``post_process_device``; what a subclass that fills the temporal-context slot replaces"""
        return post_process_device(frames, seg_off, labels, **options)

    def _options(self, global_mean=None, global_std=None):
        return dict(rasta=bool(self.rasta), delta=bool(self.delta), double_delta=bool(self.double_delta), delta_filter=self.delta_filter,
                    mask=self.mask, feat_norm=self._feat_norm(), global_mean=global_mean, global_std=global_std)

    def _feat_norm(self):
        if self.feat_norm is not None and self.feat_norm not in MODES:
            logging.warning('Wrong feature normalisation type')     # the reference warns and goes on without a normalisation
            return None
        return self.feat_norm

    def post_processing(self, feat, label, global_mean=None, global_std=None):
        """RASTA, deltas, the mask, the normalisation and the selection of the speech frames of one utterance (:201-245) ->
        ``(feat, label)``.  ``label`` is updated in place by RASTA as in the reference; the result is float64 once RASTA ran, of the
        input's dtype otherwise."""
        if self.dct_pca and not (self.delta or self.double_delta or self._BUILDS_CONTEXT):
            raise NotImplementedError("dct_pca is not built (sidekit_amd.features_context.ContextFeaturesServer builds it)")
        if self.sdc and not (self.delta or self.double_delta or self.dct_pca or self._BUILDS_CONTEXT):
            raise NotImplementedError("sdc is not built (sidekit_amd.features_context.ContextFeaturesServer builds it)")
        torch = _torch()
        feat = numpy.asarray(feat)
        label = numpy.ones(feat.shape[0], dtype=bool) if label is None else label
        if self.rasta and feat.shape[0] < 3:
            raise IndexError("RASTA copies frame 2 over frames 0 and 1: the utterance has fewer than 3 frames")
        if label.shape[0] == 2 and numpy.all(label):     # the reference's label_fusion reads two frames as two channels that overlap
            label[...] = False
        dtype = numpy.float64 if self.rasta or not numpy.issubdtype(feat.dtype, numpy.floating) else feat.dtype
        out, lab, _ = self._process(numpy.asarray(feat, dtype=numpy.float32), None, torch.as_tensor(numpy.array(label, dtype=bool)),
                                    keep_all_features=True, **self._options(global_mean, global_std))
        label[...] = lab.cpu().numpy()
        feat = out.cpu().numpy().astype(dtype)
        if not self.keep_all_features:
            feat, label = feat[label], label[label]
        return feat, label

    def _device(self, cep, label=None, **options):
        """One utterance (numpy) through ``post_process_device`` with ``options`` alone -> (float32 numpy result, bool numpy labels)"""
        torch = _torch()
        cep = numpy.asarray(cep)
        out, lab, _ = post_process_device(numpy.asarray(cep, dtype=numpy.float32), None, torch.as_tensor(_host_labels(label, cep.shape[0])), **options)
        return out.cpu().numpy(), lab.cpu().numpy()

    def _mask(self, cep):
        """The columns the mask lists"""
        columns = list(self.mask)
        if not columns:
            raise Exception('filter list is empty')
        return numpy.take(cep, columns, axis=1)

    def _normalize(self, label, cep, global_mean=None, global_std=None):
        """Normalise ``cep`` in place by ``feat_norm``; the sliding modes and the warp use the reference's window of 301"""
        if self._feat_norm() is not None:
            normalise_host(cep, label, self.feat_norm, 301, global_mean, global_std)

    def _delta_and_2delta(self, cep):
        """``cep`` with its deltas (and, with ``double_delta``, theirs) appended as further columns; as it is without ``delta``"""
        if not self.delta:
            return cep
        wide, _ = self._device(cep, delta=True, double_delta=bool(self.double_delta), delta_filter=self.delta_filter)
        return numpy.hstack((cep, wide[:, numpy.shape(cep)[1]:]))

    def _rasta(self, cep, label):
        """``(cep, label)`` after RASTA filtering, frames 0-1 and their labels replaced by frame 2 and its label (``label`` is updated
        in place); as they are without ``rasta``"""
        if not self.rasta:
            return cep, label
        if numpy.shape(cep)[0] < 3:
            raise IndexError("RASTA copies frame 2 over frames 0 and 1: the utterance has fewer than 3 frames")
        filtered, fused = self._device(cep, label, rasta=True)
        label[...] = fused
        return filtered.astype(numpy.float64), label

    def load(self, show, channel=0, input_feature_filename=None, label=None, start=None, stop=None):
        """``(feat, label)`` of a show, post-processed.  One result is kept: a call with the ``(show, input_feature_filename, start,
        stop)`` of the one before returns it again.  A given ``input_feature_filename`` becomes the ``feature_filename_structure``."""
        key = (show, input_feature_filename, (start, stop))
        if self.previous_load is not None and key == (self.show, self.input_feature_filename, self.start_stop):
            return self.previous_load
        self._unbuilt()
        self.show, self.input_feature_filename, self.start_stop = key
        name = None
        if input_feature_filename is not None:
            self.feature_filename_structure = input_feature_filename
            name = input_feature_filename.format(show)
        self.previous_load = self.get_features(show, channel=channel, input_feature_filename=name, label=label, start=start, stop=stop)
        return self.previous_load

    def _source(self, show, channel, input_feature_filename, label, start, stop):
        """The source rows ``start:stop`` of a show, the first / last one replicated where the range leaves the stream
        (``read_hdf5_segment``, ``sidekit/frontend/io.py:636-688``) -> ``(feat, label, global_mean, global_std)``"""
        self._unbuilt()
        if input_feature_filename is not None:
            self.feature_filename_structure = input_feature_filename
        got = self.features_extractor.extract(show, channel, input_audio_filename=input_feature_filename)
        feat, own = numpy.asarray(got[0]), got[1]
        global_mean, global_std = (got[2], got[3]) if len(got) == 4 else (None, None)
        if feat.ndim == 1:
            feat = feat[:, numpy.newaxis]
        length = feat.shape[0]
        first = 0 if start is None else start
        last = length if stop is None else stop
        before, after = max(-first, 0), max(last - length, 0)
        first, last = max(first, 0), min(last, length)
        if label is None:
            label = numpy.ones(last - first, dtype=bool) if own is None else numpy.asarray(own).astype(bool).squeeze()[first:last]
        feat = numpy.pad(feat[first:last], ((before, after), (0, 0)), mode='edge')
        label = numpy.pad(numpy.asarray(label).astype(bool), (before, after), mode='edge')
        return feat, label, global_mean, global_std

    def get_features(self, show, channel=0, input_feature_filename=None, label=None, start=None, stop=None):
        """``(feat, label)`` of one show from the features extractor, post-processed (:448-492)"""
        feat, label, global_mean, global_std = self._source(show, channel, input_feature_filename, label, start, stop)
        if self.global_cmvn and global_mean is not None:
            return self.post_processing(feat, label, global_mean, global_std)
        return self.post_processing(feat, label)

    def get_features_per_speaker(self, show, idmap, channel=0, input_feature_filename=None, label=None):
        raise NotImplementedError("get_features_per_speaker is not built (it re-runs the reference's numpy VAD per speaker)")

    def get_tandem_features(self, show, channel=0, label=None, start=None, stop=None):
        raise NotImplementedError("sources (tandem features from several servers) are not built")

    def mean_std(self, show, channel=0, start=None, stop=None):
        """What a global mean and deviation are accumulated from: the number of frames of a show, their sum and the sum of their
        squares per coefficient (the name is the reference's)"""
        frames = self.load(show, channel=channel, start=start, stop=stop)[0]
        return len(frames), frames.sum(axis=0), numpy.square(frames).sum(axis=0)

    @staticmethod
    def _lists(show_list, channel_list, feature_filename_list, label_list, start_list, stop_list):
        n = len(show_list)
        if channel_list is None:
            channel_list = numpy.zeros(n)
        empty = lambda v: numpy.empty(n, dtype='|O') if v is None else v   # noqa: E731
        return zip(show_list, channel_list, empty(feature_filename_list), empty(label_list), empty(start_list), empty(stop_list))

    def stack_features(self, show_list, channel_list=None, feature_filename_list=None, label_list=None, start_list=None, stop_list=None):
        """The frames of every show, loaded one after the other and stacked (:608-642)"""
        return numpy.vstack([self.load(*args)[0] for args in self._lists(show_list, channel_list, feature_filename_list, label_list, start_list, stop_list)])

    def stack_features_device(self, show_list, channel_list=None, feature_filename_list=None, label_list=None, start_list=None, stop_list=None):
        """``stack_features`` that stays on the card: the source rows of every show are stacked, uploaded once and post-processed as one
        ragged batch -> ``(frames, seg_off)``: a float32 CUDA matrix and the S + 1 row offsets of the shows (a host int64 array), as
        ``em_split_device`` / ``accumulate_stat_device`` / ``gmm_llr_device`` take them.  A show's rows are the bits ``load`` returns for it."""
        torch = _torch()
        feats, labels, means, stds = [], [], [], []
        for show, channel, name, label, start, stop in self._lists(show_list, channel_list, feature_filename_list, label_list, start_list, stop_list):
            filename = None if name is None else name.format(show)
            feat, label, global_mean, global_std = self._source(show, int(channel), filename, label, start, stop)
            if self.rasta and feat.shape[0] < 3:
                raise IndexError("RASTA copies frame 2 over frames 0 and 1: {} has fewer than 3 frames".format(show))
            feats.append(numpy.asarray(feat, dtype=numpy.float32))
            labels.append(label)
            means.append(global_mean)
            stds.append(global_std)
        off = numpy.concatenate(([0], numpy.cumsum([f.shape[0] for f in feats]))).astype(numpy.int64)
        if self.global_cmvn and any(m is not None for m in means):
            raise NotImplementedError("global_cmvn with per-show vectors is not built for the stacked batch: use stack_features")
        out, _, soff = self._process(numpy.vstack(feats), off, torch.as_tensor(numpy.concatenate(labels)),
                                     keep_all_features=self.keep_all_features, **self._options())
        return out, soff.cpu().numpy()
