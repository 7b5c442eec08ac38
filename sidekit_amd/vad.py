"""Speech-only extraction on the GPU: what ``extract_xvectors.py --vad`` does to a signal before the forward
(``sidekit/bin/extract_xvectors.py:98-151``): find speech timestamps, concatenate the speech chunks (``collect_chunks``).

The detector is the reference's own energy VAD -- ``vad_energy`` (``sidekit/mixture.py:67-113``) on ``power_spectrum``'s per-frame
log-energy (``sidekit/frontend/features.py:363-389``), smoothed by ``label_fusion`` (``sidekit/frontend/vad.py:409-428``) -- and
timestamps from ANY detector (the ``<out>_vad.json`` cache a reference run leaves behind, Silero's included) are applied as they are.
Kernels: ``csrc/vad.hip``.  There is no CPU fallback.

The label-to-sample rule is this project's own (the reference's labels select feature frames, its x-vector path never maps them back to
samples): frame ``t`` owns samples ``[t * shift, (t + 1) * shift)`` and the last frame owns the tail of the utterance.
"""
import ctypes

import numpy
import torch

from . import _lib

NWIN, SHIFT, PREFAC = 400, 160, 0.97          # power_spectrum(fs=16000, win_time=0.025, shift=0.01, prefac=0.97)
# FeaturesExtractor._vad (sidekit/features_extractor.py:671-673); fusion_win: label_fusion's default window
ENERGY_DEFAULTS = dict(nb_train_it=8, flooring=0.0001, ceiling=1.5, alpha=0.2, fusion_win=3)


def n_frames(n, nwin=NWIN, shift=SHIFT):
    """Frames ``framing`` cuts from n samples (0 below one window, where the reference is undefined)."""
    return (int(n) - nwin) // shift + 1 if n >= nwin else 0


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check_batch(batch):
    if not torch.is_tensor(batch) or not batch.is_cuda:
        raise RuntimeError("sidekit_amd.vad computes on the GPU only (no CPU fallback): pass a CUDA tensor")
    if batch.dim() == 1:
        batch = batch.unsqueeze(0)
    if batch.dim() != 2 or batch.dtype not in (torch.float32, torch.int16) or batch.stride(1) != 1:
        raise ValueError(f"expected a (B, L) float32 or int16 batch with contiguous rows, got {tuple(batch.shape)} {batch.dtype}")
    return batch


def _ld(batch):
    return batch.stride(0) if batch.shape[0] > 1 else batch.shape[1]


def _dtype(batch):
    return _lib.XT_I16 if batch.dtype == torch.int16 else _lib.XT_F32


def _device_lengths(lengths, B, L, dev):
    if lengths is None:
        return torch.full((B,), L, dtype=torch.int32, device=dev)
    if torch.is_tensor(lengths) and lengths.is_cuda:
        t = lengths.to(torch.int32)
    else:
        t = torch.as_tensor(numpy.ascontiguousarray(numpy.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths, dtype=numpy.int32))).to(dev)
    if t.shape != (B,):
        raise ValueError(f"lengths must have shape ({B},)")
    return t.contiguous()


def frame_log_energy(batch, lengths=None, nwin=NWIN, shift=SHIFT, prefac=PREFAC):
    """``power_spectrum``'s log-energy of every row: -> ``(le float64 (B, T), nframes int32 (B,))`` on the device; T = the frames of the
    batch's width, columns from ``nframes[b]`` on are zero."""
    batch = _check_batch(batch)
    B, L = batch.shape
    dev = batch.device
    lens = _device_lengths(lengths, B, L, dev)
    T = max(1, n_frames(_ld(batch), nwin, shift))
    le = torch.empty((B, T), dtype=torch.float64, device=dev)
    nframes = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().sk_frame_log_energy(batch.data_ptr(), _dtype(batch), _ld(batch), lens.data_ptr(), B, nwin, shift, float(prefac),
                                                  le.data_ptr(), T, nframes.data_ptr(), _stream(dev)))
    return le, nframes


def vad_energy_device(le, nframes, nb_train_it=8, flooring=0.0001, ceiling=1.5, alpha=0.2, fusion_win=3):
    """``vad_energy`` + ``label_fusion(win=fusion_win)`` per row: -> ``(label uint8 (B, T), threshold float64 (B,))`` on the device.
    A degenerate row (no frame, constant or non-finite log-energy, nothing labelled) keeps every frame and has threshold NaN."""
    if not (torch.is_tensor(le) and le.is_cuda and le.dtype == torch.float64 and le.dim() == 2 and le.is_contiguous()):
        raise ValueError("le must be a contiguous float64 (B, T) CUDA tensor")
    B, T = le.shape
    nframes = nframes.to(device=le.device, dtype=torch.int32).contiguous()
    if nframes.shape != (B,):
        raise ValueError(f"nframes must have shape ({B},)")
    label = torch.empty((B, T), dtype=torch.uint8, device=le.device)
    thr = torch.empty(B, dtype=torch.float64, device=le.device)
    with torch.cuda.device(le.device):
        _lib.check(_lib.lib().sk_vad_energy(le.data_ptr(), nframes.data_ptr(), B, T, int(nb_train_it), float(flooring), float(ceiling), float(alpha),
                                            int(fusion_win), label.data_ptr(), thr.data_ptr(), _stream(le.device)))
    return label, thr


def segments_csr(segments, B):
    """Per-row lists of ``{"start", "end"}`` dicts or ``(start, end)`` pairs -> ``(seg_off int32 (B + 1,), seg int32 (2 n,))``."""
    if len(segments) != B:
        raise ValueError(f"expected one segment list per row ({B}), got {len(segments)}")
    off, flat = [0], []
    for row in segments:
        for s in row:
            a, b = (s["start"], s["end"]) if isinstance(s, dict) else s
            flat += [int(a), int(b)]
        off.append(len(flat) // 2)
    return numpy.asarray(off, dtype=numpy.int32), numpy.asarray(flat, dtype=numpy.int32)


def collect_chunks_device(batch, lengths=None, labels=None, nframes=None, segments=None, shift=SHIFT, out=None):
    """The gather.  With ``labels`` / ``nframes`` (device, from :func:`vad_energy_device`): sample s of row b is kept iff
    ``labels[b][min(s // shift, nframes[b] - 1)]`` -> ``(out, out_len int32 (B,) ON THE DEVICE)``.  With ``segments`` (one list of
    ``{"start", "end"}`` per row, host): ``collect_chunks`` of the reference -> ``(out, out_len numpy int32 (B,))``, no read-back; the
    ranges are validated first (inside the row, ascending, no overlap: ``ValueError`` otherwise, nothing is enqueued).  ``out``: a
    (B, >= L) buffer of the batch's dtype that does not overlap it (allocated if None); columns from ``out_len[b]`` on are not written."""
    batch = _check_batch(batch)
    B, L = batch.shape
    dev = batch.device
    if (labels is None) == (segments is None):
        raise ValueError("pass either labels (+ nframes) or segments")
    if out is None:
        out = torch.empty((B, _ld(batch)), dtype=batch.dtype, device=dev)
    if out.dtype != batch.dtype or out.dim() != 2 or out.shape[0] != B or out.stride(1) != 1 or out.device != dev:
        raise ValueError("out must be a (B, >= L) tensor of the batch's dtype on its device")
    lib = _lib.lib()
    with torch.cuda.device(dev):
        if labels is not None:
            lens = _device_lengths(lengths, B, L, dev)
            out_len = torch.empty(B, dtype=torch.int32, device=dev)
            _lib.check(lib.sk_collect_labels(batch.data_ptr(), _dtype(batch), _ld(batch), lens.data_ptr(), labels.data_ptr(), labels.shape[1],
                                             nframes.data_ptr(), B, shift, out.data_ptr(), _ld(out), out_len.data_ptr(), _stream(dev)))
            return out, out_len
        h_lens = numpy.full(B, L, dtype=numpy.int32) if lengths is None else numpy.ascontiguousarray(
            numpy.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths, dtype=numpy.int32))
        if h_lens.shape != (B,):
            raise ValueError(f"lengths must have shape ({B},)")
        seg_off, seg = segments_csr(segments, B)
        d_csr = torch.as_tensor(numpy.concatenate([seg_off, seg])).to(dev)          # one upload: [seg_off | seg]
        h_out = numpy.zeros(B, dtype=numpy.int32)
        _lib.check(lib.sk_collect_segments(batch.data_ptr(), _dtype(batch), _ld(batch), h_lens.ctypes.data, seg_off.ctypes.data, seg.ctypes.data,
                                           d_csr.data_ptr(), d_csr.data_ptr() + 4 * (B + 1), B, out.data_ptr(), _ld(out), h_out.ctypes.data,
                                           _stream(dev)))
        d_csr.record_stream(torch.cuda.current_stream(dev))
        return out, h_out


def speech_only(batch, lengths=None, vad="energy", nwin=NWIN, shift=SHIFT, prefac=PREFAC, return_labels=False, **energy):
    """Drop non-speech samples from a padded batch: -> ``(compacted batch, new lengths as a list)``, ready for
    ``Xtractor.forward(batch, is_eval=True, lengths=lengths)``.  ``vad="energy"`` (keywords of :data:`ENERGY_DEFAULTS` may be overridden)
    runs log-energy, detector and gather on the current stream; the B new lengths come back through a pinned buffer and an event (the
    forward takes them from host memory), not a device-wide synchronise.  ``vad=[[{"start", "end"}, ...], ...]`` applies timestamps:
    no read-back at all.  ``return_labels``: also the ``(label, nframes, threshold)`` device tensors of the energy path."""
    batch = _check_batch(batch)
    B, L = batch.shape
    if not isinstance(vad, str):
        out, out_len = collect_chunks_device(batch, lengths, segments=vad)
        return out, [int(v) for v in out_len]
    if vad != "energy":
        raise NotImplementedError(f"vad={vad!r}: only the energy detector is built ('energy'), or pass timestamps")
    kw = dict(ENERGY_DEFAULTS)
    kw.update(energy)
    dev = batch.device
    lens = _device_lengths(lengths, B, L, dev)
    le, nframes = frame_log_energy(batch, lens, nwin, shift, prefac)
    label, thr = vad_energy_device(le, nframes, **kw)
    out, out_len = collect_chunks_device(batch, lens, labels=label, nframes=nframes, shift=shift)
    pinned = torch.empty(B, dtype=torch.int32, pin_memory=True)
    pinned.copy_(out_len, non_blocking=True)
    ready = torch.cuda.Event()
    ready.record(torch.cuda.current_stream(dev))
    ready.synchronize()
    new = [int(v) for v in pinned.numpy()]
    return (out, new, (label, nframes, thr)) if return_labels else (out, new)


# ---- labels <-> the reference's timestamp lists ------------------------------------------------------------------------------------------
def labels_to_segments(label, n, shift=SHIFT):
    """Frame labels of an utterance of n samples -> maximal runs of kept samples as ``(start, end)`` pairs, under the label-to-sample
    rule above.  No frame at all keeps the whole signal."""
    label = numpy.asarray(label).astype(bool)
    n = int(n)
    if label.shape[0] < 1:
        return [(0, n)] if n > 0 else []
    edges = numpy.flatnonzero(numpy.diff(numpy.concatenate([[False], label, [False]]).astype(numpy.int8)))
    last = label.shape[0]
    return [(int(s) * shift, n if e == last else int(e) * shift) for s, e in zip(edges[::2], edges[1::2])]


def timestamps_from_labels(label, n, shift=SHIFT):
    """The shape ``extract_xvectors.py`` caches in ``<out>_vad.json``: a list of ``{"start", "end"}`` sample ranges; an utterance with
    nothing labelled keeps everything (the driver's ``len(speech_timestamps) == 0`` fallback, :137-138)."""
    segs = labels_to_segments(label, n, shift) or [(0, int(n))]
    return [{"start": s, "end": e} for s, e in segs]
