"""``sidekit.frontend.vad``: ``vad_energy`` (sidekit/frontend/vad.py:332-378, identical to sidekit/mixture.py:67-113) and ``label_fusion``
(:409-428) by their reference names -- numpy in, numpy out, computed on the GPU (``sk_vad_energy``, csrc/vad.hip).  As everywhere in this
package there is no CPU fallback.

Not built: ``vad_snr`` (adds random noise and a spectral-subtraction pass), ``vad_percentil``, and the two-channel overlap removal of
``label_fusion``.
"""
import numpy


def _device():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("sidekit_amd.frontend.vad computes on the GPU only (no CPU fallback) and no GPU is visible")
    return torch.device("cuda", torch.cuda.current_device())


def vad_energy(log_energy, distrib_nb=3, nb_train_it=8, flooring=0.0001, ceiling=1.0, alpha=2):
    """-> ``(label bool (T,), threshold)``: a 3-component GMM on the standardised log-energy, frames above ``mu_max - alpha * sigma_max``.
    Unlike the reference, which returns an all-False label and a NaN threshold there, a degenerate input (constant or non-finite
    log-energy, nothing above the threshold) keeps every frame (threshold NaN)."""
    import torch
    from ..vad import vad_energy_device
    if distrib_nb != 3:
        raise NotImplementedError(f"vad_energy: distrib_nb={distrib_nb}; only the 3-component mixture is built")
    le = numpy.ascontiguousarray(numpy.asarray(log_energy, dtype=numpy.float64).reshape(1, -1))
    if le.shape[1] == 0:
        return numpy.zeros(0, dtype=bool), numpy.nan
    dev = _device()
    nframes = torch.tensor([le.shape[1]], dtype=torch.int32, device=dev)
    label, thr = vad_energy_device(torch.from_numpy(le).to(dev), nframes, nb_train_it, flooring, ceiling, alpha, fusion_win=0)
    return label[0].cpu().numpy().astype(bool), float(thr[0].item())


def label_fusion(label, win=3):
    """Morphological closing then opening of a single channel's labels (1-D, or 2-D with one row), window ``win`` (odd).  The
    two-channel form of the reference (overlap removal between two speakers' labels) is not built."""
    import ctypes
    import torch
    from .. import _lib
    lab = numpy.asarray(label)
    rows = lab.reshape(1, -1) if lab.ndim == 1 else lab
    if rows.ndim != 2 or rows.shape[0] != 1:
        raise NotImplementedError("label_fusion: single-channel labels only (the two-channel overlap removal is not built)")
    if win < 3 or win % 2 == 0:
        raise ValueError(f"label_fusion: win must be odd and >= 3 (got {win})")
    T = rows.shape[1]
    if T == 0:
        return lab.copy()
    dev = _device()
    # The fusion has no entry point of its own: it is the tail of sk_vad_energy.  The labels go in as a two-level "log-energy" with no EM
    # iteration, where the mixture still is what it was initialised to (mu_max = 2, sigma = 1) and the threshold is 2 - alpha.
    le = torch.from_numpy(numpy.ascontiguousarray(rows.astype(bool).astype(numpy.float64))).to(dev)
    if not rows.any() or rows.all():
        return lab.astype(bool)                 # closing and opening leave a constant row as it is
    # standardised 0 / 1 labels are (x - p) / sqrt(p (1 - p)); with no EM iteration the mixture keeps mu_max = 2, sigma = 1, so
    # threshold = 2 - alpha: alpha is set to put it at the midpoint between the two standardised levels
    p = float(rows.astype(bool).mean())
    sd = (p * (1.0 - p)) ** 0.5
    mid = 0.5 * ((0.0 - p) / sd + (1.0 - p) / sd)
    nframes = torch.tensor([T], dtype=torch.int32, device=dev)
    out = torch.empty((1, T), dtype=torch.uint8, device=dev)
    thr = torch.empty(1, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().sk_vad_energy(le.data_ptr(), nframes.data_ptr(), 1, T, 0, 0.0001, 1.0, 2.0 - mid, int(win), out.data_ptr(), thr.data_ptr(),
                                            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    fused = out[0].cpu().numpy().astype(bool)
    if numpy.isnan(thr.item()):                 # the detector's keep-everything rule fired: the opening left nothing
        fused = numpy.zeros(T, dtype=bool)
    return fused.reshape(lab.shape)
