"""``sidekit.frontend.features``: ``compute_delta`` (``sidekit/frontend/features.py:133-166``, ``sc_feat_delta``) and the cepstral front
end -- ``mfcc`` and ``power_spectrum`` (:363-477) computed on the GPU (``sc_mfcc``, csrc/cepstrum.hip) from the host-made tables of the
reference: ``trfbank`` (:226-305), the symmetric Hann window and the orthonormal DCT-II basis.  ``plp`` (:888-966) is computed on the GPU
too (``sidekit_amd.plp``), from the host-made ``fft2barkmx`` bank (:480-522); ``lpc2spec``, whose output the reference discards, is not
built.  ``pca_dct`` (:169-194) and ``shifted_delta_cepstral`` (:197-223) run on the GPU through ``sidekit_amd.features_context``.
There is no CPU fallback; importing the module needs neither a GPU nor torch."""
import numpy

from .. import PARAM_TYPE


def hz2mel(f, htk=True):
    """Hertz -> mel, the HTK formula (the reference's default; Slaney's scale is not built)"""
    if not htk:
        raise NotImplementedError("hz2mel: htk=False (Slaney's mel scale) is not built")
    return 2595 * numpy.log10(1 + f / 700.)


def mel2hz(z, htk=True):
    """mel -> Hertz, the HTK formula"""
    if not htk:
        raise NotImplementedError("mel2hz: htk=False (Slaney's mel scale) is not built")
    return 700. * (10**(z / 2595.) - 1)


def hz2bark(f):
    """Hertz -> bark, the reference's ``6 asinh(f / 600)``"""
    return 6. * numpy.arcsinh(f / 600.)


def bark2hz(z):
    """bark -> Hertz"""
    return 600. * numpy.sinh(z / 6.)


def fft2barkmx(n_fft, fs, nfilts=0, width=1., minfreq=0., maxfreq=8000):
    """The weights that sum FFT bins into critical bands -> float64 ``(nfilts, n_fft)`` whose columns above ``n_fft / 2`` are zero:
    ``nfilts`` bands (0: one per bark and one more) whose centres are equally spaced in bark from ``minfreq`` to ``min(maxfreq, fs / 2)``,
    each ``10 ** (min(0, d + 0.5, -2.5 (d - 0.5)) / width)`` at a bin ``d`` bark above its centre, computed on the host."""
    maxfreq = min(maxfreq, fs / 2.)
    lowest = hz2bark(minfreq)
    span = hz2bark(maxfreq) - lowest
    if nfilts == 0:
        nfilts = numpy.ceil(span) + 1
    nfilts = int(nfilts)
    step = span / (nfilts - 1)
    bins = hz2bark(numpy.arange(n_fft // 2 + 1) * fs / n_fft)
    wts = numpy.zeros((nfilts, n_fft))
    for i in range(nfilts):
        centre = lowest + i * step
        rising, falling = bins - centre + 0.5, -2.5 * (bins - centre - 0.5)
        wts[i, :n_fft // 2 + 1] = 10 ** (numpy.minimum(0., numpy.minimum(rising, falling) / width))
    return wts


def _band_edges(lowfreq, maxfreq, nlinfilt, nlogfilt, midfreq):
    """The nfilt + 2 edge frequencies of the triangles -> ``(edges, nlinfilt, nlogfilt)``.  The precision of every step is the
    reference's: float32 edges for the linear and the mixed bank, float64 ones for the mel bank."""
    nfilt = nlinfilt + nlogfilt
    if nlogfilt == 0:
        edges = numpy.zeros(nfilt + 2, dtype=PARAM_TYPE)
        step = (maxfreq - lowfreq) / (nlinfilt + 1)
        edges[:] = lowfreq + numpy.arange(nlinfilt + 2) * step
        return edges
    if nlinfilt == 0:
        mel_lo, mel_hi = hz2mel(lowfreq), hz2mel(maxfreq)
        step = (mel_hi - mel_lo) / (nfilt + 1)
        return mel2hz(mel_lo + numpy.arange(nlogfilt + 2) * step)
    # linear triangles below midfreq, mel-spaced ones above; a linear one is added while the first mel step is narrower than the linear step
    edges = numpy.zeros(nfilt + 2, dtype=PARAM_TYPE)
    step = (min([midfreq, maxfreq]) - lowfreq) / (nlinfilt + 1)
    edges[:nlinfilt] = lowfreq + numpy.arange(nlinfilt) * step
    mel_lo, mel_hi = hz2mel(min([1000, maxfreq])), hz2mel(maxfreq)
    mel_step = (mel_hi - mel_lo) / (nlogfilt + 1)
    while mel2hz(mel_step) < step:
        nlinfilt, nlogfilt = nlinfilt + 1, nlogfilt - 1
        edges[:nlinfilt] = lowfreq + numpy.arange(nlinfilt) * step
        mel_lo = hz2mel(edges[nlinfilt - 1] + 2 * step)
        mel_step = (mel_hi - mel_lo) / (nlogfilt + 1)
    mels = numpy.zeros(nlogfilt + 2, dtype=PARAM_TYPE)
    mels[:] = mel_lo + numpy.arange(nlogfilt + 2) * mel_step
    edges[nlinfilt:] = mel2hz(mels)
    return edges


def trfbank(fs, nfft, lowfreq, maxfreq, nlinfilt, nlogfilt, midfreq=1000):
    """The triangular filter bank of the cepstral front end -> ``(fbank float32 (nfilt, nfft // 2 + 1), frequences)``: ``nlinfilt``
    linearly spaced triangles, ``nlogfilt`` mel-spaced ones, or both (linear below ``midfreq``), each of height
    ``2 / (upper edge - lower edge)``.  As in the reference the rising side covers the bins above the lower edge up to the centre's bin,
    and the falling side stops one bin short of the upper edge's bin."""
    nfilt = nlinfilt + nlogfilt
    frequences = _band_edges(lowfreq, maxfreq, nlinfilt, nlogfilt, midfreq)
    bank = numpy.zeros((nfilt, nfft // 2 + 1), dtype=PARAM_TYPE)
    bin_hz = numpy.arange(nfft) / (1. * nfft) * fs
    widths = frequences[2:] - frequences[:-2]
    peaks = 2. / widths               # as arrays: the division stays in the precision of the edges
    for i, (low, cen, hi) in enumerate(zip(frequences[:-2], frequences[1:-1], frequences[2:])):
        height = peaks[i]
        first, peak, last = (numpy.floor(edge * nfft / fs) + 1 for edge in (low, cen, hi))
        rising = numpy.arange(first, peak, dtype=int)
        falling = numpy.arange(peak, min(last, nfft), dtype=int)[:-1]
        bank[i][rising] = height / (cen - low) * (bin_hz[rising] - low)
        bank[i][falling] = height / (hi - cen) * (hi - bin_hz[falling])
    return bank, frequences


def dct_basis(nbasis, length):
    """The first ``nbasis`` rows of the orthonormal DCT-II basis of ``length`` points (what the reference takes from
    ``scipy.fftpack.idct(numpy.eye(nbasis, length), norm='ortho')``), float64"""
    # cos(pi k / (2 length)), k = row * (2 column + 1), with k folded into the first quadrant as an integer: the zeros are exact
    k = (numpy.arange(nbasis)[:, None] * (2 * numpy.arange(length)[None, :] + 1)) % (4 * length)
    k = numpy.where(k > 2 * length, 4 * length - k, k)
    sign = numpy.where(k > length, -1.0, 1.0)
    k = numpy.where(k > length, 2 * length - k, k)
    basis = numpy.sqrt(2. / length) * sign * numpy.where(k == length, 0.0, numpy.cos(numpy.pi * k / (2 * length)))
    basis[:1] *= numpy.sqrt(0.5)
    return basis


def hann_window(length):
    """The symmetric Hann window ``power_spectrum`` applies (``numpy.hanning``), float32 as the kernel holds it"""
    return numpy.hanning(length).astype(PARAM_TYPE)


def frame_shape(fs, win_time, shift):
    """-> ``(window_length, shift in samples, n_fft)`` as ``power_spectrum`` derives them"""
    window_length = int(round(win_time * fs))
    return window_length, int(shift * fs), 2 ** int(numpy.ceil(numpy.log2(window_length)))


def _signal(input_sig):
    sig = numpy.asarray(input_sig)
    if sig.ndim != 1:
        raise ValueError("expected a one-dimensional signal, got shape {}".format(sig.shape))
    return numpy.ascontiguousarray(sig if sig.dtype == numpy.int16 else sig.astype(numpy.float32))


def power_spectrum(input_sig,
                   fs=8000,
                   win_time=0.025,
                   shift=0.01,
                   prefac=0.97):
    """-> ``(spec float32 (frames, n_fft / 2 + 1), log_energy float32 (frames,))`` of a signal at the int16 scale: frames of
    ``round(win_time * fs)`` samples every ``int(shift * fs)``, pre-emphasised inside the frame, the log-energy of the unwindowed frame,
    the power spectrum of the Hann-windowed one.  Unlike the reference a signal of exactly one window gives one row."""
    from ..features_extractor import mfcc_device, to_device
    wav, nsamples = to_device(_signal(input_sig))
    frames, _, spec = mfcc_device(wav, nsamples, fs=fs, lowfreq=0, maxfreq=fs / 2, nlinfilt=2, nlogfilt=0, nwin=win_time, nceps=1, shift=shift,
                                  prefac=prefac, get_spec=True)
    return spec.cpu().numpy().astype(PARAM_TYPE), frames[:, 0].cpu().numpy().astype(PARAM_TYPE)


def mfcc(input_sig,
         lowfreq=100, maxfreq=8000,
         nlinfilt=0, nlogfilt=24,
         nwin=0.025,
         fs=16000,
         nceps=13,
         shift=0.01,
         get_spec=False,
         get_mspec=False,
         prefac=0.97):
    """-> ``[ceps (frames, nceps), log_energy (frames,), spec or None, mspec or None]``, float32: the cepstra 1 .. nceps of the log outputs
    of the ``trfbank`` triangles on ``power_spectrum``, the log-energy, and on request the power spectrum and the log filter-bank outputs."""
    from ..features_extractor import mfcc_device, to_device
    wav, nsamples = to_device(_signal(input_sig))
    got = mfcc_device(wav, nsamples, fs=fs, lowfreq=lowfreq, maxfreq=maxfreq, nlinfilt=nlinfilt, nlogfilt=nlogfilt, nwin=nwin, nceps=nceps,
                      shift=shift, prefac=prefac, get_spec=get_spec)
    frames = got[0].cpu().numpy().astype(PARAM_TYPE)
    return [frames[:, 1:1 + nceps], frames[:, 0], got[2].cpu().numpy().astype(PARAM_TYPE) if get_spec else None,
            frames[:, 1 + nceps:] if get_mspec else None]


def plp(input_sig,
        nwin=0.025,
        fs=16000,
        plp_order=13,
        shift=0.01,
        get_spec=False,
        get_mspec=False,
        prefac=0.97,
        rasta=True):
    """-> ``[cepstra (frames, plp_order), log_energy (frames,), spec or None, post_spectrum or None]``, float32: the liftered cepstra of
    the LPC model of order ``plp_order - 1`` fitted to the compressed critical-band spectrum (``sidekit_amd.plp``: ``sc_mfcc`` under the
    ``fft2barkmx`` bank, ``sc_feat_rasta`` with ``rasta``, ``sc_plp_cepstra``), the log-energy, and on request the power spectrum and
    the compressed critical-band spectrum.  ``rasta=True`` filters with ``normfeat.rasta_filt``, the function the reference means and
    does not import."""
    from ..features_extractor import to_device
    from ..plp import plp_device
    wav, nsamples = to_device(_signal(input_sig))
    frames = plp_device(wav, nsamples, fs=fs, nwin=nwin, nceps=plp_order, shift=shift, prefac=prefac, rasta=rasta)[0].cpu().numpy().astype(PARAM_TYPE)
    spec = power_spectrum(input_sig, fs=fs, win_time=nwin, shift=shift, prefac=prefac)[0] if get_spec else None
    return [frames[:, 1:1 + plp_order], frames[:, 0], spec, frames[:, 1 + plp_order:] if get_mspec else None]


def compute_delta(features, win=3, method='filter', filt=numpy.array([.25, .5, .25, 0, -.25, -.5, -.25])):
    """The delta coefficients of ``features`` (frames x coefficients) -> float32, as the reference executes them:
    ``numpy.convolve(column, filt)[win:-win]``, a 'same' convolution with zeros (not the replicated edge frames the reference builds and
    leaves unused) outside the stream.  ``method='diff'``: ``filt`` is -1 at its first tap and 1 at its last.  ``filt`` must have
    ``2 win + 1`` taps (the reference fails with a broadcast error otherwise)."""
    from ..features_server import delta_device
    features = numpy.asarray(features)
    if method == 'diff':
        filt = numpy.zeros(2 * win + 1, dtype=PARAM_TYPE)
        filt[0] = -1
        filt[-1] = 1
    filt = numpy.asarray(filt, dtype=numpy.float64).reshape(-1)
    if filt.shape[0] != 2 * win + 1:
        raise ValueError('the delta filter has {} taps, the window 2 * {} + 1'.format(filt.shape[0], win))
    return delta_device(numpy.asarray(features, dtype=numpy.float32), None, filt).cpu().numpy().astype(PARAM_TYPE)


def pca_dct(cep, left_ctx=12, right_ctx=12, p=None):
    """DCT-PCA (McLaren and Lei, 2015) of ``cep`` (frames x coefficients) -> float64 holding the float32 device values: the DCT over
    time of each coefficient's window of ``left_ctx + 1 + right_ctx`` frames (the stream's first and last frame repeated past its ends),
    ``(frames, D W)``, projected by ``p`` (``(D W, Q)``) when given -- as one product, on the f64 matrix cores
    (``sidekit_amd.features_context.pca_dct_device``)."""
    from ..features_context import pca_dct_device
    return pca_dct_device(numpy.asarray(cep, dtype=numpy.float32), None, left_ctx, right_ctx, p).cpu().numpy().astype(numpy.float64)


def shifted_delta_cepstral(cep, d=1, p=3, k=7):
    """``cep`` with its shifted delta cepstra appended -> float64 ``(frames, D (k + 1))`` holding the float32 device values: block ``b``
    is frame ``t + b p - d`` less frame ``t + b p + d`` (what the reference computes: its difference filter is flipped by
    ``numpy.convolve``), the stream's first and last frame repeated past its ends.  ``ValueError`` while ``(k - 1) p > 3 k``: the
    reference pads ``3 k + d`` frames whatever ``p`` is and past that bound reads zeros, then wraps its index
    (``sidekit_amd.features_context.sdc_device``)."""
    from ..features_context import sdc_device
    return sdc_device(numpy.asarray(cep, dtype=numpy.float32), None, d, p, k).cpu().numpy().astype(numpy.float64)
