"""PLP and RASTA-PLP features on the GPU -- what ``sidekit.frontend.features.plp`` (``sidekit/frontend/features.py:888-966``) and the
functions it calls (``audspec``, ``fft2barkmx``, ``postaud``, ``dolpc``, ``levinson``, ``lpc2cep``, ``lifter``) compute, and
``PlpExtractor``, the ``FeaturesExtractor`` that serves them.  There is no CPU fallback; importing the module needs neither a GPU nor
torch.

Three launches, two without RASTA: ``sc_mfcc`` (csrc/cepstrum.hip) under the bark bank gives the log-energy and the log critical-band
energies of every frame, ``sc_feat_rasta`` (csrc/featnorm.hip) filters them per utterance, ``sc_plp_cepstra`` (csrc/plp.hip) applies
equal loudness and the 0.33 power, forms the autocorrelation, runs Levinson-Durbin, converts the LPC to cepstra and lifters them, in
float64 per frame.  torch allocates, and copies the log-energy column into the result.

``FeaturesExtractor(feature_type='plp')`` stays refused: PLP is a class of its own, as full covariances are ``FullMixture``.

Differences from the reference:
  * ``plp(..., rasta=True)`` of the reference stops with ``NameError``: its module never imports ``rasta_filt``.  The function meant is
    ``sidekit.frontend.normfeat.rasta_filt``, which ``sc_feat_rasta`` reproduces; that is what runs here;
  * ``ceps_number`` is the number of cepstra, the LPC order plus one, as in the reference; it must lie in [2, bands - 1].  The reference
    breaks at 1 (its ``spec2cep`` returns nothing) and above bands - 1 (``levinson`` refuses the order);
  * ``lower_frequency``, ``higher_frequency``, ``filter_bank`` and ``filter_bank_size`` do not reach the reference's ``plp``: the bark
    bank always spans 0 to ``min(8000, fs / 2)`` Hz with ``ceil(hz2bark(fs / 2)) + 1`` bands (21 at 16 kHz, 17 at 8 kHz).  They are
    ignored here too, and ``filter_bank_size`` reads the number of bands;
  * the power spectrum, the bank sums and their logs are float32 (``sc_mfcc``); the reference rounds the spectrum to float32 and
    continues in float64.  ``lpc2spec``, whose output the reference discards, is not built;
  * what ``features_extractor`` lists for every extractor: one row for a one-frame signal, the part-length refusal, arrays for HDF5.
"""
import numpy

from . import _lib
from .features_extractor import FeaturesExtractor, _device_tables, _frame_offsets, _resident_batch
from .frontend.features import bark2hz, fft2barkmx, frame_shape, hann_window, hz2bark

MIN_BANDS, MAX_BANDS = _lib.SC_PLP_MIN_BANDS, _lib.SC_PLP_MAX_BANDS
LIFT = 0.6                       # the exponent of the reference's lifter


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("sidekit_amd.plp computes on the GPU only (no CPU fallback) and no GPU is visible")
    return torch


def bark_bands(fs):
    """The number of critical bands ``audspec`` gives a signal sampled at ``fs``"""
    return int(numpy.ceil(hz2bark(fs / 2)) + 1)


def equal_loudness(fs, nb):
    """``postaud``'s equal-loudness weights of ``nb`` bands whose centres are equally spaced in bark from 0 to ``fs / 2``, float64"""
    fsq = bark2hz(numpy.linspace(0, hz2bark(fs / 2.), num=nb)) ** 2
    return ((fsq / (fsq + 1.6e5)) ** 2) * ((fsq + 1.44e6) / (fsq + 9.61e6))


def autocorrelation_weights(nb, order):
    """``acw`` float64 (order + 1, nb): lag k of the real inverse FFT of the spectrum ``y`` mirrored to ``2 (nb - 1)`` points is
    ``sum_j acw[k][j] y[j]``"""
    M = 2 * (nb - 1)
    k, j = numpy.arange(order + 1)[:, None], numpy.arange(nb)[None, :]
    acw = 2.0 * numpy.cos(numpy.pi * ((j * k) % M) / (nb - 1)) / M
    acw[:, 0] = 1.0 / M
    acw[:, nb - 1] = numpy.where(numpy.arange(order + 1) % 2 == 0, 1.0, -1.0) / M
    return acw


def lifter_weights(nceps, lift=LIFT):
    """``lifter``'s weights of ``nceps`` cepstra: 1, then ``n ** lift``"""
    return numpy.hstack((1.0, numpy.arange(1, nceps) ** lift))


def plp_tables(fs, n_fft, window_length, nceps):
    """What the launches read besides the samples -> ``(window, bank, bank_lo, bank_hi, eql, acw, lift)``: the float32 Hann window, the
    float32 bark bank ``fft2barkmx(n_fft, fs, nb, 1., 0., min(8000, fs / 2))[:, :n_fft / 2 + 1]``, the first and one-past-last non-zero
    float32 entry of each band (int32; weights too small for float32 are zeros, and that is accepted), and in float64 the
    equal-loudness weights (nb,), the cosine-transform weights (nceps, nb) and the lifter (nceps,)."""
    nb = bark_bands(fs)
    bank = numpy.ascontiguousarray(fft2barkmx(n_fft, fs, nb, 1., 0., min(8000, fs / 2))[:, :n_fft // 2 + 1], dtype=numpy.float32)
    lo, hi = numpy.zeros(nb, dtype=numpy.int32), numpy.zeros(nb, dtype=numpy.int32)
    for i, row in enumerate(bank):
        support = numpy.nonzero(row)[0]
        if support.size:
            lo[i], hi[i] = support[0], support[-1] + 1
    return (hann_window(window_length), bank, lo, hi, equal_loudness(fs, nb), numpy.ascontiguousarray(autocorrelation_weights(nb, nceps - 1)),
            lifter_weights(nceps))


def _launch_tables(fs, n_fft, window_length, nceps):
    """``plp_tables`` and the one-row DCT ``sc_mfcc`` asks for (its cepstrum is not read)"""
    tables = plp_tables(fs, n_fft, window_length, nceps)
    return tables + (numpy.zeros((1, tables[1].shape[0]), dtype=numpy.float32),)


def _check_nceps(nceps, nb):
    if isinstance(nceps, bool) or not isinstance(nceps, (int, numpy.integer)) or not 2 <= nceps <= nb - 1:
        raise ValueError("plp: {!r} cepstra (the LPC order plus one) with {} critical bands: 2 to {} are built".format(nceps, nb, nb - 1))


def plp_device(wav, nsamples=None, *, fs=16000, nwin=0.025, nceps=13, shift=0.01, prefac=0.97, rasta=True, scale=1.0):
    """The PLP front end of a resident batch: ``wav`` (B, L) float32 or int16 CUDA, ``nsamples`` (B,) or None = L ->
    ``(frames (N, 1 + nceps + nb) float32 CUDA, seg_off int64 (B + 1,) CUDA)``, as ``post_process_device`` takes them.  Columns:
    energy | cep | post_spectrum (the compressed critical-band spectrum the LPC model is fitted to).  Rows, ``scale`` and the frame
    geometry are ``mfcc_device``'s.  With ``rasta`` the log critical-band energies of each utterance pass through ``rasta_filt``: its
    four leading frames then hold the cepstra of a flat spectrum."""
    torch = _torch()
    wav = _resident_batch(torch, wav)
    B, L = wav.shape
    dev = wav.device
    window_length, shift_sample, n_fft = frame_shape(fs, nwin, shift)
    nb = bark_bands(fs)
    if n_fft not in (256, 512) or not 1 <= shift_sample <= window_length or not MIN_BANDS <= nb <= MAX_BANDS:
        raise ValueError(f"plp: a window of {window_length} samples (n_fft {n_fft}; 256 and 512 are built), a shift of {shift_sample} and {nb} "
                         f"critical bands ({MIN_BANDS} to {MAX_BANDS}) are outside what sc_mfcc and sc_plp_cepstra support")
    _check_nceps(nceps, nb)
    window, bank, lo, hi, eql, acw, lift, dct = _device_tables(torch, (dev, fs, n_fft, window_length, int(nceps)), _launch_tables)
    lens, off, N = _frame_offsets(torch, wav, nsamples, window_length, shift_sample)
    D = 1 + nceps + nb
    frames = torch.empty((N, D), dtype=torch.float32, device=dev)
    if N:       # an empty tensor has no address to pass
        band = torch.empty((N, 2 + nb), dtype=torch.float32, device=dev)          # sc_mfcc's row: energy | one unused cepstrum | log bands
        _lib.launch("sc_mfcc", dev, wav, _lib.XT_I16 if wav.dtype == torch.int16 else _lib.XT_F32, wav.stride(0) if B > 1 else L, float(scale), lens,
                    off, B, N, window_length, shift_sample, n_fft, float(prefac), window, bank, lo, hi, nb, dct, 1, band, 2 + nb, None, n_fft // 2 + 1)
        logband, ldb = band[:, 2:], 2 + nb
        if rasta:
            logband, ldb = torch.empty((N, nb), dtype=torch.float32, device=dev), nb
            _lib.launch("sc_feat_rasta", dev, band[:, 2:], 2 + nb, off, B, nb, logband, nb)
        _lib.launch("sc_plp_cepstra", dev, logband, ldb, N, nb, nceps - 1, eql, acw, lift, frames[:, 1:], D, frames[:, 1 + nceps:], D)
        frames[:, 0] = band[:, 0]
    return frames, off


class PlpExtractor(FeaturesExtractor):
    """A ``FeaturesExtractor`` whose cepstra are PLP, or RASTA-PLP with ``rasta_plp`` (the default, as in the reference): the same
    constructor, ``extract_batch_device``, ``extract_from_signal``, ``extract``, dither, energy VAD and refusals.  ``feature_type``
    reads ``'plp'``, ``filter_bank_size`` the number of critical bands; ``lower_frequency``, ``higher_frequency`` and ``filter_bank``
    are kept and ignored; ``ceps_number`` outside [2, bands - 1] is a ``ValueError``.  The ``fb`` columns hold the compressed
    critical-band spectrum, ``plp``'s ``post_spectrum``."""

    def __init__(self,
                 audio_filename_structure=None,
                 feature_filename_structure=None,
                 sampling_frequency=None,
                 lower_frequency=None,
                 higher_frequency=None,
                 filter_bank=None,
                 filter_bank_size=None,
                 window_size=None,
                 shift=None,
                 ceps_number=None,
                 vad=None,
                 snr=None,
                 pre_emphasis=None,
                 save_param=None,
                 keep_all_features=None,
                 feature_type=None,
                 rasta_plp=None,
                 compressed='percentile'):
        super().__init__(audio_filename_structure, feature_filename_structure, sampling_frequency, lower_frequency, higher_frequency, filter_bank,
                         filter_bank_size, window_size, shift, ceps_number, vad, snr, pre_emphasis, save_param, keep_all_features, feature_type,
                         rasta_plp, compressed)
        if self.feature_type not in ('mfcc', 'plp'):     # 'mfcc' is the parent's reading of None
            raise ValueError("PlpExtractor extracts 'plp' features, not feature_type={!r}".format(self.feature_type))
        self.feature_type = 'plp'
        self.filter_bank_size = bark_bands(self.sampling_frequency)
        _check_nceps(self.ceps_number, self.filter_bank_size)

    def _check_feature_type(self):
        _check_nceps(self.ceps_number, self.filter_bank_size)

    def _check_filter_bank(self):
        pass      # the bark bank is fixed by the sampling frequency

    def _front_end_device(self, wav, nsamples):
        return plp_device(wav, nsamples, fs=self.sampling_frequency, nwin=self.window_size, nceps=self.ceps_number, shift=self.shift,
                          prefac=self.pre_emphasis, rasta=bool(self.rasta_plp))

