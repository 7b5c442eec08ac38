"""``sidekit.features_extractor``: ``FeaturesExtractor`` (``sidekit/features_extractor.py:54``) -- log-energy, cepstra, log filter-bank
outputs and the energy VAD of an audio file or of a resident batch of signals, computed on the GPU: ``sc_mfcc`` (csrc/cepstrum.hip) for
the frames, ``sk_vad_energy`` (csrc/vad.hip) for the labels.  There is no CPU fallback; importing the module needs neither a GPU nor torch.

``FeaturesServer(features_extractor=FeaturesExtractor(...))`` works: ``extract`` returns ``(feat, label, global_mean, global_std)``, the
columns chosen by ``save_param`` in the order energy, cep, fb (the order in which the reference's ``read_hdf5`` concatenates them).

Differences from the reference:
  * a signal of exactly one frame gives one row (the reference's ``framing(...).squeeze()`` breaks there); a signal shorter than one
    window gives the reference's empty arrays;
  * a signal longer than one of the reference's parts (``shift_sample * 6 250 000 + window_sample`` samples, beyond which it keeps only
    the last part) is refused with ``ValueError``;
  * the arithmetic is float32 whatever the signal's type (the reference computes a float64 signal in float64);
  * the energy VAD keeps every frame of a degenerate signal (``sidekit_amd.vad.vad_energy_device``);
  * ``extract`` returns arrays, not an HDF5 handle.
PLP and RASTA-PLP features come from a class of its own, ``sidekit_amd.plp.PlpExtractor``, which derives from this one;
``FeaturesExtractor(feature_type='plp')`` itself is refused with ``NotImplementedError``, in a message that names that class.
Not built, refused with ``NotImplementedError``: the ``'snr'``, ``'percentil'``, ``'lbl'`` and ``'dnn'`` detectors, noise and
reverberation files, ``.sph`` input, and the HDF5 writers ``save``, ``save_list`` and ``save_multispeakers``.
"""
import collections
import os

import numpy

from . import PARAM_TYPE, _lib
from .frontend.features import dct_basis, frame_shape, hann_window, trfbank

PART_FRAMES = 250 * 25000        # the reference cuts a signal into parts of this many shifts plus one window
MAX_FILT = 128                   # SC_MFCC_MAX_FILT
_UNBUILT_VAD = ('snr', 'percentil', 'lbl', 'dnn')

MAX_TABLES = 16                  # table sets kept on the device, least recently used first out

# what ``repr`` prints, filled from the attributes
_REPR = ("\t show: {show} keep_all_features: {keep_all_features}\n\t audio_filename_structure: {audio_filename_structure}  \n"
         "\t feature_filename_structure: {feature_filename_structure}  \n\t pre-emphasis: {pre_emphasis} \n"
         "\t lower_frequency: {lower_frequency}  higher_frequency: {higher_frequency} \n\t sampling_frequency: {sampling_frequency} \n"
         "\t filter bank: {filter_bank_size} filters of type {filter_bank}\n\t ceps_number: {ceps_number} \n"
         "\t window_size: {window_size} shift: {shift} \n\t vad: {vad}  snr: {snr} \n")

_tables = collections.OrderedDict()


def _in_samples(seconds, rate):
    """A duration as a whole number of samples, truncated; None while either is unset"""
    return None if None in (seconds, rate) else int(seconds * rate)


def _device_tables(torch, key, make=None):
    """The tables of ``make(*key[1:])`` (``host_tables`` unless given) on device ``key[0]``, from a cache of the ``MAX_TABLES`` most
    recently used sets; the makers take different numbers of arguments, so their keys cannot meet"""
    if key in _tables:
        _tables.move_to_end(key)
    else:
        _tables[key] = tuple(torch.from_numpy(t).to(key[0]) for t in (make or host_tables)(*key[1:]))
        while len(_tables) > MAX_TABLES:
            _tables.popitem(last=False)
    return _tables[key]


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("sidekit_amd.features_extractor computes on the GPU only (no CPU fallback) and no GPU is visible")
    return torch


def host_tables(fs, n_fft, window_length, lowfreq, maxfreq, nlinfilt, nlogfilt, nceps):
    """What ``sc_mfcc`` reads besides the samples -> ``(window, bank, bank_lo, bank_hi, dct)``: float32 Hann window, float32 ``trfbank``
    matrix, the first and one-past-last non-zero bin of each filter (int32), rows 1 .. nceps of the DCT basis in float32."""
    bank = numpy.ascontiguousarray(trfbank(fs, n_fft, lowfreq, maxfreq, nlinfilt, nlogfilt)[0], dtype=numpy.float32)
    lo, hi = numpy.zeros(bank.shape[0], dtype=numpy.int32), numpy.zeros(bank.shape[0], dtype=numpy.int32)
    for i, row in enumerate(bank):
        support = numpy.nonzero(row)[0]
        if support.size:
            lo[i], hi[i] = support[0], support[-1] + 1
    dct = numpy.ascontiguousarray(dct_basis(nceps + 1, bank.shape[0])[1:], dtype=numpy.float32)
    return hann_window(window_length), bank, lo, hi, dct


def to_device(signal):
    """A host signal (1-D float32 or int16) -> ``(wav (1, n), nsamples int32 (1,))`` on the current device"""
    torch = _torch()
    dev = torch.device("cuda", torch.cuda.current_device())
    sig = numpy.ascontiguousarray(signal).reshape(1, -1)
    wav = torch.empty((1, max(sig.shape[1], 1)), dtype=torch.int16 if sig.dtype == numpy.int16 else torch.float32, device=dev)
    if sig.shape[1]:
        wav[:, :sig.shape[1]] = torch.from_numpy(sig).to(dev)
    return wav, torch.tensor([sig.shape[1]], dtype=torch.int32, device=dev)


def _resident_batch(torch, wav):
    """``wav`` (B, L) or (L,) float32 or int16 CUDA with contiguous rows -> the (B, L) tensor; anything else is refused"""
    if not torch.is_tensor(wav) or not wav.is_cuda:
        raise RuntimeError("sidekit_amd.features_extractor computes on the GPU only (no CPU fallback): pass a CUDA tensor")
    if wav.dim() == 1:
        wav = wav.unsqueeze(0)
    if wav.dim() != 2 or wav.dtype not in (torch.float32, torch.int16) or wav.stride(1) != 1 or wav.shape[0] < 1 or wav.shape[1] < 1:
        raise ValueError(f"expected a (B, L) float32 or int16 batch with contiguous rows, got {tuple(wav.shape)} {wav.dtype}")
    return wav


def _frame_offsets(torch, wav, nsamples, window_length, shift_sample):
    """-> ``(lens int32 (B,), off int64 (B + 1,), N)``: the samples of each row (``nsamples`` or None = L, at most L), the row offsets of
    the stacked frames, ``max((n_b - window) // shift + 1, 0)`` an utterance, and their number, read back once"""
    B, L = wav.shape
    if nsamples is None:
        lens = torch.full((B,), L, dtype=torch.int32, device=wav.device)
    else:
        lens = torch.as_tensor(nsamples).to(device=wav.device, dtype=torch.int32).contiguous()
        if lens.shape != (B,):
            raise ValueError(f"nsamples must have shape ({B},)")
    lens = lens.clamp(max=L)
    count = (torch.div(lens.to(torch.int64) - window_length, shift_sample, rounding_mode='floor') + 1).clamp(min=0)
    off = torch.cat((torch.zeros(1, dtype=torch.int64, device=wav.device), count.cumsum(0))).contiguous()
    return lens, off, int(off[-1].item())


def mfcc_device(wav, nsamples=None, *, fs=16000, lowfreq=100, maxfreq=8000, nlinfilt=0, nlogfilt=24, nwin=0.025, nceps=13, shift=0.01, prefac=0.97,
                scale=1.0, get_spec=False):
    """The cepstral front end of a resident batch: ``wav`` (B, L) float32 or int16 CUDA, ``nsamples`` (B,) or None = L ->
    ``(frames (N, 1 + nceps + nfilt) float32 CUDA, seg_off int64 (B + 1,) CUDA)``, as ``post_process_device`` takes them; with
    ``get_spec`` the power spectrum ``(N, n_fft / 2 + 1)`` comes third.  Columns: energy | cep | fb.  Utterance b owns rows
    ``[seg_off[b], seg_off[b + 1])``, ``max((n_b - window) // shift + 1, 0)`` of them.  A sample is multiplied by ``scale`` on load: the
    reference works at the int16 scale, so a float signal in [-1, 1) wants ``scale=32768``."""
    torch = _torch()
    wav = _resident_batch(torch, wav)
    B, L = wav.shape
    dev = wav.device
    window_length, shift_sample, n_fft = frame_shape(fs, nwin, shift)
    nfilt = nlinfilt + nlogfilt
    if n_fft not in (256, 512) or not 1 <= shift_sample <= window_length or not 1 <= nfilt <= MAX_FILT or not 1 <= nceps <= nfilt - 1:
        raise ValueError(f"mfcc: a window of {window_length} samples (n_fft {n_fft}; 256 and 512 are built), a shift of {shift_sample}, {nfilt} filters "
                         f"(1 to {MAX_FILT}) and {nceps} cepstra (1 to filters - 1) are outside what sc_mfcc supports")
    window, bank, lo, hi, dct = _device_tables(torch, (dev, fs, n_fft, window_length, lowfreq, maxfreq, nlinfilt, nlogfilt, nceps))
    lens, off, N = _frame_offsets(torch, wav, nsamples, window_length, shift_sample)
    D = 1 + nceps + nfilt
    frames = torch.empty((N, D), dtype=torch.float32, device=dev)
    spec = torch.empty((N, n_fft // 2 + 1), dtype=torch.float32, device=dev) if get_spec else None
    ld = wav.stride(0) if B > 1 else L
    if N:       # an empty tensor has no address to pass
        _lib.launch("sc_mfcc", dev, wav, _lib.XT_I16 if wav.dtype == torch.int16 else _lib.XT_F32, ld, float(scale), lens, off, B, N, window_length,
                    shift_sample, n_fft, float(prefac), window, bank, lo, hi, nfilt, dct, nceps, frames, D, spec, n_fft // 2 + 1)
    return (frames, off, spec) if get_spec else (frames, off)


def dither(signal):
    """The reference's dither: a float32 copy of ``signal`` with ``0.0001 * randn`` of seed 0 added into it (``numpy.random.seed(0)``: the
    global generator is reseeded, as the reference does)"""
    sig = numpy.array(signal, dtype=numpy.float32).reshape(-1)
    numpy.random.seed(0)
    sig += 0.0001 * numpy.random.randn(sig.shape[0])
    return sig


class FeaturesExtractor(object):
    """A FeaturesExtractor processes an audio file in WAVE (PCM 16 bits, mono) or RAW PCM format and extracts filter banks, cepstral
    coefficients and log-energy, and performs a speech activity detection."""

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
        self.audio_filename_structure = audio_filename_structure
        self.feature_filename_structure = '{}' if feature_filename_structure is None else feature_filename_structure
        self.sampling_frequency = 8000 if sampling_frequency is None else sampling_frequency
        self.lower_frequency = lower_frequency
        self.higher_frequency = higher_frequency
        self.filter_bank = filter_bank
        self.filter_bank_size = filter_bank_size
        self.window_size = window_size
        self.shift = shift
        self.ceps_number = ceps_number
        self.vad = vad
        self.snr = snr
        self.pre_emphasis = 0.97 if pre_emphasis is None else pre_emphasis
        self.save_param = ["energy", "cep", "fb", "bnf", "vad"] if save_param is None else save_param
        self.keep_all_features = keep_all_features
        self.feature_type = 'mfcc' if feature_type is None else feature_type
        self.rasta_plp = True if rasta_plp is None else rasta_plp
        if compressed is not None:
            self.compressed = compressed
        self.show = 'empty'
        self.window_sample = _in_samples(self.window_size, self.sampling_frequency)
        self.shift_sample = _in_samples(self.shift, self.sampling_frequency)

    def __repr__(self):
        return _REPR.format(**vars(self))

    # ---- what is refused ---------------------------------------------------------------------------------------------------------------
    def _check_feature_type(self):
        if self.feature_type == 'plp':
            raise NotImplementedError("feature_type='plp' is not built here: sidekit_amd.plp.PlpExtractor extracts plp and RASTA-plp features")
        if self.feature_type != 'mfcc':
            raise NotImplementedError("feature_type={!r} is not built (only 'mfcc')".format(self.feature_type))

    def _check_filter_bank(self):
        if self.filter_bank not in ("lin", "log"):
            raise ValueError("filter_bank must be 'lin' or 'log' (got {!r})".format(self.filter_bank))

    def _check_options(self, noise_file_name=None, reverb_file_name=None):
        self._check_feature_type()
        if self.vad in _UNBUILT_VAD:
            raise NotImplementedError("vad={!r} is not built (None and 'energy' are)".format(self.vad))
        if self.vad not in (None, 'energy'):
            raise ValueError("unknown vad {!r}".format(self.vad))
        if noise_file_name is not None:
            raise NotImplementedError("noise_file_name: adding noise from a file is not built")
        if reverb_file_name is not None:
            raise NotImplementedError("reverb_file_name: adding reverberation from a file is not built")
        self._check_filter_bank()

    def _mfcc_options(self):
        size = {"lin": 0, "log": 0}       # _check_options has let only these two through
        size[self.filter_bank] = self.filter_bank_size
        return dict(fs=self.sampling_frequency, lowfreq=self.lower_frequency, maxfreq=self.higher_frequency, nlinfilt=size["lin"], nlogfilt=size["log"],
                    nwin=self.window_size, nceps=self.ceps_number, shift=self.shift, prefac=self.pre_emphasis)

    def _front_end_device(self, wav, nsamples):
        """-> ``(frames, seg_off)`` of a resident batch, columns energy | cep | fb: the part a subclass with other cepstra replaces"""
        return mfcc_device(wav, nsamples, **self._mfcc_options())

    # ---- the resident batch ------------------------------------------------------------------------------------------------------------
    def extract_batch_device(self, wav, nsamples=None):
        """``wav`` (B, L) float32 or int16 CUDA at the int16 scale, ``nsamples`` (B,) -> ``(frames (N, 1 + ceps_number + filter_bank_size),
        seg_off int64 (B + 1,), labels bool (N,))`` on the device, all columns, no dither: what ``post_process_device`` takes."""
        self._check_options()
        _torch()
        frames, off = self._front_end_device(wav, nsamples)
        return frames, off, self.vad_labels_device(frames, off)[0]

    def vad_labels_device(self, frames, off):
        """The detector ``vad`` names on the log-energy column of stacked frames -> ``(labels bool (N,), threshold float64 (B,))`` on the
        device.  ``None``: every frame, thresholds of -inf.  ``'energy'``: ``sk_vad_energy`` with the arguments of the reference's ``_vad``
        (8 iterations, flooring 0.0001, ceiling 1.5, alpha 0.2, no fusion) on the log-energy widened to float64; torch re-lays the stacked
        rows into the padded ``(B, T)`` the detector reads.  An utterance without a frame has threshold NaN."""
        self._check_options()
        torch = _torch()
        N, dev = frames.shape[0], frames.device
        if self.vad is None or N == 0:
            return (torch.ones(N, dtype=torch.bool, device=dev),
                    torch.full((off.shape[0] - 1,), float("nan") if self.vad else float("-inf"), dtype=torch.float64, device=dev))
        from .vad import vad_energy_device
        count = off[1:] - off[:-1]
        B, T = count.shape[0], int(count.max().item())
        rows = torch.arange(N, dtype=torch.int64, device=dev)
        utt = torch.bucketize(rows, off[1:], right=True)          # the utterance of a row: empty utterances own none
        t = rows - off[utt]
        le = torch.zeros((B, T), dtype=torch.float64, device=dev)
        le[utt, t] = frames[:, 0].double()
        label, thr = vad_energy_device(le, count.to(torch.int32), nb_train_it=8, flooring=0.0001, ceiling=1.5, alpha=0.2, fusion_win=0)
        return label[utt, t].bool(), thr

    # ---- one signal --------------------------------------------------------------------------------------------------------------------
    def _empty(self):
        return (numpy.empty((0, 1), dtype='int8'), numpy.empty((0, 1), dtype=PARAM_TYPE), numpy.empty((0, self.ceps_number), dtype=PARAM_TYPE),
                numpy.empty((0, self.filter_bank_size), dtype=PARAM_TYPE))

    def _from_signal(self, signal):
        """-> ``(frames, labels)`` on the device for a host signal, dithered as the reference's; None below one window"""
        if signal.shape[0] < self.window_sample:
            return None
        if signal.shape[0] > self.shift_sample * PART_FRAMES + self.window_sample:
            raise ValueError("a signal of {} samples is longer than one part of the reference ({} samples), which keeps the last part only"
                             .format(signal.shape[0], self.shift_sample * PART_FRAMES + self.window_sample))
        _torch()
        frames, _, labels = self.extract_batch_device(*to_device(dither(signal)))
        return frames, labels

    def extract_from_signal(self, signal,
                            sample_rate,
                            noise_file_name=None,
                            snr=10,
                            reverb_file_name=None,
                            reverb_level=-26.):
        """``signal`` (1-D, or 2-D whose column 0 is taken; int16 scale) -> ``(label bool (T,), energy (T,), cep (T, ceps_number),
        fb (T, filter_bank_size))``, float32.  The reference's dither is added first, into a float32 copy: the caller's array is not
        written."""
        self._check_options(noise_file_name, reverb_file_name)
        signal = numpy.asarray(signal)
        if signal.ndim == 2:
            signal = signal[:, 0]
        got = self._from_signal(signal)
        if got is None:
            return self._empty()
        frames, labels = got[0].cpu().numpy(), got[1].cpu().numpy()
        nceps = self.ceps_number
        return labels, frames[:, 0].copy(), frames[:, 1:1 + nceps].copy(), frames[:, 1 + nceps:].copy()

    # ---- one file ----------------------------------------------------------------------------------------------------------------------
    def _read(self, audio_filename, channel):
        ext = os.path.splitext(audio_filename)[-1].lower()
        if ext == '.sph':
            raise NotImplementedError(".sph input is not built (PCM 16 bits .wav, .pcm and .raw are)")
        if ext in ('.pcm', '.raw'):
            if channel != 0:
                raise ValueError("a raw PCM file has one channel")
            return numpy.fromfile(audio_filename, dtype='<i2').astype(numpy.float32)
        if ext not in ('.wav', '.wave'):
            raise TypeError("Unknown extension of audio file")
        from .pipeline import probe_wavs, read_pcm16
        kind, ns, rate, offset = probe_wavs([audio_filename], threads=1)
        if kind[0] < 0:
            raise IOError("cannot open {}".format(audio_filename))
        if kind[0] != 1:
            raise NotImplementedError("{}: only PCM 16 bits mono wav files are built".format(audio_filename))
        if channel != 0:
            raise ValueError("{} has one channel".format(audio_filename))
        if rate[0] != self.sampling_frequency:
            raise NotImplementedError("{} is sampled at {} Hz, not {}: resampling on read is not built".format(audio_filename, rate[0], self.sampling_frequency))
        pcm = numpy.zeros((1, max(int(ns[0]), 1)), dtype=numpy.int16)
        read_pcm16([audio_filename], offset, ns, [0], pcm, threads=1)
        return pcm[0, :int(ns[0])].astype(numpy.float32)

    def extract(self, show, channel,
                input_audio_filename=None,
                output_feature_filename=None,
                backing_store=False,
                noise_file_name=None,
                snr=10,
                reverb_file_name=None,
                reverb_level=-26.):
        """The frames of one channel of an audio file -> ``(feat float32 (T, D), label bool (T,), global_mean (D,), global_std (D,))``,
        what ``FeaturesServer`` takes from its extractor: the columns ``save_param`` names, in the order energy, cep, fb; the mean and the
        population standard deviation of the labelled frames (zeros and ones without one).  Nothing is written:
        ``output_feature_filename`` only becomes the ``feature_filename_structure`` and ``backing_store`` is not read."""
        self._check_options(noise_file_name, reverb_file_name)
        if input_audio_filename is not None:
            self.audio_filename_structure = input_audio_filename
        if output_feature_filename is not None:
            self.feature_filename_structure = output_feature_filename
        self.show = show
        signal = self._read(self.audio_filename_structure.format(show), channel)
        nceps, nfilt = self.ceps_number, self.filter_bank_size
        columns = numpy.concatenate([numpy.arange(a, b) for name, a, b in (("energy", 0, 1), ("cep", 1, 1 + nceps), ("fb", 1 + nceps, 1 + nceps + nfilt))
                                     if name in self.save_param] or [numpy.arange(0)]).astype(numpy.int64)
        if columns.size == 0:
            raise ValueError("save_param names none of 'energy', 'cep' and 'fb'")
        got = self._from_signal(signal)
        if got is None:
            return (numpy.empty((0, columns.size), dtype=PARAM_TYPE), numpy.empty(0, dtype=bool), numpy.zeros(columns.size, dtype=PARAM_TYPE),
                    numpy.ones(columns.size, dtype=PARAM_TYPE))
        import torch
        from .features_server import segment_moments_device
        frames, labels = got
        feat = frames[:, torch.as_tensor(columns, device=frames.device)].contiguous()
        mean, std = segment_moments_device(feat[labels])
        return (feat.cpu().numpy(), labels.cpu().numpy(), mean[0].cpu().numpy().astype(PARAM_TYPE), std[0].cpu().numpy().astype(PARAM_TYPE))

    # ---- the HDF5 writers --------------------------------------------------------------------------------------------------------------
    def save(self, show, channel=0, input_audio_filename=None, output_feature_filename=None, noise_file_name=None, snr=10, reverb_file_name=None,
             reverb_level=-26.):
        raise NotImplementedError("save: the HDF5 feature-file writers are not built (extract returns the arrays)")

    def save_list(self, show_list, channel_list, audio_file_list=None, feature_file_list=None, noise_file_list=None, snr_list=None,
                  reverb_file_list=None, reverb_levels=None, num_thread=1):
        raise NotImplementedError("save_list: the HDF5 feature-file writers are not built (extract returns the arrays)")

    def save_multispeakers(self, idmap, channel=0, input_audio_filename=None, output_feature_filename=None, keep_all=True, skip_existing_file=False,
                           compressed='percentile'):
        raise NotImplementedError("save_multispeakers: the HDF5 feature-file writers are not built (extract returns the arrays)")
