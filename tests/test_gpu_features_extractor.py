"""The cepstral front end on the GPU (csrc/cepstrum.hip ``sc_mfcc``, sidekit_amd/features_extractor.py) against the float64 evaluation of
its formulas on the same float32 operands (tests/tools/mfcc_f64.py) and the reference's own outputs (tests/golden/extractor.npz).

Accuracy bound, per configuration and output (energy, fb, cep; the spectrum relative to the frame's largest bin): the maximum deviation
from the float64 evaluation is at most 4 x the larger of the two CPU yardsticks the golden file records for that configuration -- the
reference's float32 outputs and a scipy single-precision route, each against the same float64 evaluation.  4, because the kernel is
the same class of computation as the single-precision route and adds three error sources to it: the 1-ulp hardware log2 in place of
libm's half-ulp log, a float32 window, a different butterfly order.

Measured on an MI355X (maximum over the rows of a configuration; the bound in brackets; profiles/mfcc_bench.json):
  configuration  energy             fb                 cep                spectrum
  0              1.03e-6 [4.13e-6]  2.28e-5 [5.36e-5]  7.87e-6 [2.42e-5]  4.84e-7 [1.55e-6]
  1              1.01e-6 [4.21e-6]  3.54e-6 [1.97e-5]  1.01e-5 [2.76e-5]  4.29e-7 [1.59e-6]
  2              9.94e-7 [4.24e-6]  3.84e-6 [1.32e-5]  1.48e-5 [3.38e-5]  4.58e-7 [1.30e-6]
  3              9.84e-7 [4.20e-6]  1.10e-5 [2.73e-5]  8.17e-6 [2.54e-5]  4.19e-7 [1.49e-6]
(the CPU single-precision route has its largest filter-bank deviation, 1.3e-5, in filter 1, whose bins pre-emphasis leaves two
millionths of the frame's largest).
The bitwise tests are exact.
"""
import os
import sys
import wave

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import mfcc_f64 as mf  # noqa: E402

pytestmark = pytest.mark.gpu
CONFIGS = range(len(mf.CONFIGS))
SENTINEL = -12345.0


class Case:
    """One configuration: its rows, tables, float64 evaluation (computed once) and yardsticks"""

    def __init__(self, c, golden):
        from sidekit_amd import features_extractor
        self.c, self.cfg = c, mf.CONFIGS[c]
        self.window, self.shift, self.n_fft = mf.frame_shape(self.cfg)
        self.nfilt, self.nceps = self.cfg["nlinfilt"] + self.cfg["nlogfilt"], self.cfg["nceps"]
        self.D = 1 + self.nceps + self.nfilt
        self.rows = mf.signals(self.cfg, int(golden[f"c{c}_seed"]))
        self.bank = golden[f"c{c}_bank"]
        self.tables = features_extractor.host_tables(self.cfg["fs"], self.n_fft, self.window, self.cfg["lowfreq"], self.cfg["maxfreq"],
                                                     self.cfg["nlinfilt"], self.cfg["nlogfilt"], self.nceps)
        self.want = [mf.mfcc_f64(r.astype(numpy.float32), self.cfg, self.bank) for r in self.rows]
        self.counts = [w[0].shape[0] for w in self.want]
        self.yard = numpy.maximum(golden[f"c{c}_yard_reference"].max(axis=0), golden[f"c{c}_yard_single"].max(axis=0))
        self.golden = golden

    def extractor(self, **kw):
        from sidekit_amd.features_extractor import FeaturesExtractor
        cfg = self.cfg
        return FeaturesExtractor(sampling_frequency=cfg["fs"], lower_frequency=cfg["lowfreq"], higher_frequency=cfg["maxfreq"],
                                 filter_bank="lin" if cfg["nlogfilt"] == 0 else "log", filter_bank_size=self.nfilt, window_size=cfg["nwin"],
                                 shift=cfg["shift"], ceps_number=self.nceps, pre_emphasis=mf.PREFAC, **kw)


@pytest.fixture(scope="module")
def cases(golden_dir):
    golden = numpy.load(os.path.join(golden_dir, "extractor.npz"))
    return [Case(c, golden) for c in CONFIGS]


def _batch(rows, dtype, dev, pad=3):
    """rows -> (wav (B, L) on the device, its tail filled with a value no row holds; nsamples)"""
    import torch
    L = max(r.shape[0] for r in rows) + pad
    wav = numpy.full((len(rows), L), 7777, dtype=dtype)
    for i, r in enumerate(rows):
        wav[i, :r.shape[0]] = r
    return torch.from_numpy(wav).to(dev), torch.tensor([r.shape[0] for r in rows], dtype=torch.int32, device=dev)


def _launch(case, rows, dev, dtype=numpy.int16, extra=0, spec=False):
    """sc_mfcc through the C ABI -> (out (N, D + extra) prefilled with SENTINEL, spec or None, offsets)"""
    import torch
    from sidekit_amd import _lib
    wav, lens = _batch(rows, dtype, dev)
    counts = [mf.n_frames(r.shape[0], case.cfg) for r in rows]
    off = torch.tensor(numpy.concatenate(([0], numpy.cumsum(counts))), dtype=torch.int64, device=dev)
    N, nb = int(sum(counts)), case.n_fft // 2 + 1
    out = torch.full((max(N, 1), case.D + extra), SENTINEL, dtype=torch.float32, device=dev)
    sp = torch.full((max(N, 1), nb + extra), SENTINEL, dtype=torch.float32, device=dev) if spec else None
    key = ("tables", case.c, str(dev))
    if key not in _launch.__dict__:
        _launch.__dict__[key] = [torch.from_numpy(t).to(dev) for t in case.tables]
    window, bank, lo, hi, dct = _launch.__dict__[key]
    _lib.launch("sc_mfcc", dev, wav, _lib.XT_I16 if dtype == numpy.int16 else _lib.XT_F32, wav.stride(0), 1.0, lens, off, len(rows), N, case.window,
                case.shift, case.n_fft, mf.PREFAC, window, bank, lo, hi, case.nfilt, dct, case.nceps, out, case.D + extra, sp, nb + extra)
    torch.cuda.synchronize(dev)
    return out.cpu().numpy(), None if sp is None else sp.cpu().numpy(), numpy.concatenate(([0], numpy.cumsum(counts)))


@pytest.fixture(scope="module")
def whole(gpu, cases):
    """every configuration's seven rows as one int16 batch, computed once"""
    return [_launch(case, case.rows, gpu, extra=3, spec=True) for case in cases]


@pytest.mark.parametrize("c", CONFIGS)
def test_accuracy_against_the_float64_evaluation(gpu, cases, whole, c):
    case, (out, spec, off) = cases[c], whole[c]
    assert case.counts[:5] == [0, 1, 1, 2, 5] and 257 <= case.counts[5] == case.counts[6] <= 259
    worst = numpy.zeros(4)
    for r, want in enumerate(case.want):
        rows = out[off[r]:off[r + 1]]
        got = (rows[:, 0], rows[:, 1 + case.nceps:case.D], rows[:, 1:1 + case.nceps], spec[off[r]:off[r + 1], :case.n_fft // 2 + 1])
        assert all(numpy.isfinite(g).all() for g in got), f"row {r}"
        worst = numpy.maximum(worst, mf.deviations(got, want))
    print(f"configuration {c}: energy / fb / cep / spectrum deviation from float64 {worst}, bound {4 * case.yard}")
    assert numpy.all(worst <= 4 * case.yard), (worst, 4 * case.yard)


@pytest.mark.parametrize("c", CONFIGS)
def test_columns_beyond_the_outputs_and_rows_without_frames_are_untouched(gpu, cases, whole, c):
    case, (out, spec, off) = cases[c], whole[c]
    assert numpy.all(out[:, case.D:] == SENTINEL) and numpy.all(spec[:, case.n_fft // 2 + 1:] == SENTINEL)
    assert numpy.all(out[:, :case.D] != SENTINEL), "every row of every utterance with a frame is written"
    none, _, _ = _launch(case, [case.rows[0], case.rows[0][:5]], gpu, spec=False)
    assert numpy.all(none == SENTINEL), "a batch without a frame writes nothing"


@pytest.mark.parametrize("c", CONFIGS)
def test_bits_do_not_depend_on_the_batch_the_order_or_the_sample_type(gpu, cases, whole, c):
    case, (out, spec, off) = cases[c], whole[c]
    again, spec2, _ = _launch(case, case.rows, gpu, extra=3, spec=True)
    assert again.tobytes() == out.tobytes() and spec2.tobytes() == spec.tobytes(), "two runs"
    as_float, _, _ = _launch(case, [r.astype(numpy.float32) for r in case.rows], gpu, dtype=numpy.float32, extra=3)
    assert as_float.tobytes() == out.tobytes(), "float32 samples holding the same integers"
    order = [5, 0, 3, 6, 1, 4, 2]
    shuffled, _, soff = _launch(case, [case.rows[i] for i in order], gpu)
    for pos, r in enumerate(order):
        assert shuffled[soff[pos]:soff[pos + 1], :case.D].tobytes() == out[off[r]:off[r + 1], :case.D].tobytes(), f"row {r} in a shuffled batch"
    for r in (1, 2, 3, 4, 5, 6):
        alone, sp, _ = _launch(case, [case.rows[r]], gpu, spec=True)
        assert alone[:, :case.D].tobytes() == out[off[r]:off[r + 1], :case.D].tobytes(), f"row {r} alone"
        assert sp.tobytes() == spec[off[r]:off[r + 1], :case.n_fft // 2 + 1].tobytes()


def test_a_zero_frame_gives_minus_infinity_as_numpy_does(gpu, cases):
    case = cases[0]
    out, _, _ = _launch(case, [numpy.zeros(case.window, dtype=numpy.int16)], gpu)
    assert numpy.all(numpy.isneginf(out[0, 0])) and numpy.all(numpy.isneginf(out[0, 1 + case.nceps:case.D]))


@pytest.mark.parametrize("c", CONFIGS)
def test_energy_vad_labels_equal_the_reference(gpu, cases, c):
    import torch
    case = cases[c]
    fx = case.extractor(vad="energy")
    wav, lens = _batch(case.rows, numpy.int16, gpu)
    frames, off, labels = fx.extract_batch_device(wav, lens)
    assert frames.shape == (sum(case.counts), case.D) and off.cpu().tolist() == numpy.concatenate(([0], numpy.cumsum(case.counts))).tolist()
    again, thr = fx.vad_labels_device(frames, off)
    assert torch.equal(again, labels)
    labels, thr, off = labels.cpu().numpy(), thr.cpu().numpy(), off.cpu().numpy()
    checked = 0
    for r in range(len(case.rows)):
        if f"c{c}_r{r}_label" not in case.golden:
            continue
        want, want_thr = case.golden[f"c{c}_r{r}_label"], float(case.golden[f"c{c}_r{r}_thr"])
        assert numpy.isfinite(want_thr) and want.any()
        assert numpy.array_equal(labels[off[r]:off[r + 1]], want), f"row {r}"
        assert abs(thr[r] - want_thr) <= 1e-4, (r, thr[r], want_thr)
        checked += 1
    assert checked == 4
    none = case.extractor().extract_batch_device(wav, lens)[2]
    assert none.dtype == torch.bool and bool(none.all()) and none.shape == (sum(case.counts),)


def test_extract_from_signal_reproduces_the_reference(gpu, cases):
    from sidekit_amd.frontend import features as fe
    case, g = cases[0], cases[0].golden
    sig = case.rows[5].astype(numpy.float32)
    keep = sig.copy()
    label, energy, cep, fb = case.extractor().extract_from_signal(sig, 16000)
    assert numpy.array_equal(sig, keep), "the caller's signal is not written"
    assert label.dtype == bool and label.all() and numpy.array_equal(label, g["surface_none_label"])
    assert energy.dtype == cep.dtype == fb.dtype == numpy.float32
    assert (energy.shape, cep.shape, fb.shape) == (g["surface_energy"].shape, g["surface_cep"].shape, g["surface_fb"].shape)
    bound = 4 * case.yard[:3] + g["surface_yard_reference"][:3]
    dev = [float(numpy.abs(a.astype(numpy.float64) - g[k]).max()) for a, k in ((energy, "surface_energy"), (fb, "surface_fb"), (cep, "surface_cep"))]
    print(f"extract_from_signal: energy / fb / cep deviation from the reference {dev}, bound {bound}")
    assert numpy.all(numpy.array(dev) <= bound), (dev, bound)
    label = case.extractor(vad="energy").extract_from_signal(sig[:, None], 16000)[0]
    assert numpy.array_equal(label, g["surface_energy_label"])
    # the numpy front doors on the undithered signal: the same kernel, so the same bits as the resident batch
    ceps, le, spec, mspec = fe.mfcc(case.rows[4], get_spec=True, get_mspec=True)
    out, sp, _ = _launch(case, [case.rows[4]], gpu, spec=True)
    assert ceps.tobytes() == out[:, 1:14].tobytes() and le.tobytes() == out[:, 0].tobytes() and mspec.tobytes() == out[:, 14:].tobytes()
    assert spec.tobytes() == sp.tobytes()
    assert fe.mfcc(case.rows[4].astype(numpy.float32))[2:] == [None, None]
    spec2, le2 = fe.power_spectrum(case.rows[4], fs=16000)
    assert spec2.tobytes() == sp.tobytes() and le2.tobytes() == le.tobytes()
    one = fe.mfcc(case.rows[1])
    assert one[0].shape == (1, 13) and one[1].shape == (1,), "a signal of exactly one frame gives one row"
    assert fe.mfcc(case.rows[0])[0].shape == (0, 13)


def test_features_server_loads_from_wav_files_what_the_resident_path_computes(gpu, cases, tmp_path):
    import torch
    from sidekit_amd.features_extractor import dither
    from sidekit_amd.features_server import FeaturesServer, post_process_device
    from sidekit_amd.mixture import em_split_device
    case = cases[0]
    # three signals long enough for the detector to label more than one frame (cmvn of a single labelled frame divides by zero)
    shows = {"a": case.rows[5], "b": mf.signals(case.cfg, 1)[5][:30000], "c": case.rows[6]}
    for show, pcm in shows.items():
        with wave.open(str(tmp_path / (show + ".wav")), "wb") as w:
            w.setnchannels(1), w.setsampwidth(2), w.setframerate(16000)
            w.writeframes(pcm.astype("<i2").tobytes())
    fx = case.extractor(audio_filename_structure=str(tmp_path / "{}.wav"), vad="energy")
    opts = dict(feat_norm="cmvn", delta=True)
    server = FeaturesServer(features_extractor=fx, **opts)
    for show, pcm in shows.items():
        feat, label = server.load(show)
        wav, lens = _batch([dither(pcm)], numpy.float32, gpu, pad=0)
        frames, off, labels = fx.extract_batch_device(wav, lens)
        want, want_labels, _ = post_process_device(frames, off, labels, **opts)
        assert feat.shape == (mf.n_frames(pcm.shape[0], case.cfg), 2 * case.D) and numpy.isfinite(feat).all() and 1 < label.sum() < label.shape[0]
        assert numpy.array_equal(feat.astype(numpy.float32), want.cpu().numpy()) and numpy.array_equal(label, want_labels.cpu().numpy()), show
    feat, label, mean, std = fx.extract("a", 0)
    assert feat.shape == (case.counts[5], case.D) and 0 < label.sum() < label.shape[0] and mean.shape == std.shape == (case.D,)
    assert numpy.abs(mean - feat[label].astype(numpy.float64).mean(axis=0)).max() < 1e-4 and numpy.abs(std - feat[label].astype(numpy.float64).std(axis=0)).max() < 1e-4
    only = case.extractor(audio_filename_structure=str(tmp_path / "{}.wav"), save_param=["cep", "vad"]).extract("a", 0)
    assert only[0].shape == (case.counts[5], case.nceps) and only[1].all() and only[0].tobytes() == numpy.ascontiguousarray(
        case.extractor(audio_filename_structure=str(tmp_path / "{}.wav")).extract("a", 0)[0][:, 1:1 + case.nceps]).tobytes()
    (tmp_path / "raw.pcm").write_bytes(shows["b"].astype("<i2").tobytes())
    assert case.extractor().extract("raw", 0, input_audio_filename=str(tmp_path / "{}.pcm"))[0].tobytes() == \
        case.extractor().extract("b", 0, input_audio_filename=str(tmp_path / "{}.wav"))[0].tobytes()
    frames, off = FeaturesServer(features_extractor=fx, keep_all_features=False, **opts).stack_features_device(list(shows))
    assert frames.is_cuda and frames.dtype == torch.float32 and frames.shape[1] == 2 * case.D and len(off) == 4 and off[-1] == frames.shape[0]
    ubm, llk = em_split_device(frames, 2, iterations=(1,))
    assert numpy.all(numpy.isfinite(llk)) and numpy.all(numpy.isfinite(ubm.mu)) and ubm.mu.shape == (2, 2 * case.D)
