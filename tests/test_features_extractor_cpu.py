"""The cepstral front end without a GPU (sidekit_amd/features_extractor.py, frontend/features.py, csrc/cepstrum.hip): the entry point's own
header against its binding table and the built library, its argument checks through the C ABI, the reference's parameter lists, the
host tables against the reference's bit for bit (tests/golden/extractor.npz), the refusals and the package wiring."""
import inspect
import os
import re
import subprocess
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

import mfcc_f64 as mf  # noqa: E402
import sidekit_amd  # noqa: E402
from sidekit_amd import _lib, features_extractor  # noqa: E402
from sidekit_amd.features_extractor import FeaturesExtractor  # noqa: E402
from sidekit_amd.frontend import features as fe  # noqa: E402

GOLDEN = numpy.load(os.path.join(ROOT, "tests", "golden", "extractor.npz"))


def _extractor(cfg=mf.CONFIGS[0], **kw):
    opts = dict(sampling_frequency=cfg["fs"], lower_frequency=cfg["lowfreq"], higher_frequency=cfg["maxfreq"],
                filter_bank="lin" if cfg["nlogfilt"] == 0 else "log", filter_bank_size=cfg["nlinfilt"] + cfg["nlogfilt"], window_size=cfg["nwin"],
                shift=cfg["shift"], ceps_number=cfg["nceps"])
    opts.update(kw)
    return FeaturesExtractor(**opts)


def test_header_binding_table_and_library_agree():
    import ctypes
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sidekit_amd", "cepstrum.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?(?:int|char\s*\*|void)\s*\**\s*((?:xt|sc|sk)_\w+)\s*\(", src, flags=re.M)))
    assert declared == ["sc_mfcc"]
    assert sorted(_lib.CEPSTRUM_SIGNATURES) == declared, "ctypes binding table and header disagree"
    others = (set(_lib.SIGNATURES) | set(_lib.GAUSSIAN_SIGNATURES) | set(_lib.MIXTURE_SIGNATURES) | set(_lib.IVECTOR_SIGNATURES)
              | set(_lib.GMM_SCORING_SIGNATURES) | set(_lib.FEATURES_SIGNATURES))
    assert not set(_lib.CEPSTRUM_SIGNATURES) & others, "the table is disjoint from the other tables"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "sc_mfcc"), "sc_mfcc declared in include/sidekit_amd/cepstrum.h but not exported"
    res, args = _lib.CEPSTRUM_SIGNATURES["sc_mfcc"]
    fn = _lib.lib().sc_mfcc
    assert fn.restype is res and fn.argtypes == args
    ctype = {"void*": _lib._P, "int32_t": _lib._I32, "int64_t": _lib._I64, "double": _lib._F64}
    params = re.search(r"int sc_mfcc\((.*?)\);", re.sub(r"\s+", " ", src)).group(1).split(",")
    kinds = ["void*" if "*" in q else q.replace("const", "").split()[0] for q in params]
    assert [ctype[k] for k in kinds] == args, kinds
    assert int(re.search(r"#define SC_MFCC_MAX_FILT (\d+)", src).group(1)) == _lib.SC_MFCC_MAX_FILT == features_extractor.MAX_FILT == 128


def test_entry_point_checks_its_arguments_before_anything_is_enqueued():
    """SK_EARG through the C ABI on a host with no GPU: nothing was enqueued, or there would have been a HIP error instead."""
    lib = _lib.lib()
    p = 4096   # any non-null address: a refused call dereferences nothing

    def call(wav=p, dtype=_lib.XT_F32, wav_ld=16000, scale=1.0, ns=p, off=p, B=2, N=10, nwin=400, shift=160, n_fft=512, prefac=0.97, window=p,
             bank=p, lo=p, hi=p, nfilt=24, dct=p, nceps=13, out=p, ld=38, spec=None, lds=0):
        return lib.sc_mfcc(wav, dtype, wav_ld, scale, ns, off, B, N, nwin, shift, n_fft, prefac, window, bank, lo, hi, nfilt, dct, nceps, out, ld,
                           spec, lds, None)

    cases = {name + " null": call(**{name: None}) for name in ("wav", "ns", "off", "window", "bank", "lo", "hi", "dct", "out")}
    cases.update({"dtype bf16": call(dtype=_lib.XT_BF16), "dtype f64": call(dtype=_lib.XT_F64), "n_fft 1024": call(n_fft=1024, nwin=600),
                  "n_fft 128": call(n_fft=128, nwin=100), "n_fft 0": call(n_fft=0), "nwin = n_fft / 2": call(nwin=256), "nwin = n_fft + 1": call(nwin=513),
                  "nwin 128 at 256": call(n_fft=256, nwin=128), "nwin 257 at 256": call(n_fft=256, nwin=257), "nwin 0": call(nwin=0),
                  "shift 0": call(shift=0), "shift < 0": call(shift=-160), "shift > nwin": call(shift=401), "nfilt 0": call(nfilt=0, nceps=1),
                  "nfilt 129": call(nfilt=129, ld=200), "nceps = nfilt": call(nceps=24, ld=64), "nceps 0": call(nceps=0), "nceps < 0": call(nceps=-1),
                  "ld too small": call(ld=37), "B = 0": call(B=0), "B < 0": call(B=-1), "N < 0": call(N=-1), "wav_ld 0": call(wav_ld=0),
                  "lds too small": call(spec=p, lds=256)})
    assert all(rc == _lib.SK_EARG for rc in cases.values()), {k: v for k, v in cases.items() if v != _lib.SK_EARG}
    assert "sc_mfcc" in _lib.last_error()
    # no frame is nothing to do, not an error; the ends of every supported range pass the checks (N = 0: nothing is enqueued either)
    assert call(N=0) == call(N=0, B=1) == call(N=0, dtype=_lib.XT_I16) == _lib.SK_OK
    assert call(N=0, nwin=257) == call(N=0, nwin=512, shift=512) == call(N=0, n_fft=256, nwin=129, shift=1) == call(N=0, n_fft=256, nwin=256) == _lib.SK_OK
    assert call(N=0, nfilt=128, nceps=127, ld=256) == call(N=0, nfilt=2, nceps=1, ld=4) == call(N=0, spec=p, lds=257) == _lib.SK_OK
    assert call(N=0, n_fft=256, nwin=200, spec=p, lds=129) == _lib.SK_OK


def test_reference_parameter_lists():
    expect = {
        "__init__": "(self, audio_filename_structure=None, feature_filename_structure=None, sampling_frequency=None, lower_frequency=None, "
                    "higher_frequency=None, filter_bank=None, filter_bank_size=None, window_size=None, shift=None, ceps_number=None, vad=None, "
                    "snr=None, pre_emphasis=None, save_param=None, keep_all_features=None, feature_type=None, rasta_plp=None, "
                    "compressed='percentile')",
        "extract": "(self, show, channel, input_audio_filename=None, output_feature_filename=None, backing_store=False, noise_file_name=None, "
                   "snr=10, reverb_file_name=None, reverb_level=-26.0)",
        "extract_from_signal": "(self, signal, sample_rate, noise_file_name=None, snr=10, reverb_file_name=None, reverb_level=-26.0)"}
    for name, sig in expect.items():
        assert str(inspect.signature(getattr(FeaturesExtractor, name))) == sig, name
    functions = {fe.mfcc: "(input_sig, lowfreq=100, maxfreq=8000, nlinfilt=0, nlogfilt=24, nwin=0.025, fs=16000, nceps=13, shift=0.01, get_spec=False, "
                          "get_mspec=False, prefac=0.97)",
                 fe.power_spectrum: "(input_sig, fs=8000, win_time=0.025, shift=0.01, prefac=0.97)",
                 fe.trfbank: "(fs, nfft, lowfreq, maxfreq, nlinfilt, nlogfilt, midfreq=1000)"}
    for fn, sig in functions.items():
        assert str(inspect.signature(fn)) == sig, fn.__name__


def test_constructor_defaults_attributes_and_repr():
    fx = FeaturesExtractor()
    assert (fx.audio_filename_structure, fx.feature_filename_structure, fx.sampling_frequency, fx.pre_emphasis, fx.feature_type, fx.rasta_plp) == \
        (None, '{}', 8000, 0.97, 'mfcc', True)
    assert fx.save_param == ["energy", "cep", "fb", "bnf", "vad"] and fx.compressed == 'percentile' and fx.show == 'empty'
    assert fx.window_sample is None and fx.shift_sample is None and fx.vad is None and fx.keep_all_features is None
    fx = _extractor(vad="energy", snr=40, keep_all_features=True, audio_filename_structure="a/{}.wav")
    assert (fx.window_sample, fx.shift_sample) == (400, 160)
    assert _extractor(mf.CONFIGS[1]).window_sample == 200 and _extractor(mf.CONFIGS[2]).window_sample == 512
    assert repr(fx) == ('\t show: empty keep_all_features: True\n\t audio_filename_structure: a/{}.wav  \n\t feature_filename_structure: {}  \n'
                        '\t pre-emphasis: 0.97 \n\t lower_frequency: 100  higher_frequency: 8000 \n\t sampling_frequency: 16000 \n'
                        '\t filter bank: 24 filters of type log\n\t ceps_number: 13 \n\t window_size: 0.025 shift: 0.01 \n\t vad: energy  snr: 40 \n')


def test_host_tables_equal_the_reference_bit_for_bit():
    for c, cfg in enumerate(mf.CONFIGS):
        window_length, shift, n_fft = fe.frame_shape(cfg["fs"], cfg["nwin"], cfg["shift"])
        assert (window_length, shift, n_fft) == mf.frame_shape(cfg)
        bank, freqs = fe.trfbank(cfg["fs"], n_fft, cfg["lowfreq"], cfg["maxfreq"], cfg["nlinfilt"], cfg["nlogfilt"])
        want = GOLDEN[f"c{c}_bank"]
        assert bank.dtype == numpy.float32 == want.dtype and bank.shape == want.shape
        assert bank.tobytes() == want.tobytes(), f"configuration {c}: trfbank differs from the reference's"
        assert numpy.asarray(freqs).dtype == GOLDEN[f"c{c}_frequences"].dtype and numpy.asarray(freqs).tobytes() == GOLDEN[f"c{c}_frequences"].tobytes()
        window, bank2, lo, hi, dct = features_extractor.host_tables(cfg["fs"], n_fft, window_length, cfg["lowfreq"], cfg["maxfreq"], cfg["nlinfilt"],
                                                                     cfg["nlogfilt"], cfg["nceps"])
        assert window.dtype == dct.dtype == numpy.float32 and lo.dtype == hi.dtype == numpy.int32
        assert window.tobytes() == GOLDEN[f"c{c}_window"].tobytes() and bank2.tobytes() == want.tobytes()
        assert dct.shape == (cfg["nceps"], want.shape[0]) and dct.tobytes() == GOLDEN[f"c{c}_dct"].tobytes()
        for i, row in enumerate(want):
            assert not row[:lo[i]].any() and not row[hi[i]:].any() and row[lo[i]] != 0 and row[hi[i] - 1] != 0 and 0 <= lo[i] < hi[i] <= n_fft // 2 + 1
    assert numpy.abs(fe.dct_basis(14, 24) @ fe.dct_basis(24, 24).T - numpy.eye(14, 24)).max() < 1e-14, "orthonormal rows"


def test_trfbank_mixed_branch():
    """linear triangles below 1 kHz and mel-spaced ones above: float32 edges, ascending, each filter with a support of its own"""
    bank, freqs = fe.trfbank(16000, 512, 100, 8000, 5, 19)
    assert bank.shape == (24, 257) and bank.dtype == numpy.float32 and freqs.dtype == numpy.float32 and freqs.shape == (26,)
    assert numpy.all(numpy.diff(freqs) > 0) and freqs[0] == 100 and abs(freqs[-1] - 8000) < 1e-2
    assert numpy.all(bank >= 0) and numpy.all(bank.sum(axis=1) > 0)
    assert fe.hz2mel(700.) == pytest.approx(2595 * numpy.log10(2.)) and fe.mel2hz(fe.hz2mel(1234.5)) == pytest.approx(1234.5)


def test_unbuilt_options_raise():
    sig = numpy.zeros(16000, dtype=numpy.float32)
    for kw, word in ((dict(feature_type='plp'), "plp"), (dict(vad='snr'), "snr"), (dict(vad='percentil'), "percentil"), (dict(vad='lbl'), "lbl"),
                     (dict(vad='dnn'), "dnn")):
        with pytest.raises(NotImplementedError, match=word):
            _extractor(**kw).extract_from_signal(sig, 16000)
        with pytest.raises(NotImplementedError, match=word):
            _extractor(**kw).extract("show", 0, input_audio_filename="x.wav")
    fx = _extractor()
    for kw, word in ((dict(noise_file_name="n.wav"), "noise"), (dict(reverb_file_name="r.wav"), "reverb")):
        with pytest.raises(NotImplementedError, match=word):
            fx.extract_from_signal(sig, 16000, **kw)
        with pytest.raises(NotImplementedError, match=word):
            fx.extract("show", 0, input_audio_filename="x.wav", **kw)
    with pytest.raises(NotImplementedError, match="sph"):
        fx.extract("show", 0, input_audio_filename="{}.sph")
    with pytest.raises(NotImplementedError, match="save"):
        fx.save("show")
    with pytest.raises(NotImplementedError, match="save_list"):
        fx.save_list(["show"], [0])
    with pytest.raises(NotImplementedError, match="save_multispeakers"):
        fx.save_multispeakers(None)
    with pytest.raises(NotImplementedError, match="htk"):
        fe.hz2mel(100., htk=False)


def test_refusals_and_empty_results_that_need_no_gpu():
    fx = _extractor()
    label, energy, cep, fb = fx.extract_from_signal(numpy.zeros(399, dtype=numpy.float32), 16000)
    assert (label.shape, energy.shape, cep.shape, fb.shape) == ((0, 1), (0, 1), (0, 13), (0, 24)) and label.dtype == numpy.int8
    assert energy.dtype == cep.dtype == fb.dtype == numpy.float32
    short = _extractor(shift=1e-4, window_size=0.02)       # a shift of one sample: one part of the reference is 6 250 320 samples
    assert (short.shift_sample, short.window_sample) == (1, 320)
    with pytest.raises(ValueError, match="longer than one part"):
        short.extract_from_signal(numpy.zeros(6250321, dtype=numpy.float32), 16000)
    with pytest.raises(ValueError, match="lin"):
        _extractor(filter_bank="mel").extract_from_signal(numpy.zeros(16000, dtype=numpy.float32), 16000)


def test_without_a_gpu_the_compute_calls_raise(monkeypatch, tmp_path):
    import wave
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    sig = (numpy.arange(16000) % 200 - 100).astype(numpy.float32)
    keep = sig.copy()
    path = str(tmp_path / "a.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(16000)
        w.writeframes(sig.astype("<i2").tobytes())
    fx = _extractor()
    calls = (lambda: fe.mfcc(sig), lambda: fe.power_spectrum(sig, fs=16000), lambda: fx.extract_from_signal(sig, 16000),
             lambda: fx.extract("a", 0, input_audio_filename=path), lambda: fx.extract_batch_device(sig, None),
             lambda: features_extractor.mfcc_device(sig), lambda: features_extractor.to_device(sig))
    for call in calls:
        with pytest.raises(RuntimeError, match="no GPU is visible"):
            call()
    numpy.testing.assert_array_equal(sig, keep)


def test_package_wiring():
    assert "features_extractor" in sidekit_amd.SUBMODULES
    assert sidekit_amd._LAZY["FeaturesExtractor"] == "features_extractor" and sidekit_amd.FeaturesExtractor is FeaturesExtractor
    code = ("import sidekit_amd; sidekit_amd.install_as_sidekit(); from sidekit.features_extractor import FeaturesExtractor; "
            "from sidekit.frontend.features import mfcc, power_spectrum, trfbank; import sidekit; "
            "assert FeaturesExtractor is sidekit_amd.features_extractor.FeaturesExtractor is sidekit.FeaturesExtractor; "
            "assert mfcc is sidekit_amd.frontend.features.mfcc; "
            "sidekit.FeaturesServer(features_extractor=FeaturesExtractor(sampling_frequency=16000))")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
    code = ("import sys, sidekit_amd, sidekit_amd.features_extractor; sidekit_amd.FeaturesExtractor(); import sidekit_amd._lib as l; "
            "assert 'torch' not in sys.modules and l._lib is None")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
