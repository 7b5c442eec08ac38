"""Writes tests/golden/extractor.npz: what the REFERENCE's cepstral front end computes on synthetic signals -- ``trfbank``, ``mfcc``
(sidekit/frontend/features.py:226-305, :363-477), the energy labels and threshold of ``FeaturesExtractor._vad`` and, for one signal,
``FeaturesExtractor.extract_from_signal`` (sidekit/features_extractor.py) -- with the yardsticks the kernel is held to.

The reference's modules are imported with the package-shell recipe of make_vad_golden.py (no reference text is copied), with two more
shims: ``numpy.int`` (``trfbank`` uses the alias numpy 1.24 dropped) and a stand-in for ``sidekit.frontend.io``, whose file readers
``features_extractor`` imports and the calls made here never reach.

Four configurations (tests/tools/mfcc_f64.py CONFIGS), seven rows each: one sample short of a window, one window, one sample short of two
frames, two frames, five frames, 2.6 s of bursts of white noise and 2.6 s of the same kind passed through a moving average.  No signal
is stored: the tool regenerates them from the stored seeds.  Per configuration the file holds the bank, the float32 window and DCT
tables, the reference's outputs of every row with at least two frames (``power_spectrum`` cannot be called below two frames), and per
row and output the maximum deviation from the float64 evaluation (mfcc_f64) of (a) the reference's float32 outputs and (b) the CPU
single-precision route (mfcc_single): the two yardsticks.

Before writing, the generator asserts that the float64 evaluation reproduces the reference and the single-precision route within
3e-5 (16 ulp of a float32 between 16 and 32, the magnitude of the largest outputs; the yardsticks come out at 1e-6 to 1.3e-5), and
that no frame's standardised log-energy lies within 1e-3 of the VAD threshold in the reference alone (seeds are tried until one
satisfies that).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_extractor_golden.py
"""
import importlib
import os
import sys
import types
import warnings

import numpy

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

import make_vad_golden  # noqa: E402
import mfcc_f64 as mf  # noqa: E402

MARGIN = 1e-3
TOLERANCE = 3e-5
SURFACE = (0, 5)      # configuration and row whose extract_from_signal outputs are stored


def import_extractor_reference():
    features, vad, mixture = make_vad_golden.import_vad_reference()
    if not hasattr(numpy, "int"):
        numpy.int = int
    io = types.ModuleType("sidekit.frontend.io")
    for name in ("read_audio", "read_label", "write_hdf5", "_add_reverb", "_add_noise"):
        setattr(io, name, None)
    sys.modules["sidekit.frontend.io"] = io
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        extractor = importlib.import_module("sidekit.features_extractor")
    return features, mixture, extractor


def make_extractor(extractor, cfg, vad):
    lin = cfg["nlogfilt"] == 0
    return extractor.FeaturesExtractor(sampling_frequency=cfg["fs"], lower_frequency=cfg["lowfreq"], higher_frequency=cfg["maxfreq"],
                                       filter_bank="lin" if lin else "log", filter_bank_size=cfg["nlinfilt"] + cfg["nlogfilt"],
                                       window_size=cfg["nwin"], shift=cfg["shift"], ceps_number=cfg["nceps"], vad=vad, pre_emphasis=mf.PREFAC)


def reference_rows(cfg, rows, features, extractor):
    """Per row: the reference's mfcc outputs (None below two frames), labels, threshold and margin of its energy VAD"""
    fx = make_extractor(extractor, cfg, "energy")
    out = []
    for pcm in rows:
        sig = pcm.astype(numpy.float32)
        T = mf.n_frames(sig.shape[0], cfg)
        if T < 2:
            out.append(None)
            continue
        with numpy.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            cep, energy, _, fb = features.mfcc(sig, lowfreq=cfg["lowfreq"], maxfreq=cfg["maxfreq"], nlinfilt=cfg["nlinfilt"], nlogfilt=cfg["nlogfilt"],
                                               nwin=cfg["nwin"], fs=cfg["fs"], nceps=cfg["nceps"], shift=cfg["shift"], get_spec=False, get_mspec=True,
                                               prefac=mf.PREFAC)
            label, thr = fx._vad(cep, energy, fb, sig)
        assert cep.dtype == energy.dtype == fb.dtype == numpy.float32 and energy.shape == (T,)
        label = numpy.asarray(label, dtype=bool)
        margin = numpy.inf
        if numpy.isfinite(thr) and label.any():
            le = energy.astype(numpy.float64)
            margin = numpy.abs((le - numpy.mean(le)) / numpy.std(le) - thr).min()
        out.append(dict(energy=energy, fb=fb, cep=cep, label=label, thr=float(thr), margin=float(margin)))
    return out


def main():
    features, mixture, extractor = import_extractor_reference()
    fx = {"margin": MARGIN, "prefac": mf.PREFAC}
    for c, cfg in enumerate(mf.CONFIGS):
        window, shift, n_fft = mf.frame_shape(cfg)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            bank, freqs = features.trfbank(cfg["fs"], n_fft, cfg["lowfreq"], cfg["maxfreq"], cfg["nlinfilt"], cfg["nlogfilt"])
        assert bank.dtype == numpy.float32 and bank.shape == (cfg["nlinfilt"] + cfg["nlogfilt"], n_fft // 2 + 1)
        for seed in range(300 + 100 * c, 400 + 100 * c):
            rows = mf.signals(cfg, seed)
            ref = reference_rows(cfg, rows, features, extractor)
            worst = min(r["margin"] for r in ref if r is not None)
            if worst >= MARGIN:
                break
        else:
            raise SystemExit("no seed keeps every frame away from its threshold")
        print(f"config {c}: window {window}, shift {shift}, n_fft {n_fft}, seed {seed}, smallest |z - threshold| = {worst:.3e}")
        fx[f"c{c}_seed"] = seed
        fx[f"c{c}_bank"] = bank
        fx[f"c{c}_frequences"] = numpy.asarray(freqs)
        fx[f"c{c}_window"] = numpy.hanning(window).astype(numpy.float32)
        dct = features.dct_basis(cfg["nceps"] + 1, bank.shape[0])[1:]
        assert numpy.abs(dct - mf.dct_f64(cfg["nceps"], bank.shape[0])).max() < 1e-14, "the reference's dct_basis is the matrix of the float64 evaluation"
        # where the basis is exactly zero the reference's FFT leaves a residue of 1e-17, which is not kept
        fx[f"c{c}_dct"] = numpy.where(numpy.abs(dct) < 1e-15, 0.0, dct).astype(numpy.float32)
        yard_ref, yard_single = numpy.zeros((len(rows), 4)), numpy.zeros((len(rows), 4))
        for r, pcm in enumerate(rows):
            sig = pcm.astype(numpy.float32)
            want = mf.mfcc_f64(sig, cfg, bank)
            assert want[0].shape[0] == mf.n_frames(sig.shape[0], cfg)
            yard_single[r] = mf.deviations(mf.mfcc_single(sig, cfg, bank), want)
            if ref[r] is not None:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    spec = features.power_spectrum(sig, fs=cfg["fs"], win_time=cfg["nwin"], shift=cfg["shift"], prefac=mf.PREFAC)[0]
                yard_ref[r] = mf.deviations((ref[r]["energy"], ref[r]["fb"], ref[r]["cep"], spec), want)
                assert yard_ref[r].max() < TOLERANCE, (c, r, yard_ref[r])
                for name in ("energy", "fb", "cep", "label"):
                    fx[f"c{c}_r{r}_{name}"] = ref[r][name]
                fx[f"c{c}_r{r}_thr"] = ref[r]["thr"]
            assert yard_single[r].max() < TOLERANCE, (c, r, yard_single[r])
            print(f"  row {r} ({mf.ROWS[r]}): {sig.shape[0]} samples, {want[0].shape[0]} frames; energy / fb / cep / spec deviation from float64: "
                  f"reference {yard_ref[r]}, single precision {yard_single[r]}" + ("" if ref[r] is None else
                  f"; threshold {ref[r]['thr']:.4f}, {int(ref[r]['label'].sum())} speech frames"))
        fx[f"c{c}_yard_reference"] = yard_ref
        fx[f"c{c}_yard_single"] = yard_single
    # extract_from_signal of the reference on one signal: it dithers a float32 copy in place and cuts it into parts itself
    c, r = SURFACE
    cfg = mf.CONFIGS[c]
    sig = mf.signals(cfg, int(fx[f"c{c}_seed"]))[r].astype(numpy.float32)
    for vad in (None, "energy"):
        with numpy.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            label, energy, cep, fb = make_extractor(extractor, cfg, vad).extract_from_signal(sig.copy(), cfg["fs"])
        tag = "energy" if vad else "none"
        fx[f"surface_{tag}_label"] = numpy.asarray(label, dtype=bool)
        if vad is None:
            fx["surface_energy"], fx["surface_cep"], fx["surface_fb"] = energy, cep, fb
            dithered = sig.copy()
            numpy.random.seed(0)
            dithered += 0.0001 * numpy.random.randn(dithered.shape[0])
            want = mf.mfcc_f64(dithered, cfg, fx[f"c{c}_bank"])
            fx["surface_yard_reference"] = numpy.array(mf.deviations((energy, fb, cep, None), want))
            print("extract_from_signal: deviation of the reference from float64 on the dithered signal", fx["surface_yard_reference"])
    path = os.path.join(HERE, "extractor.npz")
    numpy.savez_compressed(path, **fx)
    print("extractor.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
