"""Writes tests/golden/plp.npz: what the REFERENCE's PLP front end computes on synthetic signals -- ``fft2barkmx``, ``postaud``'s
equal-loudness weights, ``plp`` (sidekit/frontend/features.py:480-522, :647-691, :888-966) and, for one signal,
``FeaturesExtractor(feature_type='plp').extract_from_signal`` with its energy labels -- with the yardsticks the GPU chain is held to.

The reference's modules are imported with the recipes of make_vad_golden.py and make_extractor_golden.py (no reference text is
copied).  One more repair is needed: the reference's ``plp(..., rasta=True)`` calls ``rasta_filt``, which its features module never
imports, and stops with ``NameError``.  This script sets ``rasta_filt`` on the imported features module to
``sidekit.frontend.normfeat.rasta_filt``, the only function of that name in the reference.

Four configurations (tests/tools/plp_f64.py CONFIGS: 16 kHz and 8 kHz, each without and with RASTA; 13 cepstra at 16 kHz, the largest
allowed, 16, at 8 kHz), seven rows each with the frame counts of tests/tools/mfcc_f64.py (0, 1, 1, 2, 5 and two of about 258).  No
signal is stored: the tool regenerates them from the stored seeds.  The reference is given the samples as float64, so everything it
returns is float64 (its power spectrum alone is rounded to float32 on the way).  Per sampling frequency the file holds the bark bank
and the equal-loudness weights; per configuration and row with at least two frames (``power_spectrum`` cannot be called below two) the
reference's cepstra, ``post_spectrum`` and log-energy, and ``logband``: the log critical-band energies as they enter the exponential,
after ``rasta_filt`` where the configuration has it, obtained by calling the functions ``plp`` calls on the same signal.  ``logband`` is
the operand on which the two float64 evaluations -- the reference's and tests/tools/plp_f64.py's restatement of the kernel's formulas
-- are compared; the largest deviation is printed and stored (``float64_deviation``), and tests/test_plp_reference_cpu.py bounds it.
Per row and output the file records the maximum deviation from the float64 evaluation of the whole chain on the float32 signal
(plp_f64.plp_f64) of (a) the reference's outputs rounded to float32 and (b) the CPU route with a single-precision head
(plp_f64.plp_single): the two yardsticks.

The seed of the 16 kHz rows is searched so that no frame's standardised log-energy lies within 1e-3 of the energy VAD's threshold for
the dithered signal whose ``extract_from_signal`` outputs are stored.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_plp_golden.py
"""
import importlib
import os
import sys
import warnings

import numpy

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

import make_extractor_golden  # noqa: E402
import plp_f64 as pf  # noqa: E402

MARGIN = 1e-3
TOLERANCE = 3e-5      # as make_extractor_golden.py: no yardstick may be wider
SURFACE = (1, 5)      # configuration (16 kHz, RASTA) and row whose extract_from_signal outputs are stored
FIRST_SEED = {16000: 700, 8000: 800}


def import_plp_reference():
    features, mixture, extractor = make_extractor_golden.import_extractor_reference()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        normfeat = importlib.import_module("sidekit.frontend.normfeat")
    features.rasta_filt = normfeat.rasta_filt          # the import the reference's features module lacks
    return features, normfeat, extractor


def make_extractor(extractor, cfg, vad):
    return extractor.FeaturesExtractor(sampling_frequency=cfg["fs"], window_size=cfg["nwin"], shift=cfg["shift"], ceps_number=cfg["nceps"], vad=vad,
                                       pre_emphasis=pf.PREFAC, feature_type="plp", rasta_plp=cfg["rasta"])


def reference_row(features, normfeat, cfg, sig):
    """``plp`` on a float64 signal and the operand of its tail -> dict, or None below two frames"""
    if pf.mf.n_frames(sig.shape[0], pf.head_cfg(cfg)) < 2:
        return None
    with numpy.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cep, energy, _, post = features.plp(sig, nwin=cfg["nwin"], fs=cfg["fs"], plp_order=cfg["nceps"], shift=cfg["shift"], get_spec=False,
                                            get_mspec=True, prefac=pf.PREFAC, rasta=cfg["rasta"])
        spec = features.power_spectrum(sig, cfg["fs"], cfg["nwin"], cfg["shift"], pf.PREFAC)[0]
        logband = numpy.log(features.audspec(spec, cfg["fs"])[0])
        if cfg["rasta"]:
            logband = normfeat.rasta_filt(logband)
    assert cep.dtype == energy.dtype == post.dtype == logband.dtype == numpy.float64
    return dict(cep=cep, energy=energy, post=post, logband=logband)


def surface(features, extractor, cfg, pcm, bank32, eql):
    """``extract_from_signal`` of the reference on one float32 signal (it dithers a copy in place) without and with the energy VAD ->
    (dict of arrays, smallest |z - threshold|)"""
    out, sig = {}, pcm.astype(numpy.float32)
    for vad in (None, "energy"):
        fx = make_extractor(extractor, cfg, vad)
        with numpy.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            label, energy, cep, fb = fx.extract_from_signal(sig.copy(), cfg["fs"])
        out["surface_{}_label".format(vad or "none")] = numpy.asarray(label, dtype=bool)
    out["surface_energy"], out["surface_cep"], out["surface_post"] = energy, cep, fb
    with numpy.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        label, thr = fx._vad(cep, energy, fb, sig)
    assert numpy.array_equal(numpy.asarray(label, dtype=bool), out["surface_energy_label"]) and numpy.isfinite(thr) and label.any()
    le = energy.astype(numpy.float64)
    margin = float(numpy.abs((le - numpy.mean(le)) / numpy.std(le) - thr).min())
    dithered = sig.copy()
    numpy.random.seed(0)
    dithered += 0.0001 * numpy.random.randn(dithered.shape[0])
    out["surface_yard_reference"] = numpy.array(pf.deviations((energy, cep, fb), pf.plp_f64(dithered, cfg, bank32, eql)))
    return out, margin


def main():
    features, normfeat, extractor = import_plp_reference()
    fx = {"margin": MARGIN, "prefac": pf.PREFAC}
    tables, seeds = {}, {}
    for fs in (16000, 8000):
        cfg = next(c for c in pf.CONFIGS if c["fs"] == fs)
        window, shift, n_fft = pf.mf.frame_shape(pf.head_cfg(cfg))
        nb = pf.bands(cfg)
        bank = features.fft2barkmx(n_fft, fs, nb, 1., 0., min(8000, fs / 2))[:, :n_fft // 2 + 1]
        eql = features.postaud(numpy.ones((1, nb)), fs / 2.)[1]
        assert bank.shape == (nb, n_fft // 2 + 1) and eql.shape == (nb,) and bank.dtype == eql.dtype == numpy.float64
        fx[f"fs{fs}_bank"], fx[f"fs{fs}_eql"] = bank, eql
        tables[fs] = (bank.astype(numpy.float32), eql)
        seeds[fs] = FIRST_SEED[fs]
    # the rows of the sampling frequency whose extract_from_signal outputs are stored: the first seed that keeps the detector decided
    cfg = pf.CONFIGS[SURFACE[0]]
    for seed in range(FIRST_SEED[cfg["fs"]], FIRST_SEED[cfg["fs"]] + 100):
        got, margin = surface(features, extractor, cfg, pf.signals(cfg, seed)[SURFACE[1]], *tables[cfg["fs"]])
        if margin >= MARGIN:
            break
    else:
        raise SystemExit("no seed keeps every frame away from its threshold")
    fx.update(got)
    seeds[cfg["fs"]] = seed
    print(f"extract_from_signal at seed {seed}: smallest |z - threshold| = {margin:.3e}; energy / cep / post deviation of the reference from float64 "
          f"on the dithered signal {got['surface_yard_reference']}")
    worst64 = 0.0
    for c, cfg in enumerate(pf.CONFIGS):
        bank32, eql = tables[cfg["fs"]]
        nb, nceps = pf.bands(cfg), cfg["nceps"]
        acw, lift = pf.acw_f64(nb, nceps - 1), pf.lift_f64(nceps)
        rows = pf.signals(cfg, seeds[cfg["fs"]])
        fx[f"c{c}_seed"] = seeds[cfg["fs"]]
        yard_ref, yard_single = numpy.zeros((len(rows), 3)), numpy.zeros((len(rows), 3))
        print(f"config {c}: fs {cfg['fs']}, {nb} bands, {nceps} cepstra, rasta {cfg['rasta']}, seed {seeds[cfg['fs']]}")
        for r, pcm in enumerate(rows):
            sig = pcm.astype(numpy.float32)
            want = pf.plp_f64(sig, cfg, bank32, eql)
            assert want[0].shape[0] == pf.mf.n_frames(sig.shape[0], pf.head_cfg(cfg))
            yard_single[r] = pf.deviations(pf.plp_single(sig, cfg, bank32, eql), want)
            assert yard_single[r].max() < TOLERANCE, (c, r, yard_single[r])
            ref = reference_row(features, normfeat, cfg, pcm.astype(numpy.float64))
            dev64 = [0.0, 0.0]
            if ref is not None:
                assert all(numpy.isfinite(v).all() for v in ref.values())
                cep, y = pf.plp_cepstra_f64(ref["logband"], eql, acw, lift)
                dev64 = [float(numpy.abs(cep - ref["cep"]).max()), float((numpy.abs(y - ref["post"]).max(axis=1) / ref["post"].max(axis=1)).max())]
                worst64 = max(worst64, *dev64)
                yard_ref[r] = pf.deviations(tuple(ref[k].astype(numpy.float32) for k in ("energy", "cep", "post")), want)
                assert yard_ref[r].max() < TOLERANCE, (c, r, yard_ref[r])
                for name, value in ref.items():
                    fx[f"c{c}_r{r}_{name}"] = value
            print(f"  row {r} ({pf.ROWS[r]}): {want[0].shape[0]} frames; energy / cep / post deviation from float64: reference {yard_ref[r]}, "
                  f"single-precision head {yard_single[r]}; the two float64 evaluations on the reference's operands: cep {dev64[0]:.3e}, post {dev64[1]:.3e}")
        fx[f"c{c}_yard_reference"] = yard_ref
        fx[f"c{c}_yard_single"] = yard_single
    fx["float64_deviation"] = worst64
    print(f"largest deviation between the two float64 evaluations: {worst64:.3e}")
    path = os.path.join(HERE, "plp.npz")
    numpy.savez_compressed(path, **fx)
    print("plp.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
