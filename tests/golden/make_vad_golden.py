"""Writes tests/golden/vad.npz: synthetic PCM16 utterances and what the REFERENCE computes on them -- ``power_spectrum``'s log-energy
(sidekit/frontend/features.py:363-389), ``vad_energy`` (sidekit/mixture.py:67-113) at the parameters ``FeaturesExtractor._vad`` passes
(flooring 0.0001, ceiling 1.5, alpha 0.2) and at the function's defaults, and scipy's grey closing then opening (what ``label_fusion``
applies, sidekit/frontend/vad.py:409-428) of those labels.

The reference's modules are imported with the package-shell recipe of make_golden.py (no reference text is copied).  The rows are the
smallest shapes at which the kernels can go wrong: fewer than one window of samples, exactly one frame, two frames, 1 s, 4 s plus a tail that
is no multiple of the shift, 11 s (more frames than a workgroup has threads) and a constant signal.  ``power_spectrum`` itself cannot be
called below two frames (its ``framing`` squeezes a single frame to one dimension and is undefined below one window); the one-frame row's
log-energy comes from the reference's ``pre_emphasis`` on that frame.

Before writing, the generator asserts that no frame of any utterance with a finite threshold has |z - threshold| < 1e-6 (seeds are tried
until the reference alone satisfies that), and that the tests' numpy restatement (tests/tools/vad_numpy.py) agrees with the reference.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_vad_golden.py
"""
import importlib
import os
import sys
import types
import warnings

import numpy
import scipy.ndimage

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

import make_golden  # noqa: E402
import vad_numpy as vn  # noqa: E402

LENGTHS = (300, 400, 560, 16000, 64077, 176033, 8000)      # the last row is constant
PARAMS = {"fx": dict(flooring=0.0001, ceiling=1.5, alpha=0.2), "default": {}}
MARGIN = 1e-6


def import_vad_reference():
    make_golden.import_reference()
    fe = types.ModuleType("sidekit.frontend")          # a shell: the package's own __init__ pulls in the file readers
    fe.__path__ = [os.path.join(make_golden.REF, "sidekit", "frontend")]
    sys.modules["sidekit.frontend"] = fe
    if not hasattr(numpy.lib, "pad"):                  # numpy >= 2 dropped the alias `framing` calls
        numpy.lib.pad = numpy.pad
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return (importlib.import_module("sidekit.frontend.features"), importlib.import_module("sidekit.frontend.vad"),
                importlib.import_module("sidekit.mixture"))


def synth(seed):
    """Bursts of loud noise between stretches of faint noise, as int16; the last row is a constant."""
    rs = numpy.random.RandomState(seed)
    rows = []
    for n in LENGTHS[:-1]:
        x, pos, loud = numpy.zeros(n), 0, bool(rs.randint(2))
        while pos < n:
            d = int(rs.uniform(0.08, 0.5) * 16000)
            amp = rs.uniform(1500, 9000) if loud else rs.uniform(15, 60)
            seg = rs.randn(min(d, n - pos)) * amp * (0.6 + 0.4 * numpy.sin(numpy.arange(min(d, n - pos)) / rs.uniform(300, 900)))
            x[pos:pos + d] = seg
            pos, loud = pos + d, not loud
        rows.append(numpy.clip(numpy.round(x), -32768, 32767).astype(numpy.int16))
    rows.append(numpy.full(LENGTHS[-1], 1234, dtype=numpy.int16))
    return rows


def reference_outputs(rows, features, vad, mixture):
    out = {"le": [], "nframes": []}
    for tag in PARAMS:
        out.update({f"label_{tag}": [], f"thr_{tag}": [], f"fused_{tag}": [], f"margin_{tag}": []})
    for pcm in rows:
        sig = pcm.astype(numpy.float64) / 32768.0
        nf = vn.n_frames(sig.shape[0])
        if nf >= 2:
            _, le = features.power_spectrum(sig, fs=16000, win_time=0.025, shift=0.01, prefac=0.97)
        elif nf == 1:
            le = numpy.log((vad.pre_emphasis(sig[:vn.NWIN], 0.97) ** 2).sum())[None]
        else:
            le = numpy.zeros(0)
        assert le.shape == (nf,) and le.dtype == numpy.float64
        out["le"].append(le)
        out["nframes"].append(nf)
        for tag, kw in PARAMS.items():
            if nf == 0:
                label, thr = numpy.zeros(0, dtype=bool), numpy.nan
            else:
                with numpy.errstate(all="ignore"), warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    label, thr = mixture.vad_energy(le, distrib_nb=3, nb_train_it=8, **kw)
            label = numpy.asarray(label, dtype=bool)
            u8 = label.astype(numpy.uint8)
            fused = scipy.ndimage.grey_opening(scipy.ndimage.grey_closing(u8, size=3), size=3).astype(bool) if nf else label
            if nf and nf != 2:     # label_fusion reads a two-row input as two channels: only the scipy calls are pinned for two frames
                assert numpy.array_equal(numpy.asarray(vad.label_fusion(label[None, :].copy(), 3)[0], dtype=bool), fused)
            margin = numpy.inf
            if numpy.isfinite(thr):
                z = (le - numpy.mean(le)) / numpy.std(le)
                margin = numpy.abs(z - thr).min()
            out[f"label_{tag}"].append(label)
            out[f"thr_{tag}"].append(float(thr))
            out[f"fused_{tag}"].append(fused)
            out[f"margin_{tag}"].append(margin)
    return out


def main():
    features, vad, mixture = import_vad_reference()
    for seed in range(100, 200):
        rows = synth(seed)
        ref = reference_outputs(rows, features, vad, mixture)
        worst = min(min(ref[f"margin_{tag}"]) for tag in PARAMS)
        print(f"seed {seed}: smallest |z - threshold| = {worst:.3e}")
        if worst >= MARGIN:
            break
    else:
        raise SystemExit("no seed keeps every frame away from its threshold")
    # the restatement against the reference
    for r, pcm in enumerate(rows):
        le = vn.frame_log_energy(pcm)
        assert le.shape == ref["le"][r].shape
        if le.size:
            assert numpy.abs(le - ref["le"][r]).max() <= 1e-12, (r, numpy.abs(le - ref["le"][r]).max())
        for tag, kw in PARAMS.items():
            thr_ref, lab_ref = ref[f"thr_{tag}"][r], ref[f"label_{tag}"][r]
            label, thr, _ = vn.vad_energy(ref["le"][r], **kw)
            if numpy.isfinite(thr_ref) and lab_ref.any():
                assert numpy.array_equal(label, lab_ref), (r, tag)
                assert abs(thr - thr_ref) <= 1e-9 * abs(thr_ref), (r, tag, thr, thr_ref)
                assert numpy.array_equal(vn.label_fusion(lab_ref, 3), ref[f"fused_{tag}"][r]), (r, tag)
            else:
                assert numpy.isnan(thr) and label.all(), (r, tag)
        print(f"row {r}: {pcm.shape[0]} samples, {ref['nframes'][r]} frames, thresholds",
              {tag: ref[f"thr_{tag}"][r] for tag in PARAMS}, "speech frames", {tag: int(ref[f"label_{tag}"][r].sum()) for tag in PARAMS})
    fx = {"seed": seed, "lengths": numpy.array([p.shape[0] for p in rows], dtype=numpy.int32), "pcm16": numpy.concatenate(rows),
          "nframes": numpy.array(ref["nframes"], dtype=numpy.int32), "le": numpy.concatenate(ref["le"]), "nwin": vn.NWIN, "shift": vn.SHIFT,
          "prefac": vn.PREFAC, "margin": MARGIN}
    for tag, kw in PARAMS.items():
        fx[f"label_{tag}"] = numpy.concatenate(ref[f"label_{tag}"])
        fx[f"fused_{tag}"] = numpy.concatenate(ref[f"fused_{tag}"])
        fx[f"thr_{tag}"] = numpy.array(ref[f"thr_{tag}"])
        fx[f"params_{tag}"] = numpy.array([kw.get("flooring", 0.0001), kw.get("ceiling", 1.0), kw.get("alpha", 2.0)])
    path = os.path.join(HERE, "vad.npz")
    numpy.savez_compressed(path, **fx)
    print("vad.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
