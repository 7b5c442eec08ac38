"""What the cepstral front end costs (GPU box):

    python scripts/mfcc_bench.py --out profiles/mfcc_bench.json

Workload: int16 noise bursts at 16 kHz (``RandomState(9)``), 1 024 utterances of 10 s and one utterance of 10 s, the first
configuration of the tests (25 ms window, 10 ms shift, 24 mel filters on 100-8000 Hz, 13 cepstra: 998 frames an utterance, 38 floats a
frame).  Measured, each after WARMUP calls as the median of REPS windows of CALLS calls between two device events (``spread`` = max -
min of the windows):
  * ``sc_mfcc`` alone through ``mfcc_device`` (tables cached; the call includes the torch integer ops that make the row offsets and
    the one read-back of the row count), with and without the spectrum, for int16 and float32 samples;
  * comparator (a): the same formulas written with torch on the same card -- ``unfold``, ``torch.fft.rfft``, two matmuls -- in chunks
    of 128 utterances (the unfolded frames of all 1 024 would take 1.6 GB), with its largest difference from the kernel's result;
  * comparator (b): the float64 numpy restatement of the tests (tests/tools/mfcc_f64.py) on the host for ONE utterance, and the kernel
    on that utterance alone;
  * accuracy: the kernel's maximum deviation from the float64 evaluation per configuration and output on the rows of the tests, with
    the bound the tests hold it to (4 x the larger CPU yardstick of tests/golden/extractor.npz).
Counted from the shapes, not from hardware counters: the bytes a frame needs at least (its ``shift`` new samples in, 1 + nceps + nfilt
floats out) and the bytes the kernel asks for (every sample of the window once per frame, the same floats out); how many of the
overlapping reads the caches absorb is not measured.
Fails without a GPU; nothing is a ratio fixed in advance.
"""
import argparse
import json
import os
import sys
import time

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

UTTERANCES, SECONDS, CHUNK = 1024, 10, 128
WARMUP, REPS, CALLS = 2, 7, 3


def median(v):
    s = sorted(v)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def measure(torch, fn, calls=CALLS, reps=REPS):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return {"median_ms": median(ms), "spread_ms": max(ms) - min(ms), "ms": ms}


def torch_route(torch, wav, tables, window_length, shift, n_fft, prefac, nceps):
    """energy | cep | fb of every frame of a (B, L) batch of full rows, plain torch in float32"""
    window, bank, dct = tables
    out = []
    for r0 in range(0, wav.shape[0], CHUNK):
        x = wav[r0:r0 + CHUNK].float().unfold(1, window_length, shift)
        y = x - prefac * torch.cat((x[..., :1], x[..., :-1]), dim=-1)
        X = torch.fft.rfft(y * window, n_fft)
        fb = torch.log((X.real ** 2 + X.imag ** 2) @ bank.T)
        out.append(torch.cat((torch.log((y * y).sum(-1, keepdim=True)), fb @ dct.T, fb), dim=-1).reshape(-1, 1 + nceps + bank.shape[0]))
    return torch.cat(out)


def accuracy(torch, dev):
    import mfcc_f64 as mf
    from sidekit_amd.features_extractor import mfcc_device
    golden = numpy.load(os.path.join(ROOT, "tests", "golden", "extractor.npz"))
    res = {}
    for c, cfg in enumerate(mf.CONFIGS):
        rows = mf.signals(cfg, int(golden[f"c{c}_seed"]))
        worst = numpy.zeros(4)
        for pcm in rows:
            want = mf.mfcc_f64(pcm.astype(numpy.float32), cfg, golden[f"c{c}_bank"])
            if want[0].shape[0] == 0:
                continue
            opts = {k: cfg[k] for k in ("fs", "lowfreq", "maxfreq", "nlinfilt", "nlogfilt", "nwin", "nceps", "shift")}
            frames, _, spec = mfcc_device(torch.from_numpy(pcm).to(dev), None, prefac=mf.PREFAC, get_spec=True, **opts)
            f, nc = frames.cpu().numpy(), cfg["nceps"]
            worst = numpy.maximum(worst, mf.deviations((f[:, 0], f[:, 1 + nc:], f[:, 1:1 + nc], spec.cpu().numpy()), want))
        yard = numpy.maximum(golden[f"c{c}_yard_reference"].max(axis=0), golden[f"c{c}_yard_single"].max(axis=0))
        res[f"configuration {c}"] = {"config": cfg, "max_deviation": dict(zip(("energy", "fb", "cep", "spectrum_relative"), worst.tolist())),
                                     "bound_4x_yardstick": dict(zip(("energy", "fb", "cep", "spectrum_relative"), (4 * yard).tolist()))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mfcc_bench.json"))
    ap.add_argument("--utterances", type=int, default=UTTERANCES)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mfcc_bench.py measures on the GPU only: no GPU is visible")
    import mfcc_f64 as mf
    from sidekit_amd import features_extractor as fx
    dev = torch.device("cuda", 0)
    cfg = mf.CONFIGS[0]
    window_length, shift, n_fft = mf.frame_shape(cfg)
    nfilt, nceps, L = cfg["nlogfilt"], cfg["nceps"], SECONDS * cfg["fs"]
    D, T = 1 + nceps + nfilt, mf.n_frames(L, cfg)
    rs = numpy.random.RandomState(9)
    host = numpy.clip(numpy.round(rs.standard_normal((args.utterances, L)).astype(numpy.float32) * rs.uniform(20, 6000, (args.utterances, 1))),
                      -32768, 32767).astype(numpy.int16)
    pcm = torch.from_numpy(host).to(dev)
    flt = pcm.float()
    opts = {k: cfg[k] for k in ("fs", "lowfreq", "maxfreq", "nlinfilt", "nlogfilt", "nwin", "nceps", "shift")}
    opts["prefac"] = mf.PREFAC
    window, bank, _, _, dct = (torch.from_numpy(t).to(dev) for t in fx.host_tables(cfg["fs"], n_fft, window_length, cfg["lowfreq"], cfg["maxfreq"], 0,
                                                                                    nfilt, nceps))
    res = {"workload": {"utterances": args.utterances, "seconds": SECONDS, "sampling_frequency": cfg["fs"], "frames_per_utterance": T,
                        "floats_per_frame": D, "config": cfg},
           "protocol": {"warmup_calls": WARMUP, "windows": REPS, "calls_per_window": CALLS, "timer": "device events around the calls of a window"},
           "device": torch.cuda.get_device_name(0), "sc_mfcc": {}, "torch_same_card": {}, "numpy_one_utterance": {},
           "bytes_per_frame_counted_from_shapes": {
               "minimum_int16": shift * 2 + D * 4, "minimum_float32": shift * 4 + D * 4,
               "asked_for_by_the_kernel_int16": window_length * 2 + D * 4, "asked_for_by_the_kernel_float32": window_length * 4 + D * 4,
               "with_the_spectrum_add": (n_fft // 2 + 1) * 4, "hardware_counters": "not measured"}}
    for name, wav, B, spec in (("1024 x 10 s int16", pcm, args.utterances, False), ("1024 x 10 s float32", flt, args.utterances, False),
                               ("1024 x 10 s int16 with the spectrum", pcm, args.utterances, True), ("1 x 10 s int16", pcm[:1], 1, False)):
        m = measure(torch, lambda wav=wav, spec=spec: fx.mfcc_device(wav, None, get_spec=spec, **opts))
        m["frames"] = B * T
        m["frames_per_s"] = B * T / m["median_ms"] * 1e3
        m["times_real_time"] = B * SECONDS / m["median_ms"] * 1e3
        m["minimum_bytes_per_s"] = m["frames_per_s"] * ((shift * (2 if wav.dtype == torch.int16 else 4)) + D * 4)
        res["sc_mfcc"][name] = m
        print(name, f"{m['median_ms']:.3f} ms (spread {m['spread_ms']:.3f}), {m['frames_per_s']:.3e} frames/s", flush=True)
    ours = fx.mfcc_device(pcm, None, **opts)[0]
    for name, wav in (("1024 x 10 s", pcm), ("1 x 10 s", pcm[:1])):
        m = measure(torch, lambda wav=wav: torch_route(torch, wav, (window, bank, dct), window_length, shift, n_fft, mf.PREFAC, nceps), calls=1, reps=5)
        theirs = torch_route(torch, wav, (window, bank, dct), window_length, shift, n_fft, mf.PREFAC, nceps)
        key = name.replace(" s", " s int16")
        m["max_abs_difference_from_the_kernel"] = float((ours[:theirs.shape[0]] - theirs).abs().max())
        m["kernel_median_ms"] = res["sc_mfcc"][key]["median_ms"]
        m["torch_over_kernel"] = m["median_ms"] / m["kernel_median_ms"]
        res["torch_same_card"][name] = m
        print("torch", name, f"{m['median_ms']:.3f} ms, {m['torch_over_kernel']:.2f} x the kernel", flush=True)
    t0 = time.perf_counter()
    want = mf.mfcc_f64(host[0].astype(numpy.float32), cfg, bank.cpu().numpy())
    host_s = time.perf_counter() - t0
    got = ours[:T].cpu().numpy()
    res["numpy_one_utterance"] = {"frames": T, "numpy_float64_s": host_s, "kernel_median_ms": res["sc_mfcc"]["1 x 10 s int16"]["median_ms"],
                                  "numpy_over_kernel": host_s * 1e3 / res["sc_mfcc"]["1 x 10 s int16"]["median_ms"],
                                  "max_abs_difference": float(max(numpy.abs(got[:, 0] - want[0]).max(), numpy.abs(got[:, 1 + nceps:] - want[1]).max(),
                                                                  numpy.abs(got[:, 1:1 + nceps] - want[2]).max()))}
    print("numpy", f"{host_s * 1e3:.1f} ms against {res['numpy_one_utterance']['kernel_median_ms']:.3f} ms", flush=True)
    res["accuracy"] = accuracy(torch, dev)
    for k, v in res["accuracy"].items():
        print(k, v["max_deviation"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
