"""What the PLP front end costs (GPU box):

    python scripts/plp_bench.py --out profiles/plp_bench.json

Workload: the one of scripts/mfcc_bench.py -- int16 noise bursts at 16 kHz (``RandomState(9)``), 1 024 utterances of 10 s, 25 ms window,
10 ms shift, 998 frames an utterance -- through the PLP chain with 13 cepstra and 21 critical bands, with RASTA and without.
Measured, each after WARMUP calls as the median of REPS windows of CALLS calls between two device events (``spread`` = max - min of
the windows), on buffers allocated once:
  * each of the three launches alone: ``sc_mfcc`` under the bark bank, ``sc_feat_rasta``, ``sc_plp_cepstra`` (on the filtered and on
    the unfiltered log energies), and their sums; ``sc_mfcc`` under the 24 mel triangles of mfcc_bench.py for comparison (a bark band
    is non-zero over almost the whole spectrum in float32, a triangle over a few bins); the share ``sc_plp_cepstra`` adds to ``sc_mfcc``;
  * ``plp_device`` as a user calls it (the launches, the allocations, the row offsets, the copy of the log-energy column);
  * a float64 torch route for the tail on the same card, from the same float32 log energies: ``exp``, ``pow``, the cosine matmul, the
    Levinson steps and the cepstrum recursion vectorised over frames, with its largest difference from the kernel; and the float64
    bank matmul from the float32 power spectrum, which a torch route without ``sc_mfcc`` would need as well (128 utterances at a time).
Counted from the shapes, not from hardware counters: the bytes ``sc_plp_cepstra`` moves per frame and the float64 operations of its
loops.  Fails without a GPU; no threshold is set in advance.
"""
import argparse
import json
import os
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

UTTERANCES, SECONDS, FS, NCEPS, CHUNK = 1024, 10, 16000, 13, 128
NWIN, SHIFT, PREFAC = 0.025, 0.01, 0.97
WARMUP, REPS, CALLS = 2, 7, 5


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


def torch_tail(torch, logband, eql, acw, lift):
    """The formulas of include/sidekit_amd/plp.h in float64 torch, frames vectorised -> cep (N, order + 1)"""
    order = acw.shape[0] - 1
    z = (eql * torch.exp(logband.double())) ** 0.33
    y = torch.cat((z[:, 1:2], z[:, 1:-1], z[:, -2:-1]), dim=1)
    r = y @ acw.T
    A = torch.zeros((r.shape[0], order), dtype=torch.float64, device=r.device)
    P = r[:, 0].clone()
    for k in range(order):
        s = r[:, k + 1] + (A[:, :k] * r[:, 1:k + 1].flip(1)).sum(1)
        t = -s / P
        P = P * (1.0 - t * t)
        A[:, :k] = A[:, :k] + t[:, None] * A[:, :k].flip(1)
        A[:, k] = t
    c = torch.zeros((r.shape[0], order + 1), dtype=torch.float64, device=r.device)
    c[:, 0] = torch.log(P)
    for n in range(1, order + 1):
        m = torch.arange(1, n, device=r.device)
        c[:, n] = -(A[:, n - 1] + (((n - m) * A[:, :n - 1]) * c[:, 1:n].flip(1)).sum(1) / n)
    return (c * lift).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plp_bench.json"))
    ap.add_argument("--utterances", type=int, default=UTTERANCES)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("plp_bench.py measures on the GPU only: no GPU is visible")
    from sidekit_amd import _lib, features_extractor as fx, plp
    from sidekit_amd.frontend.features import frame_shape
    dev = torch.device("cuda", 0)
    B, L = args.utterances, SECONDS * FS
    window_length, shift, n_fft = frame_shape(FS, NWIN, SHIFT)
    T = (L - window_length) // shift + 1
    N, nb, order = B * T, plp.bark_bands(FS), NCEPS - 1
    D = 1 + NCEPS + nb
    rs = numpy.random.RandomState(9)
    host = numpy.clip(numpy.round(rs.standard_normal((B, L)).astype(numpy.float32) * rs.uniform(20, 6000, (B, 1))), -32768, 32767).astype(numpy.int16)
    pcm = torch.from_numpy(host).to(dev)
    window, bank, lo, hi, eql, acw, lift = (torch.from_numpy(t).to(dev) for t in plp.plp_tables(FS, n_fft, window_length, NCEPS))
    dct = torch.zeros((1, nb), dtype=torch.float32, device=dev)
    mel = [torch.from_numpy(t).to(dev) for t in fx.host_tables(FS, n_fft, window_length, 100, 8000, 0, 24, 13)]
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    off = (torch.arange(B + 1, dtype=torch.int64, device=dev) * T).contiguous()
    band = torch.empty((N, 2 + nb), dtype=torch.float32, device=dev)
    melout = torch.empty((N, 38), dtype=torch.float32, device=dev)
    filtered = torch.empty((N, nb), dtype=torch.float32, device=dev)
    frames = torch.empty((N, D), dtype=torch.float32, device=dev)

    def mfcc_bark():
        _lib.launch("sc_mfcc", dev, pcm, _lib.XT_I16, L, 1.0, lens, off, B, N, window_length, shift, n_fft, PREFAC, window, bank, lo, hi, nb, dct, 1, band,
                    2 + nb, None, n_fft // 2 + 1)

    def mfcc_mel():
        _lib.launch("sc_mfcc", dev, pcm, _lib.XT_I16, L, 1.0, lens, off, B, N, window_length, shift, n_fft, PREFAC, mel[0], mel[1], mel[2], mel[3], 24, mel[4],
                    13, melout, 38, None, n_fft // 2 + 1)

    def rasta():
        _lib.launch("sc_feat_rasta", dev, band[:, 2:], 2 + nb, off, B, nb, filtered, nb)

    def cepstra(x, ldb):
        _lib.launch("sc_plp_cepstra", dev, x, ldb, N, nb, order, eql, acw, lift, frames[:, 1:], D, frames[:, 1 + NCEPS:], D)

    res = {"workload": {"utterances": B, "seconds": SECONDS, "sampling_frequency": FS, "frames_per_utterance": T, "frames": N, "critical_bands": nb,
                        "cepstra": NCEPS, "floats_per_frame": D},
           "protocol": {"warmup_calls": WARMUP, "windows": REPS, "calls_per_window": CALLS, "timer": "device events around the calls of a window"},
           "device": torch.cuda.get_device_name(0),
           "counted_from_shapes_per_frame": {
               "bytes_sc_plp_cepstra": 4 * nb + 4 * (order + 1) + 4 * nb,
               "float64_multiply_add_pairs": {"autocorrelation": (order + 1) * nb, "levinson_sums": order * (order - 1) // 2,
                                              "levinson_updates": order * (order - 1) // 2, "cepstrum_recursion": order * (order - 1) // 2},
               "float64_exp_pow_log_div": {"exp": nb, "pow": nb, "log": 1, "div": 2 * order}, "hardware_counters": "not measured"}}
    launches = {}
    for name, fn in (("sc_mfcc bark bank", mfcc_bark), ("sc_mfcc 24 mel triangles", mfcc_mel), ("sc_feat_rasta", rasta),
                     ("sc_plp_cepstra on filtered rows", lambda: cepstra(filtered, nb)), ("sc_plp_cepstra on unfiltered rows", lambda: cepstra(band[:, 2:], 2 + nb))):
        launches[name] = measure(torch, fn)
        print(name, f"{launches[name]['median_ms']:.3f} ms (spread {launches[name]['spread_ms']:.3f})", flush=True)
    ms = {k: v["median_ms"] for k, v in launches.items()}
    res["launches"] = launches
    res["sums"] = {"rasta_plp_three_launches_ms": ms["sc_mfcc bark bank"] + ms["sc_feat_rasta"] + ms["sc_plp_cepstra on filtered rows"],
                   "plp_two_launches_ms": ms["sc_mfcc bark bank"] + ms["sc_plp_cepstra on unfiltered rows"],
                   "sc_plp_cepstra_over_sc_mfcc_bark": ms["sc_plp_cepstra on unfiltered rows"] / ms["sc_mfcc bark bank"],
                   "sc_plp_cepstra_over_sc_mfcc_mel": ms["sc_plp_cepstra on unfiltered rows"] / ms["sc_mfcc 24 mel triangles"],
                   "sc_plp_cepstra_frames_per_s": N / ms["sc_plp_cepstra on unfiltered rows"] * 1e3}
    print(res["sums"], flush=True)
    res["plp_device"] = {}
    for on in (True, False):
        m = measure(torch, lambda on=on: plp.plp_device(pcm, None, fs=FS, nwin=NWIN, nceps=NCEPS, shift=SHIFT, prefac=PREFAC, rasta=on))
        m["times_real_time"] = B * SECONDS / m["median_ms"] * 1e3
        res["plp_device"]["rasta" if on else "no rasta"] = m
        print("plp_device rasta", on, f"{m['median_ms']:.3f} ms", flush=True)
    # ---- float64 torch on the same card
    mfcc_bark()
    cepstra(band[:, 2:], 2 + nb)
    ours = frames[:, 1:1 + NCEPS].clone()
    logband = band[:, 2:].contiguous()
    rows = CHUNK * T

    def tail_all():
        return torch.cat([torch_tail(torch, logband[r0:r0 + rows], eql, acw, lift) for r0 in range(0, N, rows)])

    m = measure(torch, tail_all, calls=1, reps=5)
    m["max_abs_difference_from_the_kernel"] = float((tail_all() - ours).abs().max())
    m["over_sc_plp_cepstra"] = m["median_ms"] / ms["sc_plp_cepstra on unfiltered rows"]
    res["torch_float64_tail"] = m
    print("torch tail", f"{m['median_ms']:.3f} ms, {m['over_sc_plp_cepstra']:.1f} x the kernel, difference {m['max_abs_difference_from_the_kernel']:.3e}", flush=True)
    spec = fx.mfcc_device(pcm[:CHUNK], None, fs=FS, lowfreq=0, maxfreq=FS / 2, nlinfilt=2, nlogfilt=0, nwin=NWIN, nceps=1, shift=SHIFT, prefac=PREFAC,
                          get_spec=True)[2]
    bank64 = bank.double()
    m = measure(torch, lambda: torch.log(spec.double() @ bank64.T), calls=1, reps=5)
    m["utterances"] = CHUNK
    m["scaled_to_the_workload_ms"] = m["median_ms"] * B / CHUNK
    res["torch_float64_bank_matmul"] = m
    print("torch bank matmul", f"{m['median_ms']:.3f} ms for {CHUNK} utterances", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
