"""What the feature post-processing costs (GPU box):

    python scripts/features_bench.py --out profiles/features_bench.json

Workload: about 1 M frames of 20 cepstra in segments of 3 000 to 30 000 frames (``RandomState(5)``), about 70 % of them labelled; RASTA,
deltas and double deltas make 60 coefficients.  Measured, each after WARMUP calls as the median of REPS windows of CALLS calls between two
device events (``spread`` = max - min of the windows):
  * each kernel alone: ``sc_feat_rasta`` and ``sc_feat_delta`` on the 20 columns of all rows, ``sc_feat_moments`` and the five modes of
    ``sc_feat_norm`` (window 301) on the 60 columns of the compacted labelled rows;
  * ``post_process_device`` end to end (RASTA, deltas, double deltas, normalisation, selection of the labelled rows) for ``cmvn_sliding``
    and ``stg``;
  * comparator (a): the two windowed normalisations written with torch on the same card and the same compacted rows -- ``unfold`` windows
    in row chunks whose materialised part stays under 1 GiB, float64 sums for the sliding norm, float32 comparisons and
    ``torch.special.ndtri`` for the warp -- with its largest difference from the kernel's result;
  * comparator (b): the float64 numpy restatement of the tests (tests/tools/normfeat_numpy.py) on the host for ONE utterance of 30 000
    frames x 60, four columns at a time (its window array would not fit otherwise), and the kernel on that utterance alone.
Counted from the shapes: bytes read and written per frame and coefficient, window values visited per frame and coefficient.
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

CEPSTRA, WIN, TOTAL, SHORTEST, LONGEST, SPEECH = 20, 301, 1_000_000, 3_000, 30_000, 0.7
WARMUP, REPS, CALLS = 2, 7, 3
CHUNK_BYTES = 1 << 30


def median(v):
    s = sorted(v)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def workload(n_total=TOTAL):
    rs = numpy.random.RandomState(5)
    lens = []
    while sum(lens) < n_total:
        lens.append(int(rs.randint(SHORTEST, LONGEST + 1)))
    off = numpy.concatenate(([0], numpy.cumsum(lens))).astype(numpy.int64)
    x = (rs.standard_normal((off[-1], CEPSTRA)) * (1 + rs.rand(CEPSTRA)) + rs.standard_normal(CEPSTRA)).astype(numpy.float32)
    return x, off, rs.rand(off[-1]) < SPEECH


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


def torch_windowed(torch, x, off, win, warp):
    """cmvn_sliding (``warp`` False) or stg of compacted rows, every segment longer than ``win``: plain torch on ``unfold`` windows"""
    out = torch.empty_like(x)
    h, D = win // 2, x.shape[1]
    rows = max(1, CHUNK_BYTES // (D * win * (4 if warp else 8)))
    for a, b in zip(off[:-1], off[1:]):
        seg, n = x[a:b], b - a
        assert n > win
        U = seg.unfold(0, win, 1)      # (n - win + 1, D, win), a view: window j is centred on row j + h

        def one(W, rows_x):
            if warp:
                c = (W < rows_x[:, :, None]).sum(-1)
                return torch.special.ndtri((c.double() + 0.5) / win).float()
            Wd = W.double()
            return ((rows_x.double() - Wd.mean(-1)) / Wd.std(-1, unbiased=True)).float()

        out[a:a + h] = one(U[0:1], seg[:h])
        out[b - h:b] = one(U[-1:], seg[n - h:])
        for r0 in range(0, U.shape[0], rows):
            r1 = min(r0 + rows, U.shape[0])
            out[a + h + r0:a + h + r1] = one(U[r0:r1], seg[h + r0:h + r1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_bench.json"))
    ap.add_argument("--frames", type=int, default=TOTAL)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("features_bench.py measures on the GPU only: no GPU is visible")
    import normfeat_numpy as nfn
    from sidekit_amd import features_server as fs
    dev = torch.device("cuda", 0)
    x_host, off_host, lab_host = workload(args.frames)
    x, off, lab = torch.as_tensor(x_host).to(dev), torch.as_tensor(off_host).to(dev), torch.as_tensor(lab_host).to(dev)
    N, S = int(off_host[-1]), off_host.shape[0] - 1
    opts = dict(rasta=True, delta=True, double_delta=True, keep_all_features=False)
    full, _, _ = fs.post_process_device(x, off, lab, rasta=True, delta=True, double_delta=True)          # (N, 60), not normalised
    speech = lab.clone()
    first = off[:-1]
    speech[first] = speech[first + 2]
    speech[first + 1] = speech[first + 2]
    xs = full[speech].contiguous()
    soff = torch.cat((torch.zeros(1, dtype=torch.int64, device=dev), speech.cumsum(0)))[off].contiguous()
    soff_host = soff.cpu().numpy()
    Ns, D = xs.shape
    mean, std = fs.segment_moments_device(xs, soff)
    res = {"workload": {"frames": N, "segments": S, "cepstra": CEPSTRA, "coefficients": D, "labelled_frames": Ns, "window": WIN,
                        "shortest_segment": int(numpy.diff(off_host).min()), "longest_segment": int(numpy.diff(off_host).max())},
           "protocol": {"warmup_calls": WARMUP, "windows": REPS, "calls_per_window": CALLS, "timer": "device events around the calls of a window"},
           "device": torch.cuda.get_device_name(0), "kernels": {}, "end_to_end": {}, "torch_same_card": {}, "numpy_one_utterance": {}}
    y20, y60 = torch.empty_like(x), torch.empty_like(xs)
    kernels = {"sc_feat_rasta": (lambda: fs.rasta_device(x, off, out=y20), N * CEPSTRA),
               "sc_feat_delta": (lambda: fs.delta_device(x, off, out=y20), N * CEPSTRA),
               "sc_feat_moments": (lambda: fs.segment_moments_device(xs, soff), Ns * D)}
    for mode in ("cms", "cmvn", "cms_sliding", "cmvn_sliding", "stg"):
        kernels[f"sc_feat_norm {mode}"] = (lambda mode=mode: fs.normalise_device(xs, soff, mode, WIN, mean, std, out=y60), Ns * D)
    visits = {"sc_feat_norm cms_sliding": WIN, "sc_feat_norm cmvn_sliding": 2 * WIN, "sc_feat_norm stg": WIN, "sc_feat_delta": 7}
    for name, (fn, elements) in kernels.items():
        m = measure(torch, fn)
        m["elements"] = elements
        m["giga_elements_per_s"] = elements / m["median_ms"] * 1e-6
        m["bytes_per_element_read_plus_written"] = 4 if name == "sc_feat_moments" else 8
        if name in visits:
            m["window_values_per_element"] = visits[name]
            m["giga_window_values_per_s"] = elements * visits[name] / m["median_ms"] * 1e-6
        res["kernels"][name] = m
        print(name, f"{m['median_ms']:.3f} ms (spread {m['spread_ms']:.3f})", flush=True)
    for norm in ("cmvn_sliding", "stg"):
        m = measure(torch, lambda norm=norm: fs.post_process_device(x, off, lab, feat_norm=norm, **opts))
        m["frames_per_s"] = N / m["median_ms"] * 1e3
        res["end_to_end"][f"post_process_device {norm}"] = m
        print("post_process_device", norm, f"{m['median_ms']:.3f} ms", flush=True)
    for norm, warp in (("cmvn_sliding", False), ("stg", True)):
        ours = fs.normalise_device(xs, soff, norm, WIN, mean, std)
        theirs = torch_windowed(torch, xs, soff_host, WIN, warp)
        m = measure(torch, lambda warp=warp: torch_windowed(torch, xs, soff_host, WIN, warp), calls=1, reps=3)
        m["max_abs_difference_from_the_kernel"] = float((ours - theirs).abs().max())
        m["kernel_median_ms"] = res["kernels"][f"sc_feat_norm {norm}"]["median_ms"]
        m["torch_over_kernel"] = m["median_ms"] / m["kernel_median_ms"]
        res["torch_same_card"][norm] = m
        print("torch", norm, f"{m['median_ms']:.1f} ms, {m['torch_over_kernel']:.1f} x the kernel", flush=True)
    n1 = LONGEST
    one = xs[:n1].contiguous()
    one_host = one.cpu().numpy().astype(numpy.float64)
    for norm in ("cmvn_sliding", "stg"):
        t0 = time.perf_counter()
        want = numpy.column_stack([nfn.normalise(one_host[:, c:c + 4], norm, WIN) for c in range(0, D, 4)])
        host_s = time.perf_counter() - t0
        m = measure(torch, lambda norm=norm: fs.normalise_device(one, None, norm, WIN))
        got = fs.normalise_device(one, None, norm, WIN).cpu().numpy()
        res["numpy_one_utterance"][norm] = {"frames": n1, "coefficients": D, "numpy_s": host_s, "kernel_median_ms": m["median_ms"],
                                            "kernel_spread_ms": m["spread_ms"], "numpy_over_kernel": host_s * 1e3 / m["median_ms"],
                                            "max_abs_difference": float(numpy.abs(got - want).max())}
        print("numpy", norm, f"{host_s:.2f} s against {m['median_ms']:.3f} ms", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
