"""What the context features cost (GPU box):

    python scripts/context_bench.py --out profiles/context_bench.json

Workload: 1 M resident float32 frames (``RandomState(9)``), once as ONE segment and once as 4 096 segments of about 250 rows (drawn from 195 to
293, then shifted evenly to sum to 1 M): row tiles are per segment, so the second layout shows what position-independent bits cost.
Measured, each after WARMUP calls as the median of REPS windows (3 for the torch side) of CALLS[...] calls between two device events, the
windows 0.07 to 0.2 s long (``spread`` = max - min of the windows).  A time is that of a whole call, its host side included -- the
read-back of the flag that checks resident offsets, which synchronises, and the upload of small tables -- so a rate over it is an
end-to-end call rate, not a kernel's share of peak.  With the peak of the device memory the call allocates on top of its inputs (``torch.cuda.max_memory_allocated``):
  * ``pca_dct`` (12, 12) at D = 20 with a 500 x 60 PCA matrix: ``sc_ctx_project`` (the composite matrix resident) against the same map
    in float64 torch on the same card -- the windows gathered by clamped row indices, ``(N D, W) @ B``, then ``(N, D W) @ P``, rounded
    to float32 -- with the largest difference between the two results; counted from the shapes: 2 N (W D) Q floating-point operations,
    and their call rate over the f64 matrix peak (F64_MATRIX_TFLOPS);
  * the same without the PCA matrix: ``sc_ctx_basis`` against gather and one matmul in torch; 2 N D W W operations and the bytes
    written (4 N D W);
  * SDC (1, 3, 7) at D = 7: ``sdc_device`` (the frames copied in front and ``sc_ctx_gather``) and ``sc_ctx_gather`` alone against torch
    indexing (two clamped gathers, a subtraction, a concatenation); bytes read and written from the shapes.
The torch side builds its clamped indices inside the timed call, as the kernels do; the per-row segment bounds it builds them from
are made once outside.  Fails without a GPU; nothing is a ratio fixed in advance.

Kernel times come from a profiler run of their own, one per layout (the kernels' names do not tell the layouts apart):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o one -- python scripts/context_bench.py --trace-only one_segment

``ctx_project_kernel``, ``ctx_basis_kernel`` and ``ctx_gather_kernel`` are launched TRACE_CALLS times each on the shapes above; a
kernel's share of peak is the operations (or bytes) counted above over its average time in the ``kernel_stats`` table.
"""
import argparse
import json
import os
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOTAL, SEGMENTS, SHORTEST, LONGEST = 1_000_000, 4096, 195, 293
LEFT, RIGHT, PCA_D, PCA_Q = 12, 12, 20, 60
SDC, SDC_D = (1, 3, 7), 7
WARMUP, REPS = 3, 7
CALLS = {"project": 100, "basis": 100, "gather": 1000, "sdc_device": 500, "torch": 5, "torch_sdc": 100}   # windows of 0.07 to 0.2 s
TRACE_CALLS = 50
F64_MATRIX_TFLOPS = 78.6      # MI355X: v_mfma_f64_16x16x4_f64, 32 FLOP / clk / SIMD (csrc/dgemm_tile.h)


def median(v):
    s = sorted(v)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def layouts(n_total=TOTAL, segments=SEGMENTS):
    rs = numpy.random.RandomState(9)
    lens = rs.randint(SHORTEST, LONGEST + 1, size=segments)
    short = n_total - lens.sum()                     # spread what is missing (or too much) evenly
    lens += short // segments
    lens[:short % segments] += 1
    assert lens.sum() == n_total and lens.min() > 0
    many = numpy.concatenate(([0], numpy.cumsum(lens))).astype(numpy.int64)
    return {"one_segment": numpy.array([0, n_total], dtype=numpy.int64), "many_segments": many}


def measure(torch, fn, calls, reps=REPS):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return {"median_ms": median(ms), "spread_ms": max(ms) - min(ms), "ms": ms, "calls_per_window": calls, "windows": reps,
            "peak_device_bytes_above_inputs": int(torch.cuda.max_memory_allocated() - base)}


def row_bounds(torch, off, n):
    """per row: the first and the last row of its segment"""
    seg = torch.searchsorted(off, torch.arange(n, device=off.device), right=True) - 1
    return off[seg], off[seg + 1] - 1


def window_index(torch, lo, hi, shifts):
    t = torch.arange(lo.shape[0], device=lo.device)[:, None] + shifts[None, :]
    return torch.minimum(torch.maximum(t, lo[:, None]), hi[:, None])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "context_bench.json"))
    ap.add_argument("--frames", type=int, default=TOTAL)
    ap.add_argument("--segments", type=int, default=SEGMENTS)
    ap.add_argument("--trace-only", choices=("one_segment", "many_segments"),
                    help="launch the three kernels TRACE_CALLS times each on one layout and write nothing: the run a kernel trace is taken from")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("context_bench.py measures on the GPU only: no GPU is visible")
    from sidekit_amd import features_context as fc
    dev = torch.device("cuda", 0)
    rs = numpy.random.RandomState(9)
    N, W = args.frames, LEFT + RIGHT + 1
    x20 = torch.as_tensor((rs.standard_normal((N, PCA_D)) * (1 + rs.rand(PCA_D))).astype(numpy.float32)).to(dev)
    x7 = x20[:, :SDC_D].contiguous()
    P_host = rs.standard_normal((PCA_D * W, PCA_Q)) / numpy.sqrt(PCA_D * W)
    B_host = fc.dct_pca_basis(LEFT, RIGHT)
    M = torch.as_tensor(fc.projection_matrix(B_host, P_host, PCA_D)).to(dev)
    B, P = torch.as_tensor(B_host).to(dev), torch.as_tensor(P_host).to(dev)
    plus, minus = (torch.as_tensor(v.astype(numpy.int64)).to(dev) for v in fc.sdc_offsets(*SDC))
    shifts = torch.arange(-LEFT, RIGHT + 1, device=dev)
    res = {"workload": {"frames": N, "window": [LEFT, RIGHT], "pca": {"D": PCA_D, "rows": PCA_D * W, "Q": PCA_Q}, "sdc": {"config": list(SDC), "D": SDC_D}},
           "protocol": {"warmup_calls": WARMUP, "windows": REPS, "calls_per_window": CALLS, "times_are": "whole calls, host side included (the read-back of the offsets' check, small uploads)", "timer": "device events around the calls of a window",
                        "f64_matrix_peak_tflops": F64_MATRIX_TFLOPS},
           "device": torch.cuda.get_device_name(0), "layouts": {}}
    if args.trace_only:
        off = torch.as_tensor(layouts(N, args.segments)[args.trace_only]).to(dev)
        y_proj = torch.empty((N, PCA_Q), dtype=torch.float32, device=dev)
        y_dct = torch.empty((N, PCA_D * W), dtype=torch.float32, device=dev)
        y_sdc = torch.empty((N, SDC_D * SDC[2]), dtype=torch.float32, device=dev)
        for _ in range(TRACE_CALLS):
            fc.project_device(x20, off, M, W, LEFT, out=y_proj)
            fc.basis_device(x20, off, B, LEFT, out=y_dct)
            fc.gather_device(x7, off, *fc.sdc_offsets(*SDC), out=y_sdc)
        torch.cuda.synchronize()
        print("launched each kernel", TRACE_CALLS, "times on", args.trace_only)
        return
    for name, off_host in layouts(N, args.segments).items():
        off = torch.as_tensor(off_host).to(dev)
        lens = numpy.diff(off_host)
        lo, hi = row_bounds(torch, off, N)
        out = {"segments": int(lens.shape[0]), "shortest": int(lens.min()), "longest": int(lens.max()),
               "rows_of_64_row_tiles_over_rows": float((numpy.ceil(lens / 64.0) * 64).sum() / N)}

        def torch_dct(project):
            win = x20.double()[window_index(torch, lo, hi, shifts)]                       # (N, W, D)
            z = (win.transpose(1, 2).reshape(N * PCA_D, W) @ B).reshape(N, PCA_D * W)
            return ((z @ P) if project else z).float()

        def torch_sdc():
            return torch.cat((x7, (x7[window_index(torch, lo, hi, plus)] - x7[window_index(torch, lo, hi, minus)]).reshape(N, -1)), dim=1)

        y_proj = torch.empty((N, PCA_Q), dtype=torch.float32, device=dev)
        m = measure(torch, lambda: fc.project_device(x20, off, M, W, LEFT, out=y_proj), CALLS["project"])
        flop = 2.0 * N * PCA_D * W * PCA_Q
        m.update(flop=flop, tflops=flop / m["median_ms"] * 1e-9, call_rate_over_f64_matrix_peak=flop / m["median_ms"] * 1e-9 / F64_MATRIX_TFLOPS)
        t = measure(torch, lambda: torch_dct(True), CALLS["torch"], reps=3)
        t["max_abs_difference_from_the_kernel"] = float((torch_dct(True) - y_proj).abs().max())
        t["torch_over_kernel"] = t["median_ms"] / m["median_ms"]
        out["pca_dct sc_ctx_project"], out["pca_dct torch float64"] = m, t
        print(name, "sc_ctx_project", f"{m['median_ms']:.3f} ms (spread {m['spread_ms']:.3f}), {m['tflops']:.1f} TFLOP/s; torch {t['median_ms']:.1f} ms", flush=True)

        y_dct = torch.empty((N, PCA_D * W), dtype=torch.float32, device=dev)
        m = measure(torch, lambda: fc.basis_device(x20, off, B, LEFT, out=y_dct), CALLS["basis"])
        flop = 2.0 * N * PCA_D * W * W
        m.update(flop=flop, tflops=flop / m["median_ms"] * 1e-9, bytes_written=4 * N * PCA_D * W,
                 written_gbytes_per_s=4.0 * N * PCA_D * W / m["median_ms"] * 1e-6)
        t = measure(torch, lambda: torch_dct(False), CALLS["torch"], reps=3)
        t["max_abs_difference_from_the_kernel"] = float((torch_dct(False) - y_dct).abs().max())
        t["torch_over_kernel"] = t["median_ms"] / m["median_ms"]
        out["dct sc_ctx_basis"], out["dct torch float64"] = m, t
        del y_dct
        print(name, "sc_ctx_basis", f"{m['median_ms']:.3f} ms (spread {m['spread_ms']:.3f}); torch {t['median_ms']:.1f} ms", flush=True)

        y_sdc = torch.empty((N, SDC_D * SDC[2]), dtype=torch.float32, device=dev)
        off_plus, off_minus = fc.sdc_offsets(*SDC)
        g = measure(torch, lambda: fc.gather_device(x7, off, off_plus, off_minus, out=y_sdc), CALLS["gather"])
        moved = 4.0 * N * SDC_D * (1 + SDC[2])
        g.update(bytes_read_plus_written=moved, gbytes_per_s=moved / g["median_ms"] * 1e-6)
        m = measure(torch, lambda: fc.sdc_device(x7, off, *SDC), CALLS["sdc_device"])
        t = measure(torch, torch_sdc, CALLS["torch_sdc"], reps=3)
        t["bit_equal_to_the_kernel"] = bool(torch.equal(torch_sdc(), fc.sdc_device(x7, off, *SDC)))
        t["torch_over_sdc_device"] = t["median_ms"] / m["median_ms"]
        out["sdc sc_ctx_gather"], out["sdc sdc_device"], out["sdc torch indexing"] = g, m, t
        print(name, "sc_ctx_gather", f"{g['median_ms']:.3f} ms, sdc_device {m['median_ms']:.3f} ms; torch {t['median_ms']:.2f} ms", flush=True)
        res["layouts"][name] = out
    one, many = res["layouts"]["one_segment"], res["layouts"]["many_segments"]
    res["many_segments_over_one_segment"] = {k: many[k]["median_ms"] / one[k]["median_ms"]
                                             for k in ("pca_dct sc_ctx_project", "dct sc_ctx_basis", "sdc sc_ctx_gather")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
