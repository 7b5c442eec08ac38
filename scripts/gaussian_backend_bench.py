"""What the heteroscedastic Gaussian back-end costs in time and memory against the materialised torch route (GPU box):

    python scripts/gaussian_backend_bench.py --out profiles/gaussian_backend_bench.json

N = 1 000 000 resident float64 test rows of D = 256 scored against C = 14 and C = 1 251 classes (a language set; the speakers of a
closed set).  Two routes to the same (C, N) log-likelihood matrix ``cst_c - 0.5 |x W_c - m_c W_c|^2``, the factors ``W_c`` and the
vectors ``m_c W_c`` prepared beforehand for both:

  kernel        one ``sc_gauss_loglik`` call (what ``lid_utils.gaussian_loglik_device`` launches): the product never leaves the registers
  materialised  per class and per block of at most 1 GiB of float64 rows, ``torch.matmul(X[a:b], W_c)`` (rocBLAS), minus the vector,
                squared, summed over the row, into the same output matrix

in one process, alternating, after a warm-up of each, five event-timed calls each (median, and the max - min spread of the five).  Peak
device memory of the kernel route: ``torch.cuda.mem_get_info`` before its first call in a process whose caches were just released
(``torch.cuda.empty_cache``, ``sc_release_workspace``) and after it, the output still held: the library's own workspace is seen, torch-side
counters would miss it.  The acceptance line: that peak is at most the ``C N 8`` bytes of the output plus the library workspace (each
rounded up to the allocators' 2 MiB granule).  The time bar: the kernel's median exceeds the materialised route's by no more than that
route's own spread.  The share of the f64 matrix-core bound (``2 N C D^2`` FLOP at 78.6 TFLOP/s) is reported without a bar.

Every GPU step is a child process under its own ``timeout``; the first one that fails ends the run (no retries) and nothing is written.
"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, N, CLASSES, REPS, BLOCK_BYTES, STEP_TIMEOUT_S = 256, 1000000, (14, 1251), 5, 1 << 30, 420
PEAK_F64_TFLOPS, GRANULE = 78.6, 2 << 20


def median(v):
    s = sorted(v)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)


def step(C, n):
    import torch
    from sidekit_amd import _lib
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    g = torch.Generator(device=dev).manual_seed(C)
    means = 0.6 * torch.randn(C, D, device=dev, generator=g, dtype=torch.float64)
    X = (means[torch.randint(0, C, (n,), device=dev, generator=g)] + 0.5 * torch.randn(n, D, device=dev, generator=g, dtype=torch.float64)).contiguous()
    W = torch.randn(C, D, D, device=dev, generator=g, dtype=torch.float64).triu_() / D ** 0.5 + torch.eye(D, device=dev, dtype=torch.float64)
    cst = torch.randn(C, device=dev, generator=g, dtype=torch.float64) - 200.0
    V = torch.bmm(means[:, None, :], W)[:, 0, :].contiguous()            # m_c W_c, for the materialised route
    rows = max(1, min(n, BLOCK_BYTES // (8 * D)))
    held = {}
    tiny = torch.zeros((2, 1), dtype=torch.float64, device=dev)
    _lib.launch("sc_closed_set_llr", dev, tiny, 2, 1, 0.5, tiny)       # the library's code object is on the device before memory is measured

    def kernel():
        out = held.get("kernel")
        if out is None:
            out = held["kernel"] = torch.empty((C, n), dtype=torch.float64, device=dev)
        _lib.launch("sc_gauss_loglik", dev, X, n, D, means, W, cst, C, out)

    def materialised():
        out = held.get("materialised")
        if out is None:
            out = held["materialised"] = torch.empty((C, n), dtype=torch.float64, device=dev)
        for c in range(C):
            for a in range(0, n, rows):
                b = min(a + rows, n)
                y = torch.matmul(X[a:b], W[c])
                y -= V[c]
                torch.sum(y.square_(), dim=1, out=out[c, a:b])
            out[c].mul_(-0.5).add_(cst[c])

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        lib.sc_release_workspace()
        free0, _ = torch.cuda.mem_get_info(dev)
        fn()
        torch.cuda.synchronize()
        free1, _ = torch.cuda.mem_get_info(dev)
        return free0 - free1

    up = lambda b: (b + GRANULE - 1) // GRANULE * GRANULE   # noqa: E731
    res = {"C": C, "N": n, "output_bytes": 8 * C * n, "library_workspace_bytes": 8 * C * D}
    res["library_workspace_bytes_allocated"] = res["library_workspace_bytes"] + res["library_workspace_bytes"] // 4
    res["kernel_peak_bytes"] = peak(kernel)                              # also the warm-up of the route
    res["kernel_peak_bound_bytes"] = up(res["output_bytes"]) + up(res["library_workspace_bytes_allocated"])
    res["kernel_peak_within_output_plus_workspace"] = res["kernel_peak_bytes"] <= res["kernel_peak_bound_bytes"]
    res["materialised_peak_bytes"] = peak(materialised)
    res["materialised_block_rows"] = rows
    worst = 0.0
    for c in range(0, C, max(1, C // 8)):                                # the two routes compute the same matrix
        worst = max(worst, float((held["kernel"][c] - held["materialised"][c]).abs().max() / held["materialised"][c].abs().max()))
    res["routes_relative_max_difference"] = worst
    assert worst < 1e-9, f"the two routes differ by {worst:.2e}"
    tk, tm = [], []
    for _ in range(REPS):                                                # alternating
        tk.append(timed(kernel))
        tm.append(timed(materialised))
    flop = 2.0 * n * C * D * D
    res.update(kernel_ms=tk, materialised_ms=tm, kernel_spread_ms=max(tk) - min(tk), materialised_spread_ms=max(tm) - min(tm),
               kernel_median_ms=median(tk), materialised_median_ms=median(tm), materialised_over_kernel=median(tm) / median(tk),
               kernel_no_slower_than_materialised_beyond_its_spread=median(tk) - median(tm) <= max(tm) - min(tm),
               f64_bound_ms=flop / PEAK_F64_TFLOPS * 1e-9, kernel_tflops=flop / median(tk) * 1e-9,
               kernel_share_of_the_f64_bound=flop / median(tk) * 1e-9 / PEAK_F64_TFLOPS, materialised_launches=C * (3 * ((n + rows - 1) // rows) + 2))
    return res


def child(args):
    """One GPU step in a process of its own, under its own time limit; its last output line is its JSON result."""
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"gaussian_backend_bench: step {args} ended with status {p.returncode}; nothing after it was started")
    print(f"gaussian_backend_bench: step {args} done", file=sys.stderr, flush=True)
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=N, help="test rows (the published figures: 1 000 000)")
    ap.add_argument("--step", type=int, default=None, metavar="C", help="(internal) run the GPU step of one class count in this process")
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "gaussian_backend_bench.py measures on the GPU"
        print(json.dumps(step(args.step, args.rows)), flush=True)
        return
    out = {"D": D, "N": args.rows, "timed_repeats": REPS, "materialised_block_bytes_at_most": BLOCK_BYTES, "f64_peak_tflops": PEAK_F64_TFLOPS,
           "sc_gauss_loglik_against_materialised": {str(C): child(["--step", str(C), "--rows", str(args.rows)]) for C in CLASSES}}
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
