"""What the diagonal-GMM E-step costs in time and memory (GPU box):

    python scripts/gmm_bench.py --out profiles/gmm_bench.json

(a) one E-step (``gmm_stats_device``: ``sc_gmm_frame_loglik`` + ``sc_gmm_stats``, order 2, one segment) at C = 2 048, D = 60 on
    N = 8 000 000 resident float32 frames, against the materialised route on the same GPU: per block of rows whose (rows x C) float64
    matrix is at most 1 GiB, ``torch.matmul`` of ``[X^2, X]`` with the component operand, ``logsumexp``, ``exp``, ``torch.matmul`` of the
    posteriors with ``[1, X, X^2]``, the blocks' statistics added in block order.  In one process, alternating, after a warm-up of each,
    REPS event-timed calls each (median and max - min spread), synchronised on both sides.  Peak device memory of each route:
    ``torch.cuda.mem_get_info`` before its first call in a process whose caches were just released and after it.  The share of the f64
    matrix rate (78.6 TFLOP/s) counts 12 C D FLOP per frame.  No ratio is a bar: the fused route recomputes lp.
(b) ``StatServer.accumulate_stat_device`` on 4 096 segments of 2 000 float32 frames at C = 512, D = 60 (order 1).
(c) the reference's numpy arithmetic (log posteriors, log-sum-exp, posteriors, the three products) on 16 threads, on N / 64 of the frames
    of (a), its time scaled by 64.

Every GPU step is a child process under its own ``timeout``; the first one that fails ends the run (no retries) and nothing is written.
"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C_EM, D, N_EM, REPS, BLOCK_BYTES, STEP_TIMEOUT_S = 2048, 60, 8000000, 3, 1 << 30, 500
C_ACC, SEGMENTS, SEG_LEN = 512, 4096, 2000
PEAK_F64_TFLOPS = 78.6


def median(v):
    s = sorted(v)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)


def make_mixture(C, seed):
    import numpy
    from sidekit_amd.mixture import Mixture
    rs = numpy.random.RandomState(seed)
    m = Mixture()
    w = rs.rand(C) + 0.5
    m.w, m.mu, m.invcov = w / w.sum(), 2.0 * rs.randn(C, D), 1.0 / (0.5 + rs.rand(C, D))
    m.cov_var_ctl = 1.0 / m.invcov
    m._compute_all()
    return m


def make_frames(torch, ubm, n, dev):
    g = torch.Generator(device=dev).manual_seed(7)
    mu = torch.as_tensor(ubm.mu, dtype=torch.float32).to(dev)
    X = torch.empty((n, D), dtype=torch.float32, device=dev)
    for a in range(0, n, 1 << 20):
        b = min(n, a + (1 << 20))
        X[a:b] = mu[torch.randint(0, mu.shape[0], (b - a,), device=dev, generator=g)] + 1.1 * torch.randn(b - a, D, device=dev, generator=g)
    return X


def step_estep(n):
    import torch
    from sidekit_amd import _lib
    from sidekit_amd.mixture import gmm_stats_device
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    ubm = make_mixture(C_EM, 1)
    X = make_frames(torch, ubm, n, dev)
    mu, ic, A = (torch.as_tensor(a).to(dev) for a in (ubm.mu, ubm.invcov, ubm.A))
    G = torch.cat((ic, -2.0 * mu * ic), dim=1).t().contiguous()             # (2 D, C)
    rows = max(1, min(n, BLOCK_BYTES // (8 * C_EM)))
    held = {}
    gmm_stats_device(ubm, X[:64], None, 2)                                  # the library's code object is on the device before memory is measured

    def fused():
        held["fused"] = gmm_stats_device(ubm, X, None, 2)

    def materialised():
        st = torch.zeros((C_EM, 2 * D + 1), dtype=torch.float64, device=dev)
        llk = torch.zeros((), dtype=torch.float64, device=dev)
        for a in range(0, n, rows):
            x = X[a:min(a + rows, n)].double()
            lp = torch.matmul(torch.cat((x * x, x), dim=1), G)
            lp.add_(A).mul_(-0.5)
            lse = torch.logsumexp(lp, dim=1)
            lp.sub_(lse[:, None]).exp_()
            st += torch.matmul(lp.t(), torch.cat((torch.ones_like(x[:, :1]), x, x * x), dim=1))
            llk += lse.sum()
        held["materialised"] = (st[:, 0], st[:, 1:D + 1], st[:, D + 1:], llk)

    def peak(fn):
        torch.cuda.synchronize()
        held.clear()
        torch.cuda.empty_cache()
        lib.sc_release_workspace()
        free0, _ = torch.cuda.mem_get_info(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        free1, _ = torch.cuda.mem_get_info(dev)
        return free0 - free1, torch.cuda.max_memory_allocated(dev) - base

    res = {"C": C_EM, "D": D, "N": n, "frames": "float32", "materialised_block_rows": rows,
           "posterior_matrix_bytes_never_built": 8 * C_EM * n, "slab_workspace_bytes": 64 * C_EM * (2 * D + 1) * 8}
    res["fused_device_memory_taken_bytes"], res["fused_torch_peak_bytes"] = peak(fused)             # also the warm-up of the route
    f = [t.clone() for t in held["fused"]]
    res["materialised_device_memory_taken_bytes"], res["materialised_torch_peak_bytes"] = peak(materialised)
    m = held["materialised"]
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())   # noqa: E731
    res["routes_relative_max_difference"] = {"stat0": rel(f[0][0], m[0]), "stat1": rel(f[1][0], m[1]), "stat2": rel(f[2][0], m[2]), "llk": rel(f[3][0], m[3])}
    assert max(res["routes_relative_max_difference"].values()) < 1e-9, res["routes_relative_max_difference"]
    tf, tm = [], []
    for _ in range(REPS):
        tf.append(timed(fused))
        tm.append(timed(materialised))
    again = held["fused"]
    res["fused_runs_bit_identical"] = all(bool(torch.equal(a, b)) for a, b in zip(f, again))
    flop = 12.0 * C_EM * D * n
    res.update(fused_ms=tf, materialised_ms=tm, fused_median_ms=median(tf), materialised_median_ms=median(tm), fused_spread_ms=max(tf) - min(tf),
               materialised_spread_ms=max(tm) - min(tm), materialised_over_fused=median(tm) / median(tf), flop_counted=flop,
               fused_tflops=flop / median(tf) * 1e-9, fused_share_of_the_f64_matrix_rate=flop / median(tf) * 1e-9 / PEAK_F64_TFLOPS)
    return res


def step_accumulate(segments):
    import numpy
    import torch
    from sidekit_amd.statserver import StatServer
    dev = torch.device("cuda", 0)
    ubm = make_mixture(C_ACC, 2)
    X = make_frames(torch, ubm, segments * SEG_LEN, dev)
    off = numpy.arange(segments + 1, dtype=numpy.int64) * SEG_LEN
    server = StatServer()
    server.segset = numpy.array([f"s{i}" for i in range(segments)], dtype="|O")
    server.modelset = server.segset.copy()
    server.start, server.stop = numpy.empty(segments, dtype="|O"), numpy.empty(segments, dtype="|O")
    run = lambda: server.accumulate_stat_device(ubm, X, off)   # noqa: E731
    run()
    first = server.stat1.copy()
    t = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()                                                     # ends with the copy of the statistics to the host
        t.append((time.perf_counter() - t0) * 1e3)
    return {"C": C_ACC, "D": D, "segments": segments, "frames_per_segment": SEG_LEN, "frames": "float32", "order": 1,
            "wall_ms_including_the_copy_to_the_host": t, "median_ms": median(t), "spread_ms": max(t) - min(t),
            "frames_per_second": segments * SEG_LEN / (median(t) * 1e-3), "runs_bit_identical": bool(numpy.array_equal(first, server.stat1)),
            "stat0_row_sums_are_the_segment_length": float(numpy.abs(server.stat0.sum(1) - SEG_LEN).max())}


def step_numpy(n):
    import numpy
    ubm = make_mixture(C_EM, 1)
    rs = numpy.random.RandomState(3)
    X = (ubm.mu[rs.randint(0, C_EM, n)] + 1.1 * rs.randn(n, D)).astype(numpy.float32).astype(numpy.float64)
    t = []
    for _ in range(2):
        t0 = time.perf_counter()
        lp = -0.5 * (numpy.dot(numpy.square(X), ubm.invcov.T) - 2.0 * numpy.dot(X, numpy.transpose(ubm.mu * ubm.invcov)) + ubm.A)
        top = numpy.max(lp, axis=1)
        lse = top + numpy.log(numpy.sum(numpy.exp((lp.T - top).T), axis=1))
        pp = numpy.exp((lp.T - lse).T)
        s0, s1, s2 = pp.sum(0), numpy.dot(X.T, pp).T, numpy.dot(numpy.square(X.T), pp).T
        t.append((time.perf_counter() - t0) * 1e3)
    return {"C": C_EM, "D": D, "N": n, "threads": int(os.environ.get("OMP_NUM_THREADS", "0")), "ms": t, "best_ms": min(t),
            "scaled_to_the_frames_of_a_ms": min(t) * (N_EM / n), "check": float(s0.sum() / n)}


def child(args):
    """One step in a process of its own, under its own time limit; its last output line is its JSON result."""
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"gmm_bench: step {args} ended with status {p.returncode}; nothing after it was started")
    print(f"gmm_bench: step {args} done", file=sys.stderr, flush=True)
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=N_EM, help="frames of the E-step (the published figures: 8 000 000)")
    ap.add_argument("--segments", type=int, default=SEGMENTS)
    ap.add_argument("--step", default=None, choices=("estep", "accumulate", "numpy"), help="(internal) run one step in this process")
    args = ap.parse_args()
    if args.step:
        if args.step != "numpy":
            import torch
            assert torch.cuda.is_available(), "gmm_bench.py measures on the GPU"
        res = {"estep": lambda: step_estep(args.frames), "accumulate": lambda: step_accumulate(args.segments),
               "numpy": lambda: step_numpy(args.frames // 64)}[args.step]()
        print(json.dumps(res), flush=True)
        return
    common = ["--frames", str(args.frames), "--segments", str(args.segments)]
    out = {"timed_repeats": REPS, "f64_peak_tflops": PEAK_F64_TFLOPS, "materialised_block_bytes_at_most": BLOCK_BYTES,
           "a_one_e_step_fused_against_materialised": child(["--step", "estep"] + common),
           "b_accumulate_stat_device": child(["--step", "accumulate"] + common),
           "c_reference_numpy_arithmetic_on_a_64th": child(["--step", "numpy"] + common)}
    a, c = out["a_one_e_step_fused_against_materialised"], out["c_reference_numpy_arithmetic_on_a_64th"]
    out["numpy_scaled_over_fused"] = c["scaled_to_the_frames_of_a_ms"] / a["fused_median_ms"]
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
