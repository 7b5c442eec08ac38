"""What the full-covariance GMM kernels cost, beside torch on the same card and beside the f64 matrix rate (GPU box):

    python scripts/gmm_full_bench.py --out profiles/gmm_full_bench.json

One MI355X, D = 60, 192 000 resident float32 frames (the workload of gmm_topc_stats_bench.py: 127 segments of 300 to 3 000 frames from a
fixed seed), C = 512 and 2 048 components.  Per case, after a warm-up round, REPS rounds; a round times each of the following once, one
after the other, so the routes alternate and share whatever else the machine is doing; a timing is INNER back-to-back calls between two
device events, synchronised on both sides, divided by INNER; reported: median and max - min spread over the rounds.
  * ``frame_loglik_full_device`` (``sc_gmm_full_frame_loglik``; one GEMM-equivalent of 2 N C D^2 FLOP);
  * ``gmm_stats_full_device`` at order 1 over the 127 segments (pass A and pass B: two GEMM-equivalents);
  * ``gmm_stats_full_device`` at order 2 over one segment (pass A, pass B's lp and X' diag(pp) X: three GEMM-equivalents, of which the
    kernel computes the last one's lower triangle of tiles only);
  * one full EM iteration (``FullMixture._em_steps``: that E-step, the copies to the host and the host M-step, timed by the wall clock);
  * (a) the same quantities from torch: float64 ``bmm`` over component chunks of 3 (the centred frames, their product and its square,
    3 x 3 x N x D doubles, stay within 1 GiB), an online log-sum-exp over the chunks for pass A and a second sweep for the statistics; TORCH_REPS rounds
    of one call.  Peak device memory of either route is ``max_memory_allocated`` over one call beyond what was resident before it.
  * (b) the share of the 78.6 TFLOP/s f64 matrix rate each of the first three keeps, from the GEMM-equivalents above.
The data are SYNTHETIC (component means 0.25 apart per dimension under unit noise; random precision matrices with condition at most
about 10); they say nothing about speech.  No ratio is fixed in advance: the file states what was measured.

Every GPU step is a child process under its own ``timeout``; the first one that fails ends the run (no retries) and nothing is written.
"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, FRAMES, REPS, INNER, TORCH_REPS, STEP_TIMEOUT_S = 60, 192000, 3, 3, 2, 500
COMPONENTS, CHUNK, PEAK_TFLOPS = (512, 2048), 3, 78.6


def median(v):
    s = sorted(v)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def make_models(C):
    """a diagonal mixture to draw the frames from and a full one around the same means"""
    import numpy
    from gmm_topc_stats_bench import make_mixture
    from sidekit_amd.mixture_full import FullMixture
    diag = make_mixture(C)
    rs = numpy.random.RandomState(2)
    full = FullMixture()
    full.w, full.mu = diag.w.copy(), diag.mu.copy()
    q = numpy.linalg.qr(rs.randn(D, D))[0]
    full.invcov = numpy.stack([numpy.dot(q * (e * (0.6 + 0.8 * rs.rand(D))), q.T) for e in diag.invcov])
    full.invcov = 0.5 * (full.invcov + full.invcov.transpose(0, 2, 1))
    full.invchol, full.det, full.cst = numpy.empty((C, D, D)), numpy.zeros(C), numpy.zeros(C)
    full._compute_all()
    return diag, full


def timed(torch, fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def peak_bytes(torch, fn):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return int(torch.cuda.max_memory_allocated() - before)


def torch_route(torch, X64, mu, M, g, off, order):
    """(lse, stat0, stat1, stat2 or None) per segment from torch alone; order 0: lse only"""
    N, C = X64.shape[0], mu.shape[0]

    def lp_chunk(c0, c1):
        y = torch.bmm(X64[None] - mu[c0:c1, None, :], M[c0:c1].transpose(1, 2))
        return g[c0:c1, None] - 0.5 * (y * y).sum(-1)           # (chunk, N)

    lse = torch.full((N,), -float("inf"), dtype=torch.float64, device=X64.device)
    for c0 in range(0, C, CHUNK):
        lse = torch.logaddexp(lse, torch.logsumexp(lp_chunk(c0, min(C, c0 + CHUNK)), 0))
    if order == 0:
        return lse
    S = len(off) - 1
    stat0 = torch.empty((S, C), dtype=torch.float64, device=X64.device)
    stat1 = torch.empty((S, C, D), dtype=torch.float64, device=X64.device)
    stat2 = torch.empty((S, C, D, D), dtype=torch.float64, device=X64.device) if order == 2 else None
    for c0 in range(0, C, CHUNK):
        c1 = min(C, c0 + CHUNK)
        pp = torch.exp(lp_chunk(c0, c1) - lse[None])             # (chunk, N)
        for s in range(S):
            a, b = int(off[s]), int(off[s + 1])
            stat0[s, c0:c1] = pp[:, a:b].sum(1)
            stat1[s, c0:c1] = pp[:, a:b] @ X64[a:b]
            if order == 2:
                stat2[s, c0:c1] = torch.bmm((pp[:, a:b, None] * X64[None, a:b]).transpose(1, 2), X64[None, a:b].expand(c1 - c0, -1, -1))
    return lse, stat0, stat1, stat2


def step(C):
    import numpy
    import torch
    from gmm_bench import make_frames
    from gmm_topc_stats_bench import segment_lengths
    from sidekit_amd import mixture_full
    from sidekit_amd.mixture_full import frame_loglik_full_device, gmm_stats_full_device
    dev = torch.device("cuda", 0)
    diag, full = make_models(C)
    X = make_frames(torch, diag, FRAMES, dev)
    off = numpy.concatenate(([0], numpy.cumsum(segment_lengths())))
    one = numpy.array([0, FRAMES])
    N = FRAMES
    gemm = 2.0 * N * C * D * D
    runs = {"frame_loglik_full_device": (lambda: frame_loglik_full_device(full, X), 1),
            "gmm_stats_full_device_order1_127_segments": (lambda: gmm_stats_full_device(full, X, off, order=1), 2),
            "gmm_stats_full_device_order2_one_segment": (lambda: gmm_stats_full_device(full, X, one, order=2), 3)}
    X64 = X.double()
    mu, g = torch.as_tensor(full.mu).to(dev), torch.as_tensor(numpy.log(full.w) + numpy.log(full.cst)).to(dev)
    M = torch.as_tensor(numpy.ascontiguousarray(full.invchol.transpose(0, 2, 1))).to(dev)
    baseline = {"frame_loglik_full_device": lambda: torch_route(torch, X64, mu, M, g, one, 0),
                "gmm_stats_full_device_order1_127_segments": lambda: torch_route(torch, X64, mu, M, g, off, 1),
                "gmm_stats_full_device_order2_one_segment": lambda: torch_route(torch, X64, mu, M, g, one, 2)}
    slabs1, slabs2 = mixture_full._slabs(int(numpy.diff(off).max()), C), mixture_full._slabs(N, C)
    workspace = {"frame_loglik_full_device": 0,
                 "gmm_stats_full_device_order1_127_segments": slabs1 * (len(off) - 1) * C * (1 + D) * 8 if slabs1 > 1 else 0,
                 "gmm_stats_full_device_order2_one_segment": slabs2 * C * (1 + D + D * D) * 8 if slabs2 > 1 else 0}
    times = {name: [] for name in runs}
    for rep in range(REPS + 1):
        for name, (fn, _) in runs.items():
            t = timed(torch, fn, INNER)
            if rep:   # round 0 warms every shape up
                times[name].append(t)
    out = {"segments": len(off) - 1}
    for name, (fn, gemms) in runs.items():
        t = times[name]
        r = {"ms": t, "median_ms": median(t), "spread_ms": max(t) - min(t), "gemm_equivalents": gemms,
             "tflops": gemms * gemm / (median(t) * 1e-3) / 1e12, "peak_bytes": peak_bytes(torch, fn)}
        r["share_of_f64_matrix_rate"] = r["tflops"] / PEAK_TFLOPS
        r["library_workspace_bytes"] = workspace[name]      # the stream's lease, which torch's allocator does not see
        tt = [timed(torch, baseline[name], 1) for _ in range(TORCH_REPS + 1)][1:]
        r["torch"] = {"ms": tt, "median_ms": median(tt), "spread_ms": max(tt) - min(tt), "peak_bytes": peak_bytes(torch, baseline[name])}
        r["torch_over_kernels"] = r["torch"]["median_ms"] / r["median_ms"]
        out[name] = r
    ours, theirs = gmm_stats_full_device(full, X, one, order=2), torch_route(torch, X64, mu, M, g, one, 2)
    out["difference_to_torch_max_abs_over_largest"] = {
        k: float((a - b).abs().max() / b.abs().max()) for k, a, b in (("stat0", ours[0], theirs[1]), ("stat1", ours[1], theirs[2]),
                                                                       ("stat2", ours[2], theirs[3]))}
    del ours, theirs
    em = []
    for rep in range(REPS + 1):
        model = make_models(C)[1]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        llk = model._em_steps(X, 1)
        torch.cuda.synchronize()
        if rep:
            em.append((time.perf_counter() - t0) * 1e3)
    out["em_iteration_wall"] = {"ms": em, "median_ms": median(em), "spread_ms": max(em) - min(em), "llk": float(llk[0])}
    return out


def child(args):
    """One step in a process of its own, under its own time limit; its last output line is its JSON result."""
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, "-W", "ignore::RuntimeWarning", os.path.abspath(__file__)] + args,
                       capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"gmm_full_bench: step {args} ended with status {p.returncode}; nothing after it was started")
    print(f"gmm_full_bench: step {args} done", file=sys.stderr, flush=True)
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, type=int, choices=COMPONENTS, help="(internal) run one mixture size in this process")
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "gmm_full_bench.py measures on the GPU"
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
        print(json.dumps(step(args.step)), flush=True)
        return
    out = {"timed_rounds": REPS, "calls_per_timing": INNER, "torch_rounds": TORCH_REPS, "D": D, "frames": FRAMES, "frame_dtype": "float32",
           "f64_matrix_rate_tflops": PEAK_TFLOPS, "flop_per_gemm_equivalent": "2 N C D^2", "torch_component_chunk": CHUNK,
           "data": "synthetic: component means 0.25 apart per dimension under unit noise, random precision matrices; says nothing about speech",
           "cases": {f"C{C}": child(["--step", str(C)]) for C in COMPONENTS}}
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
