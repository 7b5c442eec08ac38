"""What joint factor analysis costs in time and memory (GPU box):

    python scripts/jfa_bench.py --out profiles/jfa_bench.json [--sessions 8192]

Synthetic resident statistics at C = 2 048, D = 60 (``stat0`` (N, C), ``stat1`` (N, C D), float64, generated on the device from a seed),
N = 8 192 sessions of 1 024 models, ranks of 100.  Three steps, each a child process under its own ``timeout``:
(a) ``sc_jfa_shift`` (one call: gather, low-rank product, shift, centring, whitening) against the unfused route on the same card in the
    same process, twice: the product by ``torch.matmul`` and by ``sc_dgemm_nn``, each followed by torch element-wise operations.  The
    three routes alternate, REPEATS times after a warm-up of each; per route the median, the fastest and the slowest time (device
    events, synchronised on both sides) and torch's peak allocation above what was resident before the call.  The bytes the pass has to
    move (read ``stat1``, write ``out``) over the median give the achieved bandwidth.
(b) one within-class EM iteration end to end (``_e_step`` over all sessions in device batches, then the host M-step with its copies),
    host clock around synchronised work, after one warm-up iteration.
(c) ``jfa_score_device`` at 1 024 models against all the sessions as segments, host clock around a synchronised call, after a warm-up
    on a slice.
The first step that fails ends the run (no retries) and nothing is written.
"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, D, SESSIONS, MODELS, RANK, REPEATS, STEP_TIMEOUT_S = 2048, 60, 8192, 1024, 100, 7, 420
WORKSPACE = 4 << 30


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); out = fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b), out


def make_ubm(seed=1):
    import numpy
    from sidekit_amd.mixture import Mixture
    rs = numpy.random.RandomState(seed)
    m = Mixture()
    w = rs.rand(C) + 0.5
    m.w, m.mu, m.invcov = w / w.sum(), 2.0 * rs.randn(C, D), 1.0 / (0.5 + rs.rand(C, D))
    m.cov_var_ctl = 1.0 / m.invcov
    m.cst, m.det = numpy.zeros(C), numpy.zeros(C)
    m._compute_all()
    return m


def make_statistics(torch, ubm, n, dev):
    """about 3 000 frames per session spread over the components; first-order statistics around the means"""
    g = torch.Generator(device=dev).manual_seed(7)
    mu, sd = torch.as_tensor(ubm.mu).to(dev), torch.as_tensor(ubm.invcov).to(dev).rsqrt()
    stat0 = torch.empty((n, C), dtype=torch.float64, device=dev)
    stat1 = torch.empty((n, C * D), dtype=torch.float64, device=dev)
    for a in range(0, n, 1024):
        b = min(n, a + 1024)
        s0 = 3000.0 / C * 2.0 * torch.rand((b - a, C), dtype=torch.float64, device=dev, generator=g)
        noise = torch.randn((b - a, C, D), dtype=torch.float64, device=dev, generator=g)
        stat0[a:b] = s0
        stat1[a:b] = (s0[:, :, None] * mu + s0.sqrt()[:, :, None] * sd * (noise + 0.2)).view(b - a, C * D)
    return stat0, stat1


def setup(n):
    import numpy
    import torch
    dev = torch.device("cuda", 0)
    ubm = make_ubm()
    stat0, stat1 = make_statistics(torch, ubm, n, dev)
    rs = numpy.random.RandomState(5)
    models = max(1, min(MODELS, n))
    labels = rs.permutation(numpy.arange(n) % models)
    return torch, dev, ubm, stat0, stat1, labels, rs


def step_shift(n):
    import numpy
    from sidekit_amd import factor_analyser as fa, jfa_scoring as js
    torch, dev, ubm, stat0, stat1, labels, rs = setup(n)
    models = int(labels.max()) + 1
    W = torch.as_tensor(0.05 * rs.randn(C * D, RANK)).to(dev)
    Wt = W.t().contiguous()
    H = torch.as_tensor(rs.randn(models, RANK)).to(dev)
    rows = torch.as_tensor(labels.astype(numpy.int32)).to(dev)
    rows64 = rows.long()
    mean = torch.as_tensor(ubm.get_mean_super_vector()).to(dev)
    scale = torch.as_tensor(ubm.get_invcov_super_vector()).to(dev).sqrt()
    out = torch.empty_like(stat1)

    def finish(product):
        return ((stat1.view(n, C, D) - stat0[:, :, None] * (mean.view(1, C, D) + product.view(n, C, D))) * scale.view(1, C, D)).view(n, C * D)

    routes = {"sc_jfa_shift": lambda: js.jfa_shift_device(stat0, stat1, W, H, rows, mean, scale, out=out),
              "torch_matmul_and_elementwise": lambda: finish(torch.matmul(H[rows64], Wt)),
              "sc_dgemm_nn_and_elementwise": lambda: finish(fa.dgemm_nn_device(H[rows64], Wt))}
    res = {"sessions": n, "models": models, "C": C, "D": D, "R": RANK, "repeats": REPEATS,
           "resident_bytes_before_the_call": (stat0.numel() + stat1.numel() + out.numel() + W.numel() + Wt.numel()) * 8,
           "bytes_the_pass_must_move": 2 * stat1.numel() * 8, "product_flop": 2.0 * n * C * D * RANK}
    want = routes["sc_jfa_shift"]().clone()
    times, peaks = {k: [] for k in routes}, {}
    for name, fn in routes.items():   # warm-up, agreement and peak memory of every route
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        got = fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated(dev) - base
        res.setdefault("relative_max_difference_to_sc_jfa_shift", {})[name] = float((got - want).abs().max() / want.abs().max())
        del got
    for _ in range(REPEATS):
        for name, fn in routes.items():
            ms, got = timed(fn)
            times[name].append(ms)
            del got
    for name in routes:
        res[name] = {"median_ms": statistics.median(times[name]), "fastest_ms": min(times[name]), "slowest_ms": max(times[name]),
                     "all_ms": times[name], "torch_peak_bytes_above_resident": peaks[name]}
    fused = res["sc_jfa_shift"]
    fused["gathered_factors_workspace_bytes"] = n * RANK * 8   # the library's own allocation, outside torch's count
    fused["achieved_bytes_per_s_over_the_bytes_the_pass_must_move"] = res["bytes_the_pass_must_move"] / (fused["median_ms"] * 1e-3)
    fused["product_tflops"] = res["product_flop"] / (fused["median_ms"] * 1e-3) * 1e-12
    for name in ("torch_matmul_and_elementwise", "sc_dgemm_nn_and_elementwise"):
        res[name]["median_over_sc_jfa_shift_median"] = res[name]["median_ms"] / fused["median_ms"]
        res[name]["fastest_over_sc_jfa_shift_slowest"] = res[name]["fastest_ms"] / fused["slowest_ms"]
    return res


def step_within(n):
    import numpy
    from sidekit_amd import factor_analyser as fa, jfa_scoring as js
    torch, dev, ubm, stat0, stat1, labels, rs = setup(n)
    models = int(labels.max()) + 1
    F = torch.as_tensor(0.05 * rs.randn(C * D, RANK)).to(dev)
    y = torch.as_tensor(rs.randn(models, RANK)).to(dev)
    G = 0.05 * rs.randn(C * D, RANK)
    rows = torch.as_tensor(labels.astype(numpy.int32)).to(dev)
    mean = torch.as_tensor(ubm.get_mean_super_vector()).to(dev)
    scale = torch.as_tensor(ubm.get_invcov_super_vector()).to(dev).sqrt()
    batch = fa._batch_rows(n, C, D, RANK, WORKSPACE)

    def iteration():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc = js._e_step(torch, stat0, stat1, G, mean, scale, batch, F, y, rows)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        new = fa.tv_m_step(*acc, n, True)
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, new

    iteration()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    e_ms, m_ms, new = iteration()
    return {"sessions": n, "models": models, "rank_f": RANK, "rank_g": RANK, "device_batch_sessions": batch, "max_workspace_bytes": WORKSPACE,
            "e_step_with_the_copy_of_the_accumulators_ms": e_ms, "host_m_step_ms": m_ms, "iteration_ms": e_ms + m_ms,
            "torch_peak_bytes_above_the_resident_statistics": torch.cuda.max_memory_allocated(dev) - base,
            "resident_statistics_bytes": (stat0.numel() + stat1.numel()) * 8, "G_finite_after_the_iteration": bool(numpy.isfinite(new).all())}


def step_score(n):
    import numpy
    from sidekit_amd import jfa_scoring as js
    torch, dev, ubm, stat0, stat1, labels, rs = setup(n)
    models = int(labels.max()) + 1
    mean, sigma = ubm.get_mean_super_vector(), 1.0 / ubm.get_invcov_super_vector()
    rank = 96   # y and x of a model are estimated jointly: the two ranks together stay within the posterior's 192
    V, U, Dm = 0.05 * rs.randn(C * D, rank), 0.05 * rs.randn(C * D, rank), 0.1 * (0.5 + rs.rand(C * D))
    e0, e1 = stat0[:models].clone(), stat1[:models].clone()
    js.jfa_score_device(ubm, e0[:64], e1[:64], stat0[:64], stat1[:64], mean, sigma, V, U, Dm)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.perf_counter()
    scores = js.jfa_score_device(ubm, e0, e1, stat0, stat1, mean, sigma, V, U, Dm)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return {"models": models, "segments": n, "rank_v": rank, "rank_u": rank, "ms": ms, "scoring_bytes": js.SCORING_BYTES,
            "final_product_flop": 2.0 * models * n * C * D, "torch_peak_bytes_above_resident": torch.cuda.max_memory_allocated(dev) - base,
            "scores_finite": bool(torch.isfinite(scores).all()), "trials_per_s": models * n / (ms * 1e-3)}


STEPS = {"shift": step_shift, "within": step_within, "score": step_score}


def child(args):
    """One step in a process of its own, under its own time limit; its last output line is its JSON result."""
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"jfa_bench: step {args} ended with status {p.returncode}; nothing after it was started")
    print(f"jfa_bench: step {args} done", file=sys.stderr, flush=True)
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sessions", type=int, default=SESSIONS)
    ap.add_argument("--step", default=None, choices=tuple(STEPS), help="(internal) run one step in this process")
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "jfa_bench.py measures on the GPU"
        print(json.dumps(STEPS[args.step](args.sessions)), flush=True)
        return
    out = {"a_shift_fused_against_unfused": child(["--step", "shift", "--sessions", str(args.sessions)]),
           "b_within_class_em_iteration": child(["--step", "within", "--sessions", str(args.sessions)]),
           "c_jfa_score_device": child(["--step", "score", "--sessions", str(args.sessions)])}
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
