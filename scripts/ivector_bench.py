"""What total-variability training and i-vector extraction cost in time and memory (GPU box):

    python scripts/ivector_bench.py --out profiles/ivector_bench.json [--sessions 100000]

Synthetic resident statistics at C = 2 048, D = 60 (``stat0`` (N, C), ``stat1`` (N, C D), float64, generated on the device from a seed),
ranks R = 128 and R = 192.  Per rank, in a process of its own:
(a) one EM iteration split into its phases, each event-timed and synchronised on both sides, summed over the device batches: the Gram
    matrices (``sc_tv_gram``), whitening (torch element-wise), the packed sums ``stat0 . G`` and the projections ``S_w . F``
    (``sc_dgemm_nn``), the posterior kernel (``sc_tv_posterior``), the three accumulators (``sc_gemm_tn``), and the host M-step with the
    copy of the accumulators to the host and of the new ``F`` back (host clock).  A warm-up batch of every shape runs first.
(b) extraction alone (``extract_ivectors_device`` with ``uncertainty``), host clock around a synchronised call.
(c) the posterior kernel's rates: the R^3 FLOP per session the algorithm needs (three triangular stages of R^3 / 6 multiply-adds), the
    FP64 operations it executes (ten per term: the dots are compensated) beside the 78.6 TFLOP/s vector peak, and the time its LDS reads
    (two of 8 bytes per term) would take at 256 B / clk / CU on 256 CUs at 2.4 GHz.
(d) peak device memory: ``torch.cuda.mem_get_info`` before and after, and torch's own peak, over (a) and (b).
(e) the batched torch route over the same unpacked matrices when ``torch.linalg.cholesky`` + ``torch.cholesky_inverse`` run on the
    build: its time and peak memory for one device batch, beside the posterior kernel's for the same batch.
and once, on the host: (f) the same E-step by the numpy restatement (tests/tools/ivector_numpy.py) over 300 sessions, one batch of the
reference, scaled to the corpus.

The E-step's cost is proportional to the sessions, so ``--sessions`` below the corpus's 100 000 measures a part and the record states
both what was measured and the figure scaled to 100 000 (the Gram matrices and the M-step do not scale and are not scaled).  Every GPU
step is a child process under its own ``timeout``; the first one that fails ends the run (no retries) and nothing is written.
"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

C, D, CORPUS, RANKS, HOST_SESSIONS, STEP_TIMEOUT_S = 2048, 60, 100000, (128, 192), 300, 900
PEAK_F64_TFLOPS, LDS_BYTES_PER_S = 78.6, 256 * 256 * 2.4e9
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


def step_gpu(rank, n):
    import numpy
    import torch
    from sidekit_amd import _lib, factor_analyser as fa
    dev = torch.device("cuda", 0)
    ubm = make_ubm()
    F = 0.05 * numpy.random.RandomState(rank).randn(C * D, rank)
    P = fa.packed_size(rank)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(dev)
    stat0, stat1 = make_statistics(torch, ubm, n, dev)
    whitener = fa._whitener(torch, ubm, dev)
    rows = fa._batch_rows(n, C, D, rank, WORKSPACE)
    ones = torch.ones((rows, 1), dtype=torch.float64, device=dev)
    res = {"R": rank, "P": P, "C": C, "D": D, "sessions_measured": n, "device_batch_sessions": rows, "max_workspace_bytes": WORKSPACE,
           "resident_statistics_bytes": (stat0.numel() + stat1.numel()) * 8}

    def e_step(F_d, phases):
        def add(name, fn):
            ms, out = timed(fn)
            phases[name] = phases.get(name, 0.0) + ms
            return out
        G = add("gram", lambda: fa.tv_gram_device(F_d, C))
        acc = None
        for a in range(0, n, rows):
            s0 = stat0[a:a + rows]
            sw = add("whiten", lambda: fa._whiten(s0, stat1[a:a + rows], whitener))
            Lp = add("packed_sums_gemm", lambda: fa.dgemm_nn_device(s0, G))
            B = add("projection_gemm", lambda: fa.dgemm_nn_device(sw, F_d))
            e_h = torch.empty_like(B)
            add("posterior_kernel", lambda: _lib.launch("sc_tv_posterior", dev, Lp, B, Lp.shape[0], rank, e_h, Lp, None))
            part = add("accumulators", lambda: (fa.gemm_tn_device(s0, Lp), fa.gemm_tn_device(e_h, sw), fa.gemm_tn_device(ones[:s0.shape[0]], Lp)))
            acc = part if acc is None else tuple(t.add_(p) for t, p in zip(acc, part))
        return acc

    F_d = torch.as_tensor(F).to(dev)
    warm = {}
    # warm-up: one full batch and the tail batch's shapes
    e_step(F_d, warm)
    torch.cuda.reset_peak_memory_stats(dev)
    phases = {}
    acc = e_step(F_d, phases)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _A, _C, _R = acc[0].cpu().numpy(), acc[1].cpu().numpy(), acc[2].cpu().numpy()[0]
    t1 = time.perf_counter()
    F_new = fa.tv_m_step(_A, _C, _R, n, True)
    t2 = time.perf_counter()
    F_back = torch.as_tensor(F_new).to(dev)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    phases["host_m_step_with_transfers"] = (t3 - t0) * 1e3
    res["m_step_parts_ms"] = {"accumulators_to_host": (t1 - t0) * 1e3, "solves_and_cholesky": (t2 - t1) * 1e3, "F_to_device": (t3 - t2) * 1e3}
    res["F_finite_after_the_iteration"] = bool(numpy.isfinite(F_new).all())
    scale = CORPUS / float(n)
    fixed = ("gram", "host_m_step_with_transfers")
    res["em_iteration_phases_ms"] = phases
    res["em_iteration_ms"] = sum(phases.values())
    res["em_iteration_phases_scaled_to_the_corpus_ms"] = {k: v if k in fixed else v * scale for k, v in phases.items()}
    res["em_iteration_scaled_to_the_corpus_ms"] = sum(res["em_iteration_phases_scaled_to_the_corpus_ms"].values())
    res["m_step_share_of_the_scaled_iteration"] = phases["host_m_step_with_transfers"] / res["em_iteration_scaled_to_the_corpus_ms"]
    gemm_flop = {"packed_sums_gemm": 2.0 * n * C * P, "projection_gemm": 2.0 * n * C * D * rank,
                 "accumulators": 2.0 * n * (C * P + rank * C * D + P)}
    res["gemm_tflops"] = {k: v / phases[k] * 1e-9 for k, v in gemm_flop.items()}
    terms = n * rank ** 3 / 2.0
    pk = phases["posterior_kernel"] * 1e-3
    res["posterior_kernel"] = {"ms": phases["posterior_kernel"], "us_per_session": pk / n * 1e6, "algorithm_gflops": 2.0 * terms / pk * 1e-9,
                               "executed_fp64_tflops_counting_ten_per_term": 10.0 * terms / pk * 1e-12,
                               "share_of_the_f64_vector_peak": 10.0 * terms / pk * 1e-12 / PEAK_F64_TFLOPS,
                               "lds_read_bytes": 16.0 * terms, "lds_bound_ms": 16.0 * terms / LDS_BYTES_PER_S * 1e3,
                               "time_over_lds_bound": pk / (16.0 * terms / LDS_BYTES_PER_S),
                               "lds_bytes_per_workgroup": (P + 3 * rank + 512) * 8}
    # extraction alone
    fa.extract_ivectors_device(stat0[:rows], stat1[:rows], ubm, F_back, uncertainty=True, max_workspace_bytes=WORKSPACE)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    iv, sigma = fa.extract_ivectors_device(stat0, stat1, ubm, F_back, uncertainty=True, max_workspace_bytes=WORKSPACE)
    torch.cuda.synchronize()
    res["extraction_ms"] = (time.perf_counter() - t0) * 1e3
    res["extraction_scaled_to_the_corpus_ms"] = res["extraction_ms"] * scale
    res["ivectors_finite"] = bool(torch.isfinite(iv).all() and torch.isfinite(sigma).all())
    free1, _ = torch.cuda.mem_get_info(dev)
    res["device_memory_taken_bytes_with_the_statistics"] = free0 - free1
    res["torch_peak_bytes_with_the_statistics"] = torch.cuda.max_memory_allocated(dev)
    # the batched torch route on one device batch, beside the posterior kernel on the same batch
    b = min(rows, n)
    s0, sw = stat0[:b], fa._whiten(stat0[:b], stat1[:b], whitener)
    G = fa.tv_gram_device(F_back, C)
    Lp, B = fa.dgemm_nn_device(s0, G), fa.dgemm_nn_device(sw, F_back)
    e_h = torch.empty_like(B)
    diag = torch.empty_like(B)
    ours_ms, _ = timed(lambda: _lib.launch("sc_tv_posterior", dev, Lp, B, b, rank, e_h, None, diag))
    route = {"sessions": b, "posterior_kernel_ms_same_batch": ours_ms}
    try:
        iu = torch.triu_indices(rank, rank, device=dev)

        def torch_route():
            full = torch.zeros((b, rank, rank), dtype=torch.float64, device=dev)
            full[:, iu[0], iu[1]] = Lp
            full = full + full.transpose(1, 2) - torch.diag_embed(full.diagonal(dim1=1, dim2=2)) + torch.eye(rank, dtype=torch.float64, device=dev)
            inv = torch.cholesky_inverse(torch.linalg.cholesky(full))
            eh = torch.einsum("nij,nj->ni", inv, B)
            return eh, inv + eh[:, :, None] * eh[:, None, :]
        torch_route()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        ms, (eh, _) = timed(torch_route)
        route.update(torch_ms=ms, torch_peak_bytes=torch.cuda.max_memory_allocated(dev) - base,
                     e_h_relative_max_difference=float((eh - e_h).abs().max() / eh.abs().max()))
    except Exception as exc:   # the build lacks the batched routine: recorded, not a failure of the run
        route["torch_route_not_available"] = repr(exc)[:300]
    res["batched_torch_route"] = route
    return res


def step_numpy(rank):
    import numpy
    import ivector_numpy as ivn
    ubm = make_ubm()
    rs = numpy.random.RandomState(3)
    n = HOST_SESSIONS
    stat0 = 3000.0 / C * 2.0 * rs.rand(n, C)
    stat1 = (stat0[:, :, None] * ubm.mu + numpy.sqrt(stat0)[:, :, None] / numpy.sqrt(ubm.invcov) * (rs.randn(n, C, D) + 0.2)).reshape(n, C * D)
    F = 0.05 * numpy.random.RandomState(rank).randn(C * D, rank)
    t0 = time.perf_counter()
    G = ivn.gram(F, C, D)
    t1 = time.perf_counter()
    sw = ivn.whiten(stat0, stat1, ubm.mu, ubm.invcov)
    e_h, e_hh = ivn.e_step(stat0, sw, F, G)
    acc = ivn.accumulate(stat0, sw, e_h, e_hh)
    t2 = time.perf_counter()
    return {"R": rank, "sessions": n, "threads": int(os.environ.get("OMP_NUM_THREADS", "0")), "gram_ms": (t1 - t0) * 1e3, "batch_ms": (t2 - t1) * 1e3,
            "scaled_to_the_corpus_ms": (t2 - t1) * 1e3 * CORPUS / n + (t1 - t0) * 1e3, "check": float(acc[2].sum())}


def child(args):
    """One step in a process of its own, under its own time limit; its last output line is its JSON result."""
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"ivector_bench: step {args} ended with status {p.returncode}; nothing after it was started")
    print(f"ivector_bench: step {args} done", file=sys.stderr, flush=True)
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sessions", type=int, default=CORPUS, help="sessions measured (the corpus the figures are scaled to: 100 000)")
    ap.add_argument("--step", default=None, choices=("gpu", "numpy"), help="(internal) run one step in this process")
    ap.add_argument("--rank", type=int, default=RANKS[0])
    args = ap.parse_args()
    if args.step:
        if args.step == "gpu":
            import torch
            assert torch.cuda.is_available(), "ivector_bench.py measures on the GPU"
        res = step_gpu(args.rank, args.sessions) if args.step == "gpu" else step_numpy(args.rank)
        print(json.dumps(res), flush=True)
        return
    out = {"corpus_sessions": CORPUS, "f64_peak_tflops": PEAK_F64_TFLOPS, "lds_peak_bytes_per_s": LDS_BYTES_PER_S}
    for rank in RANKS:
        gpu = child(["--step", "gpu", "--rank", str(rank), "--sessions", str(args.sessions)])
        host = child(["--step", "numpy", "--rank", str(rank)])
        e_step_scaled = gpu["em_iteration_scaled_to_the_corpus_ms"] - gpu["em_iteration_phases_ms"]["host_m_step_with_transfers"]
        out[f"rank_{rank}"] = {"device": gpu, "host_numpy_restatement_one_reference_batch": host,
                               "host_e_step_over_device_e_step_at_the_corpus": host["scaled_to_the_corpus_ms"] / e_step_scaled}
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
