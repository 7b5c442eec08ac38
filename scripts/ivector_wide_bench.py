"""What total variability costs at the ranks above 192 (GPU box):

    python scripts/ivector_wide_bench.py --out profiles/ivector_wide_bench.json [--sessions 1024]

Synthetic resident statistics at C = 2 048, D = 60 as in scripts/ivector_bench.py (whose generators this script imports), ranks
R = 192, 400 and 600.  Per rank, in a process of its own under its own time limit:
(a) the posterior kernel (``sc_tvw_posterior``) on one device batch: per batch and per session, and its share of the 78.6 TFLOP/s f64
    matrix rate for the Rp^3 FLOP of its tile products (Rp = R rounded up to 64; a third each in U, Y = U^-T and Y' Y);
(b) at R = 192 the same batch through ``sc_tv_posterior``;
(c) the same batch through batched float64 ``torch.linalg.cholesky`` + ``torch.cholesky_inverse`` on the same card, with torch's peak
    memory, beside the kernel's scratch;
(d) one host ``scipy.linalg.inv`` per session over 16 threads (32 sessions measured);
(e) one EM iteration by phase (event-timed, synchronised on both sides, summed over the device batches) with the device M-step and
    with the host M-step (accumulators copied to the host, ``tv_m_step``, ``F`` copied back; host clock);
(f) extraction alone (``extract_ivectors_wide_device`` with ``uncertainty``);
(g) at R = 600 the latency of a launch with 1, 4 and 256 sessions (one workgroup per session, so 1 and 4 sessions run on as many CUs).
Every GPU step is a child process under its own ``timeout``; the first one that fails ends the run (no retries) and nothing is written.
"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

C, D, RANKS, STEP_TIMEOUT_S, HOST_SESSIONS = 2048, 60, (192, 400, 600), 420, 32
PEAK_F64_TFLOPS = 78.6
WORKSPACE = 16 << 30


def step_gpu(rank, n):
    import numpy
    import scipy.linalg
    import torch
    from multiprocessing.pool import ThreadPool
    import ivector_bench as nb
    from sidekit_amd import _lib, factor_analyser as fa, factor_analyser_wide as faw
    timed = nb.timed
    dev = torch.device("cuda", 0)
    ubm = nb.make_ubm()
    F = 0.05 * numpy.random.RandomState(rank).randn(C * D, rank)
    stat0, stat1 = nb.make_statistics(torch, ubm, n, dev)
    whitener = fa._whitener(torch, ubm, dev)
    rows = faw._batch_rows(n, C, D, rank, WORKSPACE)
    Rp = (rank + 63) // 64 * 64
    res = {"R": rank, "Rp": Rp, "C": C, "D": D, "sessions": n, "device_batch_sessions": rows, "max_workspace_bytes": WORKSPACE,
           "kernel_scratch_bytes_per_session": faw.workspace_bytes(1, rank)}
    F_d = torch.as_tensor(F).to(dev)
    G = faw.tv_gram_wide_device(F_d, C)
    s0 = stat0[:rows]
    sw = fa._whiten(s0, stat1[:rows], whitener)
    Lp = fa.dgemm_nn_device(s0, G)
    B = fa.dgemm_nn_device(sw, F_d)
    e_h, out = torch.empty_like(B), torch.empty_like(Lp)
    need = faw.workspace_bytes(rows, rank)
    work = torch.empty(need // 8, dtype=torch.float64, device=dev)

    def wide(k=rows):
        _lib.launch("sc_tvw_posterior", dev, Lp, B, k, rank, 1.0, e_h, out, None, work, need)

    wide()
    ms = min(timed(wide)[0] for _ in range(3))
    flop = float(Rp) ** 3
    res["posterior_kernel"] = {"batch_sessions": rows, "ms_per_batch": ms, "us_per_session": 1e3 * ms / rows, "flop_per_session": flop,
                               "tflops": flop * rows / ms / 1e9, "share_of_f64_matrix_peak": flop * rows / ms / 1e9 / PEAK_F64_TFLOPS}
    if rank <= fa.TV_MAX_RANK:
        narrow = lambda: _lib.launch("sc_tv_posterior", dev, Lp, B, rows, rank, e_h, out, None)   # noqa: E731
        narrow()
        res["narrow_kernel_same_batch_ms"] = min(timed(narrow)[0] for _ in range(3))
    if rank == 600:
        res["latency_ms_by_sessions"] = {str(k): min(timed(lambda: wide(k))[0] for _ in range(3)) for k in (1, 4, 256)}
    # the batched torch route on the same matrices
    iu = torch.triu_indices(rank, rank, device=dev)
    lam = torch.zeros((rows, rank, rank), dtype=torch.float64, device=dev)
    lam[:, iu[0], iu[1]] = Lp
    lam[:, iu[1], iu[0]] = Lp
    lam += torch.eye(rank, dtype=torch.float64, device=dev)
    route = lambda: torch.cholesky_inverse(torch.linalg.cholesky(lam))   # noqa: E731
    inv = route()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    res["torch_cholesky_inverse_same_batch"] = {"ms": min(timed(route)[0] for _ in range(3)),
                                               "peak_bytes_above_inputs": torch.cuda.max_memory_allocated(dev) - base + lam.numel() * 8}
    wide()
    e = out[:, [i * rank - i * (i - 1) // 2 for i in range(rank)]] - e_h * e_h
    res["kernel_against_torch_route_diag_rel"] = float((e - torch.diagonal(inv, dim1=1, dim2=2)).abs().max() / torch.diagonal(inv, dim1=1, dim2=2).abs().max())
    host = lam[:HOST_SESSIONS].cpu().numpy()
    del lam, inv
    t = time.time()
    with ThreadPool(16) as pool:
        pool.map(scipy.linalg.inv, list(host))
    res["host_scipy_inv_16_threads_ms_per_session"] = 1e3 * (time.time() - t) / HOST_SESSIONS
    del work, out

    # one EM iteration by phase
    ones = torch.ones((rows, 1), dtype=torch.float64, device=dev)

    def e_step(phases):
        def add(name, fn):
            t_ms, o = timed(fn)
            phases[name] = phases.get(name, 0.0) + t_ms
            return o
        Gm = add("gram", lambda: faw.tv_gram_wide_device(F_d, C))
        acc = None
        for a in range(0, n, rows):
            b0 = stat0[a:a + rows]
            bw = add("whiten", lambda: fa._whiten(b0, stat1[a:a + rows], whitener))
            lp = add("packed_sums_gemm", lambda: fa.dgemm_nn_device(b0, Gm))
            bb = add("projection_gemm", lambda: fa.dgemm_nn_device(bw, F_d))
            eh = torch.empty_like(bb)
            add("posterior_kernel_with_scratch_allocation", lambda: faw._posterior_launch(torch, lp, bb, 1.0, eh, lp, None))
            part = add("accumulators", lambda: (fa._count_weighted_sums(b0, lp), fa.gemm_tn_device(eh, bw), fa.gemm_tn_device(ones[:b0.shape[0]], lp)))
            acc = part if acc is None else tuple(x.add_(p) for x, p in zip(acc, part))
        return acc

    e_step({})
    phases = {}
    acc = e_step(phases)
    faw.tv_m_step_device(acc[0], acc[1], acc[2], n, True)
    phases["m_step_device"], F_new = timed(lambda: faw.tv_m_step_device(acc[0], acc[1], acc[2], n, True))
    torch.cuda.synchronize()
    t = time.time()
    F_host = fa.tv_m_step(acc[0].cpu().numpy(), acc[1].cpu().numpy(), acc[2].cpu().numpy()[0], n, True)
    fa._f64(torch, F_host, dev)
    torch.cuda.synchronize()
    phases["m_step_host"] = 1e3 * (time.time() - t)
    res["em_iteration_ms"] = phases
    res["m_step_device_against_host_rel"] = float(numpy.abs(F_new.cpu().numpy() - F_host).max() / numpy.abs(F_host).max())
    faw.extract_ivectors_wide_device(stat0, stat1, ubm, F, uncertainty=True, max_workspace_bytes=WORKSPACE)
    torch.cuda.synchronize()
    t = time.time()
    faw.extract_ivectors_wide_device(stat0, stat1, ubm, F, uncertainty=True, max_workspace_bytes=WORKSPACE)
    torch.cuda.synchronize()
    res["extraction_ms"] = 1e3 * (time.time() - t)
    res["torch_peak_bytes"] = torch.cuda.max_memory_allocated(dev)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sessions", type=int, default=1024)
    ap.add_argument("--step", type=int, default=None, help="(internal) run one rank in this process")
    args = ap.parse_args()
    if args.step is not None:
        return step_gpu(args.step, args.sessions)
    record = {"C": C, "D": D, "sessions": args.sessions, "peak_f64_matrix_tflops": PEAK_F64_TFLOPS, "ranks": {}}
    for rank in RANKS:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", str(rank), "--sessions", str(args.sessions)]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(proc.stderr[-2000:])
        if proc.returncode != 0:
            sys.exit(f"rank {rank}: exit status {proc.returncode}; stopping, nothing written")
        line = [ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        record["ranks"][str(rank)] = json.loads(line[len("RESULT "):])
        print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
