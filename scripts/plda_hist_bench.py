"""What the all-pairs PLDA histograms cost in time and memory against the materialised route (GPU box):

    python scripts/plda_hist_bench.py --out profiles/plda_hist_bench.json

Resident float64 x-vectors of D = 256 (PLDA rank 128), a set scored against itself, self-trials dropped; three measurements:

(a) at N = 16 384 and 32 768: ``sc_plda_hist`` (what ``iv_scoring.plda_histograms`` launches; the host algebra and the centring are done
    beforehand for both routes) against the materialised route -- ``plda_matrix_device`` over row blocks of at most 1 GiB of float64
    scores, each block binned on the device with the kernel's expression ``(v - lo) * (8192 / (hi - lo))``, floor, clip, and counted
    with ``torch.bincount`` -- in one process, alternating, after a warm-up of each, five timed repeats each (median, and the spread of
    the five).  Peak device memory of a route: ``torch.cuda.mem_get_info`` before its first call in a process whose caches were just
    released (``torch.cuda.empty_cache``, ``sc_release_workspace``) and after it, while torch's allocator still holds every block the
    route needed at its peak: the library's own workspace is seen, torch-side counters would miss it.
(b) N = 100 000 matrix-free alone (the matrix would be 80 GB): three timed calls after a warm-up.
(c) at the sizes of (a), ``sc_plda_hist`` against ``sc_plda_fast`` alone (the same preparation launch, the f64 GEMM writing its
    N x N matrix and nothing else): the share of the f64 GEMM's rate that the histogram kernel keeps.

Every GPU step is a child process under its own ``timeout``; the first one that fails ends the run (no retries) and nothing is written.
"""
import argparse, ctypes, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, RANK, SIZES, BIG, REPS, BLOCK_BYTES, STEP_TIMEOUT_S = 256, 128, (16384, 32768), 100000, 5, 1 << 30, 300
NB = 8192


def median(v):
    s = sorted(v)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)


def corpus(n, dev):
    """n centred float64 rows with speaker structure, the PLDA model they were drawn from, and the operands of the device calls."""
    import numpy, torch
    from sidekit_amd import iv_scoring
    rs = numpy.random.RandomState(5)
    F = rs.randn(D, RANK) / numpy.sqrt(D)
    A = rs.randn(D, D) / numpy.sqrt(D)
    Sigma = 0.5 * (A @ A.T) + 0.5 * numpy.eye(D)
    mu = rs.randn(D)
    Phi, Psi, cst = iv_scoring.plda_parameters(mu, F, Sigma)
    g = torch.Generator(device=dev).manual_seed(n)
    n_spk = max(2, n // 16)
    lab = torch.randint(0, n_spk, (n,), device=dev, generator=g, dtype=torch.int32)
    y = torch.randn(n_spk, RANK, device=dev, generator=g, dtype=torch.float64)
    chol = torch.as_tensor(numpy.linalg.cholesky(Sigma), device=dev)
    x = (y @ torch.as_tensor(F.T, device=dev))[lab.long()] + torch.randn(n, D, device=dev, generator=g, dtype=torch.float64) @ chol.T
    x = x.contiguous()                                                # centred: the model's mean is not added
    phi, psi = torch.as_tensor(Phi, device=dev).contiguous(), torch.as_tensor(Psi, device=dev).contiguous()
    s = x[:: max(1, n // 2048)][:2048].contiguous()
    z = iv_scoring.plda_matrix_device(s, s, Phi, Psi, cst)
    z = z[~torch.eye(z.shape[0], dtype=torch.bool, device=dev)]
    zmin, zmax = float(z.min()), float(z.max())
    del z
    return x, lab, phi, psi, float(cst), zmin - 0.25 * (zmax - zmin), zmax + 0.25 * (zmax - zmin)


def step_size(n, big):
    import torch
    from sidekit_amd import _lib
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    x, lab, phi, psi, cst, lo, hi = corpus(n, dev)
    inv_width = NB / (hi - lo)
    ht, hn = torch.empty(NB, dtype=torch.int64, device=dev), torch.empty(NB, dtype=torch.int64, device=dev)

    def matrix_free():
        _lib.check(lib.sc_plda_hist(x.data_ptr(), n, x.data_ptr(), n, D, phi.data_ptr(), psi.data_ptr(), cst, 1.0, lab.data_ptr(), lab.data_ptr(), 0,
                                    lo, hi, NB, ht.data_ptr(), hn.data_ptr(), st))

    rows = max(1, min(n, BLOCK_BYTES // (8 * n)))
    counts = torch.zeros(2 * NB, dtype=torch.int64, device=dev)

    def materialised():
        counts.zero_()
        for a in range(0, n, rows):
            b = min(a + rows, n)
            z = torch.empty((b - a, n), dtype=torch.float64, device=dev)
            _lib.check(lib.sc_plda_fast(x[a:b].data_ptr(), b - a, x.data_ptr(), n, D, phi.data_ptr(), psi.data_ptr(), cst, 1.0, z.data_ptr(), st))
            bins = ((z - lo) * inv_width).floor_().clamp_(0, NB - 1).long()
            bins += (lab[a:b, None] != lab[None, :]) * NB
            bins[torch.arange(b - a, device=dev), torch.arange(a, b, device=dev)] = 2 * NB        # the self-trials: a bin that is cut off
            counts.add_(torch.bincount(bins.reshape(-1), minlength=2 * NB + 1)[:2 * NB])

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        lib.sc_release_workspace()
        free0, _ = torch.cuda.mem_get_info(dev)
        fn()
        torch.cuda.synchronize()
        free1, _ = torch.cuda.mem_get_info(dev)
        return free0 - free1

    res = {"N": n, "hist_range": [lo, hi]}
    res["matrix_free_peak_bytes"] = peak(matrix_free)                 # also the warm-up of the route
    res["pairs_counted"] = int(ht.sum() + hn.sum())
    assert res["pairs_counted"] == n * (n - 1)
    res["scores_in_end_bins"] = int(ht[0] + hn[0] + ht[-1] + hn[-1])
    ctiles = (D + 63) // 64
    res["library_workspace_bytes"] = 8 * (((n * D + 1) & ~1) + 2 * ctiles * n)
    res["library_workspace_bytes_allocated"] = res["library_workspace_bytes"] + res["library_workspace_bytes"] // 4
    res["histogram_bytes"] = 2 * NB * 8
    if big:
        res["matrix_free_ms"] = [timed(matrix_free) for _ in range(3)]
        res["score_matrix_bytes"] = 8 * n * n
        return res
    res["materialised_peak_bytes"] = peak(materialised)
    assert torch.equal(counts[:NB], ht) and torch.equal(counts[NB:], hn), "the two routes count differently"
    res["materialised_block_rows"] = rows
    res["score_matrix_bytes"] = 8 * n * n
    tf, tm = [], []
    for _ in range(REPS):                                             # alternating
        tf.append(timed(matrix_free))
        tm.append(timed(materialised))
    res.update(matrix_free_ms=tf, materialised_ms=tm, matrix_free_spread_ms=max(tf) - min(tf), materialised_spread_ms=max(tm) - min(tm),
               materialised_over_matrix_free=median(tm) / median(tf),
               matrix_free_no_slower_than_materialised_within_the_spread=median(tf) - median(tm) <= max(max(tf) - min(tf), max(tm) - min(tm)))
    # (c) against sc_plda_fast alone, the matrix allocated once outside the timed region
    z = torch.empty((n, n), dtype=torch.float64, device=dev)
    fast = lambda: _lib.check(lib.sc_plda_fast(x.data_ptr(), n, x.data_ptr(), n, D, phi.data_ptr(), psi.data_ptr(), cst, 1.0, z.data_ptr(), st))
    timed(fast)
    th, tg = [], []
    for _ in range(REPS):
        th.append(timed(matrix_free))
        tg.append(timed(fast))
    flop = 2.0 * n * n * D
    res["c"] = {"sc_plda_hist_ms": th, "sc_plda_fast_ms": tg, "sc_plda_hist_tflops": flop / median(th) * 1e-9, "sc_plda_fast_tflops": flop / median(tg) * 1e-9,
                "share_of_the_f64_gemm_rate_kept": median(tg) / median(th)}
    return res


def child(args):
    """One GPU step in a process of its own, under its own time limit; its last output line is its JSON result."""
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"plda_hist_bench: step {args} ended with status {p.returncode}; nothing after it was started")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", type=int, default=None, metavar="N", help="(internal) run the GPU step of one size in this process")
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "plda_hist_bench.py measures on the GPU"
        print(json.dumps(step_size(args.step, args.step == BIG)), flush=True)
        return
    out = {"D": D, "plda_rank": RANK, "timed_repeats": REPS, "materialised_block_bytes_at_most": BLOCK_BYTES,
           "a_matrix_free_against_materialised": {str(n): child(["--step", str(n)]) for n in SIZES}}
    out["b_matrix_free_alone"] = child(["--step", str(BIG)])
    out["c_sc_plda_hist_against_sc_plda_fast"] = {n: r.pop("c") for n, r in out["a_matrix_free_against_materialised"].items()}
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
