"""What cohort normalisation of PLDA scores costs (GPU box):

    python scripts/plda_norm_bench.py --parent-lib build_alt/parent/sidekit_amd/csrc/libsidekit_amd.so --out profiles/plda_norm_bench.json

Resident centred float64 x-vectors of D = 256 (PLDA rank 128); three measurements:

(a) ``sc_plda_cohort_moments`` (N rows against a cohort of M) against the materialised route -- ``plda_matrix_device`` over row blocks of
    at most 1 GiB of float64 scores, ``torch.var_mean(block, dim=1, unbiased=False)`` on each -- at 16 384 x 16 384 and 100 000 x 20 000:
    each route in a process of its own (a warm-up, then five event-timed repeats), its peak device memory from ``torch.cuda.mem_get_info``
    before the first call and after it (torch's allocator and the library's workspace both still hold what the route needed), and
    ``sc_plda_fast`` over the same row blocks alone: the share of the f64 GEMM's rate that the moments kernel keeps.
(b) ``sc_plda_hist_norm`` with both pairs (s-norm) against ``sc_plda_hist``, alternating in one process, at 16 384^2 and 32 768^2.
(c) ``sc_plda_hist`` of this build against the parent commit's build (``scripts/build_variant.sh parent`` in a checkout of the parent), in
    alternating child processes -- a process holds one build -- three each, five timed calls per size: the HN_NONE instantiation is the
    parent's kernel, so this build's median of medians must lie within the spread of the parent's own three medians.

Every GPU step is a child process under its own ``timeout``; the first one that fails ends the run (no retries) and nothing is written.
"""
import argparse, ctypes, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, RANK, MOMENT_SIZES, HIST_SIZES, REPS, ROUNDS, BLOCK_BYTES, STEP_TIMEOUT_S = 256, 128, ((16384, 16384), (100000, 20000)), (16384, 32768), 5, 3, 1 << 30, 300
NB = 8192


def median(v):
    s = sorted(v)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def timed(fn, reps=1):
    import torch
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def model():
    import numpy
    from sidekit_amd import iv_scoring
    rs = numpy.random.RandomState(5)
    F = rs.randn(D, RANK) / numpy.sqrt(D)
    A = rs.randn(D, D) / numpy.sqrt(D)
    Sigma = 0.5 * (A @ A.T) + 0.5 * numpy.eye(D)
    return F, Sigma, iv_scoring.plda_parameters(numpy.zeros(D), F, Sigma)


def rows(n, seed, F, Sigma, dev):
    """n centred float64 rows with speaker structure drawn from the model, and their labels."""
    import numpy, torch
    g = torch.Generator(device=dev).manual_seed(seed)
    n_spk = max(2, n // 16)
    lab = torch.randint(0, n_spk, (n,), device=dev, generator=g, dtype=torch.int32)
    y = torch.randn(n_spk, RANK, device=dev, generator=g, dtype=torch.float64)
    chol = torch.as_tensor(numpy.linalg.cholesky(Sigma), device=dev)
    x = (y @ torch.as_tensor(F.T, device=dev))[lab.long()] + torch.randn(n, D, device=dev, generator=g, dtype=torch.float64) @ chol.T
    return x.contiguous(), lab


def step_moments(n, m, route):
    import torch
    from sidekit_amd import _lib
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    F, Sigma, (Phi, Psi, cst) = model()
    x, _ = rows(n, n, F, Sigma, dev)
    c, _ = rows(m, m + 1, F, Sigma, dev)
    phi, psi = torch.as_tensor(Phi, device=dev).contiguous(), torch.as_tensor(Psi, device=dev).contiguous()
    mean, std = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    blk = max(1, min(n, BLOCK_BYTES // (8 * m)))

    def matrix_free():
        _lib.check(lib.sc_plda_cohort_moments(x.data_ptr(), n, c.data_ptr(), m, D, phi.data_ptr(), psi.data_ptr(), float(cst), 1.0, -1, mean.data_ptr(),
                                              std.data_ptr(), st))

    def blocks(reduce):
        buf = torch.empty((blk, m), dtype=torch.float64, device=dev)
        for r0 in range(0, n, blk):
            nr = min(blk, n - r0)
            _lib.check(lib.sc_plda_fast(x[r0:].data_ptr(), nr, c.data_ptr(), m, D, phi.data_ptr(), psi.data_ptr(), float(cst), 1.0, buf.data_ptr(), st))
            if reduce:
                var, mu = torch.var_mean(buf[:nr], dim=1, unbiased=False)
                mean[r0:r0 + nr], std[r0:r0 + nr] = mu, var.sqrt()

    fn = {"matrix_free": matrix_free, "materialised": lambda: blocks(True), "gemm_alone": lambda: blocks(False)}[route]
    torch.cuda.synchronize(); torch.cuda.empty_cache(); lib.sc_release_workspace()
    free0 = torch.cuda.mem_get_info(dev)[0]
    timed(fn)                                                         # warm-up; what it allocated is still held
    peak = free0 - torch.cuda.mem_get_info(dev)[0]
    return {"ms": timed(fn, REPS), "peak_device_bytes": peak, "row_block": blk, "mean_checksum": float(mean.sum()) if route != "gemm_alone" else None,
            "std_min": float(std.min()) if route != "gemm_alone" else None}


def hist_operands(n, dev):
    import torch
    from sidekit_amd import iv_scoring
    F, Sigma, (Phi, Psi, cst) = model()
    x, lab = rows(n, n, F, Sigma, dev)
    phi, psi = torch.as_tensor(Phi, device=dev).contiguous(), torch.as_tensor(Psi, device=dev).contiguous()
    s = x[:: max(1, n // 2048)][:2048].contiguous()
    z = iv_scoring.plda_matrix_device(s, s, Phi, Psi, cst)
    z = z[~torch.eye(z.shape[0], dtype=torch.bool, device=dev)]
    zmin, zmax = float(z.min()), float(z.max())
    return x, lab, phi, psi, float(cst), zmin - 0.25 * (zmax - zmin), zmax + 0.25 * (zmax - zmin), (F, Sigma)


def step_hist(lib_path):
    """One build's sc_plda_hist, bound by hand: the parent's build lacks the new symbols sidekit_amd._lib binds."""
    import torch
    from sidekit_amd import _lib
    hip_rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(hip_rt):
        ctypes.CDLL(hip_rt, mode=ctypes.RTLD_GLOBAL)
    dll = ctypes.CDLL(os.path.abspath(lib_path))
    fast, fn = dll.sc_plda_fast, dll.sc_plda_hist
    fast.restype, fast.argtypes = _lib.SIGNATURES["sc_plda_fast"]
    fn.restype, fn.argtypes = _lib.SIGNATURES["sc_plda_hist"]
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ht, hn = torch.empty(NB, dtype=torch.int64, device=dev), torch.empty(NB, dtype=torch.int64, device=dev)
    F, Sigma, (Phi, Psi, cst) = model()
    phi, psi = torch.as_tensor(Phi, device=dev).contiguous(), torch.as_tensor(Psi, device=dev).contiguous()
    res = {}
    for n in HIST_SIZES:
        x, lab = rows(n, n, F, Sigma, dev)
        s = x[:: max(1, n // 2048)][:2048].contiguous()                # the range, from a sample scored by the build under test
        z = torch.empty((s.shape[0], s.shape[0]), dtype=torch.float64, device=dev)
        assert fast(s.data_ptr(), s.shape[0], s.data_ptr(), s.shape[0], D, phi.data_ptr(), psi.data_ptr(), float(cst), 1.0, z.data_ptr(), st) == 0
        z = z[~torch.eye(z.shape[0], dtype=torch.bool, device=dev)]
        zmin, zmax = float(z.min()), float(z.max())
        lo, hi = zmin - 0.25 * (zmax - zmin), zmax + 0.25 * (zmax - zmin)

        def call():
            assert fn(x.data_ptr(), n, x.data_ptr(), n, D, phi.data_ptr(), psi.data_ptr(), float(cst), 1.0, lab.data_ptr(), lab.data_ptr(), 0, lo, hi, NB,
                      ht.data_ptr(), hn.data_ptr(), st) == 0
        timed(call)
        res[str(n)] = {"ms": timed(call, REPS), "pairs_counted": int(ht.sum() + hn.sum())}
        assert res[str(n)]["pairs_counted"] == n * (n - 1)
    dll.sc_release_workspace()
    return res


def step_norm():
    import torch
    from sidekit_amd import _lib
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ht, hn = torch.empty(NB, dtype=torch.int64, device=dev), torch.empty(NB, dtype=torch.int64, device=dev)
    res = {}
    for n in HIST_SIZES:
        x, lab, phi, psi, cst, lo, hi, (F, Sigma) = hist_operands(n, dev)
        c, _ = rows(2000, 7, F, Sigma, dev)
        me, se, mt, sd = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(4))
        psi_t = psi.t().contiguous()
        for mean, std, p in ((me, se, psi), (mt, sd, psi_t)):
            _lib.check(lib.sc_plda_cohort_moments(x.data_ptr(), n, c.data_ptr(), 2000, D, phi.data_ptr(), p.data_ptr(), cst, 1.0, -1, mean.data_ptr(),
                                                  std.data_ptr(), st))
        head = (x.data_ptr(), n, x.data_ptr(), n, D, phi.data_ptr(), psi.data_ptr(), cst, 1.0, lab.data_ptr(), lab.data_ptr(), 0)
        tail = (NB, ht.data_ptr(), hn.data_ptr(), st)
        plain = lambda: _lib.check(lib.sc_plda_hist(*head, lo, hi, *tail))
        norm = lambda: _lib.check(lib.sc_plda_hist_norm(*head, me.data_ptr(), se.data_ptr(), mt.data_ptr(), sd.data_ptr(), -30.0, 30.0, *tail))
        timed(plain), timed(norm)
        assert int(ht.sum() + hn.sum()) == n * (n - 1)
        ts = {"plain": [], "norm": []}
        for _ in range(REPS):                                         # alternating
            ts["plain"] += timed(plain)
            ts["norm"] += timed(norm)
        res[str(n)] = {"sc_plda_hist_ms": ts["plain"], "sc_plda_hist_norm_s_ms": ts["norm"], "norm_over_plain": median(ts["norm"]) / median(ts["plain"]),
                       "scores_in_end_bins": int(ht[0] + hn[0] + ht[-1] + hn[-1]), "cohort_std_min": float(torch.minimum(se.min(), sd.min()))}
    return res


def child(args):
    """One GPU step in a process of its own, under its own time limit; its last output line is its JSON result."""
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"plda_norm_bench: step {args} ended with status {p.returncode}; nothing after it was started")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "build_alt", "parent", "sidekit_amd", "csrc", "libsidekit_amd.so"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=["moments", "hist", "norm"], help="(internal) run one GPU step in this process")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--m", type=int, default=0)
    ap.add_argument("--route", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "plda_norm_bench.py measures on the GPU"
        res = step_moments(args.n, args.m, args.route) if args.step == "moments" else step_hist(args.lib) if args.step == "hist" else step_norm()
        print(json.dumps(res), flush=True)
        return
    from sidekit_amd import _lib
    assert os.path.exists(args.parent_lib), f"{args.parent_lib}: build the parent commit's library first (scripts/build_variant.sh parent, in a checkout of the parent)"
    a = {}
    for n, m in MOMENT_SIZES:
        r = {route: child(["--step", "moments", "--n", str(n), "--m", str(m), "--route", route]) for route in ("matrix_free", "materialised", "gemm_alone")}
        t = {k: median(v["ms"]) for k, v in r.items()}
        a[f"{n}x{m}"] = {"sc_plda_cohort_moments": r["matrix_free"], "materialised_row_blocks_plus_var_mean": r["materialised"], "sc_plda_fast_row_blocks_alone": r["gemm_alone"],
                         "materialised_over_matrix_free": t["materialised"] / t["matrix_free"], "share_of_the_f64_gemm_rate": t["gemm_alone"] / t["matrix_free"],
                         "tflops_matrix_free": 2.0 * n * m * D / (t["matrix_free"] * 1e-3) / 1e12, "cohort_matrix_bytes": 8 * n * m}
    b = child(["--step", "norm"])
    runs = {"parent": [], "this": []}
    for _ in range(ROUNDS):                                           # alternating processes
        runs["parent"].append(child(["--step", "hist", "--lib", args.parent_lib]))
        runs["this"].append(child(["--step", "hist", "--lib", _lib.LIB_PATH]))
    c = {}
    for n in map(str, HIST_SIZES):
        med = {k: [median(r[n]["ms"]) for r in v] for k, v in runs.items()}
        spread = max(med["parent"]) - min(med["parent"])
        delta = median(med["this"]) - median(med["parent"])
        c[n] = {"parent_medians_ms": med["parent"], "this_medians_ms": med["this"], "parent_spread_ms": spread, "this_minus_parent_ms": delta,
                "this_over_parent": median(med["this"]) / median(med["parent"]), "within_the_parents_own_spread": abs(delta) <= spread}
    out = {"D": D, "rank": RANK, "timed_calls": REPS, "processes_per_build": ROUNDS, "a_cohort_moments_against_the_materialised_route": a,
           "b_sc_plda_hist_norm_s_against_sc_plda_hist": b, "c_sc_plda_hist_this_build_against_parent": c}
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
