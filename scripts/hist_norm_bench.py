"""What the normalised all-pairs histograms cost, and that the unnormalised ones cost what they did (GPU box):

    python scripts/hist_norm_bench.py --parent-lib build_alt/parent/sidekit_amd/csrc/libsidekit_amd.so --out profiles/hist_norm_bench.json

N = 16 384 and 65 536 unit x-vectors of D = 256 scored against themselves, a cohort of 2 000; three measurements:

(a) ``sc_cosine_hist`` of this build against the parent commit's build of the library (``scripts/build_variant.sh parent`` run in a
    checkout of the parent), in alternating child processes -- a process holds one build -- three each: per process a warm-up call and
    ten event-timed calls per size.  The spread of the parent's own three medians is the yardstick: this build's median of medians
    must not exceed the parent's by more than it.
(b) ``sc_cosine_hist_norm`` with both pairs (s-norm) against ``sc_cosine_hist``, alternating in one process: the price of the epilogue
    (two IEEE divisions per score), reported as a ratio.
(c) at N = 16 384, the materialised route -- ``sc_cosine`` into an (N, N) float32 tensor, ``sc_norm_apply``, ``torch.histc`` over the
    matrix (one histogram, no target / non-target split: the cheaper job) -- against the matrix-free call: time and the peak of
    torch-allocated memory over the region (neither route uses the library's own workspace: the statistics are made beforehand for
    both).  At N = 65 536 only the bytes the matrix would need are recorded.

Every GPU step is a child process under its own ``timeout``; the first one that fails ends the run (no retries) and nothing is written.
"""
import argparse, ctypes, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, COHORT, SIZES, REPS, ROUNDS, STEP_TIMEOUT_S = 256, 2000, (16384, 65536), 10, 3, 240


def median(v):
    s = sorted(v)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def corpus(n, dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(n)
    x = torch.nn.functional.normalize(torch.randn(n, D, device=dev, generator=g), dim=1).contiguous()
    lab = torch.randint(0, 1000, (n,), device=dev, generator=g, dtype=torch.int32)
    return x, lab


def timed(fn, reps=1):
    import torch
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def step_hist(lib_path):
    """One build's sc_cosine_hist, bound by hand: the parent's build has no sc_cosine_hist_norm for sidekit_amd._lib to bind."""
    import torch
    from sidekit_amd import _lib
    hip_rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(hip_rt):
        ctypes.CDLL(hip_rt, mode=ctypes.RTLD_GLOBAL)
    fn = ctypes.CDLL(os.path.abspath(lib_path)).sc_cosine_hist
    fn.restype, fn.argtypes = _lib.SIGNATURES["sc_cosine_hist"]
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ht, hn = torch.empty(8192, dtype=torch.int64, device=dev), torch.empty(8192, dtype=torch.int64, device=dev)
    res = {}
    for n in SIZES:
        x, lab = corpus(n, dev)

        def call():
            assert fn(x.data_ptr(), n, x.data_ptr(), n, D, lab.data_ptr(), lab.data_ptr(), 0, -1.0, 1.0, 8192, ht.data_ptr(), hn.data_ptr(), st) == 0
        timed(call)                                                   # warm-up: the code object
        res[str(n)] = {"ms": timed(call, REPS), "pairs_counted": int(ht.sum() + hn.sum())}
        assert res[str(n)]["pairs_counted"] == n * (n - 1)
    return res


def step_norm():
    import torch
    from sidekit_amd import _lib
    from sidekit_amd import score_normalization as sn
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ht, hn = torch.empty(8192, dtype=torch.int64, device=dev), torch.empty(8192, dtype=torch.int64, device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    cohort = torch.nn.functional.normalize(torch.randn(COHORT, D, device=dev, generator=g), dim=1).contiguous()
    res = {"b": {}}
    for n in SIZES:
        x, lab = corpus(n, dev)
        mean, std = sn.cohort_stats_device(x, cohort)
        lo, hi = sn.normalised_range_from_sample(x, x, cohort, "s")
        head = (x.data_ptr(), n, x.data_ptr(), n, D, lab.data_ptr(), lab.data_ptr(), 0)
        tail = (8192, ht.data_ptr(), hn.data_ptr(), st)
        plain = lambda: _lib.check(lib.sc_cosine_hist(*head, -1.0, 1.0, *tail))
        norm = lambda: _lib.check(lib.sc_cosine_hist_norm(*head, mean.data_ptr(), std.data_ptr(), mean.data_ptr(), std.data_ptr(), lo, hi, *tail))
        timed(plain), timed(norm)
        assert int(ht.sum() + hn.sum()) == n * (n - 1)
        in_end_bins = int(ht[0] + hn[0] + ht[-1] + hn[-1])
        ts = {"plain": [], "norm": []}
        for _ in range(REPS):                                         # alternating
            ts["plain"] += timed(plain)
            ts["norm"] += timed(norm)
        res["b"][str(n)] = {"sc_cosine_hist_ms": ts["plain"], "sc_cosine_hist_norm_s_ms": ts["norm"], "hist_range": [lo, hi], "scores_in_end_bins": in_end_bins,
                            "norm_over_plain": median(ts["norm"]) / median(ts["plain"])}
        if n != SIZES[0]:
            continue

        def materialised():
            z = torch.empty((n, n), dtype=torch.float32, device=dev)
            _lib.check(lib.sc_cosine(x.data_ptr(), n, x.data_ptr(), n, D, z.data_ptr(), st))
            _lib.check(lib.sc_norm_apply(z.data_ptr(), n, n, mean.data_ptr(), std.data_ptr(), mean.data_ptr(), std.data_ptr(), st))
            return torch.histc(z, bins=8192, min=lo, max=hi)

        def region(fn):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            ms = timed(fn)[0]
            return ms, torch.cuda.max_memory_allocated(dev) - base
        region(materialised)                                          # warm-up: the allocator's blocks, histc's code
        tm, pm, tf, pf = [], 0, [], 0
        for _ in range(5):
            ms, rise = region(materialised); tm.append(ms); pm = max(pm, rise)
            ms, rise = region(norm); tf.append(ms); pf = max(pf, rise)
        res["c"] = {"N": n, "materialised": "sc_cosine into (N, N) float32 + sc_norm_apply (both pairs) + torch.histc(bins=8192) over the matrix",
                    "matrix_free": "sc_cosine_hist_norm (both pairs)", "materialised_ms": tm, "matrix_free_ms": tf,
                    "materialised_over_matrix_free": median(tm) / median(tf), "materialised_peak_torch_bytes": pm, "matrix_free_peak_torch_bytes": pf,
                    "library_workspace_bytes": 0, "score_matrix_bytes": 4 * n * n}
    res["score_matrix_bytes_at_%d" % SIZES[1]] = 4 * SIZES[1] * SIZES[1]
    return res


def child(args):
    """One GPU step in a process of its own, under its own time limit; its last output line is its JSON result."""
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"hist_norm_bench: step {args} ended with status {p.returncode}; nothing after it was started")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "build_alt", "parent", "sidekit_amd", "csrc", "libsidekit_amd.so"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=["hist", "norm"], help="(internal) run one GPU step in this process")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "hist_norm_bench.py measures on the GPU"
        print(json.dumps(step_hist(args.lib) if args.step == "hist" else step_norm()), flush=True)
        return
    from sidekit_amd import _lib
    assert os.path.exists(args.parent_lib), f"{args.parent_lib}: build the parent commit's library first (scripts/build_variant.sh parent, in a checkout of the parent)"
    runs = {"parent": [], "this": []}
    for _ in range(ROUNDS):                                           # alternating processes
        runs["parent"].append(child(["--step", "hist", "--lib", args.parent_lib]))
        runs["this"].append(child(["--step", "hist", "--lib", _lib.LIB_PATH]))
    norm = child(["--step", "norm"])
    a = {}
    for n in map(str, SIZES):
        ms = {k: [r[n]["ms"] for r in v] for k, v in runs.items()}
        med = {k: [median(r) for r in v] for k, v in ms.items()}
        spread = max(med["parent"]) - min(med["parent"])
        delta = median(med["this"]) - median(med["parent"])
        a[n] = {"parent_ms": ms["parent"], "this_ms": ms["this"], "parent_medians_ms": med["parent"], "this_medians_ms": med["this"],
                "parent_spread_ms": spread, "this_minus_parent_ms": delta, "no_slower_than_parent_within_its_spread": delta <= spread}
    out = {"D": D, "cohort": COHORT, "sizes": list(SIZES), "timed_calls_per_process_and_size": REPS, "processes_per_build": ROUNDS,
           "a_sc_cosine_hist_this_build_against_parent": a, "b_sc_cosine_hist_norm_s_against_sc_cosine_hist": norm["b"],
           "c_materialised_against_matrix_free": norm["c"], "score_matrix_bytes_at_%d" % SIZES[1]: norm["score_matrix_bytes_at_%d" % SIZES[1]]}
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
