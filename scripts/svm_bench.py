"""What training the SVM back end costs in time and memory (GPU box):

    python scripts/svm_bench.py --out profiles/svm_bench.json [--models 1024] [--background 1024 4096]

M = 1 024 single-session models against B background supervectors of D = 512 x 60, seeded float64 data resident on the device.  Per B, two
child processes, each under its own ``timeout``:
(a) ``device``: after a warm-up of every shape, REPEATS rounds of the parts of ``svm_train_device`` one by one -- the Gram GEMMs (background
    block, target rows, the targets' own blocks), the solver (``sc_svm_train``, one workgroup per model), the ``W`` GEMM -- and of the whole
    of ``svm_train_device``; device events, synchronised on both sides; the median, the fastest and the slowest.  Torch's peak allocation
    above the resident supervectors during the whole call; the iterations the models took.  It leaves the Gram blocks of the first
    ``--baseline-models`` models in a temporary file for (b).
(b) ``baseline``: what a user has today -- the same Gram copied to the host and one scikit-learn libsvm fit per model
    (``SVC(kernel='precomputed')`` at libsvm's defaults, the reference's cost) over 16 worker processes, the machine's CPU allowance; a
    subset of the models, host clock, extrapolated to M in proportion.  This process never opens the GPU.
The first step that fails ends the run (no retries) and nothing is written.
"""
import argparse, json, os, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, MODELS, BACKGROUND, REPEATS, STEP_TIMEOUT_S, WORKERS = 512 * 60, 1024, (1024, 4096), 5, 420, 16


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); out = fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b), out


def spread(ms):
    return {"median_ms": statistics.median(ms), "fastest_ms": min(ms), "slowest_ms": max(ms), "all_ms": ms}


def step_device(B, M, n_base, gram_file):
    import numpy
    import torch
    from sidekit_amd import svm_training as st
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(11)
    bg = torch.randn((B, D), dtype=torch.float64, device=dev, generator=g)
    en = torch.randn((M, D), dtype=torch.float64, device=dev, generator=g) + 0.05
    model_of = numpy.arange(M)
    en_off, ee_off = numpy.arange(M + 1), numpy.arange(M)

    def gram():
        return torch.matmul(bg, bg.t()), torch.matmul(en, bg.t()), (en * en).sum(dim=1)   # what svm_train_device forms at one session each

    k_bb, k_eb, k_ee = gram()
    cost = torch.as_tensor(1.0 / ((torch.diagonal(k_bb).sum() + k_ee) / (B + 1)).cpu().numpy()).to(dev)

    def solve():
        return st.svm_solve_device(k_bb, k_eb, k_ee, en_off, ee_off, cost)

    coef = solve()[0]

    def weights():
        return -(torch.matmul(coef[:, :B], bg) + coef[:, B:B + 1] * en)

    def whole():
        return st.svm_train_device(bg, en, model_of)

    weights(); whole()
    torch.cuda.synchronize()
    parts = {"gram_gemms": gram, "solver_sc_svm_train": solve, "w_gemm": weights, "svm_train_device": whole}
    times = {k: [] for k in parts}
    for _ in range(REPEATS):
        for name, fn in parts.items():
            ms, out = timed(fn)
            times[name].append(ms)
            del out
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    W, b, info = whole()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    iters = info["iterations"].cpu().numpy()
    numpy.savez(gram_file, k_bb=k_bb.cpu().numpy(), k_eb=k_eb[:n_base].cpu().numpy(), k_ee=k_ee[:n_base].cpu().numpy(),
                rho=b[:n_base].cpu().numpy())
    res = {"B": B, "M": M, "D": D, "points_per_problem": B + 1, "repeats": REPEATS, "eps": 1e-3,
           "lds_bytes_per_workgroup": (B + 1) * 24 + 1024, "gram_flop": 2.0 * D * (B * B + M * B + M),
           "w_gemm_flop": 2.0 * D * M * (B + 1), "resident_supervector_bytes": (bg.numel() + en.numel()) * 8,
           "torch_peak_bytes_above_resident_in_svm_train_device": peak,
           "iterations": {"min": int(iters.min()), "median": float(numpy.median(iters)), "max": int(iters.max()), "sum": int(iters.sum())},
           "all_converged": bool((info["status"] == 0).all().item()), "W_finite": bool(torch.isfinite(W).all().item())}
    for name in parts:
        res[name] = spread(times[name])
    res["gram_gemms"]["tflops"] = res["gram_flop"] / (res["gram_gemms"]["median_ms"] * 1e-3) * 1e-12
    res["w_gemm"]["tflops"] = res["w_gemm_flop"] / (res["w_gemm"]["median_ms"] * 1e-3) * 1e-12
    res["solver_sc_svm_train"]["microseconds_per_iteration_of_a_workgroup_if_all_ran_at_once"] = \
        res["solver_sc_svm_train"]["median_ms"] * 1e3 / max(1, int(iters.max()))
    return res


_GRAM = None   # a worker's copy of the Gram blocks, read once


def _load(gram_file):
    import numpy
    global _GRAM
    z = numpy.load(gram_file)
    _GRAM = z["k_bb"], z["k_eb"], z["k_ee"]


def _fit(i):
    import numpy
    from sklearn.svm import SVC
    k_bb, row, kee = _GRAM[0], _GRAM[1][i], _GRAM[2][i]
    B = k_bb.shape[0]
    t0 = time.perf_counter()
    K = numpy.empty((B + 1, B + 1))
    K[:B, :B] = k_bb
    K[B, :B] = K[:B, B] = row
    K[B, B] = kee
    clf = SVC(kernel="precomputed", C=1 / numpy.mean(numpy.diag(K)))
    clf.fit(K, numpy.array([2] * B + [1]))
    return time.perf_counter() - t0, float(-clf.intercept_[0])


def step_baseline(M, gram_file):
    import multiprocessing
    import numpy
    assert "torch" not in sys.modules
    z = numpy.load(gram_file)
    rho, n, B = z["rho"], z["k_eb"].shape[0], z["k_bb"].shape[0]
    with multiprocessing.Pool(WORKERS, initializer=_load, initargs=(gram_file,)) as pool:
        pool.map(_fit, range(min(n, WORKERS)), chunksize=1)   # the workers have read the Gram blocks and imported scikit-learn
        t0 = time.perf_counter()
        out = pool.map(_fit, range(n), chunksize=1)
        wall = time.perf_counter() - t0
    fits = [t * 1e3 for t, _ in out]
    return {"B": int(B), "models_fitted": n, "worker_processes": WORKERS, "wall_s_for_the_subset": wall,
            "extrapolated_wall_s_for_all_models": wall * M / n, "one_fit_in_its_worker": spread(fits),
            "largest_rho_difference_to_the_device_at_the_default_tolerance": float(numpy.abs(numpy.array([r for _, r in out]) - rho).max())}


def child(args):
    """One step in a process of its own, under its own time limit; its last output line is its JSON result."""
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"svm_bench: step {args} ended with status {p.returncode}; nothing after it was started")
    print(f"svm_bench: step {args} done", file=sys.stderr, flush=True)
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--models", type=int, default=MODELS)
    ap.add_argument("--background", type=int, nargs="+", default=list(BACKGROUND))
    ap.add_argument("--baseline-models", type=int, default=32, help="models the host baseline fits (extrapolated to --models)")
    ap.add_argument("--step", default=None, choices=("device", "baseline"), help="(internal) run one step in this process")
    ap.add_argument("--gram-file", default=None, help="(internal)")
    args = ap.parse_args()
    if args.step == "device":
        import torch
        assert torch.cuda.is_available(), "svm_bench.py measures on the GPU"
        print(json.dumps(step_device(args.background[0], args.models, min(args.models, args.baseline_models), args.gram_file)), flush=True)
        return
    if args.step == "baseline":
        print(json.dumps(step_baseline(args.models, args.gram_file)), flush=True)
        return
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for B in args.background:
            gram_file = os.path.join(tmp, f"gram_{B}.npz")
            common = ["--models", str(args.models), "--background", str(B), "--baseline-models", str(args.baseline_models), "--gram-file", gram_file]
            dev = child(["--step", "device"] + common)
            base = child(["--step", "baseline"] + common)
            os.remove(gram_file)
            base["extrapolated_wall_over_svm_train_device_median"] = base["extrapolated_wall_s_for_all_models"] / (dev["svm_train_device"]["median_ms"] * 1e-3)
            out[f"B_{B}"] = {"device": dev, "host_baseline_scikit_learn_libsvm": base}
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
