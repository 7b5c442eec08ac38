"""PLDA training on resident x-vectors against the host (GPU box): N = 1 048 576 float32 x-vectors, D = 256, 6 000 classes with a
long-tailed count distribution, rank 128, 10 iterations.

    python scripts/plda_train_bench.py > profiles/plda_train_bench.json                      # (a) device, (b) host restatement, scatter roof
    rocprofv3 --kernel-trace --stats -d DIR -o plda -- python scripts/plda_train_bench.py --one-call
    python scripts/plda_train_bench.py --kernel-stats DIR/.../plda_kernel_stats.csv ...       # (c) folds the per-kernel times in

(a) ``plda_device`` timed with events after a warm-up call, median of five.  (b) the tests' numpy restatement
(tests/tools/plda_em_numpy.py, eigen form) on the same values widened to float64, at the thread count the environment sets: the
stand-in for the reference, whose class sums alone are one Python pass over all N model ids per class.  The scatter kernel
(``dgemm_tn_kernel``, K = N) is set beside ``sc_plda_fast`` at 16 384^2 as scripts/scoring_bench.py times it, in the same process.
"""
import argparse, csv, ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import numpy
import torch
from sidekit_amd import _lib, factor_analyser as fa

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--classes", type=int, default=6000)
ap.add_argument("--one-call", action="store_true", help="one warm-up and one plda_device call, nothing else (for a kernel trace)")
ap.add_argument("--no-host", action="store_true", help="skip the host restatement")
ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of --one-call")
args = ap.parse_args()
N, D, C, RANK, ITERS = args.n, 256, args.classes, 128, 10
F64_PEAK = 78.6
dev = torch.device("cuda", 0)
rs = numpy.random.RandomState(0)
p = 1.0 / numpy.arange(1, C + 1) ** 0.8                      # long tail: a few classes of thousands of sessions, most of a few dozen
lab = numpy.concatenate((numpy.arange(C), rs.choice(C, N - C, p=p / p.sum())))
rs.shuffle(lab)
g = torch.Generator(device=dev).manual_seed(0)
centres = torch.randn(C, D, device=dev, generator=g)
xv = centres[torch.as_tensor(lab, device=dev)] + 1.5 * torch.randn(N, D, device=dev, generator=g)
xv = torch.nn.functional.normalize(xv, dim=1).contiguous()  # float32, as the extractor leaves them
del centres
counts = numpy.bincount(lab)


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); r = fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b), r


model = fa.plda_device(xv, lab, RANK, ITERS)                  # warm-up: workspace, code objects
if args.one_call:
    fa.plda_device(xv, lab, RANK, ITERS)
    torch.cuda.synchronize()
    sys.exit(0)
out = {"N": N, "D": D, "classes": C, "rank": RANK, "iterations": ITERS, "input": "float32, resident",
       "sessions_per_class": {"min": int(counts.min()), "median": float(numpy.median(counts)), "max": int(counts.max())}}
out["a_plda_device_ms"] = sorted(device_ms(lambda: fa.plda_device(xv, lab, RANK, ITERS))[0] for _ in range(5))
out["a_plda_device_ms_median"] = out["a_plda_device_ms"][2]
index = fa.ClassIndex(lab)
torch.cuda.synchronize()
out["class_sums_ms_median"] = sorted(device_ms(lambda: fa.class_sums_device(xv, index))[0] for _ in range(5))[2]
mean_d = (fa.class_sums_device(xv, index)[1] / N)
t = sorted(device_ms(lambda: fa.gemm_tn_device(xv, None, None, mean_d, mean_d))[0] for _ in range(5))[2]
fl = 2.0 * N * D * D
out["scatter"] = {"kernel": "dgemm_tn_kernel<4, float> + slab_reduce_kernel (sc_gemm_tn, K = N)", "ms_median": t, "TFLOP/s": fl / t / 1e9,
                  "frac_f64_peak": fl / t / 1e9 / F64_PEAK}
M = 16384
e, tt = torch.randn(M, D, device=dev, dtype=torch.float64), torch.randn(M, D, device=dev, dtype=torch.float64)
phi, psi = torch.randn(D, D, device=dev, dtype=torch.float64) / D, torch.randn(D, D, device=dev, dtype=torch.float64) / D
od = torch.empty(M, M, device=dev, dtype=torch.float64)
st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
run = lambda: _lib.check(_lib.lib().sc_plda_fast(e.data_ptr(), M, tt.data_ptr(), M, D, phi.data_ptr(), psi.data_ptr(), 0.5, 1.0, od.data_ptr(), st))
run(); torch.cuda.synchronize()
t = sorted(device_ms(run)[0] for _ in range(5))[2]
fl = 2.0 * M * M * D + 3 * 2.0 * M * D * D
out["sc_plda_fast_16384"] = {"kernel": "plda_prep_kernel + dgemm_nt_kernel<4>", "ms_median": t, "TFLOP/s": fl / t / 1e9, "frac_f64_peak": fl / t / 1e9 / F64_PEAK}
out["scatter_frac_of_dgemm_nt_frac"] = out["scatter"]["frac_f64_peak"] / out["sc_plda_fast_16384"]["frac_f64_peak"]
del e, tt, od
if not args.no_host:
    import plda_em_numpy as pen
    X = xv.cpu().numpy()
    t0 = time.perf_counter()
    host = pen.em(X, lab, RANK, ITERS)
    out["b_host_restatement_s"] = time.perf_counter() - t0
    out["b_host_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or None
    out["speedup_a_over_b"] = out["b_host_restatement_s"] * 1e3 / out["a_plda_device_ms_median"]
    out["device_vs_host"] = {"Sigma": float(pen.rel(model[2], host[2])), "FF'": float(pen.rel(model[1].dot(model[1].T), host[1].dot(host[1].T)))}
if args.kernel_stats:
    with open(args.kernel_stats) as f:
        rows = list(csv.DictReader(f))
    out["c_kernel_stats_one_call_plus_warmup"] = [{"kernel": r["Name"][:120], "calls": int(r["Calls"]), "total_us": float(r["TotalDurationNs"]) / 1e3,
                                                   "percent": float(r["Percentage"])} for r in rows if float(r["Percentage"]) >= 0.05]
print(json.dumps(out, indent=1))
