"""Back-end normalisation on resident x-vectors against the host (GPU box): the corpus of scripts/plda_train_bench.py, N = 1 048 576
float32 x-vectors, D = 256, 6 000 classes with a long-tailed count distribution.

    python scripts/backend_bench.py --out profiles/backend_bench.json

(a) ``backend.lda_device`` (rank 128) and three iterations of ``sphNorm`` (``spectral_norm_estimate_device`` + ``spectral_norm_apply_device``),
timed with events after a warm-up call, median of five; the host's D x D algebra is inside the timed region.  (b) the tests' numpy
restatement (tests/tools/backend_numpy.py) on the same values widened to float64, at the thread count the environment sets: the stand-in
for the reference, which runs one Python pass over all N model ids per class.  (c) ``sc_scatter_within`` beside the plain ``sc_gemm_tn``
scatter, alternating in one process: the price of the gathered centres.  (d) ``sc_whiten_rows`` beside ``sc_dgemm_nn`` on a float64 copy
followed by a row-normalising pass: what the fusion buys.  Kernel rates are the algorithm's operations and bytes (2 N D P FLOP; the rows
read once, the result written once) over the event time of the call.  The result is rewritten after every section, so a time limit on
the host part keeps the device numbers.  None of these is a pass criterion.
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import numpy
import torch
from sidekit_amd import backend, factor_analyser as fa

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--classes", type=int, default=6000)
ap.add_argument("--no-host", action="store_true", help="skip the host restatement")
ap.add_argument("--out", default=None, help="JSON file, rewritten after every section (default: stdout at the end only)")
args = ap.parse_args()
N, D, C, RANK, IT = args.n, 256, args.classes, 128, 3
F64_PEAK = 78.6
assert torch.cuda.is_available(), "backend_bench.py measures on the GPU"
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
index = fa.ClassIndex(lab)
out = {"N": N, "D": D, "classes": C, "lda_rank": RANK, "sphnorm_iterations": IT, "input": "float32, resident", "f64_matrix_peak_TFLOP/s": F64_PEAK}


def save():
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); r = fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b), r


def median5(fn):
    fn(); torch.cuda.synchronize()                          # warm-up: workspace, code objects
    return sorted(device_ms(fn)[0] for _ in range(5))


def rates(ms, flop, nbytes):
    return {"ms_median": ms, "TFLOP/s": flop / ms / 1e9, "frac_f64_peak": flop / ms / 1e9 / F64_PEAK, "GB/s": nbytes / ms / 1e6}


def sphnorm():
    means, covs, _ = backend.spectral_norm_estimate_device(xv, index, IT, "sphNorm")
    return means, covs, backend.spectral_norm_apply_device(xv, means, covs)


# (a) the functions
t = median5(lambda: backend.lda_device(xv, index, RANK))
out["a_lda_device_ms"], out["a_lda_device_ms_median"] = t, t[2]
t = median5(sphnorm)
out["a_sphnorm_estimate_apply_ms"], out["a_sphnorm_estimate_apply_ms_median"] = t, t[2]
save()

# (c) the scatter with gathered centres beside the plain one
S, colsum = fa.class_sums_device(xv, index)
Mc = S / torch.as_tensor(index.counts.astype(numpy.float64), device=dev)[:, None]
cls = torch.as_tensor(index.inverse.astype(numpy.int32)).to(dev)
mean_d = colsum / N
w = torch.as_tensor(1.0 / index.counts, device=dev)
plain = lambda: fa.gemm_tn_device(xv, None, None, mean_d, mean_d)
within = lambda: backend.scatter_within_device(xv, cls, Mc)
within_w = lambda: backend.scatter_within_device(xv, cls, Mc, w)
for fn in (plain, within, within_w):
    fn()
torch.cuda.synchronize()
ts = {"plain": [], "within": [], "within_w": []}
for _ in range(5):                                           # alternating
    for name, fn in (("plain", plain), ("within", within), ("within_w", within_w)):
        ts[name].append(device_ms(fn)[0])
fl, by = 2.0 * N * D * D, 4.0 * N * D
out["c_scatter"] = {"sc_gemm_tn (dgemm_tn_kernel<4, float> + slab_reduce_kernel)": rates(sorted(ts["plain"])[2], fl, by),
                    "sc_scatter_within (scatter_within_kernel<4, float> + slab_reduce_kernel)": rates(sorted(ts["within"])[2], fl, by + 4.0 * N),
                    "sc_scatter_within, class weights": rates(sorted(ts["within_w"])[2], fl, by + 4.0 * N),
                    "within_over_plain": sorted(ts["within"])[2] / sorted(ts["plain"])[2]}
save()

# (d) the fused row transform beside GEMM on a float64 copy + a row-normalising pass
R = torch.as_tensor(numpy.random.RandomState(1).randn(D, D) / numpy.sqrt(D), device=dev)
mu = mean_d


def unfused():
    y = fa.dgemm_nn_device(xv.double() - mu, R)
    return y / y.norm(dim=1).clamp_min(1e-8)[:, None]


fused = lambda: backend.whiten_rows_device(xv, mu, R, True)
fused32 = lambda: backend.whiten_rows_device(xv, mu, R, True, torch.float32)
proj = lambda: backend.whiten_rows_device(xv, None, R[:, :RANK].contiguous(), False)
for fn in (unfused, fused, fused32, proj):
    fn()
torch.cuda.synchronize()
ts = {"unfused": [], "fused": [], "fused32": [], "proj": []}
for _ in range(5):
    for name, fn in (("unfused", unfused), ("fused", fused), ("fused32", fused32), ("proj", proj)):
        ts[name].append(device_ms(fn)[0])
err = float((fused() - unfused()).abs().max())
fl = 2.0 * N * D * D
out["d_whiten_rows"] = {"sc_whiten_rows f32 -> f64, P 256, normalise (whiten_rows_kernel<4, float, double>)": rates(sorted(ts["fused"])[2], fl, N * D * (4.0 + 8.0)),
                        "sc_whiten_rows f32 -> f32, P 256, normalise": rates(sorted(ts["fused32"])[2], fl, N * D * (4.0 + 4.0)),
                        "sc_whiten_rows f32 -> f64, P 128, no normalise (the LDA projection)": rates(sorted(ts["proj"])[2], fl / 2, N * (4.0 * D + 8.0 * RANK)),
                        "float64 copy + centre, sc_dgemm_nn, row-normalising pass (torch)": rates(sorted(ts["unfused"])[2], fl, N * D * (4.0 + 8.0)),
                        "unfused_over_fused": sorted(ts["unfused"])[2] / sorted(ts["fused"])[2], "fused_vs_unfused_max_abs": err}
save()

# (b) the host
if not args.no_host:
    import backend_numpy as bn
    import plda_em_numpy as pen
    X = xv.cpu().numpy().astype(numpy.float64)
    out["b_host_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or None
    t0 = time.perf_counter()
    L_host = bn.lda(X, lab, RANK)
    out["b_host_lda_s"] = time.perf_counter() - t0
    out["lda_speedup_a_over_b"] = out["b_host_lda_s"] * 1e3 / out["a_lda_device_ms_median"]
    L = backend.lda_device(xv, index, RANK)
    out["lda_device_vs_host"] = {"LL'": float(pen.rel(L.dot(L.T), L_host.dot(L_host.T))), "top_gap": float(bn.top_gap(bn.lda_spectrum(X, lab)[0], RANK))}
    save()
    t0 = time.perf_counter()
    means_h, covs_h, rows_h = bn.spectral_norm_estimate(X, lab, IT, "sphNorm")
    rows_h = bn.spectral_norm_apply(X, means_h, covs_h)
    out["b_host_sphnorm_estimate_apply_s"] = time.perf_counter() - t0
    out["sphnorm_speedup_a_over_b"] = out["b_host_sphnorm_estimate_apply_s"] * 1e3 / out["a_sphnorm_estimate_apply_ms_median"]
    means, covs, rows = sphnorm()
    out["sphnorm_device_vs_host"] = {"covs[0]": float(pen.rel(covs[0], covs_h[0])),
                                     "eig(covs[2])": float(pen.rel(bn.sorted_eigenvalues(covs[2]), bn.sorted_eigenvalues(covs_h[2]))),
                                     "Gram of 1024 rows": float(pen.rel(rows[:1024].cpu().numpy().dot(rows[:1024].cpu().numpy().T), rows_h[:1024].dot(rows_h[:1024].T)))}
    save()
print(json.dumps(out, indent=1))
