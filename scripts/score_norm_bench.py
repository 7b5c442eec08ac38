"""Cohort statistics without the cohort score matrix, beside the way the previous release offered (GPU box):

    python scripts/score_norm_bench.py --out profiles/score_norm_bench.json

``cohort_stats_device(topk=None)`` (``sc_cohort_moments``: mean / std per row from the GEMM's accumulators) at (N, M, D) =
(65 536, 16 384, 256), against ``sc_cosine`` into an (N, M) float32 tensor followed by ``torch.var_mean`` over its rows.  Both run
alternately in one process after a warm-up call each, five event-timed regions each; the medians, each path's peak of torch-allocated
memory over its region, the size of the library's own workspace (the float64 partial sums, which torch does not see) and the fused
kernel's fraction of its roofline bound max(2 N M D / f32 matrix peak, ((N + M) D + 2 N) 4 B / HBM peak) are recorded.  The memory
figures are the point (no N x M allocation); the times are a report, not a pass criterion.
"""
import argparse, ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from sidekit_amd import _lib
from sidekit_amd.score_normalization import cohort_stats_device

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--m", type=int, default=16384)
ap.add_argument("--d", type=int, default=256)
ap.add_argument("--out", default=None)
args = ap.parse_args()
N, M, D = args.n, args.m, args.d
F32_PEAK_TFLOPS, HBM_PEAK_TBS = 157.3, 8.0           # MI355X: f32 matrix (= vector) peak, HBM3E peak
assert torch.cuda.is_available(), "score_norm_bench.py measures on the GPU"
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(0)
x = torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=g), dim=1).contiguous()
c = torch.nn.functional.normalize(torch.randn(M, D, device=dev, generator=g), dim=1).contiguous()
lib = _lib.lib()


def fused():
    return cohort_stats_device(x, c)


def baseline():
    s = torch.empty((N, M), dtype=torch.float32, device=dev)
    _lib.check(lib.sc_cosine(x.data_ptr(), N, c.data_ptr(), M, D, s.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    var, mean = torch.var_mean(s, dim=1, unbiased=False)
    return mean, var.sqrt()


def region(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); r = fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated(dev) - base, r


rf, rb = region(fused)[2], region(baseline)[2]              # warm-up: code objects, the workspace, the allocator's blocks
diff = {"mean_max_abs": float((rf[0] - rb[0]).abs().max()), "std_max_abs": float((rf[1] - rb[1]).abs().max())}
del rf, rb
ts, peak = {"fused": [], "baseline": []}, {"fused": 0, "baseline": 0}
for _ in range(5):                                           # alternating
    for name, fn in (("fused", fused), ("baseline", baseline)):
        ms, rise, r = region(fn)
        del r
        ts[name].append(ms)
        peak[name] = max(peak[name], rise)
flop, nbytes = 2.0 * N * M * D, 4.0 * ((N + M) * D + 2 * N)
bound_ms = max(flop / (F32_PEAK_TFLOPS * 1e12), nbytes / (HBM_PEAK_TBS * 1e12)) * 1e3
tiles_m = (M + 127) // 128
per = -(-tiles_m // 64) if tiles_m > 128 else 2             # sc_cohort_moments' slab rule (csrc/score_norm.hip)
med = {k: sorted(v)[2] for k, v in ts.items()}
out = {"N": N, "M": M, "D": D, "f32_matrix_peak_TFLOP/s": F32_PEAK_TFLOPS, "hbm_peak_TB/s": HBM_PEAK_TBS,
       "fused": "cohort_stats_device(topk=None): sc_cohort_moments (cohort_moments_kernel<false> + cohort_moments_final_kernel)",
       "baseline": "sc_cosine into an (N, M) float32 tensor + torch.var_mean(dim=1, unbiased=False) + sqrt",
       "fused_ms": ts["fused"], "baseline_ms": ts["baseline"], "fused_ms_median": med["fused"], "baseline_ms_median": med["baseline"],
       "baseline_over_fused": med["baseline"] / med["fused"],
       "fused_peak_torch_bytes": peak["fused"], "baseline_peak_torch_bytes": peak["baseline"], "score_matrix_bytes": 4 * N * M,
       "fused_library_workspace_bytes": -(-tiles_m // per) * min(N, 32768) * 16,
       "fused_TFLOP/s": flop / med["fused"] / 1e9, "roofline_bound_ms": bound_ms, "roofline_bound_by": "f32 matrix peak" if flop / (F32_PEAK_TFLOPS * 1e12) > nbytes / (HBM_PEAK_TBS * 1e12) else "HBM",
       "fused_fraction_of_roofline": bound_ms / med["fused"], "fused_vs_baseline": diff}
text = json.dumps(out, indent=1)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
print(text)
