"""What top-C GMM-UBM scoring costs beside the dense route (GPU box):

    python scripts/gmm_topc_bench.py --out profiles/gmm_topc_bench.json

The protocol is scripts/gmm_score_bench.py's: one MI355X, D = 60, 64 segments of 3 000 resident float32 frames, M = 64 and 512 models at
C = 512 and 2 048 components; after a warm-up call REPS event-timed calls each, synchronised on both sides: median and max - min spread;
each route in a process of its own.
  * the baseline: one ``gmm_llr_device`` call, the dense route (``sc_gmm_score_models``), which top-C scoring does not touch;
  * top-C, for ``top_c`` in 5, 10, 20: the lists alone (``gmm_top_components_device``), the sparse kernel alone
    (``sc_gmm_score_models_topc`` through the C ABI on resident operands, M + 1 models: the UBM is one more) and ``gmm_llr_topc_device``
    as a whole (lists, sparse kernel, the means and their difference);
  * for ``top_c`` in 1, 5, 10, 20 the mean and the largest ``|llr_topc - llr_dense|`` over the M x 64 trials.  The data are SYNTHETIC
    (frames drawn around the mixture's own means, models that are the means plus noise): the differences say how much of a frame's
    likelihood the dropped components carry on this data and nothing about the EER on speech;
  * a sweep over M at both C with ``top_c = 10``, both routes: the smallest M at which top-C is still faster than the dense route by more
    than both spreads -- below it the lists' dense pass over the UBM dominates.
Accepted: at ``top_c = 10`` ``gmm_llr_topc_device`` is faster than ``gmm_llr_device`` at every case by more than the two spreads added.

Every GPU step is a child process under its own ``timeout``; the first one that fails ends the run (no retries) and nothing is written.
"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, SEGMENTS, SEG_LEN, REPS, STEP_TIMEOUT_S = 60, 64, 3000, 5, 400
CASES = ((64, 512), (512, 512), (64, 2048), (512, 2048))       # (M, C)
TOP_C_TIMED, TOP_C_DIFFERENCE, TOP_C_ACCEPTED = (5, 10, 20), (1, 5, 10, 20), 10
SWEEP_M, SWEEP_C = (1, 2, 4, 8, 16, 32, 64), (512, 2048)
# VGPRs, scratch bytes and LDS of the two kernels (float32 frames): python scripts/kernel_regs.py sidekit_amd/csrc/gmm.hip topc, .../gmm_topc.hip score
REGISTERS = {"gmm_topc_kernel": {"vgprs": 96, "scratch_bytes": 0, "lds_bytes_D60": {"top_c_5": 77568, "top_c_10": 81408, "top_c_20": 89088},
                                 "workgroups_per_cu_D60": {"top_c_5": 2, "top_c_10": 2, "top_c_20": 1}},
             "gmm_topc_score_kernel": {"vgprs": 121, "scratch_bytes": 0, "models_per_workgroup": 4,
                                       "lds_bytes_D60": {"top_c_5": 39680, "top_c_10": 46080, "top_c_20": 58880},
                                       "workgroups_per_cu_D60": {"top_c_5": 4, "top_c_10": 3, "top_c_20": 2}}}


def median(v):
    s = sorted(v)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)


def measure(fn):
    """a warm-up call, then REPS timed calls"""
    fn()
    t = [timed(fn) for _ in range(REPS)]
    return {"ms": t, "median_ms": median(t), "spread_ms": max(t) - min(t)}


def setup(C, M):
    import numpy
    import torch
    from gmm_bench import make_frames, make_mixture
    dev = torch.device("cuda", 0)
    ubm = make_mixture(C, 1)
    X = make_frames(torch, ubm, SEGMENTS * SEG_LEN, dev)
    rs = numpy.random.RandomState(2)
    models = torch.as_tensor(ubm.mu[None] + 0.3 * rs.randn(M, C, D)).to(dev)
    off = numpy.arange(SEGMENTS + 1, dtype=numpy.int64) * SEG_LEN
    return torch, dev, ubm, X, models, off


def step_dense(cases):
    from sidekit_amd.gmm_scoring import gmm_llr_device
    out = {}
    for M, C in cases:
        torch, dev, ubm, X, models, off = setup(C, M)
        out[f"M{M}_C{C}"] = measure(lambda: gmm_llr_device(ubm, models, X, off))
        del models, X
    return out


def step_topc(cases, timed_top_c, difference_top_c):
    import numpy
    from sidekit_amd import _lib
    from sidekit_amd.gmm_scoring import gmm_llr_device, gmm_llr_topc_device, gmm_top_components_device
    out = {}
    for M, C in cases:
        torch, dev, ubm, X, models, off = setup(C, M)
        N = X.shape[0]
        res = {}
        for top_c in timed_top_c:
            r = {"lists": measure(lambda: gmm_top_components_device(ubm, X, top_c))}
            idx = gmm_top_components_device(ubm, X, top_c)
            stacked = torch.cat((models.reshape(M, C * D), torch.as_tensor(ubm.mu).to(dev).reshape(1, C * D)))
            invcov = torch.as_tensor(ubm.invcov).to(dev)
            B = torch.as_tensor(-2.0 * (numpy.log(ubm.w) + numpy.log(ubm.cst))).to(dev)
            d_off = torch.as_tensor(off.astype(numpy.int32)).to(dev)
            llk = torch.zeros((M + 1, SEGMENTS), dtype=torch.float64, device=dev)
            r["sparse_kernel"] = measure(lambda: _lib.launch("sc_gmm_score_models_topc", dev, X, _lib.XT_F32, N, D, stacked, M + 1, invcov, B, C, d_off, SEGMENTS,
                                                             SEG_LEN, None, idx, top_c, llk))
            r["sparse_kernel"]["gathered_bytes"] = 8.0 * N * top_c * (M + 2) * D     # the means of M + 1 models and the invcov row, per (frame, k)
            r["sparse_kernel"]["gathered_TB_per_s"] = r["sparse_kernel"]["gathered_bytes"] / r["sparse_kernel"]["median_ms"] * 1e-9
            r["gmm_llr_topc_device"] = measure(lambda: gmm_llr_topc_device(ubm, models, X, off, top_c=top_c))
            a, b = gmm_llr_topc_device(ubm, models, X, off, top_c=top_c), gmm_llr_topc_device(ubm, models, X, off, top_c=top_c, components=idx)
            r["runs_bit_identical"] = bool(torch.equal(a, b))
            res[f"top_c_{top_c}"] = r
            del stacked, llk, idx
        if difference_top_c:
            dense = gmm_llr_device(ubm, models, X, off)
            res["difference_to_the_dense_llr_on_synthetic_data"] = {"dense_mean_abs_llr": float(dense.abs().mean())}
            for top_c in difference_top_c:
                d = (gmm_llr_topc_device(ubm, models, X, off, top_c=top_c) - dense).abs()
                res["difference_to_the_dense_llr_on_synthetic_data"][f"top_c_{top_c}"] = {"mean_abs": float(d.mean()), "max_abs": float(d.max())}
            del dense
        out[f"M{M}_C{C}"] = res
        del models, X
    return out


def child(args):
    """One step in a process of its own, under its own time limit; its last output line is its JSON result."""
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, "-W", "ignore::RuntimeWarning", os.path.abspath(__file__)] + args,
                       capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"gmm_topc_bench: step {args} ended with status {p.returncode}; nothing after it was started")
    print(f"gmm_topc_bench: step {args} done", file=sys.stderr, flush=True)
    return json.loads(p.stdout.strip().splitlines()[-1])


def faster(dense, sparse):
    return bool(dense["median_ms"] - sparse["median_ms"] > dense["spread_ms"] + sparse["spread_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=("dense", "topc", "sweep_dense", "sweep_topc"), help="(internal) run one step in this process")
    args = ap.parse_args()
    sweep = tuple((M, C) for C in SWEEP_C for M in SWEEP_M)
    if args.step:
        import torch
        assert torch.cuda.is_available(), "gmm_topc_bench.py measures on the GPU"
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
        res = {"dense": lambda: step_dense(CASES), "topc": lambda: step_topc(CASES, TOP_C_TIMED, TOP_C_DIFFERENCE),
               "sweep_dense": lambda: step_dense(sweep), "sweep_topc": lambda: step_topc(sweep, (TOP_C_ACCEPTED,), ())}[args.step]()
        print(json.dumps(res), flush=True)
        return
    dense, topc = child(["--step", "dense"]), child(["--step", "topc"])
    out = {"timed_repeats": REPS, "D": D, "segments": SEGMENTS, "frames_per_segment": SEG_LEN, "frames": "float32",
           "data": "synthetic: frames drawn around the mixture's means, models = means + 0.3 noise; the differences to the dense ratios say nothing about the EER on speech",
           "kernels": REGISTERS, "baseline_gmm_llr_device": dense, "cases": topc}
    for case, res in topc.items():
        for top_c in TOP_C_TIMED:
            r = res[f"top_c_{top_c}"]
            r["dense_over_gmm_llr_topc_device"] = dense[case]["median_ms"] / r["gmm_llr_topc_device"]["median_ms"]
            r["faster_than_the_dense_route_by_more_than_both_spreads"] = faster(dense[case], r["gmm_llr_topc_device"])
    out["accepted"] = all(res[f"top_c_{TOP_C_ACCEPTED}"]["faster_than_the_dense_route_by_more_than_both_spreads"] for res in topc.values())
    sd, st = child(["--step", "sweep_dense"]), child(["--step", "sweep_topc"])
    out["sweep_over_M_at_top_c_10"] = {}
    for C in SWEEP_C:
        rows = {}
        for M in SWEEP_M:
            d, t = sd[f"M{M}_C{C}"], st[f"M{M}_C{C}"][f"top_c_{TOP_C_ACCEPTED}"]
            rows[f"M{M}"] = {"gmm_llr_device": d, "gmm_llr_topc_device": t["gmm_llr_topc_device"], "lists": t["lists"], "sparse_kernel": t["sparse_kernel"],
                             "dense_over_topc": d["median_ms"] / t["gmm_llr_topc_device"]["median_ms"], "topc_pays": faster(d, t["gmm_llr_topc_device"])}
        paying = [M for M in SWEEP_M if rows[f"M{M}"]["topc_pays"]]
        out["sweep_over_M_at_top_c_10"][f"C{C}"] = {"rows": rows, "smallest_M_at_which_topc_pays": min(paying) if paying else None}
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
