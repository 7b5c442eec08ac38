"""What GMM-UBM scoring costs in time and memory, for 1, 2 and 4 models per workgroup (GPU box):

    scripts/build_variant.sh gs_g1 EXTRA=-DSC_GMM_SCORE_G=1      (and gs_g2, gs_g4: three builds of the library beside the shipped one)
    python scripts/gmm_score_bench.py --out profiles/gmm_score_bench.json

Cases: M = 64 and 512 models at C = 512 and 2 048 components, D = 60, 64 segments of 3 000 resident float32 frames.
  * the new route: one ``gmm_llk_device`` call (``sc_gmm_score_models``: all models, only the M x S segment sums leave the kernel), once per
    build of the library (``SIDEKIT_AMD_LIB``), each in a process of its own;
  * the baseline, what is written against the parent commit's API: per model one ``frame_loglik_device(ubm, x, mu=model)`` on the resident
    frames (it uploads the model's means and its A vector and writes an N-vector) and the segment sums of that vector;
  * ``sc_gmm_frame_loglik`` alone on the same frames (its rate counts 4 C D FLOP per frame).
After a warm-up call REPS event-timed calls each, synchronised on both sides: median and max - min spread.  The new kernel's rate counts
2 (1 + G) C D / G FLOP per frame and model (the squares' half once per G models).  Peak device memory: ``torch.cuda.mem_get_info`` before
the first call of a process whose caches were just released and after it.  Accepted: the shipped G is faster than the baseline at
every case by more than the two spreads added.

Every GPU step is a child process under its own ``timeout``; the first one that fails ends the run (no retries) and nothing is written.
"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, SEGMENTS, SEG_LEN, REPS, STEP_TIMEOUT_S = 60, 64, 3000, 5, 400
CASES = ((64, 512), (512, 512), (64, 2048), (512, 2048))       # (M, C)
GROUPS = (1, 2, 4)
PEAK_F64_TFLOPS = 78.6
# VGPRs and scratch bytes of gmm_score_kernel<G, float>: python scripts/kernel_regs.py sidekit_amd/csrc/gmm_score.hip score_kernel -DSC_GMM_SCORE_G=<G>
REGISTERS = {1: {"vgprs": 182, "scratch_bytes": 0, "workgroups_per_cu": 2}, 2: {"vgprs": 248, "scratch_bytes": 0, "workgroups_per_cu": 2},
             4: {"vgprs": 440, "scratch_bytes": 0, "workgroups_per_cu": 1}}


def median(v):
    s = sorted(v)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)


def setup(C, M):
    import numpy
    import torch
    from gmm_bench import make_frames, make_mixture
    dev = torch.device("cuda", 0)
    ubm = make_mixture(C, 1)
    X = make_frames(torch, ubm, SEGMENTS * SEG_LEN, dev)
    rs = numpy.random.RandomState(2)
    models = ubm.mu[None] + 0.3 * rs.randn(M, C, D)
    off = numpy.arange(SEGMENTS + 1, dtype=numpy.int64) * SEG_LEN
    return torch, dev, ubm, X, models, off


def measure(torch, dev, fn):
    """peak memory of the first call, then REPS timed calls"""
    from sidekit_amd import _lib
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    _lib.lib().sc_release_workspace()
    free0, _ = torch.cuda.mem_get_info(dev)
    fn()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info(dev)
    t = [timed(fn) for _ in range(REPS)]
    return {"ms": t, "median_ms": median(t), "spread_ms": max(t) - min(t), "device_memory_taken_bytes": free0 - free1}


def step_kernel(G):
    """the new route under the library that is loaded (SIDEKIT_AMD_LIB: the build with G models per workgroup)"""
    from sidekit_amd.gmm_scoring import gmm_llk_device
    from sidekit_amd.mixture import frame_loglik_device
    out = {}
    for M, C in CASES:
        torch, dev, ubm, X, models, off = setup(C, M)
        d_models = torch.as_tensor(models).to(dev)
        held = {}
        gmm_llk_device(ubm, d_models[:1], X[:64])                           # the library's code object is on the device before memory is measured

        def run():
            held["llk"] = gmm_llk_device(ubm, d_models, X, off)[0]

        res = measure(torch, dev, run)
        first = held["llk"].clone()
        run()
        res["runs_bit_identical"] = bool(torch.equal(first, held["llk"]))
        # against the per-model route on two models
        for m in (0, M - 1):
            lse = frame_loglik_device(ubm, X, mu=models[m])
            want = lse.reshape(SEGMENTS, SEG_LEN).sum(1)
            res[f"model_{m}_relative_max_difference_to_frame_loglik"] = float((first[m] - want).abs().max() / want.abs().max())
            assert res[f"model_{m}_relative_max_difference_to_frame_loglik"] < 1e-9
        flop = 2.0 * (1 + G) * C * D / G * SEGMENTS * SEG_LEN * M
        res.update(flop_counted=flop, tflops=flop / res["median_ms"] * 1e-9, share_of_the_f64_matrix_rate=flop / res["median_ms"] * 1e-9 / PEAK_F64_TFLOPS)
        out[f"M{M}_C{C}"] = res
        del d_models, held, first
    return out


def step_baseline():
    from sidekit_amd.mixture import frame_loglik_device
    out = {}
    for M, C in CASES:
        torch, dev, ubm, X, models, off = setup(C, M)
        held = {}
        frame_loglik_device(ubm, X[:64], mu=models[0])

        def run():
            llk = torch.empty((M, SEGMENTS), dtype=torch.float64, device=dev)
            for m in range(M):
                llk[m] = frame_loglik_device(ubm, X, mu=models[m]).reshape(SEGMENTS, SEG_LEN).sum(1)
            held["llk"] = llk

        res = measure(torch, dev, run)
        one = lambda: frame_loglik_device(ubm, X)   # noqa: E731
        one()
        t = [timed(one) for _ in range(REPS)]
        flop = 4.0 * C * D * SEGMENTS * SEG_LEN
        res["frame_loglik_one_call"] = {"ms": t, "median_ms": median(t), "spread_ms": max(t) - min(t), "flop_counted": flop,
                                        "tflops": flop / median(t) * 1e-9}
        out[f"M{M}_C{C}"] = res
    return out


def child(args, lib=None):
    """One step in a process of its own, under its own time limit; its last output line is its JSON result."""
    env = dict(os.environ)
    if lib:
        env["SIDEKIT_AMD_LIB"] = lib
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, "-W", "ignore::RuntimeWarning", os.path.abspath(__file__)] + args,
                       capture_output=True, text=True, env=env)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"gmm_score_bench: step {args} ended with status {p.returncode}; nothing after it was started")
    print(f"gmm_score_bench: step {args} done", file=sys.stderr, flush=True)
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shipped", type=int, default=2, choices=GROUPS, help="SC_GMM_SCORE_G of the shipped library (csrc/gmm_score.hip)")
    ap.add_argument("--variants", default=os.path.join(ROOT, "build_alt", "gs_g{G}", "sidekit_amd", "csrc", "libsidekit_amd.so"),
                    help="where the build with G models per workgroup lies ({G} is replaced)")
    ap.add_argument("--step", default=None, choices=("kernel", "baseline"), help="(internal) run one step in this process")
    ap.add_argument("--group", type=int, default=0)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "gmm_score_bench.py measures on the GPU"
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
        print(json.dumps(step_kernel(args.group) if args.step == "kernel" else step_baseline()), flush=True)
        return
    libs = {G: args.variants.format(G=G) for G in GROUPS}
    for G, path in libs.items():
        assert os.path.exists(path), f"{path} is missing: scripts/build_variant.sh gs_g{G} EXTRA=-DSC_GMM_SCORE_G={G}"
    out = {"timed_repeats": REPS, "f64_peak_tflops": PEAK_F64_TFLOPS, "D": D, "segments": SEGMENTS, "frames_per_segment": SEG_LEN, "frames": "float32",
           "shipped_models_per_workgroup": args.shipped, "baseline_frame_loglik_per_model": child(["--step", "baseline"])}
    base = out["baseline_frame_loglik_per_model"]
    for G in GROUPS:
        row = child(["--step", "kernel", "--group", str(G)], lib=libs[G])
        for case, r in row.items():
            b = base[case]
            r["baseline_over_this"] = b["median_ms"] / r["median_ms"]
            r["faster_than_the_baseline_by_more_than_both_spreads"] = bool(b["median_ms"] - r["median_ms"] > b["spread_ms"] + r["spread_ms"])
            r["share_of_frame_loglik_rate"] = r["tflops"] / b["frame_loglik_one_call"]["tflops"]
        out[f"G{G}"] = dict(REGISTERS[G], cases=row)
    out["fastest_models_per_workgroup_by_case"] = {case: min(GROUPS, key=lambda G: out[f"G{G}"]["cases"][case]["median_ms"]) for case in base}
    out["accepted"] = all(r["faster_than_the_baseline_by_more_than_both_spreads"] for r in out[f"G{args.shipped}"]["cases"].values())
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
