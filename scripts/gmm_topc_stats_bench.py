"""What top-C Baum-Welch statistics cost beside the dense route (GPU box):

    python scripts/gmm_topc_stats_bench.py --out profiles/gmm_topc_stats_bench.json

One MI355X, D = 60, 192 000 resident float32 frames in segments of 300 to 3 000 frames (drawn from a fixed seed), C = 512 and 2 048
components, ``top_c`` = 10 and 20.  Per case, after a warm-up round, REPS rounds; a round times each of the following once, one after the
other, so the routes alternate and share whatever else the machine is doing; a timing is INNER back-to-back calls between two device
events, synchronised on both sides, divided by INNER; reported: median and max - min spread over the rounds.
  * the baseline: ``gmm_stats_device(order=1)``, the dense route (``sc_gmm_frame_loglik`` + ``sc_gmm_stats``), which this does not touch;
  * ``gmm_stats_topc_device(order=1)`` end to end (lists, posteriors, accumulation, the small operand copies);
  * its three phases alone: the lists (``gmm_top_components_device``), the posteriors (``sc_gmm_topc_posteriors`` through the C ABI on
    resident operands) and the accumulation (``sc_gmm_topc_stats`` likewise, one call for all segments).
Also recorded, beside K and held to no bound: the largest difference of stat0 and of stat1 between the two routes over the largest dense
entry -- what Gaussian selection costs in accuracy on this data.  The data are SYNTHETIC: components whose means lie 0.25 apart per
dimension under unit noise, so they overlap and the dropped tail carries weight; it says nothing about speech.
No ratio is fixed in advance: the file states what was measured.

Every GPU step is a child process under its own ``timeout``; the first one that fails ends the run (no retries) and nothing is written.
"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, FRAMES, SEG_MIN, SEG_MAX, REPS, INNER, STEP_TIMEOUT_S = 60, 192000, 300, 3000, 5, 10, 400
COMPONENTS, TOP_C = (512, 2048), (10, 20)
# VGPRs, scratch bytes and LDS of the two kernels (float32 frames, -Rpass-analysis=kernel-resource-usage)
REGISTERS = {"gmm_topc_post_kernel": {"vgprs": 38, "scratch_bytes": 0, "lds_bytes": {"top_c_10": 5632, "top_c_20": 10752}},
             "gmm_topc_stats_kernel": {"vgprs": 20, "scratch_bytes": 0, "lds_bytes_D60": {"order_1": 31232, "order_2": 61952}}}


def median(v):
    s = sorted(v)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def segment_lengths():
    """lengths in [SEG_MIN, SEG_MAX] from a fixed seed that add up to FRAMES"""
    import numpy
    rs = numpy.random.RandomState(5)
    lens = []
    while FRAMES - sum(lens) > SEG_MAX + SEG_MIN:
        lens.append(int(rs.randint(SEG_MIN, SEG_MAX + 1)))
    rest = FRAMES - sum(lens)            # in (SEG_MIN, SEG_MAX + SEG_MIN]
    lens += [rest] if rest <= SEG_MAX else [rest // 2, rest - rest // 2]
    assert sum(lens) == FRAMES and SEG_MIN <= min(lens) and max(lens) <= SEG_MAX
    return numpy.array(lens, dtype=numpy.int64)


def make_mixture(C):
    import numpy
    from sidekit_amd.mixture import Mixture
    rs = numpy.random.RandomState(1)
    m = Mixture()
    w = rs.rand(C) + 0.5
    m.w, m.mu, m.invcov = w / w.sum(), 0.25 * rs.randn(C, D), 1.0 / (0.5 + rs.rand(C, D))
    m.cov_var_ctl = 1.0 / m.invcov
    m._compute_all()
    return m


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / INNER


def step(C):
    import numpy
    import torch
    from gmm_bench import make_frames
    from sidekit_amd import _lib
    from sidekit_amd.gmm_scoring import gmm_top_components_device
    from sidekit_amd.mixture import gmm_stats_device, gmm_stats_topc_device, gmm_topc_posteriors_device
    dev = torch.device("cuda", 0)
    ubm = make_mixture(C)
    X = make_frames(torch, ubm, FRAMES, dev)
    lens = segment_lengths()
    off = numpy.concatenate(([0], numpy.cumsum(lens)))
    S, N, longest = len(lens), FRAMES, int(lens.max())
    mu, invcov = torch.as_tensor(ubm.mu).to(dev), torch.as_tensor(ubm.invcov).to(dev)
    B = torch.as_tensor(-2.0 * (numpy.log(ubm.w) + numpy.log(ubm.cst))).to(dev)
    d_off = torch.as_tensor(off.astype(numpy.int32)).to(dev)
    stat0 = torch.empty((S, C), dtype=torch.float64, device=dev)
    stat1 = torch.empty((S, C, D), dtype=torch.float64, device=dev)
    llk = torch.empty(S, dtype=torch.float64, device=dev)
    out = {"segments": S, "longest_segment": longest}
    dense = gmm_stats_device(ubm, X, off, order=1)
    for K in TOP_C:
        idx, post, lse = gmm_topc_posteriors_device(ubm, X, top_c=K)
        runs = {"gmm_stats_device": lambda: gmm_stats_device(ubm, X, off, order=1),
                "gmm_stats_topc_device": lambda: gmm_stats_topc_device(ubm, X, off, order=1, top_c=K),
                "lists": lambda: gmm_top_components_device(ubm, X, K),
                "posteriors": lambda: _lib.launch("sc_gmm_topc_posteriors", dev, X, _lib.XT_F32, N, D, mu, invcov, B, C, idx, K, post, lse),
                "accumulation": lambda: _lib.launch("sc_gmm_topc_stats", dev, X, _lib.XT_F32, N, D, C, idx, post, K, lse, d_off, S, longest, 1, stat0, stat1,
                                                    None, llk)}
        times = {name: [] for name in runs}
        for rep in range(REPS + 1):
            for name, fn in runs.items():
                t = timed(torch, fn)
                if rep:   # round 0 warms every shape up
                    times[name].append(t)
        r = {name: {"ms": t, "median_ms": median(t), "spread_ms": max(t) - min(t)} for name, t in times.items()}
        d, s = r["gmm_stats_device"], r["gmm_stats_topc_device"]
        r["dense_over_topc"] = d["median_ms"] / s["median_ms"]
        r["topc_faster_by_more_than_both_spreads"] = bool(d["median_ms"] - s["median_ms"] > d["spread_ms"] + s["spread_ms"])
        phases = sum(r[p]["median_ms"] for p in ("lists", "posteriors", "accumulation"))
        r["share_of_the_phases"] = {p: r[p]["median_ms"] / phases for p in ("lists", "posteriors", "accumulation")}
        sparse = gmm_stats_topc_device(ubm, X, off, order=1, top_c=K)
        again = gmm_stats_topc_device(ubm, X, off, order=1, top_c=K, components=idx)
        r["runs_bit_identical"] = bool(torch.equal(sparse[0], again[0]) and torch.equal(sparse[1], again[1]) and torch.equal(sparse[3], again[3]))
        r["difference_to_the_dense_statistics_on_synthetic_data"] = {
            "stat0_max_abs_over_largest": float((sparse[0] - dense[0]).abs().max() / dense[0].abs().max()),
            "stat1_max_abs_over_largest": float((sparse[1] - dense[1]).abs().max() / dense[1].abs().max()),
            "llk_max_rel": float(((sparse[3] - dense[3]) / dense[3]).abs().max()),
            "mean_posterior_mass_of_a_frames_best_component": float(post.max(dim=1).values.mean())}
        out[f"top_c_{K}"] = r
    return out


def child(args):
    """One step in a process of its own, under its own time limit; its last output line is its JSON result."""
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, "-W", "ignore::RuntimeWarning", os.path.abspath(__file__)] + args,
                       capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"gmm_topc_stats_bench: step {args} ended with status {p.returncode}; nothing after it was started")
    print(f"gmm_topc_stats_bench: step {args} done", file=sys.stderr, flush=True)
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, type=int, choices=COMPONENTS, help="(internal) run one mixture size in this process")
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "gmm_topc_stats_bench.py measures on the GPU"
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
        print(json.dumps(step(args.step)), flush=True)
        return
    out = {"timed_rounds": REPS, "calls_per_timing": INNER, "D": D, "frames": FRAMES, "frame_dtype": "float32", "order": 1,
           "segment_lengths": [SEG_MIN, SEG_MAX],
           "data": "synthetic: component means 0.25 apart per dimension under unit noise, frames drawn around them; says nothing about speech",
           "kernels": REGISTERS, "cases": {f"C{C}": child(["--step", str(C)]) for C in COMPONENTS}}
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
