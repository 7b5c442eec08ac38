"""What top-C EM costs beside dense EM, and what it trains (GPU box):

    python scripts/gmm_topc_em_bench.py --out profiles/gmm_topc_em_bench.json

One MI355X, D = 60, resident float32 frames: 192 000 (the set of the other GMM benches) and 2 000 000, drawn around the GEN_C components of
a fixed generator mixture; trained from one Gaussian to C = 512 and to C = 2 048 under the default ``iterations`` by
  * ``em_split_device``, the dense route, which this does not touch;
  * ``em_split_topc_device`` at ``top_c`` = 10 and 20, with the lists handed down the split tree alone, and with
    ``exact_lists_at`` = every second level above ``top_c`` (dense lists there, once per level).
Per case one process; after a short warm-up training of every route, REPS rounds, a round running each route once, one after the other,
so the routes alternate and share whatever else the machine is doing.  Reported per route: the wall time of a training (host clock
around a run that ends in a device synchronise: E-steps, the host M-steps and the small copies between them), median and max - min
spread over the rounds; and per level (the E / M steps between two splits) the device time per E-step of each entry point, from device
events recorded around every launch of the run itself (``sc_gmm_topc_refine`` / ``sc_gmm_topc_stats`` / ``sc_gmm_top_components``
against ``sc_gmm_frame_loglik`` + ``sc_gmm_stats``), median over the rounds of the level's mean; a level's closing refinement (lists
only) is counted with its E-steps' refinements and stated.  Quality: the dense per-frame log-likelihood (``frame_loglik_device``) of
every final model on HELD_OUT frames from the same generator, and on the training frames; components with a non-finite mean (a
component no frame lists has zero occupation and is not guarded) are counted.  The data are SYNTHETIC: generator means 0.25 apart per
dimension under unit noise, so components overlap; it says nothing about speech.  No ratio is fixed in advance: the file states what
was measured.

Every GPU step is a child process under its own ``timeout``; the first one that fails ends the run (no retries) and nothing is written.
"""
import argparse, json, math, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, GEN_C, HELD_OUT, REPS, STEP_TIMEOUT_S = 60, 1024, 192000, 3, 500
FRAMES, COMPONENTS, TOP_C = (192000, 2000000), (512, 2048), (10, 20)
DENSE = ("sc_gmm_frame_loglik", "sc_gmm_stats")
# VGPRs, scratch bytes and LDS of the kernel (both frame types, -Rpass-analysis=kernel-resource-usage)
REGISTERS = {"gmm_topc_refine_kernel": {"vgprs": 46, "sgprs": 68, "scratch_bytes": 0, "waves_per_simd": 8,
                                        "lds_bytes": {"lists_only": 0, "top_c_10": 5632, "top_c_20": 10752}}}


def median(v):
    s = sorted(v)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def num(v):
    v = float(v)
    return v if math.isfinite(v) else None


def generator():
    import numpy
    from sidekit_amd.mixture import Mixture
    rs = numpy.random.RandomState(1)
    m = Mixture()
    w = rs.rand(GEN_C) + 0.5
    m.w, m.mu, m.invcov = w / w.sum(), 0.25 * rs.randn(GEN_C, D), 1.0 / (0.5 + rs.rand(GEN_C, D))
    m.cov_var_ctl = 1.0 / m.invcov
    m._compute_all()
    return m


def draw(torch, gen, n, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    mu, sd = torch.as_tensor(gen.mu, dtype=torch.float32).to(dev), torch.as_tensor(gen.invcov, dtype=torch.float32).to(dev).rsqrt()
    X = torch.empty((n, D), dtype=torch.float32, device=dev)
    for a in range(0, n, 1 << 20):
        b = min(n, a + (1 << 20))
        c = torch.randint(0, GEN_C, (b - a,), device=dev, generator=g)
        X[a:b] = mu[c] + sd[c] * torch.randn(b - a, D, device=dev, generator=g)
    return X


class Launches(object):
    """device events around every launch through ``_lib.launch`` while a training runs, cut into levels by the M-steps"""

    def __init__(self, torch, _lib):
        self.torch, self._lib, self.real = torch, _lib, _lib.launch
        self.events, self.steps = [], []

    def __enter__(self):
        def launch(name, *args, **kw):
            a, b = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
            a.record()
            self.real(name, *args, **kw)
            b.record()
            self.events.append((name, len(self.steps), a, b))
        self._lib.launch = launch
        return self

    def __exit__(self, *exc):
        self._lib.launch = self.real

    def after_iteration(self, mixture, llk):
        self.steps.append(mixture.get_distrib_nb())

    def per_level(self):
        """{C: {"e_steps", entry point: device ms per E-step}}.  A launch made after s M-steps belongs to the level of M-step s, but for a
        selective level's closing refinement, which follows its last M-step: where a level's first E-step shows two refinements the
        first is the previous level's, as is the one after the run's last M-step."""
        self.torch.cuda.synchronize()
        n, refines = len(self.steps), {}
        assert [e[0] for e in self.events[:2]] == list(DENSE), "the start from one Gaussian"
        for i, (name, s, _, _) in enumerate(self.events):
            if name == "sc_gmm_topc_refine":
                refines.setdefault(s, []).append(i)
        closing = {v[0] for s, v in refines.items() if s == n or (s > 0 and self.steps[s - 1] != self.steps[s] and len(v) == 2)}
        out = {}
        for i, (name, s, a, b) in enumerate(self.events):
            if i < 2:
                continue
            C = self.steps[s - 1] if i in closing else self.steps[s]
            level = out.setdefault(C, {"e_steps": self.steps.count(C)})
            level[name] = level.get(name, 0.0) + a.elapsed_time(b)
        for level in out.values():
            for name in list(level):
                if name != "e_steps":
                    level[name] /= level["e_steps"]
        return out


def step(n, C):
    import numpy
    import torch
    from sidekit_amd import _lib
    from sidekit_amd.mixture import em_split_device, em_split_topc_device, frame_loglik_device
    dev = torch.device("cuda", 0)
    gen = generator()
    X, held = draw(torch, gen, n, dev, 7), draw(torch, gen, HELD_OUT, dev, 8)
    levels = [2 ** i for i in range(1, int(math.log2(C)) + 1)]
    routes = {"dense": lambda **kw: em_split_device(X, C, **kw)}
    for K in TOP_C:
        second = tuple(c for c in levels if c > K)[1::2]
        routes[f"top_c_{K}"] = lambda K=K, **kw: em_split_topc_device(X, C, top_c=K, **kw)
        routes[f"top_c_{K}_exact_lists_at_every_second_level"] = lambda K=K, second=second, **kw: em_split_topc_device(X, C, top_c=K, exact_lists_at=second, **kw)
    em_split_device(X[:20000], 64)   # warm-up: every entry point and shape class once
    for K in TOP_C:
        em_split_topc_device(X[:20000], 64, top_c=K, exact_lists_at=(32,))
    wall, device, models = {r: [] for r in routes}, {r: [] for r in routes}, {}
    for rep in range(REPS):
        for name, run in routes.items():
            with Launches(torch, _lib) as rec:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                models[name] = run(after_iteration=rec.after_iteration)
                torch.cuda.synchronize()
                wall[name].append((time.perf_counter() - t0) * 1e3)
            device[name].append(rec.per_level())
    out = {"frames": n, "components": C, "levels": levels, "held_out_frames": HELD_OUT, "routes": {}}
    for name in routes:
        ubm, llk = models[name]
        per_level = {}
        for c in device[name][0]:
            entry = {"e_steps": device[name][0][c]["e_steps"]}
            for k in device[name][0][c]:
                if k != "e_steps":
                    entry[k + "_ms_per_e_step"] = median([d[c][k] for d in device[name]])
            entry["device_ms_per_e_step"] = sum(v for k, v in entry.items() if k.endswith("_ms_per_e_step"))
            per_level[f"C{c}"] = entry
        dead = int((~numpy.isfinite(ubm.mu).all(axis=1)).sum())
        r = {"wall_ms": wall[name], "wall_median_ms": median(wall[name]), "wall_spread_ms": max(wall[name]) - min(wall[name]),
             "device_ms_in_launches": sum(v["device_ms_per_e_step"] * v["e_steps"] for v in per_level.values()),
             "per_level": per_level, "e_steps": len(llk), "last_training_llk_per_unit_of_occupation": num(llk[-1]),
             "components_with_a_non_finite_mean": dead,
             "dense_llk_per_frame_on_the_training_frames": num(frame_loglik_device(ubm, X).mean()),
             "dense_llk_per_frame_on_held_out_frames": num(frame_loglik_device(ubm, held).mean())}
        out["routes"][name] = r
    d = out["routes"]["dense"]
    for name, r in out["routes"].items():
        if name == "dense":
            continue
        r["dense_wall_over_this"] = d["wall_median_ms"] / r["wall_median_ms"]
        r["faster_than_dense_by_more_than_both_spreads"] = bool(d["wall_median_ms"] - r["wall_median_ms"] > d["wall_spread_ms"] + r["wall_spread_ms"])
        r["dense_device_ms_over_this"] = d["device_ms_in_launches"] / r["device_ms_in_launches"]
        if r["dense_llk_per_frame_on_held_out_frames"] is not None and d["dense_llk_per_frame_on_held_out_frames"] is not None:
            r["held_out_llk_minus_dense"] = r["dense_llk_per_frame_on_held_out_frames"] - d["dense_llk_per_frame_on_held_out_frames"]
    return out


def child(args):
    """One step in a process of its own, under its own time limit; its last output line is its JSON result."""
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, "-W", "ignore::RuntimeWarning", os.path.abspath(__file__)] + args,
                       capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"gmm_topc_em_bench: step {args} ended with status {p.returncode}; nothing after it was started")
    print(f"gmm_topc_em_bench: step {args} done", file=sys.stderr, flush=True)
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, nargs=2, type=int, metavar=("FRAMES", "COMPONENTS"), help="(internal) run one case in this process")
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "gmm_topc_em_bench.py measures on the GPU"
        print(json.dumps(step(*args.step)), flush=True)
        return
    out = {"timed_rounds": REPS, "D": D, "frame_dtype": "float32", "iterations": "the default of em_split_device",
           "data": f"synthetic: {GEN_C} generator components, means 0.25 apart per dimension under unit noise; says nothing about speech",
           "kernels": REGISTERS, "cases": {f"N{n}_C{C}": child(["--step", str(n), str(C)]) for n in FRAMES for C in COMPONENTS}}
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
