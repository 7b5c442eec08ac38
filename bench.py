#!/usr/bin/env python
"""Headline benchmark: x-vectors/s for 4 s @ 16 kHz utterances, HalfResNet34, bf16 trunk.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A "step" is one pass of the extraction hot path (Xtractor.forward(is_eval=True): wav -> 256-d
x-vector) over one batch of 256 synthetic utterances already resident in HBM (BASELINE.json
configs[1]); with N > 1 every rank (one process per GPU, launched by torch.distributed.run)
extracts its own shard and the x-vectors are all-gathered over RCCL, as the scoring step needs
them.  Timing: barrier + synchronize on both sides of exactly K steps, MAX over ranks, rank 0
prints ONE JSON line.

A plain run does only what that line's headline needs: set-up, W warm-up steps, ONE timed region of
exactly K steps (`ms_per_step` = its time / K), the outputs if asked for, the line.  `--dump-outputs DIR`
writes what rank 0's last timed step returned -- `logits.npy` (B x n_spk) and `embeddings.npy` (B x 256),
plus `embeddings_gathered.npy` with a process group -- as float32, inputs seeded so that two runs with the
same arguments see the same waveforms.  `--full` adds what takes runs of its own: `--regions` (5) timed
regions with the MEDIAN one reported, the same steps issued one forward at a time (`value_one_at_a_time`),
and two extra objects on the line:

  roofline     the dominant kernel (the trunk convolution shape with the largest summed device
               time), its algorithmic bytes or FLOPs per launch over its mean launch duration
               measured with HIP events on the launch stream during the timed steps.  Two shapes
               (layer 1: HBM-bound, layer 3: MFMA-bound) are within a percent of each other, so the
               timed region brackets the TWO largest classes, the runner-up rides along as
               `co_dominant`, and `trunk` carries the time-weighted fraction over every trunk
               convolution -- none of the three moves with run-to-run noise;
  cpu_baseline the oracle's CPU restatement of the same forward, timed on this box's host cores
               on a bounded sample at batch 16 and batch 1 (rank 0, N = 1 only).

The timed region runs the PRODUCT configuration of a corpus run: batches are issued through `Xtractor.submit` / `collect`
(`xt_forward_begin` / `xt_forward_end`), `Xtractor.pipeline_depth` (2) WHOLE batches in flight, each on a stream of the handle, half a step apart -- what
`sidekit_amd.pipeline.StreamingExtractor` does with the batches of a wav.scp.  A step submits one batch and collects the one submitted
depth - 1 steps earlier; every batch submitted inside the timed region is collected inside it.  (`--pipeline 1` times one forward at a time:
the two-lane split of a batch, `xt_set_lanes`; `--pipeline 3`: three in flight, +0.3-1.1 % here and -10-13 % for the streaming extractor, profiles/r06_pipeline_depth.txt.)  Either way kernels of
several batches / half batches overlap and one kernel's duration says
nothing about that kernel.  The roofline object therefore comes from a second region of the same K steps, one forward at a time on
one stream (`roofline.measured_in` says so), and `profiles/` holds the rocprofv3 trace of the serial run.  `roofline.traffic` is not
observed by this run: it is replayed from `profiles/traffic.json` (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command),
`traffic_source` names the file and its capture.

`--gpus N` (N > 1) started WITHOUT torch.distributed.run in the environment launches its N ranks
itself: a fresh `python -m torch.distributed.run ... bench.py` child is created before this process
has touched the GPU, its output is relayed and its exit code returned.  `--dry-run` replaces the GPU
step by a CPU stand-in over gloo (launch / rendezvous / gather / timing plumbing only; used by the
CPU test-suite, never a measurement).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8 TB/s
MFMA_BF16_PEAK_TF = 2500.0   # dense bf16 MFMA
MFMA_F32_PEAK_TF = 157.3     # f32-input MFMA == vector rate

# trunk convolution shapes: name -> (cin, cout, stride, w_in, taps, layer index of the input, of the output)
CONV_SHAPES = {
    "conv_L1": (32, 32, 1, 80, 9, 0, 0), "conv_L1S": (32, 32, 1, 80, 1, 0, 0),
    "conv_L2A": (32, 64, 2, 80, 9, 0, 1), "conv_L2S": (32, 64, 2, 80, 1, 0, 1), "conv_L2": (64, 64, 1, 40, 9, 1, 1),
    "conv_L3A": (64, 128, 2, 40, 9, 1, 2), "conv_L3S": (64, 128, 2, 40, 1, 1, 2), "conv_L3": (128, 128, 1, 20, 9, 2, 2),
    "conv_L4A": (128, 256, 2, 20, 9, 2, 3), "conv_L4S": (128, 256, 2, 20, 1, 2, 3), "conv_L4": (256, 256, 1, 10, 9, 3, 3),
}


def halve(h, n):
    for _ in range(n):
        h = (h + 1) // 2
    return h


# launches per forward of each shape in its two epilogue forms: (conv1 of a block: in -> out [+ fused 1x1 shortcut out],
# conv2 of a block: in + shortcut -> out), see DESIGN.md section 4
# launches per forward as (statistics form, residual form, residual form with the in-place 1x1 shortcut of a layer's first block)
CONV_FORMS = {"conv_L1": (3, 2, 1), "conv_L2A": (1, 0, 0), "conv_L2": (3, 3, 1), "conv_L3A": (1, 0, 0), "conv_L3": (5, 5, 1),
              "conv_L4A": (1, 0, 0), "conv_L4": (2, 2, 1),
              "conv_L1S": (1, 0, 0), "conv_L2S": (1, 0, 0), "conv_L3S": (1, 0, 0), "conv_L4S": (1, 0, 0)}   # A/B path only


def conv_work(name, B, T, eb):
    """Algorithmic FLOPs and bytes of ONE launch of a trunk convolution, averaged over its launches in one forward
    (every tensor the launch must read or write once)."""
    cin, cout, s, win, taps, lin, lout = CONV_SHAPES[name]
    hin, hout, wout = halve(T, lin), halve(T, lout), win // s
    n1, n2, n3 = CONV_FORMS[name]
    in_b, out_b = B * hin * win * cin * eb, B * hout * wout * cout * eb
    flops = 2.0 * B * hout * wout * cout * cin * taps
    cx = 32 if cout == 32 else cout // 2                      # channels of the block input the in-place shortcut reads
    sc_in_b, sc_flops = B * hout * wout * cx * eb, 2.0 * B * hout * wout * cout * cx
    n = n1 + n2 + n3
    nbytes = (n1 * (in_b + out_b) + n2 * (in_b + 2 * out_b) + n3 * (in_b + out_b + sc_in_b + cout * cx * eb)) / n + cout * cin * taps * eb
    return flops + n3 * sc_flops / n, nbytes


def class_roofline(name, ms, n, B, T, dtype, traffic_table):
    """Roofline record of one trunk convolution class from its summed device time `ms` over `n` launches."""
    eb = 2 if dtype == "bf16" else 4
    dur = ms / n * 1e-3
    flops, nbytes = conv_work(name, B, T, eb)
    peak_tf = MFMA_BF16_PEAK_TF if dtype == "bf16" else MFMA_F32_PEAK_TF
    ridge = peak_tf * 1e12 / (HBM_PEAK_GBS * 1e9)
    if flops / nbytes < ridge:
        ach = nbytes / dur / 1e9
        r = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS}
    else:
        ach = flops / dur / 1e12
        r = {"bound": "mfma", "achieved": ach, "peak": peak_tf, "unit": "TFLOP/s", "frac": ach / peak_tf}
    r.update({"traffic": traffic_table.get(name), "kernel": f"conv3x3_kernel<{name[5:]}, {dtype}>", "launch_us": dur * 1e6, "launches": n,
              "alg_bytes_per_launch": nbytes, "alg_flops_per_launch": flops})
    return r


def roofline(prof, B, T, dtype, per_class_ms=None):
    """`prof`: {class: (ms, launches)} of the timed region (the two largest classes, or all).  Returns the record of the
    largest class with the runner-up as `co_dominant` and the time-weighted trunk aggregate as `trunk`."""
    convs = {k: v for k, v in prof.items() if k in CONV_SHAPES and v[1]}
    if not convs:
        return None
    traffic, traffic_source = {}, None
    tpath = os.path.join(ROOT, "profiles", "traffic.json")
    if os.path.exists(tpath):
        with open(tpath) as f:
            tj = json.load(f)
        traffic = tj.get(dtype, {})
        traffic_source = "replayed from profiles/traffic.json, not observed by this run: " + tj.get("_note", "")
    order = sorted(convs, key=lambda k: -convs[k][0])
    r = class_roofline(order[0], *convs[order[0]], B, T, dtype, traffic)
    if len(order) > 1:
        r["co_dominant"] = class_roofline(order[1], *convs[order[1]], B, T, dtype, traffic)
    if per_class_ms:   # every trunk class (warmup table): sum of roofline-bound times over sum of measured times
        eb = 2 if dtype == "bf16" else 4
        peak_tf = MFMA_BF16_PEAK_TF if dtype == "bf16" else MFMA_F32_PEAK_TF
        t_meas = t_bound = 0.0
        for name, ms in per_class_ms.items():
            if name not in CONV_SHAPES:
                continue
            flops, nbytes = conv_work(name, B, T, eb)
            n = sum(CONV_FORMS[name])
            t_bound += n * max(flops / (peak_tf * 1e12), nbytes / (HBM_PEAK_GBS * 1e9)) * 1e3
            t_meas += ms
        if t_meas > 0:
            r["trunk"] = {"frac_time_weighted": t_bound / t_meas, "roofline_ms_per_step": t_bound, "measured_ms_per_step": t_meas,
                          "note": "sum over trunk convolution classes of launches x max(FLOPs / MFMA peak, bytes / HBM peak) over their measured time"}
    r["per_class_ms_per_step"] = None
    r["traffic_source"] = traffic_source
    return r


def tdnn_roofline(prof, frames):
    """BASELINE configs[3]: the TDNN's five dilated conv1d layers run as `gemm_kernel<LoadPlain>` launches on the exact-f32 MFMA.
    Algorithmic FLOPs per utterance of T' frames: 2 * [204800 (T'-4) + 786432 (T'-8) + 1835008 (T'-14)], summed
    over the batch's own frame counts; per launch = a fifth of it (one launch per layer)."""
    ms, n = prof.get("tdnn", (0.0, 0))
    if not n:
        return None
    flops = sum(2.0 * (204800 * (t - 4) + 786432 * (t - 8) + 1835008 * (t - 14)) for t in frames)
    per_forward_ms = ms / (n / 5.0)
    ach = flops / (per_forward_ms * 1e-3) / 1e12
    return {"bound": "mfma", "achieved": ach, "peak": MFMA_F32_PEAK_TF, "unit": "TFLOP/s", "frac": ach / MFMA_F32_PEAK_TF, "traffic": None,
            "traffic_source": None, "kernel": "gemm_kernel<LoadPlain> (TDNN conv1..conv5 as dilated implicit GEMMs, v_mfma_f32_32x32x2_f32)",
            "launch_us": ms / n * 1e3, "launches": int(n), "alg_flops_per_launch": flops / 5.0,
            "alg_flops_per_forward": flops, "tdnn_gemm_ms_per_step": per_forward_ms}


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(seconds, budget_s=20.0, arch="halfresnet34", lens=None):
    """The oracle (torch-CPU restatement of the reference forward) on this box's host cores: batch 16 and batch 1 on a
    one-GPU box's CPU share (16 threads) in this process, then a thread sweep (32 / 64 / 128, SURVEY 8d's "all cores") with every leg in
    its own bounded child process; `value_all_cores` is the best of the sweep with its thread count.  Core counts and CPU model stated.
    TDNN (configs[3]): the first utterances of the ragged batch, one forward per utterance as the reference would run them."""
    import subprocess
    import torch
    from oracle import xvector as oxv
    from sidekit_amd.nnet.weights import seeded_state_dict
    visible = os.cpu_count() or 1
    try:
        visible = len(os.sched_getaffinity(0))
    except Exception:
        pass
    cores = min(visible, 16)  # a one-GPU box's CPU share; more threads mostly oversubscribe the intra-op pool (the sweep shows it)
    rates, samples = {}, []
    if arch == "halfresnet34":
        sd = seeded_state_dict("halfresnet34", 7205, seed=1234)
        fwd = lambda w: oxv.halfresnet34_forward(w, sd)
        plan = ((16, cores, 0.6), (1, cores, 0.4))
    else:
        sd = seeded_state_dict("xvector", 7205, loss="aam", seed=1234)
        fwd = lambda w: oxv.tdnn_forward(w, sd)
        plan = ((1, cores, 1.0),)
    for B, threads, share in plan:
        torch.set_num_threads(threads)
        torch.manual_seed(0)
        if lens is None:
            batches = [0.1 * torch.randn(B, int(seconds * 16000))]
        else:
            batches = [0.1 * torch.randn(1, n) for n in lens[:64]]
        with torch.no_grad():
            fwd(batches[0])  # warm-up
            t0 = time.perf_counter()
            it = done = 0
            while time.perf_counter() - t0 < budget_s * share and it < 64:
                done += fwd(batches[it % len(batches)])[1].shape[0]
                it += 1
            dt = time.perf_counter() - t0
        rates[(B, threads)] = done / dt
        samples.append(f"{it} batches of {B} on {threads} threads")
    # thread sweep above the CPU share: one child process per thread count, a hard limit per leg (on a box whose share is 16 cores
    # hundreds of intra-op threads thrash: 256 threads did not finish ONE forward in 25 s in rounds 2-3 and are not tried again)
    sweep, sweep_notes = {}, []
    n_samples = int(seconds * 16000) if lens is None else int(lens[0])
    for threads in [t for t in (32, 64, 128) if t <= visible and t > cores]:
        code = ("import sys, time, torch; sys.path.insert(0, %r); from oracle import xvector as oxv; "
                "from sidekit_amd.nnet.weights import seeded_state_dict; torch.set_num_threads(%d); torch.manual_seed(0); "
                "sd = seeded_state_dict(%r, 7205, %s seed=1234); w = 0.1 * torch.randn(1, %d); f = oxv.%s\n"
                "with torch.no_grad():\n"
                "    f(w, sd); t0 = time.perf_counter(); n = 0\n"
                "    while time.perf_counter() - t0 < 5.0 and n < 64:\n"
                "        f(w, sd); n += 1\n"
                "print(n / (time.perf_counter() - t0), n)") % (
                    ROOT, threads, "halfresnet34" if arch == "halfresnet34" else "xvector", "" if arch == "halfresnet34" else "loss='aam',",
                    n_samples, "halfresnet34_forward" if arch == "halfresnet34" else "tdnn_forward")
        try:
            r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=22)
            rate, n = r.stdout.strip().splitlines()[-1].split()
            sweep[threads] = float(rate)
            samples.append(f"{n} forwards of batch 1 on {threads} threads (child process)")
        except Exception:
            sweep[threads] = None
            sweep_notes.append(f"{threads} threads: no result within 22 s")
    torch.set_num_threads(cores)
    best = max(v for (b, t), v in rates.items() if t == cores)
    done_sweep = {t: v for t, v in sweep.items() if v}
    best_t = max(done_sweep, key=done_sweep.get) if done_sweep else None
    out = {"value": best, "unit": "x-vectors/s", "cores": cores, "kind": "port", "cores_visible": visible, "cpu_model": cpu_model(),
           "value_all_cores": done_sweep.get(best_t), "cores_all": best_t,
           "thread_sweep": {str(cores): rates.get((1, cores)), **{str(t): v for t, v in sweep.items()}},
           "all_cores_note": ("batch-1 forwards per thread count, each leg in a bounded child process; value_all_cores = the best above the box's "
                              f"{cores}-thread share" + ("; " + "; ".join(sweep_notes) if sweep_notes else "") +
                              "; all visible threads (256 on the round-2/3 boxes) did not finish one forward in 25 s and are not retried"),
           "sample": f"{'; '.join(samples)}: synthetic " + (f"{seconds:g} s" if lens is None else "2-10 s") +
                     f" utterances, fp32, torch-CPU oracle (oracle/xvector.py)"}
    if arch == "halfresnet34":
        out.update(value_batch1=rates[(1, cores)], value_batch16=rates[(16, cores)])
    return out


def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


DUMP_LIMIT = 64 << 20   # bytes written by --dump-outputs, all files together


def dump_outputs(path, arrays):
    """`arrays`: name -> host array with one row per utterance, written as float32 to `path`/<name>.npy.  Where the whole set would
    pass DUMP_LIMIT, each array keeps a fixed, seeded sample of its rows (in order; arrays of equal length keep the same rows)."""
    import numpy
    os.makedirs(path, exist_ok=True)
    arrays = {k: numpy.ascontiguousarray(v, dtype=numpy.float32) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    for name, a in arrays.items():
        if total > DUMP_LIMIT:
            keep = max(1, int(a.shape[0] * (DUMP_LIMIT - (4 << 10) * len(arrays)) / total))   # 4 KB per file for the .npy header
            a = a[numpy.sort(numpy.random.RandomState(0).choice(a.shape[0], keep, replace=False))]
        numpy.save(os.path.join(path, name + ".npy"), a)


def launch_ranks(n, argv):
    """Start `n` ranks of this script under torch.distributed.run as a fresh child process and relay its output.  Called
    before anything in this process has touched the GPU (no exec of a GPU-initialised process, no fork after HIP init)."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + argv
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)   # stderr is inherited
    for line in proc.stdout:
        sys.stdout.write(line)
        sys.stdout.flush()
    return proc.wait()


def dry_run(args):
    """CPU stand-in of the benchmark loop over gloo: same launch / barrier / gather / MAX-over-ranks / JSON plumbing, no GPU work."""
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    use_dist = "RANK" in os.environ
    if use_dist:
        dist.init_process_group("gloo")
    B, E = args.batch, 256
    g = torch.Generator().manual_seed(rank)
    gathered = torch.empty(world * B, E) if use_dist else None

    def step():
        emb = torch.nn.functional.normalize(torch.randn(B, E, generator=g), dim=1)
        if use_dist:
            dist.all_gather_into_tensor(gathered, emb)
        return emb

    for _ in range(args.warmup):
        step()
    if use_dist:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        emb = step()
    if use_dist:
        dist.barrier()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    if use_dist:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        assert torch.equal(gathered[rank * B:(rank + 1) * B], emb)
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"embeddings": emb.numpy(), **({"embeddings_gathered": gathered.numpy()} if use_dist else {})})
    if rank == 0:
        print(json.dumps({"metric": "x-vectors/sec (4 s @ 16 kHz)", "value": world * B * args.steps / t.item(), "unit": "x-vectors/s",
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": t.item() / args.steps * 1e3,
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "none", "data": "dry-run (CPU stand-in, no GPU work)",
                          "config": {"workload": "dry run of the launch / gather / timing plumbing", "batch_per_gpu": B,
                                     "parallelism": f"utterance-sharded x{world} (gloo)"}}), flush=True)
    if use_dist:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--arch", default="halfresnet34", choices=["halfresnet34", "xvector"])
    ap.add_argument("--ragged", action="store_true", help="variable-length 2-10 s utterances (BASELINE configs[3] with --arch xvector --dtype fp32 --batch 512)")
    ap.add_argument("--lanes", type=int, default=0, choices=[0, 1, 2], help="0: the library default (two-lane forward), 1: serial, 2: two lanes (only without --pipeline)")
    ap.add_argument("--pipeline", type=int, default=0, choices=[0, 1, 2, 3], help="0 (default): the steps are issued through Xtractor.submit / collect with the library's "
                    "default number of whole batches in flight (Xtractor.pipeline_depth = 2; what the streaming extractor does); 2 / 3: that many; 1: one forward at a time "
                    "(the two-lane split of a batch)")
    ap.add_argument("--full", action="store_true", help="besides the headline: --regions timed regions (default 5), the roofline object, the one-forward-at-a-time "
                    "comparison and the CPU baseline (each can be dropped with --no-profile / --no-cpu-baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write rank 0's outputs of the last timed step to DIR/<name>.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile", action="store_true", help="do not bracket kernels with HIP events")
    ap.add_argument("--dry-run", action="store_true", help="CPU/gloo stand-in of the loop (plumbing test, not a measurement)")
    ap.add_argument("--regions", type=int, default=None, help="the timed region of exactly --steps steps is repeated this many times (barrier + synchronize on both sides of each); "
                    "value / ms_per_step are those of the MEDIAN region, regions_ms lists all of them.  Default: 1, with --full 5")
    ap.add_argument("--inputs", type=int, default=5, help="distinct resident input batches the steps cycle through (5 x 65.5 MB > the 256-MB Infinity Cache)")
    args = ap.parse_args()
    if args.regions is None:
        args.regions = 5 if args.full else 1

    if args.gpus > 1 and "RANK" not in os.environ:
        # launched like the N = 1 command: start the ranks ourselves, as fresh child processes created before any GPU call
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:]))
    if args.dry_run:
        return dry_run(args)

    import torch
    import torch.distributed as dist
    from sidekit_amd.nnet import Xtractor

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs WORLD_SIZE={args.gpus} (launch with torch.distributed.run)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or "RANK" in os.environ   # under torch.distributed.run the RCCL path is exercised even at N = 1
    if use_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", device_id=dev)

    dtype = args.dtype if args.arch == "halfresnet34" else "fp32"
    model = Xtractor(7205, model_archi=args.arch, loss="aam", seed=1234).to(dev).eval()
    model.compute_dtype = dtype
    B, L = args.batch, int(args.seconds * 16000)
    g = torch.Generator(device=dev).manual_seed(rank)
    # the steps cycle through several resident batches so that no step finds its waveform in the Infinity Cache
    lens = None
    if args.ragged:   # BASELINE configs[3]: variable-length 2-10 s (RandomState(0), the lengths tests/test_gpu_fullsize.py uses)
        import numpy
        lens = numpy.random.RandomState(rank).randint(32000, 160001, (B,)).tolist()
        L = max(lens)
    wavs = [0.1 * torch.randn(B, L, device=dev, generator=g) for _ in range(max(1, args.inputs))]
    # the step's x-vectors are gathered over RCCL WITHOUT stalling the next step: the collective runs on RCCL's stream
    # (async_op), two destination buffers alternate, and a step only waits for the gather issued two steps earlier; the timed
    # region ends after every gather has completed
    gathered = [torch.empty(world * B, model.embedding_size, device=dev) for _ in range(2)] if use_dist else None
    counter = [0]
    gathers = [0]
    in_flight = []
    pending = []           # tickets of submitted, not yet collected batches (pipeline 2)
    pipelined = args.pipeline != 1
    if args.pipeline > 1:
        model.pipeline_depth = args.pipeline

    def gather(emb):
        k = gathers[0]
        gathers[0] += 1
        while len(in_flight) >= 2:
            in_flight.pop(0)[0].wait()
        work = dist.all_gather_into_tensor(gathered[k % 2], emb, async_op=True)
        # the next kernels on the compute stream are ordered behind the collective (a stream-side wait, the host does not block):
        # 256 KB per rank is microseconds (0.05-0.09 ms per step)
        work.wait()
        in_flight.append((work, emb))

    def step():
        """One pass of the hot path over one batch.  Pipelined (default): the batch is SUBMITTED -- its whole forward queued on one of the
        handle's two slot streams -- and the batch submitted one step earlier is COLLECTED (and gathered), so two batches are in flight, half
        a step apart; every batch submitted inside a timed region is collected inside it (drain)."""
        wav = wavs[counter[0] % len(wavs)]
        counter[0] += 1
        if pipelined:
            pending.append(model.submit(wav, lengths=lens))
            out = None
            if len(pending) == model.pipeline_depth:
                out = model.collect(pending.pop(0))
        else:
            out = model(wav, is_eval=True, lengths=lens)
        emb = None if out is None else out[1]
        if use_dist and emb is not None:
            gather(emb)
        if emb is not None:
            last[0] = out
        return emb

    last = [None]          # (logits, x-vectors) of the batch collected last

    def drain():
        while pending:
            out = model.collect(pending.pop(0))
            last[0] = out
            if use_dist:
                gather(out[1])
        while in_flight:
            in_flight.pop(0)[0].wait()

    if args.lanes:
        model.set_lanes(args.lanes)
    model(wavs[0], is_eval=True, lengths=lens)          # creates the handle and reserves the workspace (both lanes)
    lanes = model.get_lanes() if (args.arch == "halfresnet34" and B >= 128) else 1
    overlapped = pipelined or lanes > 1                 # kernels of two batches / two half batches run side by side in the timed region

    host_enqueue = [0.0]

    def timed_region(n_steps):
        drain()
        torch.cuda.synchronize(dev)
        if use_dist:
            dist.barrier()
            torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n_steps):
            step()
        host_enqueue[0] = time.perf_counter() - t0      # the host's share: every launch of the K steps is queued, nothing awaited yet
        drain()
        torch.cuda.synchronize(dev)
        if use_dist:
            dist.barrier()
            torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, last[0]

    # Measurement plan.  An event pair per kernel launch costs ~2 us of stream time (150 pairs per step = 4-6 % of the step), and
    # with two lanes a kernel's duration includes whatever the other lane ran beside it.  So: (1) W warmup + exactly K timed steps
    # in the product configuration -> `value`; when that configuration is serial, the two largest trunk classes are bracketed in
    # it (picked from the last warmup steps, every class bracketed).  (2) Two lanes: the lanes are serialised AFTER the timed
    # region, 3 steps with every class bracketed give the per-class table, K more steps with the two largest classes bracketed
    # give the roofline object.
    per_class, focus, n_prof, prof, serial_ms, one_at_a_time_ms = None, None, 0, None, None, None
    profile = args.full and not args.no_profile

    def pick_focus(prof_w, n):
        pc = {k: round(v[0] / n, 4) for k, v in prof_w.items()}
        convs = {k: v for k, v in prof_w.items() if k in CONV_SHAPES}
        return pc, (sorted(convs, key=lambda k: -convs[k][0])[:2] if convs else None)

    n_prof_warm = min(3, args.warmup) if (profile and not overlapped) else 0
    for i in range(args.warmup):
        if n_prof_warm and i == args.warmup - n_prof_warm:
            model.set_profile(True)
            model.get_profile(reset=True)
        step()
    if n_prof_warm:
        per_class, focus = pick_focus(model.get_profile(reset=True), n_prof_warm)
        n_prof = n_prof_warm
    if profile and not overlapped:
        model.set_profile(True, slots=focus) if focus else model.set_profile(True)
        model.get_profile(reset=True)
    drain()                                             # warm-up batches still in flight are collected outside the timed region
    # The timed region -- exactly K steps between barrier + synchronize -- is run `--regions` times back to back and the MEDIAN region is
    # what the line reports: 20 steps are 0.11 s on a chip whose clock a power governor sets (+- 3 % box to box, a percent within a
    # minute), one region is one sample.  Every region is a complete measurement by the contract's definition; regions_ms has them all.
    n_regions = max(1, args.regions if not (profile and not overlapped) else 1)   # a bracketed (serial, profiled) timed region is measured once
    region_dt, enq = [], []
    for _ in range(n_regions):
        dt_r, (logits, emb) = timed_region(args.steps)
        region_dt.append(dt_r)
        enq.append(host_enqueue[0])
    assert bool(torch.isfinite(emb).all()), "non-finite x-vectors"
    if rank == 0 and args.dump_outputs:
        dumped = {"logits": logits.cpu().numpy(), "embeddings": emb.cpu().numpy()}
        if use_dist:
            dumped["embeddings_gathered"] = gathered[(gathers[0] - 1) % 2].cpu().numpy()
        dump_outputs(args.dump_outputs, dumped)
    t = torch.tensor(region_dt, dtype=torch.float64, device=dev)
    if use_dist:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)        # per region: the slowest rank
        assert torch.equal(gathered[(gathers[0] - 1) % 2][rank * B:(rank + 1) * B], emb), "all-gather returned a different block for this rank"
    region_dt = t.tolist()
    med = sorted(range(n_regions), key=lambda i: region_dt[i])[n_regions // 2]
    dt, host_enqueue[0] = region_dt[med], enq[med]
    if profile and not overlapped:
        prof = model.get_profile(reset=True)
        measured_in = "the timed region (serial lanes)"
    elif profile and rank == 0:
        def step():          # rank 0 alone from here on: the forward without the collective
            counter[0] += 1
            return model(wavs[counter[0] % len(wavs)], is_eval=True, lengths=lens)[1]
        model.set_lanes(1)
        step()
        model.set_profile(True)
        model.get_profile(reset=True)
        for _ in range(3):
            step()
        per_class, focus = pick_focus(model.get_profile(reset=True), 3)
        n_prof = 3
        model.set_profile(True, slots=focus) if focus else model.set_profile(True)
        model.get_profile(reset=True)
        drain()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        drain()
        torch.cuda.synchronize(dev)
        serial_ms = (time.perf_counter() - t0) / args.steps * 1e3
        prof = model.get_profile(reset=True)
        model.set_profile(False)
        model.set_lanes(lanes)
        if pipelined:   # for comparison: the same K steps issued one forward at a time (the split of a batch over `lanes` streams), this rank alone
            for _ in range(2):
                step()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize(dev)
            one_at_a_time_ms = (time.perf_counter() - t0) / args.steps * 1e3
        measured_in = (f"a second region of {args.steps} steps, one forward at a time on one stream (xt_set_lanes 1, {serial_ms:.3f} ms per step), run after the "
                       f"timed region: in the timed region kernels of " + (f"{model.pipeline_depth} batches in flight" if pipelined else f"the {lanes} parts of a batch") + " overlap")
    if rank == 0:
        T = 1 + L // (160 if args.arch == "halfresnet34" else 512)
        issue = (f"Xtractor.submit / collect ({model.pipeline_depth} whole batches in flight; each batch is the forward of Xtractor.forward(is_eval=True))" if pipelined
                 else "Xtractor.forward(is_eval=True), one call at a time")
        length = f"2-10 s (mean {sum(lens) / len(lens) / 16000:.2f} s, padded to {L / 16000:.2f} s)" if lens else f"{args.seconds:g} s"
        workload = (f"{'HalfResNet34' if args.arch == 'halfresnet34' else 'TDNN x-vector'} {issue}, {dtype} trunk, batch={B} per GPU, synthetic {length} @ 16 kHz "
                    f"(BASELINE.json configs[{3 if args.arch != 'halfresnet34' else 1}])")
        out = {
            "metric": "x-vectors/sec (4 s @ 16 kHz)", "value": world * B * args.steps / dt, "unit": "x-vectors/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": dtype, "data": "synthetic",
            "regions_ms": [round(x / args.steps * 1e3, 4) for x in region_dt],
            "regions_note": f"{n_regions} timed regions of exactly {args.steps} steps each (barrier + synchronize on both sides, MAX over ranks per region); value and ms_per_step are the median region's",
            "config": {"workload": workload,
                       "batch_per_gpu": B, "samples_per_utt": L, "frames_per_utt": T, "resident_input_batches": len(wavs),
                       "parallelism": f"utterance-sharded x{world}" + (" + RCCL all-gather of x-vectors" if use_dist else "")},
        }
        out["config"]["lanes"] = 1 if pipelined else lanes
        out["config"]["pipeline"] = (f"{model.pipeline_depth} batches in flight: Xtractor.submit / collect (xt_forward_begin / xt_forward_end), each batch's forward on one stream "
                                     f"of the handle; a step submits one batch and collects the one submitted {model.pipeline_depth - 1} step earlier; every batch of the timed "
                                     f"region is collected inside it" if pipelined else "1 (one forward at a time)")
        # host budget (8 ranks share one host): wall time of the K `model(...)` calls + collectives up to the point where
        # everything is queued, per step.  The forward is ONE ctypes call into the C ABI that enqueues its ~150 launches per lane from
        # C++ (no Python per kernel); as long as this stays well below ms_per_step a rank is GPU-bound with a single host thread
        out["host_enqueue_ms_per_step"] = host_enqueue[0] / args.steps * 1e3
        out["host_enqueue_frac"] = host_enqueue[0] / dt
        if one_at_a_time_ms is not None:
            out["value_one_at_a_time"] = B * 1e3 / one_at_a_time_ms     # the reference driver's issue order (one Xtractor.forward call at a time), rank 0, same run: what BENCH_r01-r03 reported as `value`
            out["one_forward_at_a_time"] = {"ms_per_step": one_at_a_time_ms, "value": B * 1e3 / one_at_a_time_ms, "lanes": lanes,
                                            "note": "the same batches issued through Xtractor.forward, one at a time (the batch split over `lanes` streams), measured on rank 0 after the timed region"}
        if profile and prof is not None:
            if args.arch == "halfresnet34":
                r = roofline(prof, B, T, dtype, per_class)
            else:
                r = tdnn_roofline(prof, [1 + n // 512 for n in (lens or [L] * B)])
            if r is not None:
                r["measured_in"] = measured_in
                if args.arch == "halfresnet34":
                    if per_class is None:
                        per_class = {k: round(v[0] / args.steps, 4) for k, v in prof.items()}
                        r["per_class_source"] = "timed region, every class bracketed"
                    else:
                        r["per_class_source"] = (f"{n_prof} steps with every class bracketed (serial lanes), before the roofline region; that region brackets "
                                                 f"{' and '.join(focus)} only")
                    r["per_class_ms_per_step"] = per_class
                    r["per_class_note"] = ("every launch of these steps is bracketed by a HIP event pair (~2 us of stream time each, ~150 launches "
                                           "per step), so the classes sum to more than serial_ms_per_step")
                if serial_ms is not None:
                    r["serial_ms_per_step"] = serial_ms
                # which schedule `frac` belongs to, at a glance: kernel durations mean something only when one kernel runs at a time
                r["schedule"] = {"of_frac": "serial: one forward at a time on ONE stream (xt_set_lanes 1)" if serial_ms is not None else "the timed region itself (serial lanes)",
                                 "serial_ms_per_step": serial_ms, "of_value": (f"pipelined: {model.pipeline_depth} whole batches in flight, each on a stream of the handle" if pipelined else f"one forward at a time, {lanes} lane(s)"),
                                 "value_ms_per_step": dt / args.steps * 1e3, "one_forward_at_a_time_ms_per_step": one_at_a_time_ms}
            out["roofline"] = r
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.seconds, arch=args.arch, lens=lens)
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
