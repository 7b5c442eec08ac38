"""What speech-only extraction costs and gains on one GPU (GPU box) -> profiles/vad_bench.json.

Part one: stand-alone device time of the three kernels (sk_frame_log_energy, sk_vad_energy, sk_collect_labels) on 256 x 4 s of int16,
to be read against the log-mel front-end's ~200 us for the same batch.
Part two: scripts/pipeline_bench.py's corpus (16-bit wav files on local disk, three quarters exactly 4 s, the rest 3-5 s) through
StreamingExtractor with vad=None and vad="energy", alternating, with the fraction of samples the detector removed; and the vad=None
regression guard: scripts/pipeline_bench.py of this tree and (``--parent-root DIR``: a built checkout of the parent commit) of the
parent, alternating in fresh processes of the same session.

Usage: python scripts/vad_bench.py [--files 16384] [--workers 8] [--repeats 3] [--parent-root DIR] [--out profiles/vad_bench.json]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy  # noqa: E402
import scipy.io.wavfile  # noqa: E402
import torch  # noqa: E402

from sidekit_amd import vad  # noqa: E402
from sidekit_amd.nnet import Xtractor  # noqa: E402
from sidekit_amd.pipeline import StreamingExtractor  # noqa: E402


def kernels(dev, B=256, L=64000, iters=50):
    rs = numpy.random.RandomState(0)
    env = numpy.repeat(numpy.where(rs.rand(B, L // 3200) < 0.5, 3000.0, 40.0), 3200, axis=1)        # 0.2 s stretches, loud or faint
    pcm = torch.from_numpy((rs.randn(B, L) * env).astype(numpy.int16)).to(dev)
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    out = torch.empty_like(pcm)
    le, nf = vad.frame_log_energy(pcm, lens)
    label, _ = vad.vad_energy_device(le, nf, **vad.ENERGY_DEFAULTS)
    steps = {"frame_log_energy": lambda: vad.frame_log_energy(pcm, lens),
             "vad_energy": lambda: vad.vad_energy_device(le, nf, **vad.ENERGY_DEFAULTS),
             "collect_labels": lambda: vad.collect_chunks_device(pcm, lens, labels=label, nframes=nf, out=out)}
    res = {"batch": B, "samples": L, "dtype": "int16", "iters": iters}
    for name, fn in steps.items():
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        res[f"{name}_us"] = round(a.elapsed_time(b) * 1000.0 / iters, 2)      # back-to-back launches: device time unless the host is the slower side
    res["three_kernels_us"] = round(sum(res[f"{k}_us"] for k in steps), 2)
    _, out_len = vad.collect_chunks_device(pcm, lens, labels=label, nframes=nf, out=out)
    res["fraction_removed"] = round(1.0 - float(out_len.sum().item()) / (B * L), 4)
    return res


def corpus(n):
    d = tempfile.mkdtemp(prefix="skwav_", dir="/tmp")
    rs = numpy.random.RandomState(0)
    base = (rs.randn(80000) * 3000).astype(numpy.int16)
    entries = []
    for i in range(n):
        m = 64000 if i % 4 else int(rs.randint(48000, 80000))
        p = os.path.join(d, f"u{i:06d}.wav")
        scipy.io.wavfile.write(p, 16000, numpy.roll(base, i)[:m])
        entries.append((f"u{i:06d}", p))
    return d, entries


def streaming(dev, n, workers, repeats):
    m = Xtractor(7205, model_archi="halfresnet34", loss="aam", seed=1234).to(dev).eval()
    m.compute_dtype = "bf16"
    d, entries = corpus(n)
    res = {"files": n, "decode_workers": workers, "runs": {"none": [], "energy": []}}
    try:
        for mode in (None, "energy"):                                       # warm-up: workspaces, pinned buffers, page cache
            dict(StreamingExtractor(m, batch_size=256, window=8, workers=workers, vad=mode).run(iter(entries[:1024])))
        for _ in range(repeats):
            for mode in (None, "energy"):
                ex = StreamingExtractor(m, batch_size=256, window=8, workers=workers, vad=mode)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = dict(ex.run(iter(entries)))
                dt = time.perf_counter() - t0
                assert len(got) == n
                res["runs"]["none" if mode is None else "energy"].append(round(n / dt, 1))
                if mode:
                    res["fraction_removed"] = round(1.0 - ex.stats["speech_samples"] / ex.stats["samples"], 4)
    finally:
        for _, p in entries:
            os.remove(p)
        os.rmdir(d)
    for k, v in res["runs"].items():
        res[f"files_per_s_{k}_median"] = float(numpy.median(v))
    return res


def child_bench(root, n, workers):
    """scripts/pipeline_bench.py of the tree at ``root`` in a fresh process -> its streaming files/s."""
    root = os.path.abspath(root)
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "pipeline_bench.py"), str(n), str(workers)], cwd=root, check=True,
                       capture_output=True, text=True, timeout=300)
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    return round(json.loads(line)["streaming_b256_files_per_s"], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16384)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vad_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"kernels": kernels(dev), "streaming": streaming(dev, args.files, args.workers, args.repeats)}
    print(json.dumps(out), flush=True)
    guard = {"now": [], "parent": []}
    for _ in range(args.repeats):                                           # the vad=None guard: same script, fresh processes, alternating
        if args.parent_root:
            guard["parent"].append(child_bench(args.parent_root, args.files, args.workers))
        guard["now"].append(child_bench(ROOT, args.files, args.workers))
    out["pipeline_bench_vad_none"] = guard
    print(json.dumps(out), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
