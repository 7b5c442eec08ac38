"""The waveform front end one kernel at a time: the two STFT kernels (csrc/frontend_fft.hip) with and without the fused mel projection, the
mel and DCT GEMMs of frontend_rows (csrc/xt_api.hip) and the two CMVN kernels (csrc/pool.hip), each against a float64 evaluation of the SAME
operands (tests/tools/frontend_f64.py).  Float32 samples go through Xtractor.features, int16 samples through a forward, both with the debug
taps on: 'power' (unfused path only), 'logmel', 'mfcc' (xvector) and the features.  Probe checkpoints replace only the front-end buffers:
``cover`` gives every bin 0 .. N/2 a weight on the fused path (the product banks leave 32 of 513 and 165 of 1025 bins unobserved), ``wide``,
``dense`` and, at n_fft 1024, ``chunks`` take the path that writes the power rows to memory, which the product banks never take; all carry a
window that is not symmetric and, for the xvector, a dense matrix in place of the DCT.

Criteria (r = the float64 value, u = 2^-24; tests/test_frontend_reference_cpu.py shows that torch's float32 evaluation passes them on these
batches and that fifteen wrong front ends do not).  Class and factor are those of tests/test_gpu_features_extractor.py: the spectrum relative
to the frame's largest bin, log-domain outputs in absolute terms, at most 4 x a CPU single-precision yardstick measured on the same operands
in the same run (1-ulp hardware log2, float32 twiddles and window, another butterfly order):

  power: every bin of every own frame within 4 x yardstick of r, relative to the frame's largest bin; yardstick = the largest such error of
    torch.fft.rfft on the float32 frames over the batch (floored at 2 u).  Pad columns and rows past an utterance's last frame exactly 0.
  logmel, unfused, against log(the power tap @ fb + 1e-6): |got - r| <= -log(1 - 2 (K + 4) u s / (s + 1e-6)) + 4 u max(|r|, 1) per element,
    K = nbp, s = the sum (all terms >= 0, so S = s): the GEMM bound of tests/tools/tdnn_f64.py in front of the log.
  logmel, fused, against the float64 chain from the samples: the two above composed -- a spectrum within 4 x yardstick of the frame's
    largest bin Pmax moves filter j's sum by at most that x Pmax x sum_k fb[k][j]: |got - r| <= 4 yardstick Pmax W_j / (s + 1e-6)
    + 2 (n_j + 4) u + 4 u max(|r|, 1); and max |got - r| over the batch <= 4 x that of torch's float32 chain from the same samples
    (floored at 8 u).  The same criteria judge the filters ``cover`` and ``wide`` share, on both paths.
    Rows past an utterance hold log(1e-6) within 2 ulp; a silent frame holds one value in every filter.
  mfcc against the logmel tap @ dct: check_gemm of tdnn_f64 with K = n_mels + 4 (per element 2 K u S; norm-relative within 16 x torch's).
  features against cmvn_ref(the tap in front): |got - r| <= (n + 2) u mean|x| / s + (n / 2 + 12) u |r| over the utterance's n rows
    (frontend_f64.cmvn_bound derives it); rows past an utterance keep the bits of the tap.

The library refuses what the shortest imaginable cases would need: fewer than n_fft / 2 + 1 samples (so 160 * 3 samples, and frame counts 1 and 2
of the CMVN kernels, cannot be reached through any entry; the shortest are 4 frames for the mel model and the TDNN's 15), which
test_lengths_the_library_refuses pins.

Measured on one MI355X (printed by the tests; DESIGN.md section 4e has the table): power 4.4e-7 of the frame's largest bin at n_fft 1024 and
4.0e-7 at 2048 (torch's float32 3.4e-7: 1.3 x, 4 x allowed); logmel 0.35 of its bound on the power tap and at most 0.30 from the samples (the
largest on silent frames, where the logarithm returns log(1e-6) 1.2 ulp off), in absolute terms 0.3 .. 1.3 x torch's float32 chain
(3e-6 .. 1.3e-4) and 2.0 x for the xvector chunks bank, whose whole error is that log(1e-6) (1.15e-6 against 5.8e-7); mfcc 1.8e-7 .. 3.4e-7 norm-relative (torch 2.2e-7 .. 3.4e-7),
0.04 of the element bound; features at most 0.32 of the CMVN bound (4 frames 0.27, 432 frames 0.007, 433 frames 0.009, 1299 frames 0.005).
"""
import os
import sys

import numpy
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import frontend_f64 as ff  # noqa: E402

from sidekit_amd.nnet import Xtractor  # noqa: E402

pytestmark = pytest.mark.gpu
ARCH_NAMES = list(ff.ARCHS)
TAPS = ("power", "logmel", "mfcc", "feats")


def _say(capsys, text):
    with capsys.disabled():
        print(f"  [{text}]", end="")


def fmt(out):
    return ", ".join(f"{k} {v:.2e}" for k, v in sorted(out.items()))


class Ctx:
    """the models under test and what the kernels gave for every batch (computed once)"""

    def __init__(self, gpu):
        torch.set_num_threads(min(16, torch.get_num_threads()))
        self.gpu = gpu
        self.sds, self.models, self.cases = {}, {}, {}

    def sd(self, arch, probe):
        if (arch, probe) not in self.sds:
            self.sds[arch, probe] = ff.probe_state_dict(arch, probe)
        return self.sds[arch, probe]

    def new_model(self, arch, probe):
        m = Xtractor(ff.N_SPK, model_archi=arch, loss="aam", seed=0).to(self.gpu).eval()
        m.compute_dtype = "fp32"
        m.load_state_dict(self.sd(arch, probe), strict=True)
        return m

    def model(self, arch, probe):
        if (arch, probe) not in self.models:
            self.models[arch, probe] = self.new_model(arch, probe)
        return self.models[arch, probe]

    def fused(self, arch, probe):
        return ff.fused_rule(ff.operands(arch, self.sd(arch, probe))[1], ff.ARCHS[arch]["n_fft"])[2]

    def run(self, m, arch, x, lengths):
        """float32 samples through features(), int16 samples through a forward, taps on -> float32 CPU tensors in the library's row layout:
        power [M][nbp] (None where the projection is fused: the tap does not exist), logmel [M][n_mels], mfcc (xvector), feats [M][80]"""
        a = ff.ARCHS[arch]
        nb = a["n_fft"] // 2 + 1
        frames = [ff.n_frames(arch, n) for n in lengths]
        sp, M = ff.spans(arch, frames)
        names = ["logmel"] + (["mfcc"] if a["dct"] else []) + (["feats"] if x.dtype == torch.int16 else [])
        try:
            m.set_debug(True)
            out = m.features(x.to(self.gpu), lengths=lengths) if x.dtype != torch.int16 else m(x.to(self.gpu), is_eval=True, lengths=lengths)
            torch.cuda.synchronize()
            raw = m.debug_taps(names)
            try:
                raw["power"] = m.debug_taps(["power"])["power"]
            except ValueError:                                # no tap of that name: the fused path ran
                raw["power"] = None
            out = out.cpu() if x.dtype != torch.int16 else None
        except RuntimeError as e:      # a HIP error: nothing more is started on this device
            pytest.exit(f"front end of {tuple(x.shape)} {x.dtype} failed on the device: {e}", returncode=3)
        width = {"power": (nb + 3) // 4 * 4, "logmel": a["n_mels"], "mfcc": a["n_out"], "feats": a["n_out"]}
        t = {n: (None if raw[n] is None else torch.from_numpy(raw[n].view(numpy.float32).copy()).reshape(-1, width[n])) for n in raw}
        for n, v in t.items():
            assert v is None or v.shape[0] == M, (n, v.shape, M)
        if out is not None:                                   # (B, 80, T) -> rows; rows past an utterance are not part of features()'s contract
            assert out.shape == (len(lengths), a["n_out"], max(frames))
            t["feats"] = (t["mfcc"] if a["dct"] else t["logmel"]).clone()
            for b, (r0, n) in enumerate(sp):
                t["feats"][r0:r0 + n] = out[b, :, :n].T
        return t

    def case(self, arch, probe, kind, pcm16=False):
        """the module's batch of ``kind`` through the model of ``probe`` -> dict(t = taps, ref = references, x, lengths)"""
        key = (arch, probe, kind, pcm16)
        if key not in self.cases:
            lengths = ff.LENGTHS[arch]
            x = ff.batch(kind, lengths, seed=11, pcm16=pcm16)
            self.cases[key] = dict(x=x, lengths=lengths, t=self.run(self.model(arch, probe), arch, x, lengths),
                                   ref=ff.references(x, lengths, arch, self.sd(arch, probe)))
        return self.cases[key]


@pytest.fixture(scope="module")
def ctx(gpu):
    return Ctx(gpu)


def same_taps(a, b, rows_a, rows_b, where):
    for n in TAPS:
        if a.get(n) is None or b.get(n) is None:
            assert a.get(n) is None and b.get(n) is None, (where, n)
            continue
        assert torch.equal(a[n][rows_a].view(torch.int32), b[n][rows_b].view(torch.int32)), (where, n)


UNFUSED = [("halfresnet34", "wide"), ("halfresnet34", "dense"), ("halfresnet34", "chunks"), ("xvector", "wide"), ("xvector", "dense")]
FUSED = [("halfresnet34", "product"), ("halfresnet34", "cover"), ("xvector", "product"), ("xvector", "cover"), ("xvector", "chunks")]


@pytest.mark.parametrize("arch,probe", UNFUSED)
def test_unfused_path_against_float64(ctx, capsys, arch, probe):
    """The path no product bank takes (the MEL = false kernels, the mel GEMM at K = nbp): white and coloured float32 batches and the white
    int16 batch, every stage on the tap in front of it.  power: all n_fft / 2 + 1 bins of every own frame, pad columns and rows past an
    utterance exactly zero; logmel against the power tap; mfcc against the logmel tap (the seeded matrix in place of the DCT); features
    against the tap in front of the CMVN."""
    assert not ctx.fused(arch, probe)
    for kind, pcm16 in (("noise", False), ("coloured", False), ("noise", True)):
        c = ctx.case(arch, probe, kind, pcm16)
        assert c["t"]["power"] is not None, "the power tap is missing: the fused path ran"
        out = ff.judge(c["t"], c["ref"], arch, ctx.sd(arch, probe))
        assert out["power"] > 0, "the kernel cannot be exact"
        _say(capsys, f"{kind}{' int16' if pcm16 else ''}: {fmt(out)}")


@pytest.mark.parametrize("arch,probe", FUSED)
def test_fused_path_against_float64(ctx, capsys, arch, probe):
    """The projection inside the STFT kernel: logmel against the float64 chain from the samples (cover: every bin 0 .. N/2 under a weight,
    filters of 1 .. 64 bins, the q >= 4 chunk loop, the last chunk over the pad columns; xvector chunks: 832 chunks, 13 rounds), rows past
    an utterance log(1e-6), the silent row one value; mfcc (product: the DCT) and the features each on the tap in front."""
    assert ctx.fused(arch, probe)
    for kind, pcm16 in (("noise", False), ("coloured", False), ("noise", True)):
        c = ctx.case(arch, probe, kind, pcm16)
        assert c["t"]["power"] is None, "a power tap exists: the unfused path ran"
        out = ff.judge(c["t"], c["ref"], arch, ctx.sd(arch, probe))
        _say(capsys, f"{kind}{' int16' if pcm16 else ''}: {fmt(out)}")


@pytest.mark.parametrize("arch", ARCH_NAMES)
def test_fused_and_unfused_agree(ctx, capsys, arch):
    """cover (fused) and wide (unfused) share every filter but the 64 / 65-bin one: a fresh model per bank, the missing 'power' tap telling
    which path ran, and the shared filters judged by the fused path's criterion on both."""
    shared = [j for j in range(ff.ARCHS[arch]["n_mels"]) if j != 7]
    lengths = ff.LENGTHS[arch]
    x = ff.batch("noise", lengths, seed=11)
    worst = {}
    for probe in ("cover", "wide"):
        t = ctx.run(ctx.new_model(arch, probe), arch, x, lengths)
        assert (t["power"] is None) == (probe == "cover"), probe
        ref = ctx.case(arch, probe, "noise")["ref"]
        worst[probe] = ff.check_logmel_chain(f"logmel ({probe})", t["logmel"], ref, ff.operands(arch, ctx.sd(arch, probe))[1], shared)
        same_taps(t, ctx.case(arch, probe, "noise")["t"], slice(None), slice(None), probe)     # a fresh model: the cached model's bits
    _say(capsys, "shared filters: " + ", ".join(f"{'fused' if p == 'cover' else 'unfused'} {w[0]:.3f} of the bound, max |got - r| {w[2]:.2e} (torch float32 {w[3]:.2e})"
                                               for p, w in worst.items()))


@pytest.mark.parametrize("arch", ARCH_NAMES)
def test_alone_and_in_the_batch_same_bits(ctx, arch):
    """Every utterance of the white batch run alone (B = 1: the uniform-length meta data; no padding behind it) has the bits of its own rows
    in the batch at every tap, on both paths; float32 samples equal to the int16 ones / 32768 give the int16 forward's bits; the same call
    twice gives the same bits."""
    for probe in ("cover", "wide"):
        c = ctx.case(arch, probe, "noise")
        sp = c["ref"]["spans"]
        for b, n in enumerate(c["lengths"]):
            one = ctx.run(ctx.model(arch, probe), arch, c["x"][b:b + 1, :n].contiguous(), [n])
            same_taps(one, c["t"], slice(0, sp[b][1]), slice(sp[b][0], sp[b][0] + sp[b][1]), (probe, b))
        again = ctx.run(ctx.model(arch, probe), arch, c["x"], c["lengths"])
        same_taps(again, c["t"], slice(None), slice(None), (probe, "twice"))
        p = ctx.case(arch, probe, "noise", pcm16=True)
        flt = ctx.run(ctx.model(arch, probe), arch, ff.as_float(p["x"]), p["lengths"])
        own = p["ref"]["own"]
        same_taps(flt, p["t"], own, own, (probe, "int16"))


@pytest.mark.parametrize("arch", ARCH_NAMES)
def test_neighbours_do_not_leak(ctx, arch):
    """The padding behind every row and every second row of the batch filled with 1e30, then NaN: every tap of the untouched utterances keeps
    its bits (fused and unfused path)."""
    for probe in ("cover", "wide"):
        c = ctx.case(arch, probe, "noise")
        sp = c["ref"]["spans"]
        for junk in (1e30, float("nan")):
            x = c["x"].clone()
            for b, n in enumerate(c["lengths"]):
                x[b, n:] = junk
            x[1::2] = junk
            got = ctx.run(ctx.model(arch, probe), arch, x, c["lengths"])
            for b in range(0, len(sp), 2):
                rows = slice(sp[b][0], sp[b][0] + sp[b][1])
                same_taps(got, c["t"], rows, rows, (probe, junk, b))


def tiled(arch, frames, seed=3):
    """a waveform of exactly ``frames`` frames: one second of white noise at 0.1, tiled"""
    n = (frames - 1) * ff.ARCHS[arch]["hop"]
    return ff.signal("noise", 16000, seed).float().repeat(n // 16000 + 1)[:n][None]


@pytest.mark.parametrize("arch", ARCH_NAMES)
def test_cmvn_at_every_frame_count(ctx, capsys, arch):
    """The shortest utterance the library takes (4 frames of the mel model, 15 of the TDNN), 431, 432 (the last of cmvn_reg_kernel), 433 and
    1299 frames (cmvn_kernel): the features against cmvn_ref(the tap in front) within the bound in u and n."""
    probe, msg = "product", []
    a = ff.ARCHS[arch]
    pre = "mfcc" if a["dct"] else "logmel"
    S = ff.CMVN_SWITCH
    for n in (ff.n_frames(arch, a["min_samples"]), S - 1, S, S + 1, 3 * (S + 1)):
        x = tiled(arch, n) if n > 15 else ff.signal("noise", a["min_samples"], 4).float()[None]
        t = ctx.run(ctx.model(arch, probe), arch, x, [x.shape[1]])
        assert t[pre].shape[0] == n
        msg.append(f"{n}: {ff.check_cmvn('feats', t['feats'], t[pre], [(0, n)]):.3f}")
    _say(capsys, "frames: largest share of the bound " + ", ".join(msg))


@pytest.mark.parametrize("arch", ARCH_NAMES)
def test_bits_across_the_cmvn_switch(ctx, arch):
    """A 100-frame utterance alone (cmvn_reg_kernel) and beside a 433-frame one (cmvn_kernel: the batch's longest decides): the same feature
    bits, and the same bits at every tap in front."""
    assert ff.CMVN_SWITCH == 432
    x100, x433 = tiled(arch, 100, seed=5), tiled(arch, 433, seed=6)
    n100, n433 = x100.shape[1], x433.shape[1]
    both = torch.full((2, n433), ff.PAD_VALUE)
    both[0, :n100] = x100[0]
    both[1] = x433[0]
    m = ctx.model(arch, "product")
    alone, pair = ctx.run(m, arch, x100, [n100]), ctx.run(m, arch, both, [n100, n433])
    same_taps(alone, pair, slice(0, 100), slice(0, 100), "switch")
    long_alone = ctx.run(m, arch, x433, [n433])
    r0 = ff.spans(arch, [100, 433])[0][1][0]
    same_taps(long_alone, pair, slice(0, 433), slice(r0, r0 + 433), "long")


def test_lengths_the_library_refuses(ctx):
    """160 * 3 samples (fewer than the reflect padding of the reference admits) and, for the TDNN, 1025 samples (3 frames < its context of 15)
    are refused before anything is launched; the next valid call gives the cached bits."""
    for arch, n in (("halfresnet34", 480), ("halfresnet34", 512), ("xvector", 1025), ("xvector", 14 * 512 - 1)):
        m = ctx.model(arch, "cover")
        with pytest.raises(ValueError):
            m.features(torch.zeros(1, n).to(ctx.gpu))
        c = ctx.case(arch, "cover", "noise")
        same_taps(ctx.run(m, arch, c["x"], c["lengths"]), c["t"], slice(None), slice(None), (arch, n))
