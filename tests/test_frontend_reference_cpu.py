"""The float64 reference of the waveform front end (tests/tools/frontend_f64.py) without a GPU: pinned to the oracle in float64, its probe
banks shown to do what they claim, torch's float32 evaluation shown to pass every criterion on the batches tests/test_gpu_frontend_kernels.py
uses, and fifteen wrong front ends shown to fail them -- three of which the suite's earlier judgement (CMVN'ed features of the product bank,
norm-relative 1e-4) lets through."""
import os
import sys

import numpy
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import frontend_f64 as ff  # noqa: E402

from oracle import frontend as ofe  # noqa: E402

F32 = torch.float32
ARCH_NAMES = list(ff.ARCHS)
_cache = {}


def _say(capsys, text):
    with capsys.disabled():
        print(f"  [{text}]", end="")


def sd_of(arch, probe):
    if (arch, probe) not in _cache:
        _cache[arch, probe] = ff.probe_state_dict(arch, probe)
    return _cache[arch, probe]


def ref_of(arch, probe, kind, short=False, pcm16=False):
    """the references of the module's batch (``short``: its first three rows and the silent one)"""
    key = (arch, probe, kind, short, pcm16)
    if key not in _cache:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        lengths = ff.LENGTHS[arch]
        lengths = lengths[:3] + lengths[-1:] if short else lengths
        _cache[key] = ff.references(ff.batch(kind, lengths, seed=11, pcm16=pcm16), lengths, arch, sd_of(arch, probe))
    return _cache[key]


def is_fused(arch, probe):
    return ff.fused_rule(ff.operands(arch, sd_of(arch, probe))[1], ff.ARCHS[arch]["n_fft"])[2]


# ---- the tool is the oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ARCH_NAMES)
def test_chain_reproduces_the_oracle_in_float64(arch, capsys):
    """product buffers: the chain's features are the oracle's melspec_frontend / mfcc_frontend evaluated in float64 on the same window, bank
    and DCT, every utterance run alone, within 1e-10 norm-relative (pre-emphasis 0.97 as the oracle's double, where the library's is
    float32(0.97): an operand, not arithmetic); the buffers themselves are the oracle's."""
    a, sd = ff.ARCHS[arch], sd_of(arch, "product")
    window, fb, dct = ff.operands(arch, sd)
    if arch == "halfresnet34":
        assert torch.equal(fb, ofe.mel_filterbank(513, 90, 7600, 80, 16000)) and torch.allclose(window, ofe.hann_window(400), atol=1e-7)
    else:
        assert torch.equal(fb, ofe.mel_filterbank(1025, 133.333, 6855.4976, 100, 16000)) and torch.equal(dct, ofe.dct_matrix(80, 100))
        assert torch.allclose(window, ofe.hann_window(1024), atol=1e-7)
    worst = 0.0
    for kind in ("noise", "coloured"):
        for b, n in enumerate(ff.LENGTHS[arch][:-1]):
            x = ff.signal(kind, n, seed=5 + b)
            mine = ff.chain([x], arch, sd, pe=0.97)["feats"]
            if arch == "halfresnet34":
                theirs = ofe.melspec_frontend(x, fb=fb.double(), window=window.double())
            else:
                theirs = ofe.mfcc_frontend(x, fb=fb.double(), dct=dct.double(), window=window.double())
            assert theirs.dtype == torch.float64 and theirs.shape == (1, a["n_out"], ff.n_frames(arch, n))
            worst = max(worst, ((mine - theirs[0].T).norm() / theirs.norm()).item())
    _say(capsys, f"{arch}: largest norm-relative distance from the float64 oracle {worst:.1e}")
    assert worst < 1e-10


def test_cmvn_ref_of_one_row_is_zero():
    x = torch.randn(5, 80, generator=torch.Generator().manual_seed(0))
    out = ff.cmvn_ref(x, [(0, 1), (1, 2)])
    assert bool((out[0] == 0).all()) and torch.equal(out[3:], x[3:].double())
    assert torch.allclose(out[1], -out[2]) and bool((out[1].abs() < 1).all()) and bool((out[1].abs() > 0.9).any())


# ---- the probes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ARCH_NAMES)
def test_probe_banks_do_what_they_claim(arch, capsys):
    """build_frontend's rule restated: product and cover are fused, wide and dense are not (width), chunks is not at n_fft 1024 (640 + 8 > 624)
    and IS at 2048 (832 + 8 <= 1264: the LDS condition cannot be reached there).  cover weights every bin and holds the widths it promises;
    the product bank leaves 32 (n_fft 1024) / 165 (2048) bins without any weight -- among them bins 0 and N/2."""
    a = ff.ARCHS[arch]
    nb = a["n_fft"] // 2 + 1
    rule = {p: ff.fused_rule(ff.operands(arch, sd_of(arch, p))[1], a["n_fft"]) for p in ff.PROBES}
    assert rule["product"][2] and rule["cover"][2] and rule["cover"][0] == 64
    assert rule["wide"] == (65, rule["cover"][1], False) or (rule["wide"][0] == 65 and not rule["wide"][2])
    assert rule["dense"][0] == nb and not rule["dense"][2]
    assert rule["chunks"][0] == 64 and rule["chunks"][1] == (640 if arch == "halfresnet34" else 832)
    assert rule["chunks"][2] == (arch == "xvector")
    for p in ff.PROBES:
        window, fb, dct = ff.operands(arch, sd_of(arch, p))
        assert fb.shape == (nb, a["n_mels"]) and bool((fb >= 0).all()) and bool((window > 0).all() if p != "product" else (window >= 0).all())
        if p != "product":
            assert not torch.equal(window, window.flip(0)) and not torch.equal(window[1:], window[1:].flip(0))
    fb = ff.operands(arch, sd_of(arch, "cover"))[1]
    assert bool((fb.sum(1) > 0).all()), "cover leaves a bin unweighted"
    widths = [int((fb[:, j] != 0).sum()) for j in range(fb.shape[1])]
    assert set(ff.SPECIAL_WIDTHS) <= set(widths) and 0 in widths and 24 in widths
    last = [j for j in range(fb.shape[1]) if fb[nb - 1, j] != 0]
    assert len(last) == 1 and widths[last[0]] % 8 != 0, "no filter ends on bin N/2 with a length that is no multiple of 8"
    nz = fb[fb != 0]
    assert nz.unique().numel() == nz.numel(), "weights are not distinct"
    wide = ff.operands(arch, sd_of(arch, "wide"))[1]
    assert [j for j in range(fb.shape[1]) if not torch.equal(fb[:, j], wide[:, j])] == [7]
    dark = ff.operands(arch, sd_of(arch, "product"))[1].sum(1) == 0
    assert int(dark.sum()) == (32 if arch == "halfresnet34" else 165) and bool(dark[0]) and bool(dark[-1])
    _say(capsys, f"{arch}: (widest filter, chunks, fused) {rule}; product leaves {int(dark.sum())} of {nb} bins unweighted")


# ---- a float32 model of the stages, with one thing wrong --------------------------------------------------------------------------------
def power_split32(frames, arch, wrong_twiddle=False):
    """the power spectrum the way the kernel makes it: the n_fft / 2-point complex transform of z[n] = x[2n] + i x[2n + 1] and the real-FFT
    split X[k] = (Z[k] + conj Z[NH - k]) / 2 - i W^k (Z[k] - conj Z[NH - k]) / 2 in complex64; ``wrong_twiddle``: bin N/4 takes W^(N/4 + 1)"""
    a = ff.ARCHS[arch]
    n_fft, win = a["n_fft"], a["win"]
    nh = n_fft // 2
    x = numpy.zeros((frames.shape[0], n_fft), numpy.float32)
    x[:, (n_fft - win) // 2:(n_fft + win) // 2] = frames.numpy()
    Z = numpy.fft.fft(x[:, 0::2] + 1j * x[:, 1::2], axis=1).astype(numpy.complex64)
    k = numpy.arange(nh + 1)
    Zk, Zm = Z[:, k % nh], numpy.conj(Z[:, (nh - k) % nh])
    kw = k.copy()
    if wrong_twiddle:
        kw[n_fft // 4] += 1
    W = numpy.exp(-2j * numpy.pi * kw / n_fft).astype(numpy.complex64)
    X = (0.5 * (Zk + Zm) - 0.5j * W * (Zk - Zm)).astype(numpy.complex64)
    return torch.from_numpy((X.real ** 2 + X.imag ** 2).astype(numpy.float32))


def project_chunks32(P, fb, drop_q4=False, pad=0.0):
    """the fused projection as mel_chunks_project walks it: 8-tap chunks from the filter's first bin, zero weights past its last, reading
    the power row with its pad columns behind bin N/2 (``pad``: what they hold); ``drop_q4``: chunks 4 and up are not added"""
    nb, n_mels = fb.shape
    row = numpy.full((P.shape[0], nb + 7), pad, numpy.float32)
    row[:, :nb] = P.numpy()
    out = numpy.zeros((P.shape[0], n_mels), numpy.float32)
    for j in range(n_mels):
        nz = numpy.nonzero(fb[:, j].numpy())[0]
        if nz.size == 0:
            continue
        st, ln = int(nz[0]), int(nz[-1] - nz[0] + 1)
        for q in range((ln + 7) // 8):
            if drop_q4 and q >= 4:
                break
            w = numpy.zeros(8, numpy.float32)
            m = min(8, ln - 8 * q)
            w[:m] = fb[st + 8 * q:st + 8 * q + m, j].numpy()
            out[:, j] += (row[:, st + 8 * q:st + 8 * q + 8] * w).sum(1)
    return torch.from_numpy(out)


def model32(ref, arch, sd, fused, mut=None, bins=None):
    """float32 taps of one batch as the library chains its stages, each on the output of the one before; ``mut`` names the one thing wrong"""
    a = ff.ARCHS[arch]
    window, fb, dct = ff.operands(arch, sd)
    nb = a["n_fft"] // 2 + 1
    nbp = (nb + 3) // 4 * 4
    P = torch.zeros(ref["M"], nbp, dtype=F32)
    for j, ((r0, n), x) in enumerate(zip(ref["spans"], ref["xs"])):
        x = x.float()
        if mut == "int16 scaled by 1/32767":
            x = x * numpy.float32(32768.0 / 32767.0)
        kw = {}
        if mut == "predecessor before the reflection":
            kw["reflect_first"] = False
        if mut == "boundary frame as an edge frame with L - 1" and j == 0:
            L = x.shape[0]
            tb = (L - a["win"] // 2) // a["hop"]
            assert tb * a["hop"] + a["win"] // 2 == L, "utterance 0 has no frame exactly on the interior boundary"
            kw["edge_L"] = (tb, L - 1)
        fr = ff.frames_ref(x, arch, window * 2 if mut == "window x 2" else window, F32, **kw)
        p = power_split32(fr, arch, True) if mut == "bin N/4 with the neighbour's twiddle" else ff.power_ref(fr, arch, F32)
        if mut == "bins 0 and N/2 swapped":
            p = p[:, [nb - 1] + list(range(1, nb - 1)) + [0]]
        if mut == "unweighted bins zeroed":
            p[:, bins] = 0
        if mut == "power x 4":
            p = p * 4
        if mut == "last frame dropped":
            p[-1] = 0
        P[r0:r0 + n, :nb] = p
    eps = 0.0 if mut == "log without the 1e-6" else ff.LOG_EPS
    if mut == "last chunk reads non-zero pad columns" or mut == "chunks q >= 4 dropped":
        if fused:
            s = project_chunks32(P[:, :nb], fb, drop_q4=mut.startswith("chunks"), pad=float("nan") if mut.startswith("last") else 0.0)
        else:                                                  # the GEMM runs over K = nbp: every filter meets the pad columns
            Pn = P.clone()
            Pn[:, nb:] = float("nan")
            s = Pn @ torch.cat([fb, torch.zeros(nbp - nb, fb.shape[1])])
        logmel = torch.log(s + eps)
    else:
        logmel = ff.logmel_ref(P[:, :nb], fb, F32, eps)
    t = {"power": None if fused else P, "logmel": logmel}
    pre = logmel
    if dct is not None:
        d = dct.reshape(a["n_out"], a["n_mels"]).T.contiguous() if mut == "DCT transposed" else dct
        pre = t["mfcc"] = ff.mfcc_ref(logmel, d, F32)
    counts = None
    if mut == "CMVN over the batch's longest length":
        counts = [min(max(ref["frames"]), ref["M"] - r0) for r0, _ in ref["spans"]]
    t["feats"] = ff.cmvn_ref(pre, ref["spans"], eps=0.0 if mut == "CMVN without eps" else 1e-5, prec=F32,
                             ddof=1 if mut == "CMVN with n - 1" else 0, counts=counts)
    return t


@pytest.mark.parametrize("arch", ARCH_NAMES)
def test_torch_float32_passes_every_criterion(arch, capsys):
    """torch's float32 evaluation of every stage, chained as the library chains them, passes every criterion on every batch of the GPU
    module (five probes, white and coloured signal, float and int16 samples).  The spectrum yardstick is floored at 2 u (4 x the floor is
    8 u of the frame's largest bin, which float32 itself stores to u), the absolute log-mel one at 8 u (4 x: two float32 ulp of
    log(1e-6)); on these batches torch's own error is above both floors everywhere, and the floors are shown on an exact evaluation."""
    worst, floors = {}, 0
    for probe in ff.PROBES:
        for kind, pcm16 in (("noise", False), ("coloured", False), ("noise", True)):
            ref = ref_of(arch, probe, kind, pcm16=pcm16)
            out = ff.judge(model32(ref, arch, sd_of(arch, probe), is_fused(arch, probe)), ref, arch, sd_of(arch, probe))
            for k, v in out.items():
                worst[k] = max(worst.get(k, 0.0), v)
            floors += int(out.get("power_yard", 1.0) == ff.POWER_FLOOR) + int(out.get("logmel_yard", 1.0) == ff.POWER_FLOOR)
            floors += int(out.get("logmel_abs_yard", 1.0) == ff.LOG_FLOOR)
            assert out.get("power_yard", 1.0) >= 2 * ff.U32 and out.get("logmel_yard", 1.0) >= 2 * ff.U32 and out.get("logmel_abs_yard", 1.0) >= 8 * ff.U32
    assert ff.power_yardstick(torch.ones(3, 4), torch.ones(3, 4).double()) == ff.POWER_FLOOR == 2 * ff.U32
    # an evaluation that happens to be exact: the yardsticks sit on their floors, and a value one float32 ulp of log(1e-6) (16 u) off still passes
    ref = ref_of(arch, "cover", "noise", short=True)
    exact = dict(ref, r32=ref["r"])
    fb = ff.operands(arch, sd_of(arch, "cover"))[1]
    got = ref["r"]["logmel"].clone()
    got[ref["own"]] += 16 * ff.U32
    assert ff.check_logmel_chain("logmel", got, exact, fb)[1::2] == (ff.POWER_FLOOR, ff.LOG_FLOOR)
    got[ref["own"]] += 32 * ff.U32
    with pytest.raises(AssertionError):
        ff.check_logmel_chain("logmel", got, exact, fb)
    _say(capsys, f"{arch}: largest over the batches " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())) + f"; yardsticks on their floor: {floors}")


MUTANTS = [  # (what is wrong, the probe that shows it, also passes the old judgement on the product bank)
    ("bins 0 and N/2 swapped", "cover", False),
    ("bins 0 and N/2 swapped", "dense", False),
    ("bin N/4 with the neighbour's twiddle", "cover", False),
    ("bin N/4 with the neighbour's twiddle", "wide", False),
    ("unweighted bins zeroed", "cover", True),
    ("power x 4", "cover", True),
    ("power x 4", "wide", True),
    ("window x 2", "cover", True),
    ("window x 2", "dense", True),
    ("predecessor before the reflection", "cover", False),
    ("predecessor before the reflection", "wide", False),
    ("boundary frame as an edge frame with L - 1", "cover", False),
    ("boundary frame as an edge frame with L - 1", "wide", False),
    ("last frame dropped", "cover", False),
    ("last frame dropped", "wide", False),
    ("chunks q >= 4 dropped", "cover", False),
    ("last chunk reads non-zero pad columns", "cover", False),
    ("last chunk reads non-zero pad columns", "wide", False),
    ("log without the 1e-6", "cover", False),
    ("log without the 1e-6", "wide", False),
    ("CMVN with n - 1", "cover", False),
    ("CMVN over the batch's longest length", "cover", False),
    ("CMVN without eps", "cover", False),
    ("DCT transposed", "cover", False),
    ("DCT transposed", "product", False),
    ("int16 scaled by 1/32767", "cover", False),
    ("int16 scaled by 1/32767", "wide", False),
]


@pytest.mark.parametrize("arch", ARCH_NAMES)
def test_wrong_front_ends_fail(arch, capsys):
    """Each wrong front end, as float32 taps on the module's white-noise batch (its first three rows and the silent one), fails at least one
    criterion, where the same model with nothing wrong passes.  The three that only change unobserved bins or a constant factor -- the 32 /
    165 unweighted bins zeroed, power x 4, window x 2 -- pass the suite's earlier judgement on the product bank (CMVN'ed features,
    norm-relative 1e-4 per utterance), and 'unweighted bins zeroed' passes every NEW criterion on the product bank too: only the cover
    bank sees those bins."""
    dark = torch.nonzero(ff.operands(arch, sd_of(arch, "product"))[1].sum(1) == 0).flatten()
    told = []
    for mut, probe, old_passes in MUTANTS:
        if mut == "DCT transposed" and arch != "xvector":
            continue
        sd, fused = sd_of(arch, probe), is_fused(arch, probe)
        ref = ref_of(arch, probe, "noise", short=True)
        ff.judge(model32(ref, arch, sd, fused), ref, arch, sd)
        with pytest.raises(AssertionError) as e:
            ff.judge(model32(ref, arch, sd, fused, mut, dark), ref, arch, sd)
        told.append(f"{mut} ({probe}): {str(e.value).split(';')[0][:60]}")
        if old_passes:
            psd, pref = sd_of(arch, "product"), ref_of(arch, "product", "noise", short=True)
            t = model32(pref, arch, psd, True, mut, dark)
            for r0, n in pref["spans"][:-1]:
                err = ff.old_judgement(t["feats"][r0:r0 + n], pref["r"]["feats"][r0:r0 + n])
                assert err < 1e-4, (mut, err)
            if mut == "unweighted bins zeroed":
                ff.judge(t, pref, arch, psd)
    with capsys.disabled():
        print("".join(f"\n    {s}" for s in told), end="")
