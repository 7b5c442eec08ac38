"""Float64 reference of the waveform front end (waveform -> power spectrum -> log-mel -> [DCT] -> CMVN) one kernel at a time, on the
kernels' actual operands (CPU only; torch + numpy), the probe checkpoints that make every spectrum bin and both projection paths
observable, and the criteria the GPU tests judge the kernels by.

Written from csrc/frontend_fft.hip (frame_input / frame_input_edge: pre-emphasis x[i] - pe x[p] with pe = float32(0.97), p = 1 for i = 0,
the STFT's reflection applied to the index BEFORE the predecessor is taken; the window and the bank as the state dict holds them),
build_frontend / frontend_rows of csrc/xt_api.hip (which bank stays fused; log(. + 1e-6); the DCT GEMM) and cmvn_kernel / cmvn_reg_kernel of
csrc/pool.hip (biased variance over the utterance's own rows, eps = 1e-5).  Each function takes what ONE kernel reads:

    frames_ref(x, arch, window)       windowed, pre-emphasised frames [T][win] of one utterance's samples (float32, or int16 / 32768: exact)
    power_ref(frames, arch)           |rfft|^2, all n_fft / 2 + 1 bins                                  -> [T][nb]
    logmel_ref(power, fb)             log(power @ fb + 1e-6)                                            -> [M][n_mels]
    mfcc_ref(logmel, dct)             logmel @ dct                                                      -> [M][n_out]
    cmvn_ref(rows, spans)             (x - mean) / sqrt(biased var + 1e-5) over each utterance's rows; other rows as they were

``prec`` is the arithmetic: float64 for the reference, float32 for "what torch gives on the same operands in single precision on the CPU"
(torch.fft.rfft of the float32 frames, a float32 matmul, torch.log) -- the yardstick of the criteria.

Rows are laid out as the library lays them out (spans()): 'halfresnet34' pads every utterance to the batch's longest, row = b T + t, the rows
past an utterance's last frame holding zero power and log(1e-6); 'xvector' is ragged, the utterances' frames one after the other.

Probe checkpoints (probe_state_dict): seeded_state_dict(..) with only the front-end buffers replaced, all weights >= 0:

    product   the bank, the window and the DCT as shipped
    cover     fused: 8 filters of 1, 7, 8, 9, 16, 17, 33 and 64 bins, then filters of 5-6 (n_fft 1024) or 9-10 bins (2048) up to bin N/2 --
              the last ends ON bin N/2 with a length that is no multiple of 8, so its last chunk reads the zeroed pad columns -- one
              filter of 24 bins across the 33- and the 64-bin ones, one all-zero filter; seeded distinct weights in [0.5, 1.5)
    wide      cover with the 64-bin filter one bin longer: unfused by width
    dense     every filter weights every bin: unfused by width
    chunks    filters of 57..64 bins, eight chunks each.  n_fft 1024: 80 x 8 = 640 chunks, 640 + 8 > 624: unfused by the LDS condition.
              n_fft 2048: 100 x 8 = 800 chunks, padded 832, 832 + 8 <= 1264: such a bank CANNOT reach the LDS condition there (100 filters of
              at most 64 bins are at most 832 chunks); it stays fused, with 13 rounds of the chunk loop, and only width unfuses at 2048.
All but ``product`` carry a seeded positive window that is not symmetric and, for the MFCC model, a seeded dense dct_mat.
"""
import math

import numpy
import torch

import tdnn_f64 as tf

U32 = 2.0 ** -24
PE = float(numpy.float32(0.97))
LOG_EPS = 1e-6
N_SPK = 16
ARCHS = {
    "halfresnet34": dict(n_fft=1024, win=400, hop=160, n_mels=80, n_out=80, window="preprocessor.MelSpec.spectrogram.window",
                         fb="preprocessor.MelSpec.mel_scale.fb", dct=None, min_samples=513),
    "xvector": dict(n_fft=2048, win=1024, hop=512, n_mels=100, n_out=80, window="preprocessor.MFCC.MelSpectrogram.spectrogram.window",
                    fb="preprocessor.MFCC.MelSpectrogram.mel_scale.fb", dct="preprocessor.MFCC.dct_mat", min_samples=14 * 512),
}
PROBES = ("product", "cover", "wide", "dense", "chunks")
SPECIAL_WIDTHS = (1, 7, 8, 9, 16, 17, 33, 64)
CMVN_SWITCH = 432                       # launch_cmvn: cmvn_reg_kernel<36> up to 36 * TG rows, TG = 12 at D = 80
# floors of the yardsticks, so that 4 x yardstick never asks for more than float32 can hold: the frame's largest bin is itself stored to u;
# a log-mel value of magnitude 8 .. 16 (log(1e-6) = -13.8) has an ulp of 16 u, and a 1-ulp log2 times ln 2 may be 2 ulp off
POWER_FLOOR = 2 * U32
LOG_FLOOR = 8 * U32
FACTOR = 4.0
# The module's batches: at most 8 rows of at most 1.5 s, the LAST row digital silence.  n_fft 1024 (hop 160): 160 * 9 + 200 -- frame 9 is
# exactly interior (its last tap on the last sample) --, one sample less, 513 (the shortest the reflect padding admits: all four frames are
# edge frames), a multiple of the hop, a length that is none, 1.5 s.  n_fft 2048 (hop 512): 512 * 14 + 512 -- frame 14 exactly interior --,
# one sample less, 512 * 14 (the 15 frames the TDNN needs), a length that is no multiple of the hop, 1.5 s; frame 1 is an edge frame by
# i0 = 0 alone in every one of them.
LENGTHS = {"halfresnet34": [160 * 9 + 200, 160 * 9 + 199, 513, 4800, 5003, 24000, 2000],
           "xvector": [512 * 14 + 512, 512 * 14 + 511, 512 * 14, 9001, 24000, 8000]}


# ---- layout ---------------------------------------------------------------------------------------------------------------------------
def n_frames(arch, n_samples):
    return 1 + int(n_samples) // ARCHS[arch]["hop"]


def spans(arch, frames):
    """[(first row, rows)] of every utterance and the number of rows of the batch"""
    if arch == "halfresnet34":
        T = max(frames)
        return [(b * T, int(f)) for b, f in enumerate(frames)], len(frames) * T
    off = numpy.concatenate(([0], numpy.cumsum(frames))).astype(int).tolist()
    return [(off[b], int(f)) for b, f in enumerate(frames)], off[-1]


def own_rows(arch, frames):
    sp, M = spans(arch, frames)
    m = torch.zeros(M, dtype=torch.bool)
    for r0, n in sp:
        m[r0:r0 + n] = True
    return m


# ---- probe checkpoints ----------------------------------------------------------------------------------------------------------------
def cover_layout(nb, n_mels, widen=0):
    """[(first bin, bins)] per filter of the ``cover`` bank; ``widen``: that many bins more for the 64-bin filter"""
    lay, at = [], 0
    for w in SPECIAL_WIDTHS:
        lay.append((at, w + (widen if w == 64 else 0)))
        at += w
    rest_n = n_mels - len(SPECIAL_WIDTHS) - 2
    rest = nb - at
    base, extra = divmod(rest, rest_n)
    for j in range(rest_n):                                   # the wider ones first: the last filter has ``base`` bins
        w = base + (1 if j < extra else 0)
        lay.append((at, w))
        at += w
    assert at == nb and 0 < base <= 64 and base % 8 != 0
    start33 = sum(SPECIAL_WIDTHS[:6])
    lay.append((start33 + 20, 24))                            # bins 20..32 of the 33-bin filter and 0..10 of the 64-bin one
    lay.append((0, 0))                                        # all zero
    return lay


def chunks_layout(nb, n_mels):
    """filters of 57..64 bins spread over the whole spectrum, the first on bin 0, the last ending on bin N/2"""
    lay = []
    for j in range(n_mels):
        w = 57 + j % 8
        lay.append((int(round(j * (nb - w) / (n_mels - 1))), w))
    return lay


def bank(arch, probe, seed=70):
    """the (nb, n_mels) float32 mel_scale.fb of a probe; None for 'product'"""
    a = ARCHS[arch]
    nb, n_mels = a["n_fft"] // 2 + 1, a["n_mels"]
    if probe == "product":
        return None
    rs = numpy.random.RandomState(seed + a["n_fft"])
    w = rs.uniform(0.5, 1.5, (nb, n_mels)).astype(numpy.float32)      # drawn once: cover and wide share every weight they both have
    if probe == "dense":
        return torch.from_numpy(w / numpy.float32(8.0))
    lay = chunks_layout(nb, n_mels) if probe == "chunks" else cover_layout(nb, n_mels, widen=1 if probe == "wide" else 0)
    fb = numpy.zeros((nb, n_mels), numpy.float32)
    for j, (st, ln) in enumerate(lay):
        fb[st:st + ln, j] = w[st:st + ln, j]
    return torch.from_numpy(fb)


def probe_state_dict(arch, probe, seed=31):
    """seeded_state_dict with the front-end buffers of ``probe``"""
    from sidekit_amd.nnet.weights import seeded_state_dict
    a = ARCHS[arch]
    sd = seeded_state_dict(arch, N_SPK, 256, "aam", seed)
    if probe == "product":
        return sd
    rs = numpy.random.RandomState(seed + 7)
    sd[a["fb"]] = bank(arch, probe)
    sd[a["window"]] = torch.from_numpy(rs.uniform(0.1, 1.0, a["win"]).astype(numpy.float32))
    if a["dct"]:
        sd[a["dct"]] = torch.from_numpy((rs.standard_normal((a["n_mels"], a["n_out"])) * 0.1).astype(numpy.float32))
    return sd


def operands(arch, sd):
    """(window, fb, dct or None) as the state dict holds them"""
    a = ARCHS[arch]
    return sd[a["window"]], sd[a["fb"]], (sd[a["dct"]] if a["dct"] else None)


def fused_rule(fb, n_fft):
    """build_frontend's decision restated on the host: (widest filter, padded chunks, fused)"""
    fb = numpy.asarray(fb)
    chunks, widest = 0, 0
    for j in range(fb.shape[1]):
        nz = numpy.nonzero(fb[:, j])[0]
        ln = int(nz[-1] - nz[0] + 1) if nz.size else 0
        widest = max(widest, ln)
        chunks += (ln + 7) // 8 if ln else 1
    chunks = (chunks + 63) // 64 * 64
    room = 2 * (n_fft // 2 + n_fft // 16) - (n_fft // 2 + 16)         # 624 floats at n_fft 1024, 1264 at 2048
    return widest, chunks, 0 < widest <= 64 and chunks + 8 <= room


# ---- signals --------------------------------------------------------------------------------------------------------------------------
def signal(kind, n, seed):
    """float64 samples: 'noise' white at 0.1 (every bin comparable), 'coloured' white noise through a one-pole low-pass plus two tones (the
    signal of tests/test_gpu_halfresnet.py: high bands 40 dB under the low ones), 'silence' zeros"""
    g = torch.Generator().manual_seed(seed)
    if kind == "silence":
        return torch.zeros(n, dtype=torch.float64)
    w = torch.randn(n, generator=g, dtype=torch.float64)
    if kind == "noise":
        return 0.1 * w
    x = torch.from_numpy(_one_pole(w.numpy(), 0.95))
    t = torch.arange(n, dtype=torch.float64) / 16000.0
    return 0.02 * x + 0.3 * torch.sin(2 * numpy.pi * 440.0 * t) + 0.05 * torch.sin(2 * numpy.pi * 3000.0 * t)


def _one_pole(w, a):
    y, acc = numpy.empty_like(w), 0.0
    for i in range(w.shape[0]):                               # y[i] = a y[i-1] + w[i]
        acc = a * acc + w[i]
        y[i] = acc
    return y


PAD_VALUE = 7.0                                               # no sample of any signal reaches it


def batch(kind, lengths, seed, pcm16=False):
    """(B, max length) float32 -- or int16 -- batch: row b holds ``lengths[b]`` samples of ``kind`` (the LAST row digital silence), the
    rest PAD_VALUE (int16: 7 * 4096, which no sample reaches either)"""
    L = max(lengths)
    x = torch.full((len(lengths), L), PAD_VALUE, dtype=torch.float64)
    for b, n in enumerate(lengths):
        x[b, :n] = signal("silence" if b == len(lengths) - 1 else kind, n, seed + b)
    if pcm16:
        return (x * 4096.0).round().clamp(-32768, 32767).to(torch.int16)
    return x.float()


def as_float(x):
    """the values the kernel computes on: float32 as they are, int16 / 32768 (exact in float32)"""
    return x.float() / 32768.0 if x.dtype == torch.int16 else x


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------
def frames_ref(x, arch, window, prec=torch.float64, pe=PE, reflect_first=True, edge_L=None):
    """[T][win]: window[k] (x[i] - pe x[p]) for i = reflect(t hop - win / 2 + k), p = i - 1 or 1 for i = 0.  ``reflect_first`` False and
    ``edge_L`` are the mutation check's: the predecessor taken before the reflection; another length in the reflection of frame ``edge_L[0]``"""
    a = ARCHS[arch]
    L, win, hop = x.shape[0], a["win"], a["hop"]
    T = 1 + L // hop
    i = torch.arange(T)[:, None] * hop - win // 2 + torch.arange(win)[None, :]
    Lr = torch.full((T, 1), L)
    if edge_L is not None:
        Lr[edge_L[0]] = edge_L[1]

    def refl(j):
        j = j.abs()
        return torch.where(j >= Lr, 2 * (Lr - 1) - j, j)
    if reflect_first:
        i = refl(i)
        p = torch.where(i == 0, torch.ones_like(i), i - 1)
    else:
        p = refl(i - 1)
        i = refl(i)
    x = x.to(prec)
    return window.to(prec)[None, :] * (x[i] - torch.tensor(pe, dtype=prec) * x[p])


def power_ref(frames, arch, prec=torch.float64):
    """|rfft(frame, n_fft)|^2 (the power does not depend on where in the n_fft points the window sits)"""
    X = torch.fft.rfft(frames.to(prec), n=ARCHS[arch]["n_fft"], dim=1)
    return X.real ** 2 + X.imag ** 2


def logmel_ref(power, fb, prec=torch.float64, eps=LOG_EPS):
    return torch.log(power.to(prec) @ fb.to(prec) + eps)


def mfcc_ref(logmel, dct, prec=torch.float64, with_S=False):
    x, d = logmel.to(prec), dct.to(prec)
    return (x @ d, x.abs() @ d.abs()) if with_S else x @ d


def cmvn_ref(rows, sp, eps=1e-5, prec=torch.float64, ddof=0, counts=None):
    """every span's rows normalised over the span, all other rows as they were.  ``ddof`` and ``counts`` (rows per span to take the
    statistics over, in place of the span's own) are the mutation check's"""
    out = rows.to(prec).clone()
    for j, (r0, n) in enumerate(sp):
        x = rows[r0:r0 + n].to(prec)
        if counts is None:
            mean, var = x.mean(0), ((x - x.mean(0)) ** 2).sum(0) / max(n - ddof, 1)
        else:
            y = rows[r0:r0 + counts[j]].to(prec)
            mean, var = y.mean(0), ((y - y.mean(0)) ** 2).mean(0)
        out[r0:r0 + n] = (x - mean) / torch.sqrt(var + eps)
    return out


def chain(xs, arch, sd, prec=torch.float64, **mut):
    """The stages one after the other from the samples of every utterance (``xs``: list of 1-D tensors), rows laid out as the library's:
    dict(power [M][nb], logmel, mfcc (xvector), feats).  Rows past an utterance hold zero power.  ``mut``: frames_ref's mutation switches."""
    window, fb, dct = operands(arch, sd)
    frames = [n_frames(arch, x.shape[0]) for x in xs]
    sp, M = spans(arch, frames)
    nb = ARCHS[arch]["n_fft"] // 2 + 1
    power = torch.zeros(M, nb, dtype=prec)
    for (r0, n), x in zip(sp, xs):
        power[r0:r0 + n] = power_ref(frames_ref(x, arch, window, prec, **mut), arch, prec)
    out = {"power": power, "logmel": logmel_ref(power, fb, prec)}
    pre = out["logmel"]
    if dct is not None:
        pre = out["mfcc"] = mfcc_ref(pre, dct, prec)
    out["feats"] = cmvn_ref(pre, sp, prec=prec)
    return out


# ---- criteria -------------------------------------------------------------------------------------------------------------------------
def power_errors(got, r):
    """per frame: max |got - r| / the frame's largest bin; a frame of zero power must be zero in every bin"""
    got, r = got.double(), r.double()
    top = r.max(1).values
    zero = top == 0
    assert bool((got[zero] == 0).all()), "a frame of zero power is not zero in every bin"
    assert bool(torch.isfinite(got).all()), "non-finite power"
    return (got[~zero] - r[~zero]).abs().max(1).values / top[~zero]


def power_yardstick(r32, r):
    e = power_errors(r32, r)
    return max(POWER_FLOOR, e.max().item() if e.numel() else 0.0)


def check_power(name, got, r, yard):
    """every bin of every frame within 4 x yard of the float64 value, relative to the frame's largest bin.  Returns the largest error."""
    e = power_errors(got, r)
    worst = e.max().item() if e.numel() else 0.0
    assert worst <= FACTOR * yard, f"{name}: spectrum off by {worst:.2e} of the frame's largest bin; torch's float32 {yard:.2e} (x {FACTOR:g} allowed)"
    return worst


def check_logmel_gemm(name, got, power, fb):
    """The unfused projection on its exact operand: s = power @ fb is a sum of K = nbp non-negative terms (S = s), so the float32 sum and the
    added 1e-6 are within d = 2 (K + 4) u s / (s + 1e-6) of s + 1e-6 relatively, i.e. within -log(1 - d) in the log; the logarithm itself
    and its rounding are given 4 u max(|r|, 1).  Returns the largest error as a share of its bound."""
    K = (power.shape[1] + 3) // 4 * 4
    s = power.double() @ fb.double()
    r = torch.log(s + LOG_EPS)
    d = 2 * (K + 4) * U32 * s / (s + LOG_EPS)
    bound = -torch.log1p(-d) + 4 * U32 * r.abs().clamp_min(1.0)
    got = got.double()
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite value"
    ratio = (got - r).abs() / bound
    bad = ~(ratio <= 1)
    if bool(bad.any()):
        i = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements outside the GEMM bound (K = {K}); first at {i}: got "
                             f"{got[i[0], i[1]].item()!r}, float64 {r[i[0], i[1]].item()!r}, bound {bound[i[0], i[1]].item():.3e}")
    return ratio.max().item()


def check_mfcc(name, got, logmel, dct):
    """the DCT GEMM on its exact operand: check_gemm of tests/tools/tdnn_f64.py with K = n_mels + 4"""
    r, S = mfcc_ref(logmel, dct, with_S=True)
    return tf.check_gemm(name, got, r, S, dct.shape[0] + 4, None, mfcc_ref(logmel, dct, torch.float32))


def cmvn_bound(pre, sp, eps=1e-5):
    """Per element, for the span's n rows, m and v the exact mean and biased variance, s = sqrt(v + eps), r = (x - m) / s:
         |got - r| <= (n + 2) u mean|x| / s  +  (n / 2 + 12) u |r|
    first term: the float32 mean of n values in any order and its division are within (n + 2) u mean|x| of m, and that shift
    passes to every x - mean; second term: x - mean rounds once (u), the sum of n squares by FMA in any order and its division by n are
    within (n + 2) u relatively, adding eps, the square root and the reciprocal (each allowed 2 ulp) halve that and add 6 u, the final
    product one more, 4 u are slack for the second-order terms.  Rows outside the spans: 0 (they must keep their bits)."""
    b = torch.zeros(pre.shape, dtype=torch.float64)
    r = cmvn_ref(pre, sp, eps)
    for r0, n in sp:
        x = pre[r0:r0 + n].double()
        s = torch.sqrt(((x - x.mean(0)) ** 2).mean(0) + eps)
        b[r0:r0 + n] = (n + 2) * U32 * x.abs().mean(0) / s + (n / 2 + 12) * U32 * r[r0:r0 + n].abs()
    return r, b


def check_cmvn(name, got, pre, sp):
    """the features against cmvn_ref(the pre-CMVN tap) within cmvn_bound; rows outside every span keep the tap's bits; an utterance of one
    row gives zeros.  Returns the largest error as a share of its bound."""
    r, b = cmvn_bound(pre, sp)
    got = got.double()
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite value"
    exact = b == 0
    assert bool((got[exact] == r[exact]).all()), f"{name}: an element that must be exact is not (rows past an utterance, or a column of equal values)"
    ratio = (got[~exact] - r[~exact]).abs() / b[~exact]
    assert bool((ratio <= 1).all()), f"{name}: off by {ratio.max().item():.2f} of the CMVN bound"
    return ratio.max().item() if ratio.numel() else 0.0


def check_logmel_chain(name, got, ref, fb, cols=None):
    """Log-mel rows of the utterances' own frames against the float64 chain from the samples, where the power is not observable (the fused
    path): the two criteria of the unfused path composed.  A spectrum within e of the frame's largest bin Pmax moves s = power @ fb of
    filter j by at most e Pmax W_j (W_j the filter's weights added up), i.e. the log by that over s + 1e-6; e = 4 x the spectrum
    yardstick of torch's float32 chain on the same samples (power_yardstick).  The projection of the filter's n_j bins and the logarithm
    are given their rigorous share as in check_logmel_gemm: 2 (n_j + 4) u + 4 u max(|r|, 1).  (A plain maximum of |got - r| over a batch is
    a blunt yardstick by itself: a one-bin filter on a bin 30 dB under the frame's largest carries a thousand times the error of its
    neighbours, in torch's evaluation as in any other, so that maximum is set by one element; it is asserted as well, at 4 x torch's own
    maximum over the same elements, floored at 8 u.)  ``cols``: the filters to judge.
    Returns (largest error as a share of its bound, the spectrum yardstick, max |got - r|, torch's max |r32 - r|)."""
    own = ref["own"]
    cols = torch.arange(fb.shape[1]) if cols is None else torch.as_tensor(cols)
    P = ref["r"]["power"][own]
    yard = power_yardstick(ref["r32"]["power"][own], P)
    fbd = fb.double()[:, cols]
    s, r = P @ fbd, ref["r"]["logmel"][own][:, cols]
    n_j = (fbd != 0).sum(0)
    bound = FACTOR * yard * P.max(1, keepdim=True).values * fbd.sum(0) / (s + LOG_EPS) + 2 * (n_j + 4) * U32 + 4 * U32 * r.abs().clamp_min(1.0)
    g = got[own][:, cols].double()
    assert bool(torch.isfinite(g).all()), f"{name}: non-finite value"
    ratio = (g - r).abs() / bound
    bad = ~(ratio <= 1)
    if bool(bad.any()):
        i = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements outside the bound of a spectrum within {FACTOR:g} x {yard:.2e} of the "
                             f"frame's largest bin; first at own row {i[0]}, filter {int(cols[i[1]])}: got {g[i[0], i[1]].item()!r}, float64 "
                             f"{r[i[0], i[1]].item()!r}, bound {bound[i[0], i[1]].item():.3e}")
    worst = (g - r).abs().max().item()
    yard_abs = max(LOG_FLOOR, (ref["r32"]["logmel"][own][:, cols].double() - r).abs().max().item())
    assert worst <= FACTOR * yard_abs, f"{name}: off by {worst:.2e} in the log; torch's float32 chain {yard_abs:.2e} (x {FACTOR:g} allowed)"
    return ratio.max().item(), yard, worst, yard_abs


def references(x, lengths, arch, sd):
    """what a batch (``x`` float32 or int16, row b holding lengths[b] samples) is judged against: the float64 chain from the samples, torch's
    float32 chain (the yardstick), and the row layout"""
    xs = [as_float(x[b, :int(n)]) for b, n in enumerate(lengths)]
    frames = [n_frames(arch, n) for n in lengths]
    sp, M = spans(arch, frames)
    return dict(xs=xs, lengths=list(lengths), frames=frames, spans=sp, M=M, own=own_rows(arch, frames), r=chain(xs, arch, sd),
                r32=chain(xs, arch, sd, torch.float32))


def judge(t, ref, arch, sd):
    """Every criterion on the taps ``t`` of one batch (float32 tensors in the library's row layout: 'power' [M][nb or nbp] or None where the
    projection is fused, 'logmel', 'mfcc' for the xvector, 'feats'), each stage on the tap in front of it.  Returns what it measured."""
    a = ARCHS[arch]
    _, fb, dct = operands(arch, sd)
    nb, own, M, out = a["n_fft"] // 2 + 1, ref["own"], ref["M"], {}
    assert t["logmel"].shape == (M, a["n_mels"]) and t["feats"].shape == (M, a["n_out"]), "tap shapes"
    if t.get("power") is not None:
        P = t["power"]
        assert P.shape[0] == M and P.shape[1] in (nb, (nb + 3) // 4 * 4), "power tap shape"
        assert bool((P[:, nb:] == 0).all()), "power: a pad column is not zero"
        assert bool((P[~own] == 0).all()), "power: a row past an utterance's last frame is not zero"
        yard = power_yardstick(ref["r32"]["power"][own], ref["r"]["power"][own])
        out["power"], out["power_yard"] = check_power("power", P[own][:, :nb], ref["r"]["power"][own], yard), yard
        out["logmel_gemm"] = check_logmel_gemm("logmel", t["logmel"], P[:, :nb], fb)
    else:
        out["logmel"], out["logmel_yard"], out["logmel_abs"], out["logmel_abs_yard"] = check_logmel_chain("logmel", t["logmel"], ref, fb)
    past = t["logmel"][~own].double()
    assert past.numel() == 0 or (past - math.log(LOG_EPS)).abs().max().item() <= 2 * 2.0 ** -20, "logmel: a row past an utterance is not log(1e-6) within 2 ulp"
    for r0, n in ref["spans"]:
        if float(ref["r"]["power"][r0:r0 + n].max()) == 0.0:          # digital silence: the same value in every filter
            row = t["logmel"][r0:r0 + n]
            assert bool((row == row[:, :1]).all()), "logmel: a silent frame differs between filters"
    pre = t["logmel"]
    if dct is not None:
        out["mfcc"], out["mfcc_torch"], out["mfcc_share"] = check_mfcc("mfcc", t["mfcc"], t["logmel"], dct)
        pre = t["mfcc"]
    out["cmvn"] = check_cmvn("feats", t["feats"], pre, ref["spans"])
    return out


def old_judgement(feats, ref):
    """what the suite judged the front end by so far: the CMVN'ed features norm-relative over the whole matrix, bound 1e-4"""
    return ((feats.double() - ref).norm() / ref.norm()).item()
