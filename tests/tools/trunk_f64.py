"""Float64 reference of ONE HalfResNet34 trunk block on the kernels' actual operands (CPU only; torch + numpy).

Written from csrc/conv3x3.hip (the three epilogue forms), csrc/se_gate.hip, csrc/trunk_misc.hip (stem), the folding in
csrc/xt_api.hip (fold_bn / make_conv / finalize_half) and oracle/xvector.py.  A block is three kernels; each function below takes what
that kernel reads and returns what it computes, before the output rounding:

    conv1_ref(x)               relu(bn1(conv1(x)))                         -> the tensor the kernel rounds and stores as o1
    gate_ref(o1)               sigmoid(fc.2 relu(fc.0 mean(bn2(conv2(o1)))))  evaluated directly (no border-sum route)
    conv2_ref(o1, gate, x)     later blocks:  z = k1 acc + k0 (rounded to the compute type: the kernel's LDS tile), out = relu(z + x)
                               first blocks:  z = k1 acc + conv1x1_s(x; scale_s w) + (k0 + shift_s), out = relu(z): ONE rounding
                               with k1 = f32(scale2 gate), k0 = f32(shift2 gate) formed in float32 as the kernel forms them

Tensors are NHWC (B, H, W, C) as the kernels hold them; ``frames`` are feature frames per utterance (an utterance owns
ceil(frames / 2**n) rows after n stride-2 stages) and rows past an utterance's length come back as zeros.  ``dtype`` is the compute type:
'bf16' rounds the matrix-core operands (conv weights, folded shortcut weights) and the gated tile to bf16, 'fp32' rounds nothing.
``prec`` is the arithmetic the formulas are evaluated in: float64 for the reference, float32 for "what torch's own float32 gives on the
same operands" (the yardstick the tolerances are derived from).  BatchNorm constants are folded in float32 exactly as the library folds
them: they are operands, not arithmetic under test.
"""
import numpy
import torch
import torch.nn.functional as F

PLANES = (32, 64, 128, 256)
NBLOCKS = (3, 4, 6, 3)
# output-row tile of conv1 / conv2 of each block's shape (csrc/conv3x3.hip, the ConvCfg table): bf16 L1, L2A, L2, L3A, L3, L4A, L4 and the fp32 ones
TILE_BF16 = {"first": (8, 4, 4, 8), "rest": (8, 8, 8, 17)}
TILE_FP32 = {"first": (8, 8, 8, 16), "rest": (8, 8, 8, 16)}


def halve(h, n):
    for _ in range(n):
        h = (h + 1) // 2
    return h


class Geom:
    """Shapes of trunk block ``block`` (0..15)."""

    def __init__(self, block):
        starts = numpy.cumsum((0,) + NBLOCKS)
        assert 0 <= block < starts[-1]
        self.block = block
        self.li = int(numpy.searchsorted(starts, block, side="right") - 1)      # layer index 0..3
        self.bi = int(block - starts[self.li])
        self.first = self.bi == 0
        self.lin = max(self.li - 1, 0) if self.first else self.li                  # stride-2 stages before the block input
        self.stride = 2 if (self.first and self.li > 0) else 1
        self.cin, self.win = 32 << self.lin, 80 >> self.lin
        self.c, self.wout = 32 << self.li, 80 >> self.li
        self.prefix = f"sequence_network.layer{self.li + 1}.{self.bi}"

    def tile(self, dtype):
        """output rows per workgroup of the block's conv1 (statistics form; it also fixes the gate kernel's tile loop)"""
        t = TILE_BF16 if dtype == "bf16" else TILE_FP32
        return t["first" if self.first else "rest"][self.li]

    def rows_in(self, frames):
        return halve(frames, self.lin)

    def rows_out(self, frames):
        return halve(frames, self.li)


def bf16r(t):
    """round to the nearest bf16 (ties to even), returned in t's own dtype"""
    return t.float().bfloat16().to(t.dtype)


def fold_bn(sd, p):
    """eval-mode BatchNorm as (scale, shift) in float32, operation by operation as fold_bn of csrc/xt_api.hip"""
    g, b, m, v = (sd[f"{p}.{k}"].float() for k in ("weight", "bias", "running_mean", "running_var"))
    s = g / torch.sqrt(v + numpy.float32(1e-5))
    return s, b - m * s


def _w(sd, key, dtype):
    w = sd[key].float()
    return bf16r(w) if dtype == "bf16" else w


def _nchw(t, prec):
    return t.to(prec).permute(2, 0, 1).unsqueeze(0)


def _nhwc(t):
    return t[0].permute(1, 2, 0)


def _frames(frames, B, rows, n):
    """rows of each utterance after n stride-2 stages; None: every allocated row"""
    return [rows] * B if frames is None else [halve(int(f), n) for f in frames]


def conv1_ref(x, sd, block, frames, dtype, prec=torch.float64, with_S=False):
    """relu(bn1(conv1(x))) before the output rounding.  x (B, H_in, W_in, C_in).  Zero padding at each utterance's own last row."""
    g = Geom(block)
    w = _w(sd, g.prefix + ".conv1.weight", dtype).to(prec)
    sc, sh = (t.to(prec)[None, :, None, None] for t in fold_bn(sd, g.prefix + ".bn1"))
    B, hin = x.shape[0], x.shape[1]
    hout = halve(hin, 1) if g.stride == 2 else hin
    out = torch.zeros(B, hout, g.wout, g.c, dtype=prec)
    S = torch.zeros_like(out) if with_S else None
    for b, n in enumerate(_frames(frames, B, hin, g.lin)):
        xb = _nchw(x[b, :n], prec)
        r = _nhwc(F.relu(F.conv2d(xb, w, stride=g.stride, padding=1) * sc + sh))
        out[b, :r.shape[0]] = r
        if with_S:
            S[b, :r.shape[0]] = _nhwc(F.conv2d(xb.abs(), w.abs(), stride=g.stride, padding=1) * sc.abs() + sh.abs())
    return (out, S) if with_S else out


def gate_ref(o1, sd, block, frames, dtype, prec=torch.float64):
    """The SE gate (B, C) from the stored o1 (B, H_out, W_out, C): plane mean of bn2(conv2(o1)) over the utterance's valid rows,
    fc.0, ReLU, fc.2, sigmoid.  The convolution is evaluated at every position; nothing is derived from border sums."""
    g = Geom(block)
    w = _w(sd, g.prefix + ".conv2.weight", dtype).to(prec)
    sc, sh = (t.to(prec) for t in fold_bn(sd, g.prefix + ".bn2"))
    fc0, fc2 = sd[g.prefix + ".se.fc.0.weight"].to(prec), sd[g.prefix + ".se.fc.2.weight"].to(prec)
    B, hout = o1.shape[0], o1.shape[1]
    gate = torch.zeros(B, g.c, dtype=prec)
    for b, n in enumerate(_frames(frames, B, hout, g.li)):
        y = F.conv2d(_nchw(o1[b, :n], prec), w, padding=1).mean(dim=(2, 3))[0] * sc + sh
        gate[b] = torch.sigmoid(fc2 @ F.relu(fc0 @ y))
    return gate


def conv2_ref(o1, gate, x, sd, block, frames, dtype, prec=torch.float64, with_S=False):
    """The block output before its rounding, and z (see the module docstring).  o1 (B, H_out, W_out, C) and gate (B, C) are what the
    kernel reads (its own upstream outputs), x (B, H_in, W_in, C_in) the block input.  Returns (out, z) or (out, z, S)."""
    g = Geom(block)
    w = _w(sd, g.prefix + ".conv2.weight", dtype).to(prec)
    sc2, sh2 = fold_bn(sd, g.prefix + ".bn2")
    if g.first:
        scs, shs = fold_bn(sd, g.prefix + ".shortcut.1")
        wf = sd[g.prefix + ".shortcut.0.weight"].float() * scs[:, None, None, None]       # finalize_half: w * scale_s[co] in float32
        wf = (bf16r(wf) if dtype == "bf16" else wf).to(prec)
    B, hout = o1.shape[0], o1.shape[1]
    out = torch.zeros(B, hout, g.wout, g.c, dtype=prec)
    z = torch.zeros_like(out)
    S = torch.zeros_like(out) if with_S else None
    gate32 = gate.float()
    for b, n in enumerate(_frames(frames, B, hout, g.li)):
        ob = _nchw(o1[b, :n], prec)
        k1 = (sc2 * gate32[b]).to(prec)[None, :, None, None]                                  # float32 products, as the epilogue forms them
        k0 = sh2 * gate32[b]
        acc = F.conv2d(ob, w, padding=1)
        if g.first:
            nin = halve(int(frames[b]), g.lin) if frames is not None else x.shape[1]
            xb = _nchw(x[b, :nin], prec)
            k0 = (k0 + shs).to(prec)[None, :, None, None]
            zb = k1 * acc + F.conv2d(xb, wf, stride=g.stride) + k0
            rb = F.relu(zb)
            if with_S:
                S[b, :n] = _nhwc(k1.abs() * F.conv2d(ob.abs(), w.abs(), padding=1) + F.conv2d(xb.abs(), wf.abs(), stride=g.stride) + k0.abs())
        else:
            k0 = k0.to(prec)[None, :, None, None]
            xb = _nchw(x[b, :n], prec)
            zb = k1 * acc + k0
            if dtype == "bf16":
                zb = bf16r(zb)                                                                # the gated tile in LDS, before the shortcut add
            rb = F.relu(zb + xb)
            if with_S:
                S[b, :n] = _nhwc(k1.abs() * F.conv2d(ob.abs(), w.abs(), padding=1) + k0.abs() + xb.abs())
        out[b, :n], z[b, :n] = _nhwc(rb), _nhwc(zb)
    return (out, z, S) if with_S else (out, z)


def stem_ref(feats, sd, frames, prec=torch.float64, with_S=False):
    """relu(shift + sum w' x) of the stem on features (B, 80, T), w' = f32(w * scale) as finalize_half folds it.  Returns (B, T, 80, 32)."""
    sc, sh = fold_bn(sd, "sequence_network.bn1")
    w = (sd["sequence_network.conv1.weight"].float() * sc[:, None, None, None]).to(prec)
    sh = sh.to(prec)[None, :, None, None]
    B, _, T = feats.shape
    out = torch.zeros(B, T, 80, 32, dtype=prec)
    S = torch.zeros_like(out) if with_S else None
    for b, n in enumerate(_frames(frames, B, T, 0)):
        xb = feats[b, :, :n].to(prec).T[None, None]                                           # (1, 1, T, 80)
        out[b, :n] = _nhwc(F.relu(F.conv2d(xb, w, padding=1) + sh))
        if with_S:
            S[b, :n] = _nhwc(F.conv2d(xb.abs(), w.abs(), padding=1) + sh.abs())
    return (out, S) if with_S else out


# ---- the operands of the block tests (tests/test_gpu_trunk_blocks.py and the CPU flip-share test use the same ones) ---------------------
def operand_state_dict(seed=20):
    """seeded_state_dict with every BatchNorm moved well away from identity: scales 0.5 .. 1.5, a tenth of them negative, shifts and
    running means of +- 0.3, variances 0.5 .. 2."""
    from sidekit_amd.nnet.weights import seeded_state_dict
    sd = seeded_state_dict("halfresnet34", 16, seed=seed)
    rs = numpy.random.RandomState(seed + 1)
    for k in list(sd):
        if not k.startswith("sequence_network.") or sd[k].dim() != 1:
            continue
        n = sd[k].numel()
        if k.endswith("running_var"):
            a = rs.uniform(0.5, 2.0, n)
        elif k.endswith("running_mean") or k.endswith(".bias"):
            a = rs.standard_normal(n) * 0.3
        elif k.endswith(".weight"):
            a = rs.uniform(0.5, 1.5, n) * numpy.where(rs.uniform(size=n) < 0.1, -1.0, 1.0)
        else:
            continue
        sd[k] = torch.from_numpy(a.astype(numpy.float32))
    return sd


def ragged_rows(block, dtype):
    """output rows of the ragged batch of a block: 1, 2 (first row = last row, coinciding corners), and both sides of its row tile"""
    th = Geom(block).tile(dtype)
    return [1, 2, th - 1, th + 1, 2 * th + 1]


def frames_for_rows(block, rows):
    """feature frames that give each utterance `rows` output rows; for a stride-2 first block the input rows alternate even / odd"""
    g = Geom(block)
    out = []
    for i, r in enumerate(rows):
        rin = r if g.stride == 1 else (2 * r if i % 2 == 0 else 2 * r - 1)
        out.append(rin << g.lin)
    return out


def block_input(block, frames, dtype, seed):
    """random block input of both signs (B, H_in, W_in, C_in) float32, pre-rounded to bf16 for the bf16 path; rows past an utterance's length are zero"""
    g = Geom(block)
    gen = torch.Generator().manual_seed(seed * 100 + block)
    hin = max(g.rows_in(f) for f in frames)
    x = 0.7 * torch.randn(len(frames), hin, g.win, g.cin, generator=gen)
    for b, f in enumerate(frames):
        x[b, g.rows_in(f):] = 0.0
    return bf16r(x) if dtype == "bf16" else x
