"""Float64 reference of what turns HalfResNet34's layer-4 output into ``att_h`` (half_from_feats of csrc/xt_api.hip: the global context,
the context GEMM and attention.0), one kernel at a time on the kernels' actual operands (CPU only; torch + numpy), the criteria the GPU
tests judge the kernels by, and the batches both test modules use.

Written from csrc/pool.hip (mean_std_kernel with RowSpan{nullptr, H4, lens, 3, 0}: utterance b's rows start at row b H4 and number
halve(frames_b, 3)), csrc/gemm.hip (launch_gemm, gemm_epilogue: bias, row bias of row group m / rows_per_group, then
tanh(relu(v) scale + shift)), finalize_half of csrc/xt_api.hip (the permutation of attention.0's columns, the bf16 copy of its x part
by f32_to_bf16: round to nearest, ties to even) and oracle/xvector.py (attentive_pooling).  Each function takes what ONE kernel reads and
returns what it computes:

    ctx_ref(layer4, frames)                  mean | unbiased std over an utterance's own rows                         -> [B][5120]
    rowbias_ref(ctx, sd)                     ctx . W1c' + b1                                                         -> [B][128]
    att_h_ref(layer4, att_rb, sd, dtype)     tanh(relu(x . W1x' + att_rb[m // H4]) scale + shift)                    -> [B H4][128]

Layer-4 rows are [B][H4][2560], the trunk's NHWC rows with columns d' = f 256 + c (the reference's channel is d = 10 c + f: the weights
are permuted once, as finalize_half does); H4 = halve(T, 3) is the fixed row stride of an utterance and only its first
halve(frames_b, 3) rows are its own: the rows after them hold whatever the workspace held, and only own rows are judged.  bf16 layer-4
values widen exactly.  ``dtype`` is the compute type: 'bf16' rounds attention.0's x columns to bf16, 'fp32' rounds nothing.  ``prec`` is
the arithmetic the formulas are evaluated in: float64 for the reference, float32 for "what torch's own float32 gives on the same
operands" (the yardstick of the norm-relative criteria).  BatchNorm is folded in float32 as the library folds it (tdnn_f64.FOLD).

Criteria (u = 2^-24; the constants are those of tdnn_f64):

  mean   |got - r| <= (n + 2) u mean|x| per element over the utterance's n own rows (check_mean).
  std    norm-relative over an utterance's 2560 columns at most 8 x the largest such error of torch's float32 std over the module's
         cases; NaN in all 2560 columns for a one-row utterance (check_std).
  att_rb |got - r| <= 2 (K + 4 + slices) u S, K = 5120 in 20 slices, S = sum |a||w| + |b1|; norm-relative at most 16 x torch's float32
         evaluation; NaN exactly where r has it (check_gemm).
  att_h  |got - r| <= |scale_n| delta_pre + 8 u with delta_pre = 2 (K + 4 + slices) u S_pre, K = 2560, S_pre = sum |x||w| + |att_rb|,
         8 slices on the bf16 path and none on the fp32 path; norm-relative over the judged rows at most 16 x torch's float32
         evaluation; NaN exactly where r has it.
         Why: delta_pre is the rigorous float32 bound of the sum ``pre`` in any order.  ReLU and tanh are 1-Lipschitz, so an error of
         pre reaches the result at most times |scale_n|.  The float32 rounding of y = relu(pre) scale + shift moves y by at most u |y|
         and the result by at most u |y| sech^2(y) < 0.45 u.  tanhf is within a few ulp of a value of at most 1, a few times u.  8 u
         covers the last two.
"""
import os
import re

import numpy
import torch

import tdnn_f64 as tf
from trunk_f64 import bf16r, halve

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
D, NA = 2560, 128                       # layer-4 columns (10 x 256), attention channels
N_SPK = 16
U32 = tf.U32
K_CTX, SLICES_CTX = 2 * D, 20           # context GEMM: 160 k-tiles of 32, eight per slice (launch_gemm)
K_X, SLICES_X = D, {"bf16": 8, "fp32": 0}   # attention.0: 40 k-tiles of 64 in eight slices on the bf16 matrix cores; one chain in fp32

# what the shapes below rest on (read_sources() reads them out of the sources; tests/test_tail_reference_cpu.py compares)
SPLIT_ROWS = 512                        # launch_gemm: K slices side by side up to this many rows, inside the workgroup above
BIG_ROWS = 2048                         # launch_gemm: 128 x 128 tiles from this many float32 rows
TILE_BF16, TILE_F32, TILE_BIG = 32, 64, 128     # BMH, BM, BM2
POOL_TG = 4                             # mean_std_kernel: row groups of a workgroup

S_ROWS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 33]
S_FRAMES = [5, 16, 19, 31, 34, 54, 57, 68, 117, 259]    # odd and even counts before each of the three halvings
M_EXTRA = [264, 263, 262, 261, 260, 258]                # six more utterances of 33 rows
L_EXTRA = [264, 257, 262]                               # three more
W_CLIPS, W_FRAMES = 513, 16


def read_sources():
    """The thresholds as the sources state them today."""
    def text(name):
        with open(os.path.join(ROOT, "sidekit_amd", "csrc", name)) as f:
            return f.read()

    def one(pattern, src, count):
        found = re.findall(pattern, src)
        assert len(found) == count and len(set(found)) == 1, f"{pattern!r}: expected {count} equal matches, found {found}"
        return int(found[0])

    gemm, pool = text("gemm.hip"), text("pool.hip")
    bm, bm2 = re.search(r"constexpr int BM = (\d+),", gemm), re.search(r"constexpr int BM2 = (\d+),", gemm)
    return {"SPLIT_ROWS": one(r"g\.M <= (\d+)", gemm, 2),                        # the bf16 form and the float32 form
            "BIG_ROWS": one(r"g\.ksplit == 1 && g\.M >= (\d+) && g\.N >= 128 && !g\.a_bf16", gemm, 1),
            "TILE_BF16": one(r"BMH = (\d+);", gemm, 1), "TILE_F32": int(bm.group(1)), "TILE_BIG": int(bm2.group(1)),
            "POOL_TG": one(r"constexpr int POOL_TG = (\d+),", pool, 1)}


# ---- the batches ----------------------------------------------------------------------------------------------------------------------
def rows_out(frames):
    """layer-4 rows an utterance of ``frames`` feature frames owns"""
    return halve(int(frames), 3)


def batch_frames(name):
    """feature frames per utterance of batch S, M or L, and the index of each utterance's features (utterance())"""
    if name == "S":
        return list(S_FRAMES), list(range(10))
    if name == "M":
        return S_FRAMES + M_EXTRA, list(range(16))
    if name == "L":
        return S_FRAMES * 6 + L_EXTRA, list(range(10)) * 6 + [16, 17, 18]
    raise KeyError(name)


def utterance(i, frames, seed=40):
    """(80, frames) float32 features of both signs; every utterance has its own offset (-1.5 .. 1.5) and scale (0.5 .. 2), so that the
    global context, and with it the row bias, differs between neighbours by far more than any bound here"""
    g = torch.Generator().manual_seed(seed * 1000 + i)
    c = torch.rand(2, generator=g)
    return torch.randn(80, frames, generator=g) * (0.5 + 1.5 * c[0]) + (3.0 * c[1] - 1.5)


def features(name, junk=1e30):
    """(feats (B, 80, T), frames) of batch S, M, L (ragged: the columns past an utterance's length hold ``junk``, never read) or W (513
    clips of 16 frames, frames = None)"""
    if name == "W":
        return torch.stack([utterance(100 + i, W_FRAMES) for i in range(W_CLIPS)]), None
    frames, idx = batch_frames(name)
    x = torch.full((len(frames), 80, max(frames)), junk)
    made = {}
    for b, (i, f) in enumerate(zip(idx, frames)):
        if i not in made:
            made[i] = utterance(i, f)
        x[b, :, :f] = made[i]
    return x, frames


def layer4_rows(raw, B, dtype):
    """the bytes of the 'layer4' tap -> [B][H4][2560] float32 (bf16 widens exactly)"""
    if dtype == "bf16":
        a = torch.from_numpy((raw.view(numpy.uint16).astype(numpy.uint32) << 16).view(numpy.float32).copy())
    else:
        a = torch.from_numpy(raw.view(numpy.float32).copy())
    return a.reshape(B, -1, D)


def counts(l4, frames):
    return [l4.shape[1]] * l4.shape[0] if frames is None else [rows_out(f) for f in frames]


def own(l4, frames):
    """bool [B H4]: the rows an utterance owns"""
    B, H4 = l4.shape[:2]
    m = torch.zeros(B, H4, dtype=torch.bool)
    for b, n in enumerate(counts(l4, frames)):
        m[b, :n] = True
    return m.reshape(-1)


def own_rows(l4, frames):
    """the own rows one utterance after the other, [sum n][2560]: the ragged layout of tdnn_f64's pooling helpers"""
    return l4.reshape(-1, D)[own(l4, frames)]


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def operand_state_dict(seed=40):
    """seeded_state_dict('halfresnet34') with the pooling's BatchNorm far from identity and its biases of the order of the sums: the rule
    of tdnn_f64.operand_state_dict on the 1-D tensors of stat_pooling; attention.0's weight scaled so that the tanh is not saturated"""
    from sidekit_amd.nnet.weights import seeded_state_dict
    sd = seeded_state_dict("halfresnet34", N_SPK, seed=seed)
    rs = numpy.random.RandomState(seed + 1)
    for k in list(sd):
        if sd[k].dim() != 1 or not k.startswith("stat_pooling."):
            continue
        n = sd[k].numel()
        if k.endswith("running_var"):
            a = numpy.exp(rs.uniform(numpy.log(0.3), numpy.log(3.0), n))
        elif k.endswith("running_mean"):
            a = rs.standard_normal(n) * 0.5
        elif k.endswith("attention.2.weight"):
            a = numpy.exp(rs.uniform(numpy.log(0.3), numpy.log(3.0), n)) * numpy.where(rs.uniform(size=n) < 1.0 / 3, -1.0, 1.0)
        elif k.endswith("attention.2.bias"):
            a = rs.standard_normal(n) * 0.5
        elif k.endswith(".bias"):
            a = rs.standard_normal(n) * 0.3
        else:
            continue
        sd[k] = torch.from_numpy(a.astype(numpy.float32))
    # the seeded trunk's layer-4 rows are of the order of 50 and attention.0's sums of the order of 80: every tanh would sit at +- 1, where
    # no error shows.  Powers of two (exact) bring x . W1x' to about 0.6 and the context term to about 1.
    w = sd["stat_pooling.attention.0.weight"]
    w[:, :D] *= 2.0 ** -7
    w[:, D:] *= 2.0 ** -6
    return sd


def operands(sd, dtype):
    """(W1x [128][2560], W1c [128][5120] = [mean | std] columns, b1, scale, shift) as the library holds them: columns in the d' order,
    W1x rounded to bf16 on the bf16 path, BatchNorm folded in float32"""
    w1 = sd["stat_pooling.attention.0.weight"].float().cpu().reshape(NA, 3 * D)
    dp = torch.arange(D)
    d = (dp % 256) * 10 + dp // 256
    w1x = w1[:, d]
    sc, sh = tf.fold_bn(sd, "stat_pooling.attention.2")
    return (bf16r(w1x) if dtype == "bf16" else w1x).contiguous(), torch.cat([w1[:, D + d], w1[:, 2 * D + d]], 1).contiguous(), \
        sd["stat_pooling.attention.0.bias"].float().cpu(), sc, sh


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------
def ctx_ref(l4, frames, prec=torch.float64):
    """[B][5120]: mean | unbiased std over each utterance's own rows; one row gives a NaN std, as the reference's torch.std does"""
    return tf.mean_std_ref(own_rows(l4, frames), counts(l4, frames), prec, shrink=0)


def rowbias_ref(ctx, sd, prec=torch.float64, with_S=False):
    """the context term of attention.0, once per utterance: ctx . W1c' + b1"""
    _, w, b1, _, _ = (t.to(prec) for t in operands(sd, "fp32"))
    x = ctx.to(prec)
    out = x @ w.T + b1
    return (out, x.abs() @ w.abs().T + b1.abs()) if with_S else out


def att_h_ref(l4, att_rb, sd, dtype, prec=torch.float64, with_S=False):
    """attention.0 on every row m of the padded layout with the row bias of utterance m // H4, ReLU, BatchNorm, tanh.  Returns [B H4][128]
    or (.., S_pre [B H4][128])"""
    w, _, _, sc, sh = (t.to(prec) for t in operands(sd, dtype))
    B, H4 = l4.shape[:2]
    x = l4.reshape(B * H4, D).to(prec)
    rb = att_rb.to(prec)[torch.arange(B * H4) // H4]
    out = torch.tanh(torch.relu(x @ w.T + rb) * sc + sh)
    return (out, x.abs() @ w.abs().T + rb.abs()) if with_S else out


# ---- criteria -------------------------------------------------------------------------------------------------------------------------
def std_yardstick(cases):
    """the largest norm-relative error of torch's float32 std against float64 over ``cases`` = [(layer-4 rows, frames)]"""
    return max(max(tf.std_errors(ctx_ref(l4, fr, torch.float32), ctx_ref(l4, fr))) for l4, fr in cases)


def check_ctx(name, got, l4, frames, yard):
    """the ctx tap against ctx_ref(layer-4 rows).  Returns (largest mean error as a share of its bound, largest std error)"""
    r = ctx_ref(l4, frames)
    n = counts(l4, frames)
    return tf.check_mean(name, got, r, own_rows(l4, frames), n, shrink=0), tf.check_std(name, got, r, yard)


def check_rowbias(name, got, ctx, sd):
    """the att_rb tap against rowbias_ref(the ctx tap).  Returns check_gemm's (error, torch's, worst share of the element bound)"""
    r, S = rowbias_ref(ctx, sd, with_S=True)
    return tf.check_gemm(name, got, r, S, K_CTX + 4 + SLICES_CTX, None, rowbias_ref(ctx, sd, torch.float32))


def check_att_h(name, got, l4, att_rb, sd, dtype, frames):
    """the att_h tap against att_h_ref(layer-4 rows, the att_rb tap) on the own rows.  check_gemm's 2 K u S with
    S = |scale_n| S_pre + 4 / K is |scale_n| 2 K u S_pre + 8 u, K = 2560 + 4 + slices."""
    K = K_X + 4 + SLICES_X[dtype]
    r, S_pre = att_h_ref(l4, att_rb, sd, dtype, with_S=True)
    sc = operands(sd, dtype)[3].double()
    return tf.check_gemm(name, got, r, sc.abs() * S_pre + 4.0 / K, K, own(l4, frames), att_h_ref(l4, att_rb, sd, dtype, torch.float32))
