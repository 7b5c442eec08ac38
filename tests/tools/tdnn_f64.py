"""Float64 reference of the TDNN x-vector path (model_archi='xvector') one kernel at a time, on the kernels' actual operands (CPU only;
torch + numpy), and the criteria the GPU tests judge the kernels by.

Written from csrc/gemm.hip (load_a: the dilated-conv operand walk k = tap * cin + c, row = m + tap * dil, zeros only from row >= a_rows;
gemm_epilogue: bias, LeakyReLU(0.2), then scale and shift), csrc/pool.hip (mean_std_kernel, l2norm_kernel), the folding and the launches in
csrc/xt_api.hip (fold_bn / finalize_tdnn / tdnn_from_rows / tail) and oracle/xvector.py.  Each function takes what ONE kernel reads and
returns what it computes:

    layer_ref(i, x_rows)        conv{i} + bias, LeakyReLU(0.2), BatchNorm of layer i = 1..5 on the rows [R][cin] the kernel reads
    mean_std_ref(conv5_rows)    mean | unbiased std over the first frames_b - 14 rows of each utterance            -> [B][3072]
    embedding_ref(pooled)       linear6 + bias                                                                      -> [B][E]
    normalise_ref(pre_norm)     l2_norm, then F.normalize(eps = 1e-12)                                              -> [B][E]
    logits_ref(emb)             s * emb . head rows normalised as the library normalises them on the host          -> [B][n_spk]

Rows are the ragged layout of the library: the utterances' frames one after the other, [R][C] with R = sum(frames), no padding between
them.  A layer's window of an utterance's last rows therefore reads into the NEXT utterance (and zeros past the batch's last row); the
rows whose whole window lies inside their own utterance are the first frames_b - c_i of each (c_i = 4, 8, 14, 14, 14: own()).  Only those
are judged, and each layer's own rows read only own rows of the layer before.

``prec`` is the arithmetic the formulas are evaluated in: float64 for the reference, float32 for "what torch's own float32 gives on the
same operands" (the yardstick of the norm-relative criteria).  BatchNorm constants are folded in float32 exactly as the library folds
them, and the head rows are normalised as the library does it: they are operands, not arithmetic under test.  ``S`` is the same formula
on absolute values, the scale of the rigorous float32 bound 2 K 2^-24 S of a sum of K terms in any order.
"""
import numpy
import torch
import torch.nn.functional as F

LAYERS = ((80, 512, 5, 1), (512, 512, 3, 2), (512, 512, 3, 3), (512, 512, 1, 1), (512, 1536, 1, 1))      # cin, cout, taps, dilation
SHRINK = (4, 8, 14, 14, 14)              # frames an utterance has lost after layer i
N_SPK = 130                              # speakers of the test models: more than one 128-column tile, no multiple of 64
AAM_S = 64.0                             # Xtractor('xvector'): s of the cosine head
U32 = 2.0 ** -24
FOLD = torch.float32                     # precision the host-side folding runs in; the library's is float32 (the oracle comparison switches it to float64)
CASE1_FRAMES = [15, 16, 17, 18, 19, 21, 22, 23, 29, 47, 64, 65]     # pooled counts 1, 2, 3, 4, 5, 7, 8, 9, 15, 33, 50, 51; R = 356


# ---- layout ---------------------------------------------------------------------------------------------------------------------------
def offsets(frames):
    return numpy.concatenate(([0], numpy.cumsum(frames))).astype(int).tolist()


def own(i, frames, extra=0):
    """bool [R]: the rows of layer i's output whose whole window lies inside their own utterance (``extra``: that many rows more, for the
    mutation check only)"""
    off = offsets(frames)
    m = torch.zeros(off[-1], dtype=torch.bool)
    for b, f in enumerate(frames):
        m[off[b]:off[b] + max(int(f) - SHRINK[i - 1] + extra, 0)] = True
    return m


def rows_of(feats, frames):
    """(B, 80, T) features -> the [R][80] rows the first layer reads (what bft_to_rows_kernel leaves)"""
    return torch.cat([feats[b, :, :int(f)].T for b, f in enumerate(frames)]).contiguous()


def unfold(x_rows, k, dil):
    """[R][cin] -> [R][k cin]: row m holds rows m, m + dil, .. of x, tap-major as load_a walks them; zeros from row R on"""
    R, cin = x_rows.shape
    xp = torch.cat([x_rows, torch.zeros((k - 1) * dil, cin, dtype=x_rows.dtype)])
    return torch.cat([xp[j * dil:j * dil + R] for j in range(k)], dim=1)


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def fold_bn(sd, p):
    """eval-mode BatchNorm as (scale, shift) in float32, operation by operation as fold_bn of csrc/xt_api.hip"""
    g, b, m, v = (sd[f"{p}.{k}"].to(FOLD) for k in ("weight", "bias", "running_mean", "running_var"))
    s = g / torch.sqrt(v + torch.tensor(1e-5, dtype=FOLD))
    return s, b - m * s


def layer_operands(i, sd):
    """(w [cout][k cin] in the [cout][k][cin] order of finalize_tdnn, bias, scale, shift) of layer i"""
    cin, cout, k, _ = LAYERS[i - 1]
    w = sd[f"sequence_network.conv{i}.weight"].float().permute(0, 2, 1).reshape(cout, k * cin).contiguous()
    sc, sh = fold_bn(sd, f"sequence_network.batch_norm{i}")
    return w, sd[f"sequence_network.conv{i}.bias"].float(), sc, sh


def head_rows(sd):
    """after_speaker_embedding.weight with every row divided by max(f32(its float64 norm), 1e-12): normalize_rows of csrc/xt_api.hip"""
    w = sd["after_speaker_embedding.weight"].to(FOLD)
    n = torch.sqrt((w.double() ** 2).sum(1)).to(FOLD).clamp_min(1e-12)
    return w / n[:, None]


def operand_state_dict(embedding_size=256, loss="aam", seed=30):
    """seeded_state_dict('xvector') with every BatchNorm far from identity: |weight| log-uniform in 0.3 .. 3 with a third of the channels
    negative, variances log-uniform in 0.3 .. 3, shifts and running means of +- 0.5, conv and linear biases of +- 0.3.  A dropped bias, a
    swapped scale and shift, or BatchNorm applied before the LeakyReLU is then of the order of the values themselves."""
    from sidekit_amd.nnet.weights import seeded_state_dict
    sd = seeded_state_dict("xvector", N_SPK, embedding_size, loss, seed)
    rs = numpy.random.RandomState(seed + 1)
    for k in list(sd):
        if sd[k].dim() != 1 or k.startswith("preprocessor."):
            continue
        n = sd[k].numel()
        if k.endswith("running_var"):
            a = numpy.exp(rs.uniform(numpy.log(0.3), numpy.log(3.0), n))
        elif k.endswith("running_mean"):
            a = rs.standard_normal(n) * 0.5
        elif ".batch_norm" in k and k.endswith(".weight"):
            a = numpy.exp(rs.uniform(numpy.log(0.3), numpy.log(3.0), n)) * numpy.where(rs.uniform(size=n) < 1.0 / 3, -1.0, 1.0)
        elif ".batch_norm" in k and k.endswith(".bias"):
            a = rs.standard_normal(n) * 0.5
        elif k.endswith(".bias"):
            a = rs.standard_normal(n) * 0.3
        else:
            continue
        sd[k] = torch.from_numpy(a.astype(numpy.float32))
    return sd


def features(frames, seed):
    """(B, 80, T) float32 features of both signs, channel 7 about 30 times the others (S is then far from uniform over the taps); columns
    past an utterance's length hold 1e30: they are never read"""
    T = max(frames)
    x = torch.randn(len(frames), 80, T, generator=torch.Generator().manual_seed(seed))
    x[:, 7] *= 30.0
    for b, f in enumerate(frames):
        x[b, :, int(f):] = 1e30
    return x


def tile_switch_frames(R):
    """the case-1 utterances five times over plus one utterance that completes R rows"""
    base = CASE1_FRAMES * 5
    last = R - sum(base)
    assert last >= 15
    return base + [last]


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------
def layer_ref(i, x_rows, frames, sd, prec=torch.float64, with_S=False):
    """Layer i (1..5) on its input rows [R][cin] as the kernel reads them (layer 1: the features as rows, later layers: the kernel's own tap
    conv{i-1}): v = sum_k w x + bias; v = leaky_relu(v, 0.2); v = v scale + shift.  Returns ([R][cout], own [R]) or (.., own, S)."""
    _, _, k, dil = LAYERS[i - 1]
    w, bias, sc, sh = (t.to(prec) for t in layer_operands(i, sd))
    A = unfold(x_rows.to(prec), k, dil)
    out = F.leaky_relu(A @ w.T + bias, 0.2) * sc + sh
    if not with_S:
        return out, own(i, frames)
    S = (A.abs() @ w.abs().T + bias.abs()) * sc.abs() + sh.abs()
    return out, own(i, frames), S


def mean_std_ref(conv5_rows, frames, prec=torch.float64, shrink=14):
    """[B][3072]: mean | unbiased std over the first frames_b - 14 rows of each utterance; one row gives a NaN std, as the reference's
    torch.std does"""
    off = offsets(frames)
    out = torch.zeros(len(frames), 2 * conv5_rows.shape[1], dtype=prec)
    D = conv5_rows.shape[1]
    for b, f in enumerate(frames):
        x = conv5_rows[off[b]:off[b] + int(f) - shrink].to(prec)
        out[b, :D] = x.mean(0)
        out[b, D:] = x.std(0) if x.shape[0] > 1 else float("nan")
    return out


def embedding_ref(pooled, sd, prec=torch.float64, with_S=False):
    """linear6 + bias on the pooled rows [B][3072]"""
    w, b = sd["before_speaker_embedding.linear6.weight"].to(prec), sd["before_speaker_embedding.linear6.bias"].to(prec)
    x = pooled.to(prec)
    out = x @ w.T + b
    return (out, x.abs() @ w.abs().T + b.abs()) if with_S else out


def half_embedding_ref(pooled, sd, prec=torch.float64, with_S=False):
    """HalfResNet34: lin_be (no bias) followed by bn_be folded in float32, on the pooled rows [B][5120] as the library holds them: both
    halves in the trunk's NHWC order d' = f 256 + c, where the reference's is d = 10 c + f (finalize_half permutes the weights once)"""
    dp = torch.arange(2560)
    d = (dp % 256) * 10 + dp // 256
    w = sd["before_speaker_embedding.lin_be.weight"][:, torch.cat([d, 2560 + d])].to(prec)
    sc, sh = (t.to(prec) for t in fold_bn(sd, "before_speaker_embedding.bn_be"))
    x = pooled.to(prec)
    out = (x @ w.T) * sc + sh
    return (out, (x.abs() @ w.abs().T) * sc.abs() + sh.abs()) if with_S else out


def normalise_ref(pre_norm, prec=torch.float64, twice=True):
    """l2_norm (no eps) followed by F.normalize(eps = 1e-12)"""
    x = pre_norm.to(prec)
    x = x / torch.norm(x, 2, 1, True)
    return F.normalize(x, dim=1, eps=1e-12) if twice else x


def logits_ref(emb, sd, s=AAM_S, prec=torch.float64, with_S=False):
    """s * emb . head_rows: the cosine head on the x-vectors the library stores"""
    w, x = head_rows(sd).to(prec), emb.to(prec)
    out = (x @ w.T) * s
    return (out, (x.abs() @ w.abs().T) * s) if with_S else out


# ---- criteria (float32 rules of tests/test_gpu_trunk_blocks.py, u = 2^-24) -----------------------------------------------------------------
def check_gemm(name, got, r, S, K, rows, r32):
    """A GEMM stage on the rows ``rows`` (bool [R] or None): the NaN pattern of the reference, |got - r| <= 2 K u S per element (K: the
    accumulated terms + 4 for bias, slope, scale and shift, + the slices of a sliced sum) and a norm-relative error of at most 16 x that
    of torch's float32 evaluation r32.  Returns (kernel's norm-relative error, torch's, largest |got - r| / (2 K u S))."""
    if rows is not None:
        got, r, S, r32 = got[rows], r[rows], S[rows], r32[rows]
    got, r32 = got.double(), r32.double()
    nan = torch.isnan(r)
    assert torch.equal(torch.isnan(got), nan), f"{name}: NaN pattern differs from the float64 reference"
    got, r, S, r32 = got[~nan], r[~nan], S[~nan], r32[~nan]
    assert got.numel() > 0, f"{name}: nothing to judge"
    ratio = (got - r).abs() / (2 * K * U32 * S)
    bad = ~(ratio <= 1)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements outside 2 K 2^-24 S (K = {K}); first: got {got[i].item()!r}, "
                             f"float64 {r[i].item()!r}, bound {(2 * K * U32 * S[i]).item():.3e}")
    err, err32 = ((got - r).norm() / r.norm()).item(), ((r32 - r).norm() / r.norm()).item()
    assert err <= 16 * err32, f"{name}: norm-relative error {err:.2e} against float64, torch's float32 evaluation {err32:.2e} (x 16 allowed)"
    return err, err32, ratio.max().item()


def check_mean(name, got, r, conv5_rows, frames, shrink=14):
    """|got - r| <= (n + 2) u mean|x| per element over the utterance's n rows: rigorous for any order of the n additions and the division.
    got, r: [B][>= D], the means in the first D columns.  Returns the largest error as a share of its bound."""
    off, D, worst = offsets(frames), conv5_rows.shape[1], 0.0
    for b, f in enumerate(frames):
        n = int(f) - shrink
        bound = (n + 2) * U32 * conv5_rows[off[b]:off[b] + n].double().abs().mean(0)
        diff = (got[b, :D].double() - r[b, :D]).abs()
        ratio = torch.where(bound > 0, diff / bound, diff / U32)       # a column of zeros (after a ReLU): the mean is exactly zero
        assert bool((diff <= bound).all()), f"{name}: utterance {b} ({n} rows): mean off by {ratio.max().item():.2f} of (n + 2) 2^-24 mean|x|"
        worst = max(worst, ratio.max().item())
    return worst


def std_errors(got, r):
    """norm-relative error of each utterance's std row (the last D columns) against float64; NaN rows (one pooled row) must be NaN in all columns"""
    D = r.shape[1] // 2
    out = []
    for b in range(r.shape[0]):
        g, x = got[b, D:].double(), r[b, D:]
        if bool(torch.isnan(x).all()):
            assert bool(torch.isnan(g).all()), f"utterance {b}: the std of one row is NaN in the reference, not in all columns here"
            continue
        assert not bool(torch.isnan(g).any()), f"utterance {b}: NaN std"
        out.append(((g - x).norm() / x.norm()).item())
    return out


def check_std(name, got, r, yardstick):
    """every utterance's std row within 8 x ``yardstick`` (the largest norm-relative error of torch's float32 std over the module's cases)
    of the float64 one.  Returns the largest error."""
    errs = std_errors(got, r)
    worst = max(errs)
    assert worst <= 8 * yardstick, f"{name}: std norm-relative error {worst:.2e}, torch's float32 std at most {yardstick:.2e} (x 8 allowed)"
    return worst


def check_normalise(name, got, r):
    """|got - r| <= (N + 8) u |r| per element: a sum of N squares in any order, a square root and two divisions, applied twice.  Rows that
    are NaN in the reference are NaN here.  Returns the largest error as a share of its bound."""
    got = got.double()
    nan = torch.isnan(r)
    assert torch.equal(torch.isnan(got), nan), f"{name}: NaN pattern differs from the float64 reference"
    ratio = ((got - r).abs() / ((r.shape[1] + 8) * U32 * r.abs()))[~nan]
    assert bool((ratio <= 1).all()), f"{name}: off by {ratio.max().item():.2f} of (N + 8) 2^-24 |r|"
    return ratio.max().item()
