"""The float64 reference of HalfResNet34's attention front (tests/tools/tail_f64.py: global context, context GEMM, attention.0) without
a GPU: the thresholds the GPU batches rest on read out of the sources, the reference pinned to the oracle's pooling in float64, and its
criteria shown to reject wrong kernels on the very operands tests/test_gpu_tail_kernels.py uses (same state dict, same features; the
layer-4 rows come from torch's float32 trunk on the CPU instead of the library's)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import tail_f64 as tl  # noqa: E402
import tdnn_f64 as tf  # noqa: E402
from test_gpu_halfresnet import _pooling_in_float64  # noqa: E402

from oracle import xvector as oxv  # noqa: E402

F32 = torch.float32
D = tl.D


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def sd():
    return tl.operand_state_dict()


@pytest.fixture(scope="module")
def trunk(sd):
    """batch M (its first ten utterances are batch S) through the oracle's float32 trunk, every utterance alone: the oracle's layer-4
    tensors (1, 256, T', 10) and the padded rows [16][33][2560] the kernels would read, |N(0, 1)| in the rows past an utterance's own"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    feats, frames = tl.features("M")
    H4 = tl.rows_out(max(frames))
    l4 = torch.randn(len(frames), H4, D, generator=torch.Generator().manual_seed(9)).abs()
    outs = []
    with torch.no_grad():
        for b, f in enumerate(frames):
            x = oxv.halfresnet34_trunk(feats[b:b + 1, :, :f], sd)
            assert x.shape == (1, 256, tl.rows_out(f), 10)
            outs.append(x)
            l4[b, :x.shape[2]] = x[0].permute(1, 2, 0).reshape(x.shape[2], D)          # [T'][10][256]: d' = f 256 + c
    return {"frames": frames, "l4": l4, "oracle": outs, "H4": H4}


def test_the_sources_state_the_thresholds_the_batches_assume():
    src = tl.read_sources()
    assert src == {k: getattr(tl, k) for k in src}, "a threshold moved: move the batches of tests/tools/tail_f64.py with it"
    H4 = 33
    for name, B in (("S", 10), ("M", 16), ("L", 63)):
        frames, idx = tl.batch_frames(name)
        assert len(frames) == B and tl.rows_out(max(frames)) == H4 and len(idx) == B
        assert [tl.rows_out(f) for f in frames[:10]] == tl.S_ROWS
    assert all(tl.rows_out(f) == H4 for f in tl.M_EXTRA + tl.L_EXTRA)
    assert H4 % tl.TILE_BF16 and H4 % tl.TILE_F32 and H4 % tl.TILE_BIG                       # tiles straddle utterances
    assert 10 * H4 <= tl.SPLIT_ROWS < 16 * H4 < tl.BIG_ROWS <= 63 * H4 and 62 * H4 < tl.BIG_ROWS
    assert 16 <= tl.SPLIT_ROWS < tl.W_CLIPS and tl.W_CLIPS * tl.rows_out(tl.W_FRAMES) < tl.BIG_ROWS
    assert min(tl.S_ROWS) < tl.POOL_TG < max(tl.S_ROWS) and tl.POOL_TG in tl.S_ROWS
    # odd and even counts before each of the three halvings
    for n in range(3):
        assert {tl.halve(f, n) % 2 for f in tl.S_FRAMES} == {0, 1}, n


def test_reference_reproduces_the_oracle_in_float64(sd, trunk, monkeypatch, capsys):
    """BatchNorm folded in float64 (the library's float32 folding makes operands, not arithmetic), the reference on the float32 layer-4
    rows of the ragged batch S gives what the oracle's pooling (oracle/xvector.py, attentive_pooling) gives in float64 on the same rows,
    every utterance alone: ctx against its mean_std_pooling, att_h against its attention.0 / ReLU / BatchNorm / tanh lines, and, with
    attention.4, the softmax and the weighted statistics on top (_pooling_in_float64 of tests/test_gpu_halfresnet.py), the pooled vector
    against its output.  The one-row utterance is NaN in the std half, in att_h and in the pooled vector on both sides."""
    monkeypatch.setattr(tf, "FOLD", torch.float64)
    frames, l4 = trunk["frames"][:10], trunk["l4"][:10]
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    dp = torch.arange(D)
    d = (dp % 256) * 10 + dp // 256
    perm = torch.cat([d, D + d])
    ctx = tl.ctx_ref(l4, frames)
    rb = tl.rowbias_ref(ctx, sd)
    h = tl.att_h_ref(l4, rb, sd, "fp32").reshape(10, trunk["H4"], tl.NA)
    pooled = _pooling_in_float64(sd, l4.reshape(10, -1, 10, 256), h, [tl.rows_out(f) for f in frames], "fp32")
    worst = {"ctx": 0.0, "att_h": 0.0, "pooled": 0.0}
    for b, f in enumerate(frames):
        n = tl.rows_out(f)
        x = trunk["oracle"][b].double().permute(0, 1, 3, 2).flatten(1, 2)                  # (1, 2560, T'), channel d = 10 c + f
        o_ctx = oxv.mean_std_pooling(x)
        o_h = F.conv1d(torch.cat([x, o_ctx.unsqueeze(2).repeat(1, 1, n)], dim=1), sd64["stat_pooling.attention.0.weight"],
                       sd64["stat_pooling.attention.0.bias"])
        o_h = torch.tanh(oxv._bn(F.relu(o_h), sd64, "stat_pooling.attention.2"))[0].T      # [T'][128]
        o_pooled = oxv.attentive_pooling(trunk["oracle"][b].double(), sd64)[0][perm]
        for name, mine, ref in (("ctx", ctx[b], o_ctx[0][perm]), ("att_h", h[b, :n], o_h), ("pooled", pooled[b], o_pooled)):
            nan = torch.isnan(ref)
            assert torch.equal(torch.isnan(mine), nan), (name, b)
            if n > 1:
                assert not bool(nan.any()), (name, b)
            else:
                assert bool(nan[D:].all() and not nan[:D].any()) if name == "ctx" else bool(nan.all()), (name, b)
            if not bool(nan.all()):
                worst[name] = max(worst[name], rel(mine[~nan], ref[~nan]))
    with capsys.disabled():
        print("  [largest norm-relative distance from the float64 oracle over the utterances: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()) + "]",
              end="")
    assert max(worst.values()) < 1e-12


# ---- mutation check -------------------------------------------------------------------------------------------------------------------
def stats32(l4, n_of, biased=False):
    """torch's float32 mean | std over rows 0 .. n_of(b, own count) - 1 of every utterance, read on through the padded layout"""
    B, H4 = l4.shape[:2]
    flat = torch.cat([l4.reshape(B * H4, D), torch.zeros(1, D)])
    out = torch.zeros(B, 2 * D)
    for b, n in enumerate(n_of):
        x = flat[b * H4:b * H4 + n]
        out[b, :D] = x.mean(0)
        out[b, D:] = x.std(0, unbiased=not biased) if n > 1 else float("nan")
    return out


def sliced(x, w, slices, drop=None, twice=None, keep=None):
    """x . w' in float32 as ``slices`` K slices added in order, one of them dropped or added twice, or only the first ``keep`` columns"""
    K = x.shape[1] if keep is None else keep
    per = x.shape[1] // slices
    tot = torch.zeros(x.shape[0], w.shape[0])
    for z in range(slices):
        a, b = z * per, min((z + 1) * per, K)
        if z == drop or a >= b:
            continue
        s = x[:, a:b] @ w[:, a:b].T
        tot = tot + s + (s if z == twice else 0.0)
    return tot


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_criteria_pass_float32_and_reject_every_mutant(sd, trunk, capsys, dtype):
    """torch's float32 evaluation of the correct formulas stands in for a correct kernel: on batches S and M of the GPU tests (bf16: the
    layer-4 rows rounded to bf16, as the bf16 trunk stores them) it passes every criterion, each stage judged on the stand-in's own
    upstream output.  Every wrong variant below fails the criteria of its stage.  The row-group variants are judged on M, where the rows
    they move belong to utterances of both batches; for them to be rejectable the row bias has to differ between neighbours by far more
    than the bound on ``pre``, which is asserted."""
    frames, H4 = trunk["frames"], trunk["H4"]
    l4 = tl.bf16r(trunk["l4"]) if dtype == "bf16" else trunk["l4"]
    B, R = len(frames), len(frames) * H4
    n = [tl.rows_out(f) for f in frames]
    w1x, w1c, b1, sc, sh = tl.operands(sd, dtype)
    x = l4.reshape(R, D)
    ctx = tl.ctx_ref(l4, frames, F32)
    rb = tl.rowbias_ref(ctx, sd, F32)
    h = tl.att_h_ref(l4, rb, sd, dtype, F32)
    yard = tl.std_yardstick([(l4[:10], frames[:10]), (l4, frames)])

    def judge_ctx(got):
        return tl.check_ctx("ctx", got, l4, frames, yard)

    def judge_rb(got):
        return tl.check_rowbias("att_rb", got, ctx, sd)

    def judge_h(got):
        return tl.check_att_h("att_h", got, l4, rb, sd, dtype, frames)

    # the stand-in passes, on M and on S alone
    shares = judge_ctx(ctx), judge_rb(rb), judge_h(h)
    tl.check_ctx("ctx", ctx[:10], l4[:10], frames[:10], yard)
    tl.check_rowbias("att_rb", rb[:10], ctx[:10], sd)
    tl.check_att_h("att_h", h[:10 * H4], l4[:10], rb[:10], sd, dtype, frames[:10])
    assert bool(torch.isnan(rb[0]).all()) and not bool(torch.isnan(rb[1:]).any())
    assert bool(torch.isnan(h[:H4]).all()) and not bool(torch.isnan(h[H4:]).any())

    # neighbouring utterances' row biases differ by order 1, far more than the largest bound on pre of any judged element
    _, S_pre = tl.att_h_ref(l4, rb, sd, dtype, with_S=True)
    delta_pre = (2 * (tl.K_X + 4 + tl.SLICES_X[dtype]) * tl.U32 * S_pre[tl.own(l4, frames)][H4:]).max().item()
    gaps = [(rb[b] - rb[b + 1]).abs().median().item() for b in range(1, B - 1)]
    assert min(gaps) > 0.1 and min(gaps) > 8 * delta_pre, (min(gaps), delta_pre)

    # the same row biases with a finite row in place of the one-row utterance's NaN: a given operand like any other, on which a
    # neighbour's row bias cannot give itself away by a NaN
    rb_fin = rb.clone()
    rb_fin[0] = rb[5] - rb[6]

    def judge_h_fin(got):
        return tl.check_att_h("att_h", got, l4, rb_fin, sd, dtype, frames)

    def att(pre=None, group=None, bn_first=False, no_tanh=False, roll=0, extra=0.0, w=w1x, rb=rb):
        """torch's float32 attention.0 with one thing wrong (all defaults: the correct formula)"""
        m = torch.arange(R)
        g = (m // H4 if group is None else group(m)).clamp(max=B - 1)
        v = (x @ w.T if pre is None else pre) + rb[g] + extra
        s, t = sc.roll(roll), sh.roll(roll)
        v = torch.relu(v * s + t) if bn_first else torch.relu(v) * s + t
        return v if no_tanh else torch.tanh(v)

    judge_h(att())
    judge_h_fin(att(rb=rb_fin))
    swapped = torch.cat([ctx[:, D:], ctx[:, :D]], 1)
    mutants = [
        ("ctx: biased std", lambda: judge_ctx(stats32(l4, n, biased=True))),
        ("ctx: count H4, the rows past the utterance's own included", lambda: judge_ctx(stats32(l4, [H4] * B))),
        ("ctx: one row more", lambda: judge_ctx(stats32(l4, [k + 1 for k in n]))),
        ("ctx: one row fewer", lambda: judge_ctx(stats32(l4, [max(k - 1, 1) for k in n]))),
        ("ctx: [std | mean]", lambda: judge_ctx(swapped)),
        ("att_rb: [std | mean] operand", lambda: judge_rb(swapped @ w1c.T + b1)),
        ("att_rb: bias b1 missing", lambda: judge_rb(ctx @ w1c.T)),
        ("att_rb: bias b1 added twice", lambda: judge_rb(ctx @ w1c.T + b1 + b1)),
        ("att_rb: one of the 20 slices dropped", lambda: judge_rb(sliced(ctx, w1c, 20, drop=19) + b1)),
        ("att_rb: one of the 20 slices added twice", lambda: judge_rb(sliced(ctx, w1c, 20, twice=7) + b1)),
        ("att_h: row bias of utterance m // (H4 - 1)", lambda: judge_h(att(group=lambda m: m // (H4 - 1)))),
        ("att_h: row bias of utterance m // (H4 + 1)", lambda: judge_h(att(group=lambda m: m // (H4 + 1)))),
        ("att_h: one row bias per 32-row tile", lambda: judge_h(att(group=lambda m: m // 32 * 32 // H4))),
        ("att_h: row bias of utterance m // (H4 - 1), no NaN row", lambda: judge_h_fin(att(group=lambda m: m // (H4 - 1), rb=rb_fin))),
        ("att_h: row bias of utterance m // (H4 + 1), no NaN row", lambda: judge_h_fin(att(group=lambda m: m // (H4 + 1), rb=rb_fin))),
        ("att_h: one row bias per 32-row tile, no NaN row", lambda: judge_h_fin(att(group=lambda m: m // 32 * 32 // H4, rb=rb_fin))),
        ("att_h: bias b1 added again",lambda: judge_h(att(extra=b1))),
        ("att_h: BatchNorm before the ReLU", lambda: judge_h(att(bn_first=True))),
        ("att_h: no tanh", lambda: judge_h(att(no_tanh=True))),
        ("att_h: scale and shift of the neighbouring channel", lambda: judge_h(att(roll=1))),
        ("att_h: K cut to 2496, the last k-tile dropped", lambda: judge_h(att(pre=sliced(x, w1x, 8, keep=2496)))),
        ("att_h: one of the eight slices dropped", lambda: judge_h(att(pre=sliced(x, w1x, 8, drop=3)))),
        ("att_h: one of the eight slices added twice", lambda: judge_h(att(pre=sliced(x, w1x, 8, twice=7)))),
    ]
    if dtype == "bf16":
        mutants.append(("att_h: float32 W1x where the bf16 path rounds it", lambda: judge_h(att(w=tl.operands(sd, "fp32")[0]))))
    judge_h(att(pre=sliced(x, w1x, 8)))           # the slices themselves are no mutant
    judge_rb(sliced(ctx, w1c, 20) + b1)
    lines, survivors = [], []
    for name, run in mutants:
        try:
            run()
            survivors.append(name)
        except AssertionError as e:
            lines.append(f"    rejected  {name}: {str(e)[:110]}")
    with capsys.disabled():
        print(f"\n  [{dtype}: torch's float32 evaluation: mean {shares[0][0]:.3f} of its bound, std {shares[0][1]:.1e} (yardstick {yard:.1e}), att_rb "
              f"{shares[1][0]:.1e} against float64 (worst element {shares[1][2]:.3f} of its bound), att_h {shares[2][0]:.1e} ({shares[2][2]:.4f}); "
              f"row biases of neighbours differ by at least {min(gaps):.2f}, bound on pre at most {delta_pre:.1e}]")
        print("\n".join(lines))
    assert not survivors, f"the criteria pass these wrong kernels: {survivors}"
