"""The float64 reference of the TDNN path (tests/tools/tdnn_f64.py) without a GPU: pinned to the oracle in float64, and its criteria shown to
reject wrong kernels on the very operands tests/test_gpu_tdnn_kernels.py uses."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import tdnn_f64 as tf  # noqa: E402

from oracle import xvector as oxv  # noqa: E402

F32 = torch.float32


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / b.norm()).item()


def chain(sd, feats, frames, prec, loss="aam"):
    """the reference functions one after the other, each on the output of the one before, in ``prec``"""
    t = {}
    x = tf.rows_of(feats, frames)
    for i in range(1, 6):
        x, _ = tf.layer_ref(i, x, frames, sd, prec)
        t[f"conv{i}"] = x
    t["pooled"] = tf.mean_std_ref(x, frames, prec)
    t["pre_norm"] = tf.embedding_ref(t["pooled"], sd, prec)
    t["emb"] = tf.normalise_ref(t["pre_norm"], prec)
    if loss == "aam":
        t["logits"] = tf.logits_ref(t["emb"], sd, prec=prec)
    return t


@pytest.mark.parametrize("loss", ["aam", "cce"])
def test_chained_reference_reproduces_the_oracle_in_float64(loss, monkeypatch, capsys):
    """Host-side folding switched to float64 (the library's float32 folding makes operands, not arithmetic), the chained reference gives the
    oracle's float64 taps conv1..5 (own rows), pooled, pre_norm, embedding and logits within 1e-12 norm-relative on the ragged case-1
    batch, every utterance run alone through the oracle.  The 15-frame utterance pools one row: its std, pre_norm, embedding and logits are
    NaN on both sides.  loss='cce': the oracle returns l2_norm(x) alone, which is normalise_ref(twice=False)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    monkeypatch.setattr(tf, "FOLD", torch.float64)
    frames = tf.CASE1_FRAMES
    sd = tf.operand_state_dict(256, loss)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    feats = tf.features(frames, seed=1)
    t = chain(sd, feats.double(), frames, torch.float64, loss)
    off = tf.offsets(frames)
    worst = 0.0
    for b, n in enumerate(frames):
        o = {}
        out = oxv.tdnn_from_feats(feats[b:b + 1, :, :n].double(), sd64, loss=loss, aam_s=tf.AAM_S, taps=o)
        for i in range(1, 6):
            ref = o[f"conv{i}"][0].T
            assert ref.shape[0] == n - tf.SHRINK[i - 1]
            mine = t[f"conv{i}"][off[b]:off[b] + ref.shape[0]]
            assert bool(tf.own(i, frames)[off[b]:off[b] + ref.shape[0]].all()) and not bool(tf.own(i, frames)[off[b] + ref.shape[0]:off[b + 1]].any())
            worst = max(worst, rel(mine, ref))
        ends = {"pooled": o["pooled"][0], "pre_norm": o["pre_norm"][0]}
        if loss == "aam":
            ends["logits"], ends["emb"] = out[0][0], out[1][0]
        else:
            ends["emb"] = out[0]
        for name, ref in ends.items():
            mine = t[name][b] if not (loss == "cce" and name == "emb") else tf.normalise_ref(t["pre_norm"], twice=False)[b]
            nan = torch.isnan(ref)
            assert torch.equal(torch.isnan(mine), nan), (name, b)
            if n != 15:
                assert not bool(nan.any()), (name, b)
            elif name == "pooled":
                assert bool(nan[1536:].all()) and not bool(nan[:1536].any())
            else:
                assert bool(nan.all()), (name, b)
            if not bool(nan.all()):
                worst = max(worst, rel(mine[~nan], ref[~nan]))
    with capsys.disabled():
        print(f"  [{loss}: largest norm-relative distance from the float64 oracle over all taps and utterances {worst:.1e}]", end="")
    assert worst < 1e-12


# ---- mutation check -------------------------------------------------------------------------------------------------------------------
def layer32(i, x, sd, dil=None, order=None, keep=None, bn_first=False, slope=0.2, bias=True, roll=0, zero_rows=None):
    """torch's float32 evaluation of layer i with one thing wrong (all defaults: the correct formula, as layer_ref(prec = float32))"""
    _, _, k, d = tf.LAYERS[i - 1]
    w, b, sc, sh = tf.layer_operands(i, sd)
    x = x.float().clone()
    if zero_rows is not None:
        x[zero_rows] = 0.0
    A = tf.unfold(x, k, d if dil is None else dil)
    cin = x.shape[1]
    if order is not None:
        A = torch.cat([A[:, j * cin:(j + 1) * cin] for j in order], dim=1)
    if keep is not None:
        A = A.clone()
        A[:, keep:] = 0.0
    v = A @ w.T + (b if bias else 0.0)
    sc, sh = sc.roll(roll), sh.roll(roll)
    if bn_first:
        return F.leaky_relu(v * sc + sh, slope)
    return F.leaky_relu(v, slope) * sc + sh


def utterance_rows(frames, start_of_tail):
    """bool [R]: the rows of every utterance from its row ``start_of_tail(frames_b)`` on"""
    off = tf.offsets(frames)
    m = torch.zeros(off[-1], dtype=torch.bool)
    for b, f in enumerate(frames):
        m[off[b] + start_of_tail(f):off[b + 1]] = True
    return m


def test_criteria_pass_float32_and_reject_every_mutant(capsys):
    """torch's float32 evaluation of the correct formulas stands in for a correct kernel: chained over the case-1 batch of the GPU tests (same
    state dict, same features) it passes every criterion of tests/test_gpu_tdnn_kernels.py, each stage judged on the stand-in's own
    upstream output.  Every wrong variant below fails the criteria of its stage.

    The two window mutants probe "which rows are still the utterance's own" from both sides.  (a) A kernel whose window is
    cut one input row short of what an utterance still owns (the last own row of the tap before is read as zero) fails on the own rows:
    own is not too wide a claim for the reference, the last own row really reads that far.  (b) A kernel that stops the window at the
    utterance's end instead of reading on into the next utterance is indistinguishable on the own rows (it passes: those rows never
    look past their utterance) and fails as soon as ONE more row per utterance is judged: own is not too narrow either.  In layers 2
    and 3 the row after the last own one still reads inside its utterance, but a row of the tap before that already depends on the
    neighbour: with layer 1 cut at the utterance's end, layers 2 and 3 pass on their own rows and fail on one row more.

    One normalisation instead of two is not a mutant these operands can reject, and no operands could: the second normalisation divides
    a unit vector by its float32 norm, 1 to within a few 2^-24, far inside (N + 8) 2^-24.  It is measured and reported, not asserted
    to fail."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    frames = tf.CASE1_FRAMES
    sd = tf.operand_state_dict(256, "aam")
    t = chain(sd, tf.features(frames, seed=1), frames, F32)
    taps = [tf.rows_of(tf.features(frames, seed=1), frames)] + [t[f"conv{i}"] for i in range(1, 6)]

    def judge_layer(i, got, extra=0):
        r, _, S = tf.layer_ref(i, taps[i - 1], frames, sd, with_S=True)
        cin, _, k, _ = tf.LAYERS[i - 1]
        return tf.check_gemm(f"conv{i}", got, r, S, cin * k + 4, tf.own(i, frames, extra), tf.layer_ref(i, taps[i - 1], frames, sd, F32)[0])

    r_pool = tf.mean_std_ref(t["conv5"], frames)
    yard = max(tf.std_errors(t["pooled"], r_pool))

    def judge_pooled(got):
        tf.check_mean("pooled", got, r_pool, t["conv5"], frames)
        tf.check_std("pooled", got, r_pool, yard)

    def judge_embedding(got):
        r, S = tf.embedding_ref(t["pooled"], sd, with_S=True)
        return tf.check_gemm("pre_norm", got, r, S, 3072 + 4 + 12, None, tf.embedding_ref(t["pooled"], sd, F32))

    def judge_logits(got):
        r, S = tf.logits_ref(t["emb"], sd, with_S=True)
        return tf.check_gemm("logits", got, r, S, 256 + 4, None, tf.logits_ref(t["emb"], sd, prec=F32))

    # the stand-in passes everything
    for i in range(1, 6):
        judge_layer(i, t[f"conv{i}"])
    judge_pooled(t["pooled"])
    judge_embedding(t["pre_norm"])
    tf.check_normalise("emb", t["emb"], tf.normalise_ref(t["pre_norm"]))
    judge_logits(t["logits"])

    def biased_std():
        p = t["pooled"].clone()
        off = tf.offsets(frames)
        for b, f in enumerate(frames):
            if f - 14 > 1:                # the NaN of a single pooled row stays: the std criterion itself has to reject the rest
                p[b, 1536:] = t["conv5"][off[b]:off[b] + f - 14].std(0, unbiased=False)
        return p

    w6, b6 = sd["before_speaker_embedding.linear6.weight"], sd["before_speaker_embedding.linear6.bias"]
    short = {i: utterance_rows(frames, lambda f, i=i: f - (tf.SHRINK[i - 2] if i > 1 else 0) - 1) for i in (1, 2, 3)}

    def next_utterance_zero(i):
        """layer i with every utterance evaluated alone: zeros past ITS last row instead of the next utterance's rows"""
        off = tf.offsets(frames)
        return torch.cat([layer32(i, taps[i - 1][off[b]:off[b + 1]], sd) for b in range(len(frames))])

    alone1 = next_utterance_zero(1)
    alone2 = layer32(2, alone1, sd)
    mutants = [
        ("layer 2: dilation 3", lambda: judge_layer(2, layer32(2, taps[1], sd, dil=3))),
        ("layer 2: dilation 1", lambda: judge_layer(2, layer32(2, taps[1], sd, dil=1))),
        ("layer 3: dilation 4", lambda: judge_layer(3, layer32(3, taps[2], sd, dil=4))),
        ("layer 3: dilation 2", lambda: judge_layer(3, layer32(3, taps[2], sd, dil=2))),
        ("layer 1: taps in reversed order", lambda: judge_layer(1, layer32(1, taps[0], sd, order=[4, 3, 2, 1, 0]))),
        ("layer 3: taps in reversed order", lambda: judge_layer(3, layer32(3, taps[2], sd, order=[2, 1, 0]))),
        ("layer 1: last tap dropped", lambda: judge_layer(1, layer32(1, taps[0], sd, keep=320))),
        ("layer 2: last tap dropped", lambda: judge_layer(2, layer32(2, taps[1], sd, keep=1024))),
        ("layer 1: K truncated to 384", lambda: judge_layer(1, layer32(1, taps[0], sd, keep=384))),
        ("layer 1: BatchNorm before the LeakyReLU", lambda: judge_layer(1, layer32(1, taps[0], sd, bn_first=True))),
        ("layer 5: BatchNorm before the LeakyReLU", lambda: judge_layer(5, layer32(5, taps[4], sd, bn_first=True))),
        ("layer 4: slope 0.02", lambda: judge_layer(4, layer32(4, taps[3], sd, slope=0.02))),
        ("layer 1: bias omitted", lambda: judge_layer(1, layer32(1, taps[0], sd, bias=False))),
        ("layer 5: bias omitted", lambda: judge_layer(5, layer32(5, taps[4], sd, bias=False))),
        ("layer 2: scale and shift of the neighbouring channel", lambda: judge_layer(2, layer32(2, taps[1], sd, roll=1))),
        ("layer 5: scale and shift of the neighbouring channel", lambda: judge_layer(5, layer32(5, taps[4], sd, roll=-1))),
        ("layer 1: window one row short at every utterance's end", lambda: judge_layer(1, layer32(1, taps[0], sd, zero_rows=short[1]))),
        ("layer 2: window one row short at every utterance's end", lambda: judge_layer(2, layer32(2, taps[1], sd, zero_rows=short[2]))),
        ("layer 3: window one row short at every utterance's end", lambda: judge_layer(3, layer32(3, taps[2], sd, zero_rows=short[3]))),
        ("layer 1: window stops at the utterance's end, one more row judged", lambda: judge_layer(1, next_utterance_zero(1), extra=1)),
        ("layer 2: layer 1 stops at the utterance's end, one more row judged", lambda: judge_layer(2, layer32(2, alone1, sd), extra=1)),
        ("layer 3: layer 1 stops at the utterance's end, one more row judged", lambda: judge_layer(3, layer32(3, alone2, sd), extra=1)),
        ("pooling: biased std", lambda: judge_pooled(biased_std())),
        ("pooling: count frames - 13", lambda: judge_pooled(tf.mean_std_ref(t["conv5"], frames, F32, shrink=13))),
        ("embedding: bias omitted", lambda: judge_embedding(t["pooled"] @ w6.T)),
        ("embedding: mean and std halves swapped", lambda: judge_embedding(torch.cat([t["pooled"][:, 1536:], t["pooled"][:, :1536]], 1) @ w6.T + b6)),
        ("logits: head rows not normalised", lambda: judge_logits(t["emb"] @ sd["after_speaker_embedding.weight"].T * tf.AAM_S)),
        ("logits: s = 30", lambda: judge_logits(tf.logits_ref(t["emb"], sd, s=30.0, prec=F32))),
    ]

    # (b), first half: on the own rows that kernel is a correct one, and so is every layer after it
    for i in (1, 2, 3):
        judge_layer(i, next_utterance_zero(i))
    judge_layer(2, layer32(2, alone1, sd))
    judge_layer(3, layer32(3, alone2, sd))
    lines, survivors = [], []
    for name, run in mutants:
        try:
            run()
            survivors.append(name)
        except AssertionError as e:
            lines.append(f"    rejected  {name}: {str(e)[:110]}")
    once = tf.normalise_ref(t["pre_norm"], F32, twice=False)
    r_emb = tf.normalise_ref(t["pre_norm"])
    share = tf.check_normalise("one normalisation", once, r_emb)
    both = tf.check_normalise("two normalisations", t["emb"], r_emb)
    lines.append(f"    dropped   one normalisation instead of two: passes, {share:.3f} of the (N + 8) 2^-24 |r| allowance against {both:.3f} with both")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not survivors, f"the criteria pass these wrong kernels: {survivors}"
