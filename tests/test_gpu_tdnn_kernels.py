"""The TDNN x-vector path one kernel at a time: the five dilated-conv GEMMs, mean / std pooling, the embedding GEMM, the double
normalisation and the cosine head, each against a float64 evaluation of the SAME operands (tests/tools/tdnn_f64.py).  Everything runs
through Xtractor(model_archi='xvector').forward_features with the debug taps on; each stage is judged on the kernel's own upstream output:
conv{i} against layer_ref(the conv{i-1} tap), pooled against mean_std_ref(the conv5 tap), pre_norm against embedding_ref(the pooled tap),
the x-vector against normalise_ref(the pre_norm tap), the logits against logits_ref(the x-vector).

Criteria (r = the float64 value, S = the same sum on absolute values, u = 2^-24; tests/test_tdnn_reference_cpu.py shows that torch's float32
evaluation passes them on these operands and that 28 wrong kernels do not):

  GEMM stages, on the rows whose window lies inside their own utterance: |got - r| <= 2 (K + 4) u S per element (K accumulated terms, + the
    number of slices of a sliced sum), norm-relative error at most 16 x that of torch's float32 evaluation, NaN where the reference is NaN.
  mean: |got - r| <= (n + 2) u mean|x| per element over the utterance's n rows.
  std: norm-relative over an utterance's 1536 columns at most 8 x the largest such error of torch's float32 std over the module's cases;
    one pooled row gives NaN in all 1536 columns.
  normalisation: |got - r| <= (N + 8) u |r| per element.

Measured on one MI355X (printed by the tests; DESIGN.md section 4d has the table).
"""
import os
import sys

import numpy
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import tdnn_f64 as tf  # noqa: E402

from sidekit_amd.nnet import Xtractor  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = torch.float32
CONVS = [f"conv{i}" for i in range(1, 6)]
ENDS = ["pooled", "pre_norm", "emb", "logits"]
LAYER_CASES = [("aam", 256), ("aam", 512), ("cce", 256)]
PARTS = [(0, 7), (7, 512), (512, 1025), (1025, 2050)]      # 7 and 505 utterances: K slices as blockIdx.z; 513 and 1025: inside a 64 x 64 workgroup


def _say(capsys, text):
    with capsys.disabled():
        print(f"  [{text}]", end="")


def same(a, b):
    """the same bits, NaN where the other is NaN"""
    if a is None or b is None:
        return a is None and b is None
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


class Ctx:
    """the models under test and what the kernels gave for every batch (computed once)"""

    def __init__(self, gpu):
        torch.set_num_threads(min(16, torch.get_num_threads()))
        self.gpu = gpu
        self.sds, self.models, self.cases = {}, {}, {}

    def sd(self, loss="aam", E=256):
        if (loss, E) not in self.sds:
            self.sds[loss, E] = tf.operand_state_dict(E, loss)
        return self.sds[loss, E]

    def new_model(self, loss="aam", E=256):
        m = Xtractor(tf.N_SPK, model_archi="xvector", loss=loss, embedding_size=E, seed=0).to(self.gpu).eval()
        m.load_state_dict(self.sd(loss, E), strict=True)
        return m

    def model(self, loss="aam", E=256):
        if (loss, E) not in self.models:
            self.models[loss, E] = self.new_model(loss, E)
        return self.models[loss, E]

    def run(self, m, feats, frames, names=tuple(CONVS + ["pooled", "pre_norm"])):
        """forward_features with the taps on -> float32 CPU tensors: conv{i} [R][cout], pooled [B][2 D], pre_norm / emb [B][E], logits or None"""
        try:
            m.set_debug(True)
            out = m.forward_features(feats.to(self.gpu), frames=frames)
            torch.cuda.synchronize()
            raw = m.debug_taps(list(names))
        except RuntimeError as e:      # a HIP error: nothing more is started on this device
            pytest.exit(f"forward_features({tuple(feats.shape)}) failed on the device: {e}", returncode=3)
        logits, emb = out if isinstance(out, tuple) else (None, out)
        B = feats.shape[0]
        c = {"emb": emb.cpu(), "logits": None if logits is None else logits.cpu()}
        for n in names:
            a = torch.from_numpy(raw[n].view(numpy.float32).copy())
            c[n] = a.reshape(B, -1) if n in ("pooled", "pre_norm") else a.reshape(-1, tf.LAYERS[int(n[4]) - 1][1])
        return c

    def case(self, key, make, loss="aam", E=256):
        """key -> dict(frames, feats, taps ..); ``make`` returns (feats, frames)"""
        key = (key, loss, E)
        if key not in self.cases:
            feats, frames = make()
            c = self.run(self.model(loss, E), feats, frames)
            c.update(frames=frames, feats=feats)
            self.cases[key] = c
        return self.cases[key]

    def case1(self, loss="aam", E=256):
        return self.case("case1", lambda: (tf.features(tf.CASE1_FRAMES, seed=1), tf.CASE1_FRAMES), loss, E)

    def switch(self, R):
        """R rows: the case-1 utterances (same features) five times over and one utterance that completes R"""
        def make():
            frames = tf.tile_switch_frames(R)
            last = tf.features(frames[-1:], seed=R)
            base = torch.full((len(tf.CASE1_FRAMES), 80, frames[-1]), 1e30)
            base[:, :, :max(tf.CASE1_FRAMES)] = tf.features(tf.CASE1_FRAMES, seed=1)
            return torch.cat([base] * 5 + [last]), frames
        return self.case(("switch", R), make)

    def alone(self, b):
        """utterance b of the case-1 batch as a batch of its own"""
        f = tf.CASE1_FRAMES[b]
        return self.case(("alone", b), lambda: (tf.features(tf.CASE1_FRAMES, seed=1)[b:b + 1, :, :f].contiguous(), [f]))

    def std_yardstick(self):
        """the largest norm-relative error of torch's float32 std against float64 over the module's pooling cases: the three case-1
        models and the 2049-row batch, each on the kernel's own conv5 tap"""
        if "yard" not in self.cases:
            worst = 0.0
            for c in [self.case1(*lc) for lc in LAYER_CASES] + [self.switch(2049)]:
                r = tf.mean_std_ref(c["conv5"], c["frames"])
                worst = max(worst, max(tf.std_errors(tf.mean_std_ref(c["conv5"], c["frames"], F32), r)))
            self.cases["yard"] = worst
        return self.cases["yard"]


@pytest.fixture(scope="module")
def ctx(gpu):
    return Ctx(gpu)


def judge_layer(i, c, sd, rows="own"):
    """conv{i} of case c against layer_ref on the tap before; ``rows``: 'own' or None for every row"""
    x = tf.rows_of(c["feats"], c["frames"]) if i == 1 else c[f"conv{i - 1}"]
    r, own, S = tf.layer_ref(i, x, c["frames"], sd, with_S=True)
    r32, _ = tf.layer_ref(i, x, c["frames"], sd, F32)
    cin, _, k, _ = tf.LAYERS[i - 1]
    return tf.check_gemm(f"conv{i}", c[f"conv{i}"], r, S, cin * k + 4, own if rows == "own" else None, r32)


def judge_embedding(c, sd, E):
    slices = 12 if E <= 256 else 0           # launch_gemm: K = 3072 is 96 k-tiles, eight per slice, when the split-K workspace is passed (E <= 256)
    r, S = tf.embedding_ref(c["pooled"], sd, with_S=True)
    return tf.check_gemm("pre_norm", c["pre_norm"], r, S, 3072 + 4 + slices, None, tf.embedding_ref(c["pooled"], sd, F32))


@pytest.mark.parametrize("loss,E", LAYER_CASES)
def test_layers_against_float64(ctx, capsys, loss, E):
    """The ragged batch of 15 .. 65 frames (pooled counts 1, 2, 3, 4, 5, 7, 8, 9, 15, 33, 50, 51; R = 356: five full 64-row tiles and 36
    rows, several tiles holding rows of three utterances; conv1's K = 400 ends in a half-empty k-tile): every stage on its own upstream tap.
    E = 512 is the embedding GEMM as one chain with l2norm_kernel as its own launch, E = 256 the K slices with the normalisation in the
    slice-adding kernel.  The 15-frame utterance pools ONE row: NaN std, pre_norm, x-vector and logits, as the reference."""
    c, sd = ctx.case1(loss, E), ctx.sd(loss, E)
    frames = c["frames"]
    assert sum(frames) == 356 and c["conv5"].shape == (356, 1536)
    msg = []
    for i in range(1, 6):
        err, err32, share = judge_layer(i, c, sd)
        msg.append(f"conv{i} {err:.1e} (torch float32 {err32:.1e}; worst element {share:.3f} of its bound)")
    r = tf.mean_std_ref(c["conv5"], frames)
    assert bool(torch.isnan(r[0, 1536:]).all()) and not bool(torch.isnan(r[1:]).any())
    mean_share = tf.check_mean("pooled", c["pooled"], r, c["conv5"], frames)
    yard = ctx.std_yardstick()
    std = tf.check_std("pooled", c["pooled"], r, yard)
    msg.append(f"mean {mean_share:.3f} of its bound, std {std:.1e} (torch float32 at most {yard:.1e}, allowed {8 * yard:.1e})")
    err, err32, share = judge_embedding(c, sd, E)
    msg.append(f"pre_norm {err:.1e} ({err32:.1e}; {share:.3f})")
    assert bool(torch.isnan(c["pre_norm"][0]).all())
    msg.append(f"x-vector {tf.check_normalise('emb', c['emb'], tf.normalise_ref(c['pre_norm'])):.3f} of (N + 8) u |r|")
    if loss == "aam":
        r, S = tf.logits_ref(c["emb"], sd, with_S=True)
        err, err32, share = tf.check_gemm("logits", c["logits"], r, S, E + 4, None, tf.logits_ref(c["emb"], sd, prec=F32))
        msg.append(f"logits {err:.1e} ({err32:.1e}; {share:.3f})")
    else:
        assert c["logits"] is None
    _say(capsys, f"{loss} E={E}: norm-relative error " + ", ".join(msg))


def test_rows_at_the_tile_switch(ctx, capsys):
    """R = 2047 (64 x 64 tiles), 2048 and 2049 (128 x 128 tiles; 2049: one row in the last tile): every own row of every tap, and the pooled
    statistics, pre_norm, x-vector and logits of every utterance, have the bits they have when the utterance runs alone (64 x 64 tiles);
    conv1 (K = 400: the half-empty k-tile in the 128 x 128 kernel) and conv5 (N = 1536) of the 2049-row batch meet the float64 criteria."""
    sd = ctx.sd()
    n1 = len(tf.CASE1_FRAMES)
    for R in (2047, 2048, 2049):
        c = ctx.switch(R)
        frames, off = c["frames"], tf.offsets(c["frames"])
        assert off[-1] == R and c["conv1"].shape[0] == R
        last = ctx.case(("last", R), lambda: (c["feats"][-1:].contiguous(), frames[-1:]))
        for b, f in enumerate(frames):
            one = last if b == len(frames) - 1 else ctx.alone(b % n1)
            for i, name in enumerate(CONVS, start=1):
                n = f - tf.SHRINK[i - 1]
                assert torch.equal(c[name][off[b]:off[b] + n], one[name][:n]), (R, b, name)
            for name in ENDS:
                assert same(c[name][b], one[name][0]), (R, b, name)
    c = ctx.switch(2049)
    e1, e5 = judge_layer(1, c, sd), judge_layer(5, c, sd)
    _say(capsys, f"R = 2049: conv1 {e1[0]:.1e} (torch float32 {e1[1]:.1e}; worst element {e1[2]:.3f} of its bound), conv5 {e5[0]:.1e} ({e5[1]:.1e}; {e5[2]:.3f})")


@pytest.mark.parametrize("sub", ["junk neighbours", "fresh model"])
def test_neighbours_do_not_leak(ctx, capsys, sub):
    """junk neighbours: every second utterance of the case-1 batch holds 1e30, then NaN: the others' own rows of every tap, their pooled
    statistics, pre_norm, x-vectors and logits keep their bits.  (Their rows after the own ones read into the filled neighbour and may be
    anything.)
    fresh model: the batch's last utterance as the FIRST call of a fresh model (workspaces sized for it alone, nothing in them from earlier
    calls): all its rows -- the tail rows read zeros past R in both runs -- have the bits they have in the batch, and the tail rows too meet
    the float64 criteria with zeros past R."""
    c = ctx.case1()
    frames, off = c["frames"], tf.offsets(c["frames"])
    if sub == "junk neighbours":
        for junk in (1e30, float("nan")):
            feats = c["feats"].clone()
            feats[1::2] = junk
            got = ctx.run(ctx.model(), feats, frames)
            for b in range(0, len(frames), 2):
                for i, name in enumerate(CONVS, start=1):
                    n = frames[b] - tf.SHRINK[i - 1]
                    assert torch.equal(got[name][off[b]:off[b] + n], c[name][off[b]:off[b] + n]), (junk, b, name)
                for name in ENDS:
                    assert same(got[name][b], c[name][b]), (junk, b, name)
        return
    f = frames[-1]
    one = ctx.run(ctx.new_model(), c["feats"][-1:, :, :f].contiguous(), [f])
    one.update(frames=[f], feats=c["feats"][-1:, :, :f])
    for name in CONVS:
        assert torch.equal(one[name], c[name][off[-2]:]), name
    for name in ENDS:
        assert same(one[name][0], c[name][-1]), name
    worst = max(judge_layer(i, one, ctx.sd(), rows=None)[2] for i in range(1, 6))
    _say(capsys, f"all {f} rows of every tap within {worst:.3f} of the element bound")


def _big_batch(ctx, model, feats, frames, names):
    """one batch and the same utterances in the parts PARTS -> (whole, parts joined), each {name: [B][..]}"""
    whole = ctx.run(model, feats, frames, names)
    parts = [ctx.run(model, feats[a:b].contiguous(), None if frames is None else frames[a:b], names) for a, b in PARTS]
    joined = {n: (None if whole[n] is None else torch.cat([p[n] for p in parts])) for n in list(names) + ["emb", "logits"]}
    return whole, joined, parts


@pytest.mark.parametrize("arch", ["xvector", "halfresnet34 fp32", "halfresnet34 bf16"])
def test_embedding_bits_at_every_batch_size(ctx, capsys, arch):
    """xvector: 2050 utterances of 17 .. 40 frames as one batch -- the embedding GEMM (M = 2050, N = 256, K = 3072 in 12 slices) runs the
    128 x 128 kernel that adds the slices itself, the five layers run 128 x 128 tiles over 58k rows, the logits 128 x 128 tiles with
    N = 130 -- and in parts of 7, 505 (slices as blockIdx.z), 513 and 1025 utterances (slices inside a 64 x 64 workgroup): the same bits.
    halfresnet34: 2050 clips of 16 frames; the context GEMM of the attention (M = 2050, N = 128, K = 5120) and the embedding GEMM (N = 256)
    both run the 128 x 128 kernel that adds its 20 K slices itself.  pooled (which the context GEMM feeds), pre_norm, x-vectors and
    logits: the same bits as in the parts.  The 513-utterance part's pre_norm meets the float64 criterion with the slices added to K."""
    if arch == "xvector":
        frames = torch.randint(17, 41, (2050,), generator=torch.Generator().manual_seed(4)).tolist()
        whole, joined, parts = _big_batch(ctx, ctx.model(), tf.features(frames, seed=4), frames, ("pooled", "pre_norm"))
    else:
        m = Xtractor(tf.N_SPK, model_archi="halfresnet34", loss="aam", seed=3).to(ctx.gpu).eval()
        m.compute_dtype = arch.split()[1]
        sd = m.state_dict()
        feats = torch.randn(2050, 80, 16, generator=torch.Generator().manual_seed(6))
        whole, joined, parts = _big_batch(ctx, m, feats, None, ("pooled", "pre_norm"))
    for name in ENDS:
        assert not bool(torch.isnan(whole[name]).any()) and torch.equal(whole[name], joined[name]), (arch, name)
    p = parts[2]
    if arch == "xvector":
        err, err32, share = judge_embedding(p, ctx.sd(), 256)
    else:
        r, S = tf.half_embedding_ref(p["pooled"], sd, with_S=True)
        err, err32, share = tf.check_gemm("pre_norm", p["pre_norm"], r, S, 5120 + 4 + 20, None, tf.half_embedding_ref(p["pooled"], sd, F32))
    _say(capsys, f"{arch}: pre_norm of 513 utterances {err:.1e} (torch float32 {err32:.1e}; worst element {share:.3f} of its bound)")


def test_same_call_twice_same_bits(ctx):
    c = ctx.case1()
    again = ctx.run(ctx.model(), c["feats"], c["frames"])
    for name in CONVS:
        assert torch.equal(again[name], c[name]), name
    for name in ENDS:
        assert same(again[name], c[name]), name


def test_argument_errors(ctx):
    """An utterance shorter than the TDNN's context of 15 frames inside an otherwise valid ragged batch is refused before anything is
    launched; the next valid call gives the bits of the case-1 batch."""
    c = ctx.case1()
    frames = list(c["frames"])
    frames[5] = 14
    m = ctx.model()
    with pytest.raises(ValueError, match="context"):
        m.forward_features(c["feats"].to(ctx.gpu), frames=frames)
    again = ctx.run(m, c["feats"], c["frames"])
    for name in CONVS:
        assert torch.equal(again[name], c[name]), name
    for name in ENDS:
        assert same(again[name], c[name]), name
