"""The trunk one kernel at a time: every block's conv1, SE gate and conv2 (Xtractor.debug_block -> xt_debug_block, the launches of the forward
with the handle's packed weights) and the stem against float64 evaluations of the SAME operands (tests/tools/trunk_f64.py), in both
precisions.  Each stage is judged on the kernel's own upstream output: o1 against conv1_ref(x), the gate against gate_ref(the kernel's o1),
the block output against conv2_ref(the kernel's o1, the kernel's gate, x).

Criteria (r = the float64 value, e = bf16(r), S = the same sum on absolute values, K = accumulated terms, delta = 2 K 2^-24 S: the rigorous
bound on a float32 accumulation of K terms in ANY order):

  bf16, o1 and the first blocks' output (one rounding): every element is e or the bf16 value next to it; at most 0.5 % differ from e.
  bf16, later blocks' output (the gated tile z is rounded, then relu(z + x) is): |got - e| <= one bf16 step of max(|z|, |e|); same 0.5 % cap.
  Either rule is the comparison of two ROUNDED values and presumes that the float32 accumulator itself is much closer to r than a bf16 step.
  Where a sum cancels to almost nothing (|r| of the order of 2^8 delta or below, a few elements in 10^5; a positive r next to the ReLU's
  zero) that does not hold for any float32 summation order -- torch's own float32 convolution lands up to five steps from e on such
  elements of these very operands (tests/test_trunk_reference_cpu.py) -- so an element also passes when |got - r| <= delta + half a bf16
  step of got.  The number of elements that needed this clause is printed per case; they count as differing from e in the 0.5 % cap.
  The cap is a condition, not a measurement: a truncating conversion flips about half the elements, float32 arithmetic alone 1e-4.
  fp32: |got - r| <= delta per element, and norm-relative at most 16 x the error of torch's float32 conv2d evaluation of the same formula.
  gate, both precisions: max |gate - gate_ref| at most 8 x the largest error of torch's float32 evaluation of gate_ref over the same cases.

Measured on one MI355X (printed by the tests; DESIGN.md section 4c has the table).
"""
import ctypes
import os
import sys

import numpy
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import trunk_f64 as tf  # noqa: E402

from sidekit_amd import _lib  # noqa: E402
from sidekit_amd.nnet import Xtractor  # noqa: E402

pytestmark = pytest.mark.gpu
BLOCKS = [0, 1, 3, 4, 7, 8, 13, 14]       # the first and a later block of every layer: every convolution shape
DTYPES = ["bf16", "fp32"]
FLIP_CAP = 5e-3
SENTINEL = -7680.0                        # exactly representable in bf16 (15 x 2^9); no kernel output (>= 0 after the ReLU, a sigmoid) can equal it
U32 = 2.0 ** -24


def _say(capsys, text):
    with capsys.disabled():
        print(f"  [{text}]", end="")


def _bf16_step(v):
    """spacing of bf16 numbers at |v| (0 for 0)"""
    _, ex = torch.frexp(v.abs().double())
    return torch.where(v == 0, torch.zeros_like(v, dtype=torch.float64), torch.ldexp(torch.ones_like(v, dtype=torch.float64), ex - 8))


def _steps(a, b):
    def key(t):
        i = t.float().bfloat16().view(torch.int16).int()
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()


def _valid(g, frames, hout):
    m = torch.zeros(len(frames), hout, dtype=torch.bool)
    for b, f in enumerate(frames):
        m[b, :g.rows_out(f)] = True
    return m


def check_bf16(name, got, r, S, K, valid, z=None):
    """the bf16 criteria of the module docstring on the valid rows; returns (share differing from e, elements that needed the cancellation clause)"""
    got, r, S = got[valid].double(), r[valid], S[valid]
    e = tf.bf16r(r)
    nan = torch.isnan(r)
    assert torch.equal(torch.isnan(got), nan), f"{name}: NaN pattern differs from the float64 reference"
    got, r, S, e = got[~nan], r[~nan], S[~nan], e[~nan]
    if z is None:
        close = _steps(got, e) <= 1
    else:
        zz = z[valid][~nan]
        close = (got - e).abs() <= _bf16_step(torch.maximum(zz.abs(), e.abs()))
    cancel = ~close & ((got - r).abs() <= 2 * K * U32 * S + got.abs() * 2.0 ** -8)
    bad = ~(close | cancel)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements off by more than a bf16 step; first: got {got[i].item()!r}, "
                             f"float64 {r[i].item()!r}, bf16 of it {e[i].item()!r}, S {S[i].item():.3e}")
    share = (got != e).double().mean().item()
    assert share <= FLIP_CAP, f"{name}: {share:.2e} of the elements differ from bf16(float64) (cap {FLIP_CAP})"
    return share, int(cancel.sum())


def check_fp32(name, got, r, S, K, valid, r32):
    """the fp32 criteria; returns (norm-relative error of the kernel, of torch's float32 evaluation)"""
    got, r, S, r32 = got[valid].double(), r[valid], S[valid], r32[valid].double()
    nan = torch.isnan(r)
    assert torch.equal(torch.isnan(got), nan), f"{name}: NaN pattern differs from the float64 reference"
    got, r, S, r32 = got[~nan], r[~nan], S[~nan], r32[~nan]
    bad = (got - r).abs() > 2 * K * U32 * S
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements outside 2 K 2^-24 S; first: got {got[i].item()!r}, float64 {r[i].item()!r}, "
                             f"bound {(2 * K * U32 * S[i]).item():.3e}")
    err, err32 = ((got - r).norm() / r.norm()).item(), ((r32 - r).norm() / r.norm()).item()
    assert err <= 16 * err32, f"{name}: norm-relative error {err:.2e} against float64, torch's float32 evaluation {err32:.2e} (x 16 allowed)"
    return err, err32


class Ctx:
    """the model under test, the operands of every case and what the kernels and the references gave for them (computed once)"""

    def __init__(self, gpu):
        torch.set_num_threads(min(16, torch.get_num_threads()))
        self.gpu = gpu
        self.sd = tf.operand_state_dict()
        self.model = Xtractor(16, model_archi="halfresnet34", loss="aam", seed=0).to(gpu).eval()
        self.model.load_state_dict(self.sd, strict=True)
        self.cases = {}

    def run(self, dtype, block, x, frames, form=0, fill=SENTINEL):
        """debug_block on float32 CPU operands -> float32 CPU results (bf16 values widen exactly)"""
        self.model.compute_dtype = dtype
        try:
            xd = x.to(torch.bfloat16 if dtype == "bf16" else torch.float32).to(self.gpu)
            o1, gate, out = self.model.debug_block(block, xd, frames=frames, form=form, fill=fill)
            torch.cuda.synchronize()
            return o1.float().cpu(), gate.cpu(), out.float().cpu()
        except RuntimeError as e:      # a HIP error: nothing more is started on this device
            pytest.exit(f"debug_block({block}, {dtype}, form {form}) failed on the device: {e}", returncode=3)

    def rows(self, dtype, block, kind):
        if kind == "ragged":
            return tf.ragged_rows(block, dtype)
        return {1: [265, 3], 14: [70, 3]}[block]      # the gate kernel's tile loop: more than 1024 / C groups of tiles (32 x 8 rows, 4 x 17 rows)

    def case(self, dtype, block, kind):
        key = (dtype, block, kind)
        if key not in self.cases:
            frames = tf.frames_for_rows(block, self.rows(dtype, block, kind))
            x = tf.block_input(block, frames, dtype, seed=1)
            o1, gate, out = self.run(dtype, block, x, frames)
            self.cases[key] = dict(frames=frames, x=x, o1=o1, gate=gate, out=out)
        return self.cases[key]


@pytest.fixture(scope="module")
def ctx(gpu):
    return Ctx(gpu)


CASES = [(b, "ragged") for b in BLOCKS] + [(1, "gateloop"), (14, "gateloop")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("block,kind", CASES)
def test_block_kernels_against_float64(ctx, capsys, dtype, block, kind):
    """conv1, the gate's arithmetic route and conv2 of one block, each on the kernel's own upstream output; no row past an utterance's length is
    written.  Ragged batches of 1, 2, TH - 1, TH + 1, 2 TH + 1 output rows (TH: the block's row tile; stride-2 blocks with even and odd
    input rows), and for blocks 1 and 14 a batch long enough for the gate kernel's loop over tile groups."""
    c = ctx.case(dtype, block, kind)
    g, sd, frames, x = tf.Geom(block), ctx.sd, c["frames"], c["x"]
    valid = _valid(g, frames, c["o1"].shape[1])
    for name in ("o1", "out"):
        assert bool((c[name][~valid] == SENTINEL).all()), f"{name}: a row past an utterance's length was written"
    assert bool((c["gate"] != SENTINEL).all())
    r1, S1 = tf.conv1_ref(x, sd, block, frames, dtype, with_S=True)
    r2, z, S2 = tf.conv2_ref(c["o1"], c["gate"], x, sd, block, frames, dtype, with_S=True)
    K1, K2 = 9 * g.cin, 9 * g.c + (g.cin if g.first else 0)
    if dtype == "bf16":
        s1, n1 = check_bf16("o1", c["o1"], r1, S1, K1, valid)
        s2, n2 = check_bf16("out", c["out"], r2, S2, K2, valid, z=None if g.first else z)
        _say(capsys, f"{dtype} block {block} {kind}: share of elements != bf16(float64) o1 {s1:.1e} out {s2:.1e}; passed on the cancellation clause {n1} / {n2} of {int(valid.sum()) * g.wout * g.c}")
    else:
        r1_32 = tf.conv1_ref(x, sd, block, frames, dtype, prec=torch.float32)
        r2_32, _ = tf.conv2_ref(c["o1"], c["gate"], x, sd, block, frames, dtype, prec=torch.float32)
        e1 = check_fp32("o1", c["o1"], r1, S1, K1, valid, r1_32)
        e2 = check_fp32("out", c["out"], r2, S2, K2, valid, r2_32)
        _say(capsys, f"{dtype} block {block} {kind}: norm-relative error o1 {e1[0]:.1e} (torch float32 {e1[1]:.1e}) out {e2[0]:.1e} (torch float32 {e2[1]:.1e})")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gates_against_float64(ctx, capsys, dtype):
    """The gate kernel derives the plane mean of bn2(conv2(o1)) from conv1's sums (total - border row - border column + corner); the
    reference convolves the kernel's o1 directly.  One and two rows are where first row = last row and the four corners coincide.  The
    allowance is 8 x the largest error of torch's float32 evaluation over the same cases: a missing or misplaced border term is of order
    1 / H or 1 / W of the mean, thousands of times that."""
    worst, worst32, where = 0.0, 0.0, None
    for block, kind in CASES:
        c = ctx.case(dtype, block, kind)
        r = tf.gate_ref(c["o1"], ctx.sd, block, c["frames"], dtype)
        r32 = tf.gate_ref(c["o1"], ctx.sd, block, c["frames"], dtype, prec=torch.float32)
        err = (c["gate"].double() - r).abs().max().item()
        if err > worst:
            worst, where = err, (block, kind)
        worst32 = max(worst32, (r32.double() - r).abs().max().item())
    _say(capsys, f"{dtype} gates: max |gate - float64| {worst:.2e} at {where}; torch float32 {worst32:.2e}, allowed {8 * worst32:.2e}")
    assert worst <= 8 * worst32, (worst, worst32, where)


@pytest.mark.parametrize("block", [8, 14])
def test_small_grid_forms(ctx, capsys, block):
    """bf16 conv2 of layers 3 and 4 in its small-grid tiling (3- / 2-row tiles): the bits of the batch tiling on the ragged batch, and the float64
    criteria themselves."""
    c = ctx.case("bf16", block, "ragged")
    g, frames, x = tf.Geom(block), c["frames"], c["x"]
    o1, gate, out = ctx.run("bf16", block, x, frames, form=1)
    assert torch.equal(o1, c["o1"]) and torch.equal(gate, c["gate"])
    assert torch.equal(out, c["out"]), "small-grid conv2 differs from the batch tiling"
    valid = _valid(g, frames, out.shape[1])
    r2, z, S2 = tf.conv2_ref(o1, gate, x, ctx.sd, block, frames, "bf16", with_S=True)
    s2, n2 = check_bf16("out", out, r2, S2, 9 * g.c, valid, z=z)
    _say(capsys, f"small-grid block {block}: share {s2:.1e}, cancellation clause {n2}")


def test_persistent_workgroups_loop_over_work_items(ctx):
    """bf16 layers 1 and 2 run as many workgroups as the chip holds and each walks several (utterance, row tile) items.  A batch of block 1 whose
    item count exceeds that grid (launch_cfg of csrc/conv3x3.hip: two workgroups of the layer-1 shape per CU, persist_cap 0) gives every
    utterance the bits it has in the small batches validated against float64 above, and alone."""
    a, b = ctx.case("bf16", 1, "ragged"), ctx.case("bf16", 1, "gateloop")
    g = tf.Geom(1)
    frames = (a["frames"] + b["frames"]) * 3
    hin = max(a["x"].shape[1], b["x"].shape[1])
    parts = []
    for c in (a, b):
        pad = torch.zeros(c["x"].shape[0], hin, g.win, g.cin)
        pad[:, :c["x"].shape[1]] = c["x"]
        parts.append(pad)
    x = torch.cat(parts * 3)
    items = len(frames) * -(-hin // g.tile("bf16"))
    grid = 2 * torch.cuda.get_device_properties(ctx.gpu).multi_processor_count
    assert items > grid, (items, grid)
    o1, gate, out = ctx.run("bf16", 1, x, frames)
    n = 0
    for rep in range(3):
        for c in (a, b):
            for i, f in enumerate(c["frames"]):
                rows = g.rows_out(f)
                assert torch.equal(o1[n, :rows], c["o1"][i, :rows]) and torch.equal(out[n, :rows], c["out"][i, :rows]), (rep, i, rows)
                assert torch.equal(gate[n], c["gate"][i])
                assert bool((out[n, rows:] == SENTINEL).all()) and bool((o1[n, rows:] == SENTINEL).all())
                n += 1
    one = ctx.run("bf16", 1, b["x"][:1], b["frames"][:1])
    assert torch.equal(one[0][0], b["o1"][0]) and torch.equal(one[1][0], b["gate"][0]) and torch.equal(one[2][0], b["out"][0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("block", [3, 14])
def test_stale_rows_do_not_leak(ctx, dtype, block):
    """Input rows past an utterance's length hold 1e30, then NaN (the product's workspaces do hold earlier calls' rows there): every valid output
    element keeps the bits it had with zeros there, and no row past the length is written."""
    c = ctx.case(dtype, block, "ragged")
    g, frames = tf.Geom(block), c["frames"]
    valid = _valid(g, frames, c["o1"].shape[1])
    for junk in (1e30, float("nan")):
        x = c["x"].clone()
        for b, f in enumerate(frames):
            x[b, g.rows_in(f):] = junk
        o1, gate, out = ctx.run(dtype, block, x, frames)
        assert torch.equal(o1[valid], c["o1"][valid]) and torch.equal(out[valid], c["out"][valid]) and torch.equal(gate, c["gate"]), junk
        assert bool((o1[~valid] == SENTINEL).all()) and bool((out[~valid] == SENTINEL).all()), junk


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("block", [1, 7])
def test_one_nan_stays_in_its_utterance(ctx, dtype, block):
    """One NaN in one utterance's input: o1 is NaN exactly where the float64 reference is, that utterance's gate and output are NaN as in the
    reference, every other utterance keeps its bits."""
    c = ctx.case(dtype, block, "ragged")
    g, frames = tf.Geom(block), c["frames"]
    hit = 3                                               # TH + 1 rows: more than one tile
    x = c["x"].clone()
    x[hit, 1, g.win // 2, 5] = float("nan")
    o1, gate, out = ctx.run(dtype, block, x, frames)
    rows = g.rows_out(frames[hit])
    r1 = tf.conv1_ref(x, ctx.sd, block, frames, dtype)
    assert 0 < int(torch.isnan(r1[hit]).sum()) < r1[hit, :rows].numel()
    assert torch.equal(torch.isnan(o1[hit, :rows]), torch.isnan(r1[hit, :rows]))
    rg = tf.gate_ref(o1, ctx.sd, block, frames, dtype)
    assert torch.equal(torch.isnan(gate), torch.isnan(rg)) and bool(torch.isnan(gate[hit]).all())
    r2, _ = tf.conv2_ref(o1, gate, x, ctx.sd, block, frames, dtype)
    assert torch.equal(torch.isnan(out[hit, :rows]), torch.isnan(r2[hit, :rows])) and bool(torch.isnan(out[hit, :rows]).all())
    for b in range(len(frames)):
        if b != hit:
            assert torch.equal(o1[b], c["o1"][b]) and torch.equal(gate[b], c["gate"][b]) and torch.equal(out[b], c["out"][b]), b


@pytest.mark.parametrize("dtype", DTYPES)
def test_same_call_twice_same_bits(ctx, dtype):
    for block in (0, 8):
        c = ctx.case(dtype, block, "ragged")
        o1, gate, out = ctx.run(dtype, block, c["x"], c["frames"])
        assert torch.equal(o1, c["o1"]) and torch.equal(gate, c["gate"]) and torch.equal(out, c["out"]), block


def test_uniform_batch_without_a_length_array(ctx):
    """frames = None (the kernels' uniform-length path) gives the bits of the same batch with explicit equal lengths"""
    for dtype in DTYPES:
        x = tf.block_input(4, [18 << 1] * 2, dtype, seed=2)
        a = ctx.run(dtype, 4, x, None)
        b = ctx.run(dtype, 4, x, [18 << 1] * 2)
        assert all(torch.equal(p, q) for p, q in zip(a, b)), dtype


def test_argument_errors_launch_nothing(ctx):
    """block out of range, form 1 where there is none, null pointers: SK_EARG with a message, and the outputs keep their pre-fill"""
    lib = _lib.lib()
    for dtype in DTYPES:
        ctx.model.compute_dtype = dtype
        h = ctx.model._handle()
        el = torch.bfloat16 if dtype == "bf16" else torch.float32
        x = torch.zeros(1, 4, 80, 32, dtype=el, device=ctx.gpu)
        o1, out = torch.full_like(x, SENTINEL), torch.full_like(x, SENTINEL)
        gate = torch.full((1, 32), SENTINEL, device=ctx.gpu)
        st = ctypes.c_void_p(torch.cuda.current_stream(ctx.gpu).cuda_stream)
        P = lambda t: t.data_ptr()   # noqa: E731
        bad = [(lib.xt_debug_block(h, 16, P(x), None, 1, 4, 0, P(o1), P(gate), P(out), st), "outside"),
               (lib.xt_debug_block(h, -1, P(x), None, 1, 4, 0, P(o1), P(gate), P(out), st), "outside"),
               (lib.xt_debug_block(h, 1, P(x), None, 1, 4, 1, P(o1), P(gate), P(out), st), "small-grid"),
               (lib.xt_debug_block(h, 1, P(x), None, 1, 4, 2, P(o1), P(gate), P(out), st), "form"),
               (lib.xt_debug_block(h, 1, None, None, 1, 4, 0, P(o1), P(gate), P(out), st), "null"),
               (lib.xt_debug_block(h, 1, P(x), None, 1, 4, 0, None, P(gate), P(out), st), "null"),
               (lib.xt_debug_block(h, 1, P(x), None, 1, 4, 0, P(o1), None, P(out), st), "null"),
               (lib.xt_debug_block(h, 1, P(x), None, 1, 4, 0, P(o1), P(gate), None, st), "null"),
               (lib.xt_debug_block(None, 1, P(x), None, 1, 4, 0, P(o1), P(gate), P(out), st), "null")]
        if dtype == "fp32":   # the small-grid tilings are bf16 only
            bad.append((lib.xt_debug_block(h, 14, P(x), None, 1, 4, 1, P(o1), P(gate), P(out), st), "small-grid"))
        for rc, word in bad:
            assert rc == _lib.SK_EARG, (rc, word)
        rc = lib.xt_debug_block(h, 16, P(x), None, 1, 4, 0, P(o1), P(gate), P(out), st)
        assert rc == _lib.SK_EARG and "outside" in _lib.last_error()
        rc = lib.xt_debug_block(h, 1, P(x), None, 1, 4, 1, P(o1), P(gate), P(out), st)
        assert rc == _lib.SK_EARG and "small-grid" in _lib.last_error()
        rc = lib.xt_debug_block(h, 1, None, None, 1, 4, 0, P(o1), P(gate), P(out), st)
        assert rc == _lib.SK_EARG and "null" in _lib.last_error()
        torch.cuda.synchronize()
        assert bool((o1 == SENTINEL).all()) and bool((out == SENTINEL).all()) and bool((gate == SENTINEL).all())
        with pytest.raises(ValueError):
            ctx.model.debug_block(16, x)
        with pytest.raises(ValueError):
            ctx.model.debug_block(1, x, frames=[5])           # more frames than the input has rows


STEM_FRAMES = [1, 15, 16, 17, 33]        # the stem tile is 16 rows


@pytest.mark.parametrize("dtype", DTYPES)
def test_stem_against_float64(ctx, capsys, dtype):
    """The stem through forward_features and the "stem" tap, on features of both signs and ragged frames around its 16-row tile (a 1-frame
    utterance included): the block criteria against relu(sum w' x + shift) in float64, w' = f32(w scale) as the library folds it."""
    T = max(STEM_FRAMES)
    feats = torch.randn(len(STEM_FRAMES), 80, T, generator=torch.Generator().manual_seed(9))
    for b, f in enumerate(STEM_FRAMES):
        feats[b, :, f:] = 1e30                                # never read
    m = ctx.model
    m.compute_dtype = dtype
    m.set_debug(True)
    try:
        m.forward_features(feats.to(ctx.gpu), frames=STEM_FRAMES)
        raw = m.debug_taps(["stem"])["stem"]
    finally:
        m.set_debug(False)
    if dtype == "bf16":
        got = torch.from_numpy((raw.view(numpy.uint16).astype(numpy.uint32) << 16).view(numpy.float32).copy())
    else:
        got = torch.from_numpy(raw.view(numpy.float32).copy())
    got = got.reshape(len(STEM_FRAMES), T, 80, 32)
    valid = torch.zeros(len(STEM_FRAMES), T, dtype=torch.bool)
    for b, f in enumerate(STEM_FRAMES):
        valid[b, :f] = True
    r, S = tf.stem_ref(feats, ctx.sd, STEM_FRAMES, with_S=True)
    if dtype == "bf16":
        share, n = check_bf16("stem", got, r, S, 10, valid)
        _say(capsys, f"bf16 stem: share of elements != bf16(float64) {share:.1e}; cancellation clause {n}")
    else:
        err = check_fp32("stem", got, r, S, 10, valid, tf.stem_ref(feats, ctx.sd, STEM_FRAMES, prec=torch.float32))
        _say(capsys, f"fp32 stem: norm-relative error {err[0]:.1e} (torch float32 {err[1]:.1e})")
