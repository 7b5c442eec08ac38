"""HalfResNet34's attention front one kernel at a time: the global context (mean_std_kernel on the padded layer-4 rows), the context GEMM
(20 K slices, consumed only as a per-utterance row bias) and attention.0 (the product with the row bias of utterance m / H4, ReLU,
BatchNorm, tanh), each against a float64 evaluation of the SAME operands (tests/tools/tail_f64.py).  Everything runs through
Xtractor(model_archi='halfresnet34').forward_features with the debug taps on; each stage is judged on the kernel's own upstream output:
ctx against ctx_ref(the layer4 tap), att_rb against rowbias_ref(the ctx tap), att_h against att_h_ref(the layer4 and att_rb taps) on the
rows an utterance owns.  The criteria are stated in tests/tools/tail_f64.py; tests/test_tail_reference_cpu.py shows that torch's float32
evaluation passes them on these operands and that 23 wrong kernels (24 on the bf16 path) do not.

Batches, as layer-4 rows per utterance (H4 = 33 rows of stride: every 32-, 64- and 128-row tile straddles utterances):
  S  1, 2, 3, 4, 5, 7, 8, 9, 15, 33: R = 330.  bf16: attention.0's eight K slices as blockIdx.y and gemm_splitk_epilogue_kernel; the
     context GEMM's 20 slices as blockIdx.z.  The one-row utterance has a NaN std, a NaN att_rb row and NaN att_h rows, alone.
  M  S and six utterances of 33 rows: R = 528 > 512.  bf16: one workgroup walks all 40 k-tiles and adds the slices itself.
  L  (fp32) S six times over and three utterances of 33 rows: R = 2079 >= 2048, gemm128_kernel<false> with the row bias.
  W  513 clips of 16 frames: the context GEMM adds its slices inside the workgroup.

Measured on one MI355X (printed by the tests; DESIGN.md section 4f has the table).
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import tail_f64 as tl  # noqa: E402

from sidekit_amd.nnet import Xtractor  # noqa: E402

pytestmark = pytest.mark.gpu
TAPS = ("layer4", "ctx", "att_rb", "att_h")
CASES = [("S", "fp32"), ("S", "bf16"), ("M", "fp32"), ("M", "bf16"), ("L", "fp32"), ("W", "fp32"), ("W", "bf16")]
H4 = 33


def _say(capsys, text):
    with capsys.disabled():
        print(f"  [{text}]", end="")


def bits(a, b):
    """the same bytes (a NaN equals only the same NaN)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Ctx:
    """the model under test and what the kernels gave for every batch (computed once)"""

    def __init__(self, gpu):
        torch.set_num_threads(min(16, torch.get_num_threads()))
        self.gpu = gpu
        self.sd = tl.operand_state_dict()
        self.model = Xtractor(tl.N_SPK, model_archi="halfresnet34", loss="aam", seed=0).to(gpu).eval()
        self.model.load_state_dict(self.sd, strict=True)
        self.cases = {}

    def run(self, dtype, feats, frames):
        """forward_features with the taps on -> layer4 [B][H4][2560], ctx [B][5120], att_rb [B][128], att_h [B H4][128], float32 on the CPU"""
        m = self.model
        m.compute_dtype = dtype
        try:
            m.set_debug(True)
            m.forward_features(feats.to(self.gpu), frames=frames)
            torch.cuda.synchronize()
            raw = m.debug_taps(list(TAPS))
            m.set_debug(False)
        except RuntimeError as e:      # a HIP error: nothing more is started on this device
            pytest.exit(f"forward_features({tuple(feats.shape)}, {dtype}) failed on the device: {e}", returncode=3)
        B = feats.shape[0]
        c = {"layer4": tl.layer4_rows(raw["layer4"], B, dtype), "frames": frames, "feats": feats}
        for n, width in (("ctx", 2 * tl.D), ("att_rb", tl.NA), ("att_h", tl.NA)):
            c[n] = torch.from_numpy(raw[n].view("float32").copy()).reshape(-1, width)
        h4 = c["layer4"].shape[1]
        assert c["ctx"].shape[0] == B and c["att_rb"].shape[0] == B and c["att_h"].shape[0] == B * h4
        assert h4 == tl.rows_out(feats.shape[2])
        return c

    def case(self, name, dtype):
        if (name, dtype) not in self.cases:
            self.cases[name, dtype] = self.run(dtype, *tl.features(name))
        return self.cases[name, dtype]

    def alone(self, b, dtype):
        """utterance b of batch S as a batch of one"""
        if ("alone", b, dtype) not in self.cases:
            f = tl.S_FRAMES[b]
            self.cases["alone", b, dtype] = self.run(dtype, tl.features("S")[0][b:b + 1, :, :f].contiguous(), [f])
        return self.cases["alone", b, dtype]

    def std_yardstick(self):
        """the largest norm-relative error of torch's float32 std against float64 over the module's cases, each on the kernel's own
        layer4 tap"""
        if "yard" not in self.cases:
            self.cases["yard"] = tl.std_yardstick([(c["layer4"], c["frames"]) for c in (self.case(*k) for k in CASES)])
        return self.cases["yard"]


@pytest.fixture(scope="module")
def ctx(gpu):
    return Ctx(gpu)


def shape_of(name, c):
    """B and R of a case, asserted to lie on the side of launch_gemm's thresholds the case is there for"""
    B, h4 = c["layer4"].shape[:2]
    R = B * h4
    if name == "W":
        assert B == tl.W_CLIPS > tl.SPLIT_ROWS and h4 == 2 and R < tl.BIG_ROWS
        return B, R
    assert h4 == H4 and H4 % tl.TILE_BF16 and H4 % tl.TILE_F32 and H4 % tl.TILE_BIG and B <= tl.SPLIT_ROWS
    assert [tl.rows_out(f) for f in c["frames"][:10]] == tl.S_ROWS and min(tl.S_ROWS) < tl.POOL_TG < max(tl.S_ROWS)
    if name == "S":
        assert (B, R) == (10, 330) and R <= tl.SPLIT_ROWS
    elif name == "M":
        assert (B, R) == (16, 528) and tl.SPLIT_ROWS < R < tl.BIG_ROWS
    else:
        assert (B, R) == (63, 2079) and R >= tl.BIG_ROWS
    return B, R


@pytest.mark.parametrize("name,dtype", CASES)
def test_context_against_float64(ctx, capsys, name, dtype):
    """ctx = [mean | std] of mean_std_kernel (<8> on bf16 rows, <4> on float32 rows; fixed row stride H4, counts from three halvings of
    the frames, on both sides of POOL_TG = 4) against ctx_ref(the layer4 tap).  The one-row utterance: NaN in all 2560 std columns."""
    c = ctx.case(name, dtype)
    shape_of(name, c)
    r = tl.ctx_ref(c["layer4"], c["frames"])
    nan = torch.isnan(r)
    if name == "W":
        assert not bool(nan.any())
    else:
        one_row = torch.tensor([tl.rows_out(f) == 1 for f in c["frames"]])
        assert bool(nan[one_row][:, tl.D:].all()) and not bool(nan[one_row][:, :tl.D].any()) and not bool(nan[~one_row].any())
    yard = ctx.std_yardstick()
    mean, std = tl.check_ctx(f"ctx ({name}, {dtype})", c["ctx"], c["layer4"], c["frames"], yard)
    _say(capsys, f"{name} {dtype}: mean {mean:.3f} of its bound, std {std:.1e} (torch float32 at most {yard:.1e}, allowed {8 * yard:.1e})")


@pytest.mark.parametrize("name,dtype", CASES)
def test_row_bias_against_float64(ctx, capsys, name, dtype):
    """att_rb = ctx . W1c' + b1 (gemm_kernel, K = 5120 in 20 slices: side by side with gemm_splitk_epilogue_kernel up to 512 utterances,
    inside the workgroup for W's 513) against rowbias_ref(the ctx tap).  NaN exactly in the one-row utterances' rows."""
    c = ctx.case(name, dtype)
    B, _ = shape_of(name, c)
    assert (B > tl.SPLIT_ROWS) == (name == "W")
    err, err32, share = tl.check_rowbias(f"att_rb ({name}, {dtype})", c["att_rb"], c["ctx"], ctx.sd)
    if name != "W":
        gaps = [(c["att_rb"][b] - c["att_rb"][b + 1]).abs().median().item() for b in range(1, 15 if name == "M" else 9)]
        assert min(gaps) > 0.1, "neighbouring utterances' row biases no longer differ by order 1: the row-group errors would go unseen"
    _say(capsys, f"{name} {dtype}: att_rb {err:.1e} (torch float32 {err32:.1e}; worst element {share:.4f} of its bound)")


@pytest.mark.parametrize("name,dtype", [k for k in CASES if k[0] != "W"])
def test_attention0_against_float64(ctx, capsys, name, dtype):
    """att_h on the rows an utterance owns against att_h_ref(the layer4 tap, the att_rb tap).  bf16: gemm_bf16_kernel<true>, S in eight
    slices of 5 k-tiles (the odd-tile-count path) as blockIdx.y, M as one walk of 40 k-tiles; fp32: gemm_kernel, and gemm128_kernel<false>
    for L.  The one-row utterances' rows are NaN, every other utterance's own rows are finite."""
    c = ctx.case(name, dtype)
    B, R = shape_of(name, c)
    own = tl.own(c["layer4"], c["frames"]).reshape(B, -1)
    got = c["att_h"].reshape(B, -1, tl.NA)
    for b, f in enumerate(c["frames"]):
        mine = got[b][own[b]]
        assert mine.shape[0] == tl.rows_out(f)
        assert bool(torch.isnan(mine).all()) if tl.rows_out(f) == 1 else bool(torch.isfinite(mine).all()), (b, f)
    err, err32, share = tl.check_att_h(f"att_h ({name}, {dtype})", c["att_h"], c["layer4"], c["att_rb"], ctx.sd, dtype, c["frames"])
    flat = got[~torch.isnan(got)]
    _say(capsys, f"{name} {dtype}: att_h {err:.1e} (torch float32 {err32:.1e}; worst element {share:.4f} of its bound; "
                 f"{(flat.abs() > 0.999).float().mean().item():.2f} of the values beyond +- 0.999)")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_bits_across_the_row_thresholds(ctx, dtype):
    """Every utterance of S has the same ctx, att_rb and own-row att_h bytes in S (R = 330), in M (R = 528: the slices inside the
    workgroup), in every copy in L (fp32: R = 2079, 128 x 128 tiles) and alone as a batch of one (another row stride)."""
    s = ctx.case("S", dtype)
    others = [(ctx.case("M", dtype), [0])] + ([(ctx.case("L", dtype), [0, 10, 20, 30, 40, 50])] if dtype == "fp32" else [])
    for b, f in enumerate(tl.S_FRAMES):
        n = tl.rows_out(f)
        one = ctx.alone(b, dtype)
        assert one["layer4"].shape[1] == n
        ref = {"ctx": s["ctx"][b], "att_rb": s["att_rb"][b], "att_h": s["att_h"][b * H4:b * H4 + n], "layer4": s["layer4"][b, :n]}
        for name in ("layer4", "ctx", "att_rb"):
            assert bits(one[name][0][:n] if name == "layer4" else one[name][0], ref[name]), (b, name, "alone")
        assert bits(one["att_h"][:n], ref["att_h"]), (b, "att_h", "alone")
        for c, starts in others:
            for b0 in starts:
                assert bits(c["layer4"][b0 + b, :n], ref["layer4"]) and bits(c["ctx"][b0 + b], ref["ctx"]), (b, b0, "ctx")
                assert bits(c["att_rb"][b0 + b], ref["att_rb"]), (b, b0, "att_rb")
                assert bits(c["att_h"][(b0 + b) * H4:(b0 + b) * H4 + n], ref["att_h"]), (b, b0, "att_h")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_stale_rows_do_not_leak(ctx, dtype):
    """S after a call of the same shape whose utterances were all of full length with 1e30, then NaN, in the feature columns past S's
    lengths (and the same junk in S's own feature columns past each length): the layer-4 workspace then holds huge or non-finite rows past
    every short utterance's own, and ctx, att_rb and the own rows of att_h keep their bytes."""
    s = ctx.case("S", dtype)
    own = tl.own(s["layer4"], s["frames"])
    for junk in (1e30, float("nan")):
        feats, frames = tl.features("S", junk=junk)
        ctx.run(dtype, feats, [feats.shape[2]] * len(frames))
        got = ctx.run(dtype, feats, frames)
        pad = got["layer4"].reshape(-1, tl.D)[~own]
        assert bool((~torch.isfinite(pad) | (pad.abs() > 1e20)).any()), "the rows past the utterances' own hold nothing stale: the test shows nothing"
        assert bits(got["layer4"].reshape(-1, tl.D)[own], s["layer4"].reshape(-1, tl.D)[own]), junk
        assert bits(got["ctx"], s["ctx"]) and bits(got["att_rb"], s["att_rb"]), junk
        assert bits(got["att_h"][own], s["att_h"][own]), junk
