"""The float64 reference of one trunk block (tests/tools/trunk_f64.py) without a GPU: pinned to the oracle, and shown not to carry noise of
its own into the bounds tests/test_gpu_trunk_blocks.py states."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import trunk_f64 as tf  # noqa: E402

from oracle import xvector as oxv  # noqa: E402

FLIP_CAP = 5e-3          # the cap tests/test_gpu_trunk_blocks.py puts on the share of bf16 elements that differ from bf16(float64)


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / b.norm()).item()


def test_chained_blocks_reproduce_the_oracle_taps():
    """Every rounding switched off, the three functions chained over all 16 blocks from the oracle's stem tap give the oracle's layer1 .. layer4
    taps on a ragged pair of 9 and 37 frames (each utterance's oracle run alone), within 1e-5 norm-relative: the oracle runs in float32."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = tf.operand_state_dict()
    frames = [9, 37]
    feats = torch.randn(2, 80, 37, generator=torch.Generator().manual_seed(3))
    taps = []
    with torch.no_grad():
        for b, n in enumerate(frames):
            t = {}
            oxv.halfresnet34_from_feats(feats[b:b + 1, :, :n], sd, taps=t)
            taps.append(t)
    x = torch.zeros(2, 37, 80, 32, dtype=torch.float64)
    for b, n in enumerate(frames):
        x[b, :n] = taps[b]["stem"][0].permute(1, 2, 0).double()
    stem = tf.stem_ref(feats, sd, frames)
    for b, n in enumerate(frames):
        assert rel(stem[b, :n], x[b, :n]) < 1e-5, ("stem", b)
    for block in range(16):
        g = tf.Geom(block)
        o1 = tf.conv1_ref(x, sd, block, frames, "fp32")
        gate = tf.gate_ref(o1, sd, block, frames, "fp32")
        x, _ = tf.conv2_ref(o1, gate, x, sd, block, frames, "fp32")
        if block + 1 == 16 or tf.Geom(block + 1).li != g.li:
            for b, n in enumerate(frames):
                ref = taps[b][f"layer{g.li + 1}"][0].permute(1, 2, 0)
                rows = g.rows_out(n)
                assert ref.shape[0] == rows
                err = rel(x[b, :rows], ref)
                assert err < 1e-5, (block, b, err)
                assert float(x[b, rows:].abs().max() if rows < x.shape[1] else 0.0) == 0.0


def _ulp_steps(a, b):
    """distance of two bf16-representable tensors in bf16 steps (sign-magnitude order)"""
    def key(t):
        i = t.float().bfloat16().view(torch.int16).int()
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()


@pytest.mark.parametrize("block", [1, 4, 8, 14])
def test_float32_arithmetic_alone_flips_few_bf16_roundings(block, capsys):
    """torch's own float32 evaluation of conv1 and of the block output against the float64 one, both rounded to bf16, on the ragged batch the GPU
    test of this block runs: the share of differing elements stays under an eighth of that test's cap -- the cap is not hiding
    the reference's own noise.  (Random operands at C = 32 / 128 / 256 gave 0, 7.2e-5, 5.1e-5.)  Nearly all of them differ by one step; the
    exceptions are sums that cancel to almost nothing, where a float32 error of 1e-7 is several steps of a value of 1e-6 (printed).  The GPU
    test's per-element rule has a clause for exactly those elements."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = tf.operand_state_dict()
    g = tf.Geom(block)
    frames = tf.frames_for_rows(block, tf.ragged_rows(block, "bf16"))
    x = tf.block_input(block, frames, "bf16", seed=1)
    shares, worst = [], 0
    o1_64 = tf.conv1_ref(x, sd, block, frames, "bf16")
    o1_32 = tf.conv1_ref(x, sd, block, frames, "bf16", prec=torch.float32)
    o1 = tf.bf16r(o1_64)
    gate = tf.gate_ref(o1, sd, block, frames, "bf16").float()
    out64, _ = tf.conv2_ref(o1, gate, x, sd, block, frames, "bf16")
    out32, _ = tf.conv2_ref(o1, gate, x, sd, block, frames, "bf16", prec=torch.float32)
    for name, a, b in (("o1", o1_32, o1_64), ("out", out32, out64)):
        steps = torch.cat([_ulp_steps(a[i, :g.rows_out(f)], b[i, :g.rows_out(f)]).flatten() for i, f in enumerate(frames)])
        share = (steps != 0).double().mean().item()
        shares.append(share)
        worst = max(worst, int(steps.max()))
        assert share < FLIP_CAP / 8, (name, share)
    with capsys.disabled():
        print(f"  [block {block}: float32-alone flip share o1 {shares[0]:.1e}, out {shares[1]:.1e}, largest distance {worst} bf16 steps]", end="")
