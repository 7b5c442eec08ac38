"""tests/tools/plp_f64.py -- the float64 restatement of the formulas of include/sidekit_amd/plp.h, which the GPU tests hold the kernel
to -- pinned to what the reference's ``plp`` computes (tests/golden/plp.npz, written by tests/golden/make_plp_golden.py).

Both are float64 evaluations of the same operands (``logband``: the reference's log critical-band energies as they enter the
exponential, after its RASTA filter where the configuration has one).  They differ in the order of their sums only: the reference
takes the autocorrelation from ``numpy.fft.ifft`` of the mirrored spectrum, divides the LPC polynomial by the error and multiplies it
back, and takes ``-log(1 / e)`` for ``log(e)``.  The generator measured the largest deviation over every recorded row: 2.805e-14, on
cepstra of magnitude up to 6 (absolute) and on ``post_spectrum`` relative to each frame's largest band (7.7e-16 there).  The bound is
16 times that, 4.5e-13, rounded up to a power of ten: 1e-12.
"""
import os
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

import plp_f64 as pf  # noqa: E402

GOLDEN = numpy.load(os.path.join(ROOT, "tests", "golden", "plp.npz"))
MEASURED, BOUND = 2.805e-14, 1e-12
RECORDED = (3, 4, 5, 6)        # the rows with at least two frames: the reference cannot be called below


def test_the_bound_is_sixteen_times_the_recorded_deviation_rounded_up_to_a_power_of_ten():
    assert float(GOLDEN["float64_deviation"]) == pytest.approx(MEASURED, rel=1e-3)
    assert BOUND == 10.0 ** numpy.ceil(numpy.log10(16 * float(GOLDEN["float64_deviation"])))


@pytest.mark.parametrize("c", range(len(pf.CONFIGS)))
def test_float64_restatement_reproduces_the_reference(c):
    cfg = pf.CONFIGS[c]
    nb, nceps = pf.bands(cfg), cfg["nceps"]
    eql = GOLDEN[f"fs{cfg['fs']}_eql"]
    acw, lift = pf.acw_f64(nb, nceps - 1), pf.lift_f64(nceps)
    rows = pf.signals(cfg, int(GOLDEN[f"c{c}_seed"]))
    counts = [pf.mf.n_frames(r.shape[0], pf.head_cfg(cfg)) for r in rows]
    assert counts[:5] == [0, 1, 1, 2, 5] and 257 <= counts[5] == counts[6] <= 259
    worst = [0.0, 0.0]
    for r in RECORDED:
        logband, want_cep, want_post = (GOLDEN[f"c{c}_r{r}_{k}"] for k in ("logband", "cep", "post"))
        assert logband.dtype == want_cep.dtype == want_post.dtype == numpy.float64
        assert logband.shape == (counts[r], nb) == want_post.shape and want_cep.shape == (counts[r], nceps)
        assert numpy.isfinite(want_cep).all() and numpy.isfinite(want_post).all()
        cep, post = pf.plp_cepstra_f64(logband, eql, acw, lift)
        worst[0] = max(worst[0], float(numpy.abs(cep - want_cep).max()))
        worst[1] = max(worst[1], float((numpy.abs(post - want_post).max(axis=1) / want_post.max(axis=1)).max()))
    print(f"configuration {c}: cep deviation {worst[0]:.3e}, post deviation relative to the frame's largest band {worst[1]:.3e}, bound {BOUND:.0e}")
    assert max(worst) <= BOUND, worst


@pytest.mark.parametrize("c", [c for c, cfg in enumerate(pf.CONFIGS) if cfg["rasta"]])
def test_the_four_leading_rasta_frames_of_a_segment_are_constant_rows(c):
    """``rasta_filt`` outputs zeros for the first four frames, so the reference's outputs there are those of a flat spectrum"""
    cfg = pf.CONFIGS[c]
    eql = GOLDEN[f"fs{cfg['fs']}_eql"]
    flat_cep, flat_post = pf.plp_cepstra_f64(numpy.zeros((1, pf.bands(cfg))), eql, pf.acw_f64(pf.bands(cfg), cfg["nceps"] - 1), pf.lift_f64(cfg["nceps"]))
    for r in RECORDED:
        logband, cep, post = (GOLDEN[f"c{c}_r{r}_{k}"] for k in ("logband", "cep", "post"))
        lead = min(4, logband.shape[0])
        assert numpy.all(logband[:lead] == 0.0)
        assert numpy.all(cep[:lead] == cep[0]) and numpy.all(post[:lead] == post[0])
        assert numpy.abs(cep[0] - flat_cep[0]).max() <= BOUND and numpy.abs(post[0] - flat_post[0]).max() <= BOUND * post[0].max()
        if logband.shape[0] > 4:
            assert numpy.all(numpy.abs(logband[4:]).max(axis=1) > 0) and not numpy.all(cep[4] == cep[0])


def test_the_yardsticks_are_recorded_for_every_row():
    for c in range(len(pf.CONFIGS)):
        ref, single = GOLDEN[f"c{c}_yard_reference"], GOLDEN[f"c{c}_yard_single"]
        assert ref.shape == single.shape == (7, 3)
        assert not ref[:3].any() and ref[3:].all(), "the reference runs from two frames on"
        assert not single[0].any() and single[1:, 0].all()
        assert max(ref.max(), single.max()) < 3e-5
