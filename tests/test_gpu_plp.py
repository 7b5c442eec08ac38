"""The PLP front end on the GPU (csrc/plp.hip ``sc_plp_cepstra``, sidekit_amd/plp.py) against the float64 evaluation of its formulas
(tests/tools/plp_f64.py, which tests/test_plp_reference_cpu.py pins to the reference) and the reference's own outputs
(tests/golden/plp.npz).

The kernel alone, on float32 operands both sides read: ``|got - want| <= 2^-23 max|want|`` over the row's output group (one float32
ulp of the group's largest value, for the rounding of the output) plus 16 times the deviation between two float64 evaluations of
different summation order that the golden generator recorded (2.805e-14; for ``post_spectrum``, which spans five decades, that term is
relative to the group's largest value too).

The chain end to end, per configuration and output (energy and cep absolute, post_spectrum relative to the frame's largest band): the
maximum deviation from the float64 evaluation on the float32 signal is at most 4 x the larger of the two CPU yardsticks the golden file
records for that configuration -- the reference's outputs rounded to float32 and a route with a single-precision FFT, float32 bank
sums and float32 logs before the float64 tail -- the rule and the rationale of tests/test_gpu_features_extractor.py: the head is
``sc_mfcc``, the same class of computation as the single-precision route, with a 1-ulp hardware log2, a float32 window and another
butterfly order; RASTA adds one rounding of its output to float32.

Measured on an MI355X (maximum over the rows of a configuration; the bound in brackets):
  configuration        energy             cep                post_spectrum
  0 (16 kHz)           1.01e-6 [4.50e-6]  9.08e-7 [2.27e-6]  5.12e-7 [1.95e-6]
  1 (16 kHz, RASTA)    1.01e-6 [4.50e-6]  3.46e-7 [9.52e-7]  3.25e-7 [1.11e-6]
  2 (8 kHz)            9.94e-7 [4.22e-6]  4.69e-7 [1.69e-6]  4.33e-7 [1.64e-6]
  3 (8 kHz, RASTA)     9.94e-7 [4.22e-6]  2.49e-7 [1.01e-6]  3.02e-7 [1.11e-6]
``extract_from_signal`` against the reference's outputs on the dithered signal: 1.91e-6 [5.57e-6], 2.79e-7 [1.08e-6], 3.15e-7 [1.16e-6].
The kernel alone reaches at most 0.49 of its bound (the rounding of the output to float32).  The bitwise tests are exact.
"""
import os
import sys
import wave

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plp_f64 as pf  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
FLOAT64_DEVIATION = 2.805e-14       # tests/test_plp_reference_cpu.py
SIZES = (1, 63, 64, 65, 257)        # rows of a launch: below, at and above one workgroup of 64, and four workgroups and one row
SHAPES = [(nb, order) for nb in (17, 21) for order in (1, 12, nb - 2)]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return numpy.load(os.path.join(golden_dir, "plp.npz"))


@pytest.fixture(scope="module")
def operands(golden):
    """nb -> (257 rows of log band energies rounded to float32, eql): a loud row of the configuration without RASTA alternating with
    a filtered row of the one with it, whose values lie around zero"""
    out = {}
    for nb, plain, filtered in ((21, 0, 1), (17, 2, 3)):
        x = numpy.empty((257, nb))
        x[0::2] = golden[f"c{plain}_r5_logband"][:129]
        x[1::2] = golden[f"c{filtered}_r6_logband"][3:131]       # the first of them is a row of zeros
        out[nb] = (x.astype(numpy.float32), golden[f"fs{pf.CONFIGS[plain]['fs']}_eql"])
    return out


def _launch(dev, x, eql, order, ldb=None, ldc=None, ldp=None, post=True):
    """sc_plp_cepstra through the C ABI -> (cep (N, ldc), post (N, ldp) or None), prefilled with SENTINEL; columns of x beyond nb hold
    a value no band holds"""
    import torch
    from sidekit_amd import _lib
    N, nb = x.shape
    ldb, ldc, ldp = ldb or nb, ldc or order + 1, ldp or nb
    xin = numpy.full((N, ldb), 7777.0, dtype=numpy.float32)
    xin[:, :nb] = x
    d_x = torch.from_numpy(xin).to(dev)
    tables = [torch.from_numpy(numpy.ascontiguousarray(t)).to(dev) for t in (eql, pf.acw_f64(nb, order), pf.lift_f64(order + 1))]
    cep = torch.full((N, ldc), SENTINEL, dtype=torch.float32, device=dev)
    out = torch.full((N, ldp), SENTINEL, dtype=torch.float32, device=dev) if post else None
    _lib.launch("sc_plp_cepstra", dev, d_x, ldb, N, nb, order, *tables, cep, ldc, out, ldp)
    torch.cuda.synchronize(dev)
    return cep.cpu().numpy(), None if out is None else out.cpu().numpy()


def _want(x, eql, order):
    nb = x.shape[1]
    return pf.plp_cepstra_f64(x.astype(numpy.float64), eql, pf.acw_f64(nb, order), pf.lift_f64(order + 1))


@pytest.mark.parametrize("nb,order", SHAPES)
def test_kernel_against_the_float64_evaluation_of_the_same_operands(gpu, operands, nb, order):
    x, eql = operands[nb]
    want_cep, want_post = _want(x, eql, order)
    assert numpy.isfinite(want_cep).all() and numpy.isfinite(want_post).all()
    worst = numpy.zeros(2)
    for N in SIZES:
        cep, post = _launch(gpu, x[:N], eql, order)
        assert cep.shape == (N, order + 1) and post.shape == (N, nb)
        for got, want, scaled in ((cep, want_cep[:N], False), (post, want_post[:N], True)):
            top = numpy.abs(want).max(axis=1, keepdims=True)
            bound = 2.0 ** -23 * top + 16 * FLOAT64_DEVIATION * (top if scaled else 1.0)
            excess = numpy.abs(got.astype(numpy.float64) - want) / bound
            worst[int(scaled)] = max(worst[int(scaled)], excess.max())
            assert numpy.all(excess <= 1.0), (N, "post" if scaled else "cep", float(excess.max()))
    print(f"nb {nb}, order {order}: largest deviation as a fraction of the bound: cep {worst[0]:.3f}, post {worst[1]:.3f}")


def test_leading_dimensions_null_post_and_a_frame_of_zero_power(gpu, operands):
    x, eql = operands[21]
    x, order = x[:130].copy(), 12
    cep, post = _launch(gpu, x, eql, order)
    wide_cep, wide_post = _launch(gpu, x, eql, order, ldb=24, ldc=order + 3, ldp=26)
    assert numpy.all(wide_cep[:, order + 1:] == SENTINEL) and numpy.all(wide_post[:, 21:] == SENTINEL), "columns beyond the outputs are untouched"
    assert wide_cep[:, :order + 1].tobytes() == cep.tobytes() and wide_post[:, :21].tobytes() == post.tobytes()
    assert numpy.all(cep != SENTINEL) and numpy.all(post != SENTINEL)
    alone, none = _launch(gpu, x, eql, order, post=False)
    assert none is None and alone.tobytes() == cep.tobytes(), "a null d_post is accepted"
    for row in (0, 63, 64, 129):
        silent = x.copy()
        silent[row] = -numpy.inf
        got_cep, got_post = _launch(gpu, silent, eql, order)
        assert numpy.isnan(got_cep[row]).all() and numpy.all(got_post[row] == 0.0), "zero power: NaN cepstra, a zero spectrum"
        keep = numpy.arange(130) != row
        assert got_cep[keep].tobytes() == cep[keep].tobytes() and got_post[keep].tobytes() == post[keep].tobytes(), "in its own row only"


@pytest.mark.parametrize("nb,order", [(17, 15), (21, 12)])
def test_bits_depend_on_the_row_alone(gpu, operands, nb, order):
    x, eql = operands[nb]
    cep, post = _launch(gpu, x, eql, order)
    again = _launch(gpu, x, eql, order)
    assert again[0].tobytes() == cep.tobytes() and again[1].tobytes() == post.tobytes(), "two runs"
    for row in (0, 1, 100, 256):
        one_cep, one_post = _launch(gpu, x[row:row + 1], eql, order)
        assert one_cep.tobytes() == cep[row:row + 1].tobytes() and one_post.tobytes() == post[row:row + 1].tobytes(), f"row {row} alone"
        same_cep, same_post = _launch(gpu, numpy.repeat(x[row:row + 1], 257, axis=0), eql, order)
        assert numpy.all(same_cep.view(numpy.uint32) == one_cep.view(numpy.uint32)) and numpy.all(same_post.view(numpy.uint32) == one_post.view(numpy.uint32)), \
            f"row {row} at every position of a batch of 257"
    for cut in (100, 64):
        head, tail = _launch(gpu, x[:cut], eql, order), _launch(gpu, x[cut:], eql, order)
        assert numpy.vstack((head[0], tail[0])).tobytes() == cep.tobytes() and numpy.vstack((head[1], tail[1])).tobytes() == post.tobytes(), f"cut at {cut}"


class Case:
    """One configuration: its rows, its float64 evaluation (computed once) and yardsticks"""

    def __init__(self, c, golden):
        self.c, self.cfg = c, pf.CONFIGS[c]
        self.nb, self.nceps = pf.bands(self.cfg), self.cfg["nceps"]
        self.D = 1 + self.nceps + self.nb
        self.rows = pf.signals(self.cfg, int(golden[f"c{c}_seed"]))
        self.bank32, self.eql = golden[f"fs{self.cfg['fs']}_bank"].astype(numpy.float32), golden[f"fs{self.cfg['fs']}_eql"]
        self.want = [pf.plp_f64(r.astype(numpy.float32), self.cfg, self.bank32, self.eql) for r in self.rows]
        self.counts = [w[0].shape[0] for w in self.want]
        self.yard = numpy.maximum(golden[f"c{c}_yard_reference"].max(axis=0), golden[f"c{c}_yard_single"].max(axis=0))

    def options(self):
        return dict(fs=self.cfg["fs"], nwin=self.cfg["nwin"], nceps=self.nceps, shift=self.cfg["shift"], prefac=pf.PREFAC, rasta=self.cfg["rasta"])

    def extractor(self, **kw):
        from sidekit_amd.plp import PlpExtractor
        return PlpExtractor(sampling_frequency=self.cfg["fs"], window_size=self.cfg["nwin"], shift=self.cfg["shift"], ceps_number=self.nceps,
                            pre_emphasis=pf.PREFAC, rasta_plp=self.cfg["rasta"], **kw)


@pytest.fixture(scope="module")
def cases(golden):
    return [Case(c, golden) for c in range(len(pf.CONFIGS))]


def _batch(rows, dtype, dev, pad=3):
    """rows -> (wav (B, L) on the device, its tail filled with a value no row holds; nsamples)"""
    import torch
    L = max(r.shape[0] for r in rows) + pad
    wav = numpy.full((len(rows), L), 7777, dtype=dtype)
    for i, r in enumerate(rows):
        wav[i, :r.shape[0]] = r
    return torch.from_numpy(wav).to(dev), torch.tensor([r.shape[0] for r in rows], dtype=torch.int32, device=dev)


@pytest.mark.parametrize("c", range(len(pf.CONFIGS)))
def test_chain_against_the_float64_evaluation(gpu, cases, c):
    from sidekit_amd.plp import plp_device
    case = cases[c]
    assert case.counts[:5] == [0, 1, 1, 2, 5] and 257 <= case.counts[5] == case.counts[6] <= 259, "RASTA segments of 0, 1, 2 and 5 frames are among the rows"
    wav, lens = _batch(case.rows, numpy.int16, gpu)
    frames, off = plp_device(wav, lens, **case.options())
    assert frames.shape == (sum(case.counts), case.D) and off.cpu().tolist() == numpy.concatenate(([0], numpy.cumsum(case.counts))).tolist()
    out, off = frames.cpu().numpy(), off.cpu().numpy()
    assert numpy.isfinite(out).all()
    worst = numpy.zeros(3)
    for r, want in enumerate(case.want):
        rows = out[off[r]:off[r + 1]]
        worst = numpy.maximum(worst, pf.deviations((rows[:, 0], rows[:, 1:1 + case.nceps], rows[:, 1 + case.nceps:]), want))
        if case.cfg["rasta"] and rows.shape[0]:
            lead = rows[:4, 1:]
            assert numpy.all(lead == lead[0]), "the four leading frames of a segment hold the outputs of a flat spectrum"
    print(f"configuration {c} (fs {case.cfg['fs']}, rasta {case.cfg['rasta']}): energy / cep / post deviation from float64 {worst}, bound {4 * case.yard}")
    assert numpy.all(worst <= 4 * case.yard), (worst, 4 * case.yard)
    # a float batch holding the same integers, alone and shuffled: the same bits
    order = [5, 0, 3, 6, 1, 4, 2]
    wav, lens = _batch([case.rows[i].astype(numpy.float32) for i in order], numpy.float32, gpu)
    shuffled, soff = plp_device(wav, lens, **case.options())
    shuffled, soff = shuffled.cpu().numpy(), soff.cpu().numpy()
    for pos, r in enumerate(order):
        assert shuffled[soff[pos]:soff[pos + 1]].tobytes() == out[off[r]:off[r + 1]].tobytes(), f"row {r} in a shuffled batch"


def test_extract_from_signal_reproduces_the_reference(gpu, cases, golden):
    from sidekit_amd.frontend import features as fe
    case, g = cases[1], golden
    sig = case.rows[5].astype(numpy.float32)
    keep = sig.copy()
    label, energy, cep, post = case.extractor().extract_from_signal(sig, 16000)
    assert numpy.array_equal(sig, keep), "the caller's signal is not written"
    assert label.dtype == bool and label.all() and numpy.array_equal(label, g["surface_none_label"])
    assert energy.dtype == cep.dtype == post.dtype == numpy.float32
    assert (energy.shape, cep.shape, post.shape) == (g["surface_energy"].shape, g["surface_cep"].shape, g["surface_post"].shape)
    bound = 4 * case.yard + g["surface_yard_reference"]
    dev = pf.deviations((energy, cep, post), tuple(g[k].astype(numpy.float64) for k in ("surface_energy", "surface_cep", "surface_post")))
    print(f"extract_from_signal: energy / cep / post deviation from the reference {dev}, bound {bound}")
    assert numpy.all(numpy.array(dev) <= bound), (dev, bound)
    label = case.extractor(vad="energy").extract_from_signal(sig[:, None], 16000)[0]
    assert 0 < label.sum() < label.shape[0] and numpy.array_equal(label, g["surface_energy_label"])
    # the numpy front door on the undithered signal: the same kernels, so the same bits as the resident batch
    from sidekit_amd.plp import plp_device
    wav, lens = _batch([case.rows[4]], numpy.int16, gpu)
    want = plp_device(wav, lens, **case.options())[0].cpu().numpy()
    ceps, le, spec, mspec = fe.plp(case.rows[4], get_spec=True, get_mspec=True)
    assert ceps.tobytes() == want[:, 1:14].tobytes() and le.tobytes() == want[:, 0].tobytes() and mspec.tobytes() == want[:, 14:].tobytes()
    assert spec.shape == (5, 257) and spec.tobytes() == fe.power_spectrum(case.rows[4], fs=16000)[0].tobytes()
    assert fe.plp(case.rows[4].astype(numpy.float32), rasta=False)[2:] == [None, None]
    assert fe.plp(case.rows[1])[0].shape == (1, 13) and fe.plp(case.rows[0])[0].shape == (0, 13)


def test_features_server_loads_from_wav_files_what_the_resident_path_computes(gpu, cases, tmp_path):
    import torch
    from sidekit_amd.features_extractor import dither
    from sidekit_amd.features_server import FeaturesServer, post_process_device
    case = cases[1]
    shows = {"a": case.rows[5], "c": case.rows[6]}
    for show, pcm in shows.items():
        with wave.open(str(tmp_path / (show + ".wav")), "wb") as w:
            w.setnchannels(1), w.setsampwidth(2), w.setframerate(16000)
            w.writeframes(pcm.astype("<i2").tobytes())
    fx = case.extractor(audio_filename_structure=str(tmp_path / "{}.wav"), vad="energy")
    opts = dict(feat_norm="cmvn", delta=True)
    server = FeaturesServer(features_extractor=fx, **opts)
    for show, pcm in shows.items():
        feat, label = server.load(show)
        wav, lens = _batch([dither(pcm)], numpy.float32, gpu, pad=0)
        frames, off, labels = fx.extract_batch_device(wav, lens)
        want, want_labels, _ = post_process_device(frames, off, labels, **opts)
        assert feat.shape == (case.counts[5], 2 * case.D) and numpy.isfinite(feat).all() and 1 < label.sum() < label.shape[0]
        assert numpy.array_equal(feat.astype(numpy.float32), want.cpu().numpy()) and numpy.array_equal(label, want_labels.cpu().numpy()), show
    feat, label, mean, std = fx.extract("a", 0)
    assert feat.shape == (case.counts[5], case.D) and 0 < label.sum() < label.shape[0] and mean.shape == std.shape == (case.D,)
    only = case.extractor(audio_filename_structure=str(tmp_path / "{}.wav"), save_param=["cep", "vad"]).extract("a", 0)
    assert only[0].shape == (case.counts[5], case.nceps) and only[1].all()
    frames, off = FeaturesServer(features_extractor=fx, keep_all_features=False, **opts).stack_features_device(list(shows))
    assert frames.is_cuda and frames.dtype == torch.float32 and frames.shape[1] == 2 * case.D and len(off) == 3 and off[-1] == frames.shape[0]
