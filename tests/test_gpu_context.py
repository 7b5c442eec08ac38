"""Context features on the GPU (sidekit_amd/features_context.py, csrc/context.hip) against the reference's own output
(tests/golden/context.npz) and the numpy restatement of the formulas (tests/tools/context_numpy.py, pinned to the reference by
tests/test_context_cpu.py).

One stacked batch per D = 5 and 13 (W D is then no multiple of the 16-wide k-step and pairs straddle frame ends): the fixture's streams
of 2, 3, 7, 40, 256, 257 and 300 rows between segments of 0, 1, L, L + R + 1 and 255 rows for the windows (3, 2) and (12, 12); the tiles
are 256 (gather), 128 (basis) and 64 rows (projection).  Stacked context and SDC are bit-equal to the fixture and the restatement.  The
two float64 kernels are held against the float64 evaluation ref64 of the same float32 operands:
    |y - ref64| <= 2^-24 |ref64| (1 + 2^-20) + K 2^-52 S_abs,   S_abs = sum_k |a_k m_k|, K the number of terms:
the single rounding to float32 (the factor 1 + 2^-20 covers that the rounding is of the computed sum, not of ref64) and the float64
accumulation of K products (each product and each partial sum within 2^-53 relative, K of each).  The bitwise tests are exact.
"""
import os
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import context_numpy as cn  # noqa: E402

pytestmark = pytest.mark.gpu
EXTRA = (0, 1, 3, 6, 12, 25, 255)        # empty, one row, L and L + R + 1 of (3, 2) and (12, 12), one row short of the gather tile


@pytest.fixture(scope="module")
def fx(golden_dir):
    with numpy.load(os.path.join(golden_dir, "context.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def fc():
    import sidekit_amd.features_context as fc
    return fc


class Batch:
    """The fixture's streams with the extra segments between them, resident"""

    def __init__(self, fx, D):
        import torch
        rs = numpy.random.RandomState(100 + D)
        golden = cn.split(fx["x_D%d" % D], cn.LENGTHS)
        extra = [(2.0 * rs.randn(n, D) + rs.randn(D)).astype(numpy.float32) for n in EXTRA]
        self.segments, self.golden_at = [], {}
        for g, e in zip(golden, extra):
            self.segments.append(e)
            self.golden_at[g.shape[0]] = len(self.segments)
            self.segments.append(g)
        self.D = D
        self.x = numpy.concatenate(self.segments)
        self.off = numpy.concatenate(([0], numpy.cumsum([s.shape[0] for s in self.segments]))).astype(numpy.int64)
        self.dev = torch.as_tensor(self.x).cuda()
        wide = torch.full((self.x.shape[0], D + 4), 7.0, dtype=torch.float32, device="cuda")
        wide[:, 3:3 + D] = self.dev
        self.block = wide[:, 3:3 + D]          # the same frames as a column block: ldx = D + 4, rows 4-byte aligned only

    def cut(self, a):
        a = a.cpu().numpy() if hasattr(a, "cpu") else a
        return [a[self.off[i]:self.off[i + 1]] for i in range(len(self.segments))]


@pytest.fixture(scope="module")
def batches(fx):
    return {D: Batch(fx, D) for D in cn.DIMS}


def _golden(fx, name):
    kind, D, lengths, cfg = cn.cases()[name]
    return dict(zip(lengths, cn.split(fx[name], lengths)))


def _bound(ref64, s_abs, K):
    return 2.0 ** -24 * numpy.abs(ref64) * (1 + 2.0 ** -20) + K * 2.0 ** -52 * s_abs


def _within(got, ref64, s_abs, K, what):
    assert got.dtype == numpy.float32 and got.shape == ref64.shape, what
    if got.size:
        excess = numpy.abs(got.astype(numpy.float64) - ref64) - _bound(ref64, s_abs, K)
        assert excess.max() <= 0, (what, float(excess.max()))


def test_stacked_context_and_sdc_are_bit_equal(fx, fc, batches):
    import torch
    for D, b in batches.items():
        for cfg in cn.SDC:
            frames = b.block if cfg == (1, 3, 7) else b.dev
            got = b.cut(fc.sdc_device(frames, b.off, *cfg))
            for i, s in enumerate(b.segments):
                assert got[i].dtype == numpy.float32 and (numpy.array_equal(got[i], cn.sdc(s, *cfg)) if s.shape[0] else got[i].shape == (0, D * (cfg[2] + 1))), (cfg, D, i)
            for n, ref in _golden(fx, "sdc_%d_%d_%d_D%d" % (cfg + (D,))).items():
                assert numpy.array_equal(got[b.golden_at[n]], ref), ("sdc against the reference", cfg, D, n)
        for win in cn.WINDOWS:
            W = win[0] + win[1] + 1
            wide = torch.full((b.x.shape[0], W * D + 5), -3.0, dtype=torch.float32, device="cuda")
            out = fc.context_device(b.block if win == (3, 2) else b.dev, b.off, win[0], win[1], out=wide[:, 2:2 + W * D])
            assert out.data_ptr() == wide[:, 2:].data_ptr() and bool((wide[:, :2] == -3.0).all()) and bool((wide[:, 2 + W * D:] == -3.0).all()), \
                "out as a column block: nothing beside it is written"
            got = b.cut(out)
            for i, s in enumerate(b.segments):
                if s.shape[0]:
                    assert numpy.array_equal(got[i], cn.context(s, *win)), (win, D, i)
            name = "ctx_%d_%d_D%d" % (win + (D,))
            if name in cn.cases():
                for n, ref in _golden(fx, name).items():
                    assert numpy.array_equal(got[b.golden_at[n]], ref), ("context against the reference", win, D, n)


def test_temporal_basis_against_float64(fx, fc, batches):
    """sc_ctx_basis: the DCT of pca_dct without a projection, and TRAPs; K = W terms"""
    import torch
    for D, b in batches.items():
        # out as a column block (ldy > D J), from a column block: the same bits, nothing beside it written
        H = fc.traps_basis(3, 2, 4)
        wide = torch.full((b.x.shape[0], 4 * D + 7), -9.0, dtype=torch.float32, device="cuda")
        out = fc.basis_device(b.block, b.off, H, 3, out=wide[:, 3:3 + 4 * D])
        assert out.data_ptr() == wide[:, 3:].data_ptr() and bool((wide[:, :3] == -9.0).all()) and bool((wide[:, 3 + 4 * D:] == -9.0).all())
        assert torch.equal(out, fc.traps_device(b.dev, b.off, 3, 2, 4))
        for win in cn.WINDOWS:
            B = cn.dct_pca_basis(*win)
            got = b.cut(fc.pca_dct_device(b.block if win == (12, 12) else b.dev, b.off, win[0], win[1]))
            for i, s in enumerate(b.segments):
                if s.shape[0]:
                    _within(got[i], cn.basis_map(s, fc.dct_pca_basis(*win), win[0]), cn.basis_abs(s, B, win[0]), B.shape[0], ("dct", win, D, i))
                else:
                    assert got[i].shape == (0, D * B.shape[0])
        for left, right, nb in ((3, 2, 4), (12, 12, 16), (12, 12, 4), (0, 2, 3)):
            H = fc.traps_basis(left, right, nb)
            got = b.cut(fc.traps_device(b.dev, b.off, left, right, nb))
            for i, s in enumerate(b.segments):
                if s.shape[0]:
                    _within(got[i], cn.basis_map(s, H, left), cn.basis_abs(s, H, left), H.shape[0], ("traps", left, right, nb, D, i))


PROJECTIONS = ((12, 12, 5, 7), (12, 12, 5, 40), (3, 2, 13, 7), (0, 2, 13, 40))


def test_windowed_projection_against_float64(fx, fc, batches):
    """sc_ctx_project: K = W D terms; Q = 7 and 40 leave partial column tiles; the column block has odd row starts (no 8-byte pairs)"""
    import torch
    for left, right, D, Q in PROJECTIONS:
        b, W = batches[D], left + right + 1
        P = fx[cn.pca_name(left, right, D, Q)]
        M = fc.projection_matrix(fc.dct_pca_basis(left, right), P, D)
        wide = torch.full((b.x.shape[0], Q + 3), 5.0, dtype=torch.float32, device="cuda")
        outs = [fc.pca_dct_device(b.dev, b.off, left, right, P), fc.pca_dct_device(b.block, b.off, left, right, P),
                fc.project_device(b.dev, b.off, M, W, left, out=wide[:, 1:1 + Q])]
        assert bool((wide[:, 0] == 5.0).all()) and bool((wide[:, 1 + Q:] == 5.0).all()), "out as a column block: nothing beside it is written"
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "the same bits from a column block, and into one"
        got = b.cut(outs[0])
        for i, s in enumerate(b.segments):
            if s.shape[0]:
                ref64, s_abs = cn.project(s, M, W, left)
                _within(got[i], ref64, s_abs, W * D, ("project", left, right, D, Q, i))
            else:
                assert got[i].shape == (0, Q)
        # the reference's two-step result, which the restatement meets within 1e-12 relative (tests/test_context_cpu.py)
        name = "pca_%d_%d_D%d_Q%d" % (left, right, D, Q)
        for n, ref in _golden(fx, name).items():
            s = b.segments[b.golden_at[n]]
            _, s_abs = cn.project(s, M, W, left)
            excess = numpy.abs(got[b.golden_at[n]] - ref) - _bound(ref, s_abs, W * D) - 1e-12 * max(numpy.abs(ref).max(), 1.0)
            assert excess.max() <= 0, (name, n, float(excess.max()))


def test_a_workgroup_that_walks_several_tiles_gives_the_same_bits(fx, fc, batches):
    """max_rows sizes grid.z and nothing else.  With max_rows = 1 there is one workgroup per segment and column chunk, which walks all the
    tiles of its segment (up to 2, 3 and 5 for the 300-row stream; 5, 9 and 18 for the 1100-row one) through the loop that stages LDS
    again behind a barrier -- what every batch of 8 192 segments or more does.  The bits are those of the default grid, where no
    workgroup takes a second tile, and for the gather those of the reference."""
    import torch
    rs = numpy.random.RandomState(3)
    long = (rs.randn(1100, 5) + numpy.arange(1100)[:, None] * 0.01).astype(numpy.float32)
    long_dev = torch.as_tensor(long).cuda()
    for D, b in batches.items():
        plus, minus = fc.sdc_offsets(1, 3, 7)
        for frames, off in ((b.dev, b.off), (b.block, b.off)) + (((long_dev, None),) if D == 5 else ()):
            one = fc.gather_device(frames, off, plus, minus, max_rows=1)
            assert torch.equal(one, fc.gather_device(frames, off, plus, minus)), ("sdc", D)
            ctx = fc.gather_device(frames, off, fc.context_offsets(12, 12), max_rows=1)
            assert torch.equal(ctx, fc.gather_device(frames, off, fc.context_offsets(12, 12))), ("context", D)
            B = fc.dct_pca_basis(12, 12)
            assert torch.equal(fc.basis_device(frames, off, B, 12, max_rows=1), fc.basis_device(frames, off, B, 12)), ("basis", D)
            left, right, Q = (12, 12, 40) if D == 5 else (3, 2, 7)
            M = fc.projection_matrix(fc.dct_pca_basis(left, right), fx[cn.pca_name(left, right, D, Q)], D)
            W = left + right + 1
            assert torch.equal(fc.project_device(frames, off, M, W, left, max_rows=1), fc.project_device(frames, off, M, W, left)), ("project", D)
            assert torch.equal(fc.project_device(frames, off, M, W, left, max_rows=100), fc.project_device(frames, off, M, W, left)), "a bound in between"
        got = b.cut(fc.gather_device(b.dev, b.off, plus, minus, max_rows=1))
        for n, ref in _golden(fx, "sdc_1_3_7_D%d" % D).items():
            assert numpy.array_equal(got[b.golden_at[n]], ref[:, D:]), ("sdc with one workgroup a segment against the reference", D, n)
    walked = fc.gather_device(long_dev, None, *fc.sdc_offsets(1, 3, 7), max_rows=1).cpu().numpy()
    assert numpy.array_equal(walked, cn.sdc(long, 1, 3, 7)[:, 5:]), "five tiles of the gather in one workgroup, against the restatement"
    H = cn.traps_basis(12, 12, 16)
    _within(fc.basis_device(long_dev, None, H, 12, max_rows=1).cpu().numpy(), cn.basis_map(long, H, 12), cn.basis_abs(long, H, 12), 25, "nine tiles of the basis")
    with pytest.raises(ValueError, match="max_rows"):
        fc.gather_device(long_dev, None, plus, minus, max_rows=0)


def test_a_tensor_is_the_pca_matrix_itself(fx, fc, batches):
    """``p`` is the reference's P whether it comes as a host array or as a tensor, resident or not"""
    import torch
    b = batches[5]
    P = fx[cn.pca_name(12, 12, 5, 7)]
    ref = fc.pca_dct_device(b.dev, b.off, 12, 12, P)
    assert torch.equal(fc.pca_dct_device(b.dev, b.off, 12, 12, torch.as_tensor(P)), ref)
    assert torch.equal(fc.pca_dct_device(b.dev, b.off, 12, 12, torch.as_tensor(P).cuda()), ref)
    out, _, _ = fc.post_process_context_device(b.dev, b.off, dct_pca=True, dct_pca_config=(12, 12, torch.as_tensor(P).cuda()))
    assert torch.equal(out, ref)


def test_a_segment_has_the_same_bits_alone_anywhere_and_again(fx, fc, batches):
    import torch
    b = batches[13]
    P = fx[cn.pca_name(3, 2, 13, 7)]
    ops = {"sdc": lambda x, off: fc.sdc_device(x, off, 1, 3, 7), "context": lambda x, off: fc.context_device(x, off, 12, 12),
           "dct": lambda x, off: fc.pca_dct_device(x, off, 12, 12), "traps": lambda x, off: fc.traps_device(x, off, 3, 2, 4),
           "project": lambda x, off: fc.pca_dct_device(x, off, 3, 2, P)}
    order = list(reversed(range(len(b.segments))))
    moved = torch.as_tensor(numpy.concatenate([b.segments[i] for i in order])).cuda()
    moved_off = numpy.concatenate(([0], numpy.cumsum([b.segments[i].shape[0] for i in order]))).astype(numpy.int64)
    for name, op in ops.items():
        whole = op(b.dev, b.off)
        assert torch.equal(whole, op(b.dev, b.off)), (name, "a second run gives the same bits")
        parts = b.cut(whole)
        again = op(moved, moved_off).cpu().numpy()
        for slot, i in enumerate(order):
            assert numpy.array_equal(again[moved_off[slot]:moved_off[slot + 1]], parts[i]), (name, "elsewhere in the batch", i)
        for i, s in enumerate(b.segments):
            if s.shape[0]:
                assert numpy.array_equal(op(torch.as_tensor(s).cuda(), None).cpu().numpy(), parts[i]), (name, "alone", i)


def _same_bits(a, b):
    """bit for bit, NaNs included (cmvn of a segment with one labelled row divides zero by zero)"""
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_post_process_context_device(fx, fc, batches):
    import torch
    from sidekit_amd.features_server import post_process_device
    b = batches[5]
    rs = numpy.random.RandomState(7)
    labels = torch.as_tensor(rs.rand(b.x.shape[0]) < 0.7).cuda()
    options = dict(rasta=True, delta=True, double_delta=True, feat_norm="cmvn", keep_all_features=False)
    for extra in (dict(), dict(dct_pca=True, sdc=True), dict(sdc=True, sdc_config=(2, 2, 3))):      # deltas come first: the others are ignored
        for got, ref in zip(fc.post_process_context_device(b.dev, b.off, labels, **extra, **options), post_process_device(b.dev, b.off, labels, **options)):
            assert _same_bits(got, ref), "with neither option in effect: post_process_device, bit for bit"
    for got, ref in zip(fc.post_process_context_device(b.dev, b.off, labels, feat_norm="stg", win=21), post_process_device(b.dev, b.off, labels, feat_norm="stg", win=21)):
        assert _same_bits(got, ref)
    # RASTA + SDC + cmvn + selection = the composition of the stages
    out, lab, off = fc.post_process_context_device(b.dev, b.off, labels, sdc=True, sdc_config=(1, 3, 7), rasta=True, feat_norm="cmvn", keep_all_features=False)
    x1, lab1, off1 = post_process_device(b.dev, b.off, labels, rasta=True)
    staged = numpy.concatenate([cn.sdc(s, 1, 3, 7) if s.shape[0] else numpy.zeros((0, 40), dtype=numpy.float32) for s in b.cut(x1)])
    ref, rlab, roff = post_process_device(torch.as_tensor(staged).cuda(), off1, lab1, feat_norm="cmvn", keep_all_features=False)
    assert out.shape[1] == 40 and _same_bits(out, ref) and torch.equal(lab, rlab) and torch.equal(off, roff)
    assert int(off[-1]) == out.shape[0] == int(lab1.sum())
    # dct_pca goes before sdc, and the mask follows it
    P = fx[cn.pca_name(12, 12, 5, 7)]
    out, _, _ = fc.post_process_context_device(b.dev, b.off, labels, dct_pca=True, dct_pca_config=(12, 12, P), sdc=True, mask=[0, 2, 6])
    assert torch.equal(out, fc.pca_dct_device(b.dev, b.off, 12, 12, P)[:, [0, 2, 6]])


class Source:
    def __init__(self, shows):
        self.shows = shows

    def extract(self, show, channel, input_audio_filename=None):
        return self.shows[show]


def test_context_features_server(fx, fc, batches):
    b = batches[5]
    rs = numpy.random.RandomState(11)
    shows = {str(n): (b.segments[b.golden_at[n]], rs.rand(n) < 0.8) for n in (40, 256, 300)}      # long enough that no SDC block is constant (cmvn would divide zero by zero)
    P = fx[cn.pca_name(12, 12, 5, 7)]
    for kw in (dict(sdc=True, rasta=True, feat_norm="cmvn", keep_all_features=False), dict(dct_pca=True, dct_pca_config=(12, 12, P), feat_norm="cms"),
               dict(dct_pca=True, dct_pca_config=(3, 2, None), sdc=True), dict(sdc=True, delta=True)):
        server = fc.ContextFeaturesServer(features_extractor=Source(shows), **kw)
        frames, off = server.stack_features_device(list(shows))
        stacked = server.stack_features(list(shows))
        assert numpy.isfinite(stacked).all() and numpy.array_equal(frames.cpu().numpy(), stacked.astype(numpy.float32))
        for i, show in enumerate(shows):
            feat, label = server.load(show)
            assert numpy.array_equal(frames[off[i]:off[i + 1]].cpu().numpy(), feat.astype(numpy.float32)), (kw, show, "a show's rows are the bits load returns")
            assert feat.shape[0] == label.shape[0]
    plain = fc.ContextFeaturesServer(features_extractor=Source(shows), sdc=True, sdc_config=(2, 2, 3))
    feat, label = plain.load("40")
    assert numpy.array_equal(feat, fx["sdc_2_2_3_D5"][12:52]) and feat.dtype == numpy.float32
    # get_context / get_traps: rows start:stop, inside and past the stream's ends, windows over the whole stream
    server = fc.ContextFeaturesServer(context=(3, 2), traps_dct_nb=4)
    s, label = shows["40"][0], fx["range_label"]
    H = cn.traps_basis(3, 2, 4)
    for i, (start, stop) in enumerate(cn.RANGES + ((20, 21), (-8, -2), (41, 47))):
        got, lab = server.get_context(s, start, stop, label)
        assert numpy.array_equal(got, cn.context(s, 3, 2, (start, stop))) and numpy.array_equal(lab, label[start:stop]) and got.dtype == numpy.float32
        if i < len(cn.RANGES):
            assert numpy.array_equal(got, fx["range_ctx_%d" % i]), "against the reference"
        got, lab = server.get_traps(s, start, stop, label)
        idx = cn.window_rows(40, 3, 6, (start, stop))
        a = s.astype(numpy.float64)[idx]
        ref64, s_abs = numpy.einsum("twc,wj->tcj", a, H).reshape(len(idx), -1), numpy.einsum("twc,wj->tcj", numpy.abs(a), numpy.abs(H)).reshape(len(idx), -1)
        _within(got, ref64, s_abs, 6, ("get_traps", start, stop))
        assert numpy.array_equal(lab, label[start:stop])
    assert server.get_context(s)[1] is None and server.get_traps(s, 2, 9)[1] is None
    one = fc.ContextFeaturesServer(context=(2, 1), traps_dct_nb=2)
    assert numpy.array_equal(one.get_context(s[:1])[0], numpy.tile(s[:1], (1, 4))), "a one-row stream follows the formula"


def test_numpy_front_doors(fx, fc, batches):
    from sidekit_amd.frontend import features as fe
    s = batches[5].segments[batches[5].golden_at[40]]
    got = fe.shifted_delta_cepstral(s, 1, 4, 4)
    assert got.dtype == numpy.float64 and numpy.array_equal(got, fx["sdc_1_4_4_D5"][12:52].astype(numpy.float64))
    P = fx[cn.pca_name(12, 12, 5, 40)]
    plain, projected = fe.pca_dct(s), fe.pca_dct(s, p=P)
    assert plain.dtype == projected.dtype == numpy.float64 and plain.shape == (40, 125) and projected.shape == (40, 40)
    B = cn.dct_pca_basis(12, 12)
    _within(plain.astype(numpy.float32), cn.basis_map(s, B, 12), cn.basis_abs(s, B, 12), 25, "pca_dct")
    assert numpy.array_equal(plain.astype(numpy.float32).astype(numpy.float64), plain), "float64 that holds the float32 device values"
    ref = fx["dct_12_12_D5"][12:52]
    assert numpy.abs(plain - ref).max() <= 2.0 ** -23 * numpy.abs(ref).max() + 1e-12
