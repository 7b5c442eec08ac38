"""Feature post-processing on the GPU (sidekit_amd/features_server.py, csrc/featnorm.hip) against the float64 numpy restatement
(tests/tools/normfeat_numpy.py, pinned to the reference by tests/test_features_reference_cpu.py) and, for the numpy surface, against the
reference's own output (tests/golden/features.npz).

One stacked batch of D = 5: the fixture's sixteen streams plus an empty, a 1-row and a 2-row segment and the lengths TILE - 1, TILE,
TILE + 1 and 2 TILE + h + 1 (TILE = 256 rows, h = 150 for the window of 301); a second one of D = 17 (the column chunk is 16) with the
lengths that matter for a tile; a third pair (``long_segments``) of segments longer than the 2048 rows one round of the tile lanes covers.  Bound against the restatement r on the same float32 inputs: |gpu - r| <= 2^-23 |r| + 1e-10 max|x| (one
rounding to float32, 2^-24 |r|, doubled; float64 summation-order differences over at most 1001 terms, for window standard deviations of
order 1, asserted > 0.1 on the restatement's side; among thousands of windows of 5 random values a few are narrower, so at window 5
cmvn_sliding is held to the bound on every value but those of such a window, under 0.1 % of them and no whole row).
Feature warping: the ranks are exact.  The bitwise tests are exact.
"""
import os
import sys

import numpy
import pytest
from scipy.special import ndtr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import normfeat_numpy as nfn  # noqa: E402
import second_trips as st  # noqa: E402

pytestmark = pytest.mark.gpu
TILE, H = 256, 150
PASS = st.FEAT_PASS        # FZ * SC_FEAT_TILE = 2048 rows: what the FZ = 8 workgroups of a segment cover before each takes another tile
LONG = [PASS, 0, PASS + 1, 7, PASS + TILE + H + 1, 2 * PASS + 7]
LONG_WIDE = [0, PASS + 1]
KEYS = [str(n) for n in (3, 4, 5, 6, 7, 8, 9, 299, 300, 301, 302, 303, 650, 900)] + ["s301", "s302"]
EXTRA = [0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + H + 1]
WIDE = [0, 1, 2, 7, TILE - 1, TILE, TILE + 1, 2 * TILE + H + 1, 302]
NORMS = ["cms", "cmvn", "cms_sliding", "cmvn_sliding", "stg"]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(numpy.load(os.path.join(golden_dir, "features.npz")))


class Batch:
    def __init__(self, segments, labels):
        self.segments, self.labels = segments, labels
        self.x = numpy.concatenate(segments).astype(numpy.float32)
        self.lab = numpy.concatenate(labels)
        self.off = numpy.concatenate(([0], numpy.cumsum([s.shape[0] for s in segments]))).astype(numpy.int64)
        self.scale = float(numpy.abs(self.x).max())
        self.cache = {}

    def ref(self, key, fn):
        """the restatement of one operation per segment, computed once"""
        if key not in self.cache:
            self.cache[key] = [fn(s.astype(numpy.float64), l) for s, l in zip(self.segments, self.labels)]
        return self.cache[key]

    def cut(self, a):
        return [a[self.off[i]:self.off[i + 1]] for i in range(len(self.segments))]


def _draw(rs, n, d):
    x = (1.5 * rs.randn(n, d) + rs.randn(d)) * (0.5 + 2 * rs.rand(d))
    lab = rs.rand(n) < 0.7
    if n > 1:
        lab[1] = True
    if n == 2:
        x[1] = x[0] + 1 + rs.rand(d)     # two rows a standard deviation of order 1 apart
    return x.astype(numpy.float32), lab


@pytest.fixture(scope="module")
def batches(fx):
    rs = numpy.random.RandomState(77)
    segs, labs = [fx["x_" + k] for k in KEYS], [fx["lab_" + k] for k in KEYS]
    for n in EXTRA:
        x, lab = _draw(rs, n, 5)
        segs.append(x)
        labs.append(lab)
    order = rs.permutation(len(segs))      # the short and the empty segments lie among the long ones
    narrow = Batch([segs[i] for i in order], [labs[i] for i in order])
    wide = Batch(*zip(*[_draw(rs, n, 17) for n in WIDE]))
    assert 3000 < narrow.x.shape[0] < 8000
    return narrow, wide


def _np(t):
    return t.cpu().numpy()


def _assert_close(what, got, want, scale):
    """|gpu - r| <= 2^-23 |r| + 1e-10 max|x|, equal where r is not finite"""
    got, want = numpy.asarray(got, dtype=numpy.float64), numpy.asarray(want, dtype=numpy.float64)
    assert got.shape == want.shape, what
    finite = numpy.isfinite(want)
    assert numpy.array_equal(numpy.isnan(got), numpy.isnan(want)) and numpy.array_equal(got[~finite & ~numpy.isnan(want)], want[~finite & ~numpy.isnan(want)]), what
    excess = numpy.abs(got - want)[finite] - (2.0 ** -23 * numpy.abs(want[finite]) + 1e-10 * scale)
    worst = excess.max() if excess.size else -1.0
    print(f"{what}: max |gpu - r| {numpy.abs(got - want)[finite].max() if excess.size else 0:.3e}")
    assert worst <= 0, f"{what}: exceeds the bound by {worst:.3e}"


def _entry(name, b, gpu, **kw):
    import torch
    from sidekit_amd import features_server as fs
    x, off = torch.as_tensor(b.x).to(gpu), torch.as_tensor(b.off).to(gpu)
    return getattr(fs, name)(x, off, **kw)


def test_rasta_delta_and_moments_against_the_restatement(gpu, batches):
    import torch
    for b in batches:
        y = _entry("rasta_device", b, gpu)
        assert y.is_cuda and y.dtype == torch.float32
        _assert_close("rasta", _np(y), numpy.concatenate(b.ref("rasta", lambda s, l: nfn.rasta(s))), b.scale)
        for taps in (None, [-1, 0, 1], [.2, .1, 0, -.1, -.2], numpy.linspace(-1, 1, 15), [2.0]):
            filt = nfn.DEFAULT_FILTER if taps is None else numpy.asarray(taps, dtype=numpy.float64)
            want = numpy.concatenate(b.ref(f"delta{len(filt)}", lambda s, l: nfn.delta(s, filt)))
            _assert_close(f"delta {len(filt)} taps", _np(_entry("delta_device", b, gpu, filt=taps)), want, b.scale)
        mean, std = _entry("segment_moments_device", b, gpu)
        assert mean.dtype == std.dtype == torch.float64 and mean.shape == (len(b.segments), b.x.shape[1])
        want = b.ref("moments", lambda s, l: nfn.moments(s))
        _assert_close("mean", _np(mean), numpy.stack([m for m, _ in want]), b.scale)
        _assert_close("std", _np(std), numpy.stack([s for _, s in want]), b.scale)
        empty = [i for i, s in enumerate(b.segments) if s.shape[0] == 0]
        assert empty and numpy.all(_np(mean)[empty] == 0.0) and numpy.all(_np(std)[empty] == 1.0)


def test_delta_writes_column_blocks_of_one_matrix(gpu, batches):
    import torch
    from sidekit_amd import features_server as fs
    b = batches[1]
    D = b.x.shape[1]
    x, off = torch.as_tensor(b.x).to(gpu), torch.as_tensor(b.off).to(gpu)
    wide = torch.full((b.x.shape[0], 3 * D), 7.0, device=gpu)
    wide[:, :D] = x
    fs.delta_device(wide[:, :D], off, out=wide[:, D:2 * D])
    fs.delta_device(wide[:, D:2 * D], off, out=wide[:, 2 * D:])
    d = fs.delta_device(x, off)
    assert torch.equal(wide[:, :D], x) and torch.equal(wide[:, D:2 * D], d) and torch.equal(wide[:, 2 * D:], fs.delta_device(d, off))
    squared = numpy.convolve(nfn.DEFAULT_FILTER, nfn.DEFAULT_FILTER)
    assert squared.shape[0] == 13
    assert not torch.equal(wide[:, 2 * D:], fs.delta_device(x, off, squared)), "delta of delta is not one convolution: the deltas outside a segment are zero"


@pytest.mark.parametrize("win", [301, 5, 1001])
def test_normalisations_against_the_restatement(gpu, batches, win):
    """every row counts as speech here: the entry itself, all five modes"""
    for b in batches:
        if win == 1001 and b is batches[0]:
            continue
        for mode in NORMS:
            want = b.ref(f"{mode}{win}", lambda s, l: nfn.normalise(s, mode, win))
            got = _np(_entry("normalise_device", b, gpu, mode=mode, win=win))
            want = numpy.concatenate(want)
            held = numpy.ones(want.shape, dtype=bool)
            if mode in ("cmvn", "cmvn_sliding"):      # the bound is for standard deviations of order 1 (a single row has none: nan on both sides)
                std = numpy.concatenate([nfn.sliding_std(s, win if mode == "cmvn_sliding" else 10 ** 9) for s in b.segments])
                held = (std > 0.1) | numpy.concatenate([numpy.full(s.shape, s.shape[0] < 2) for s in b.segments])
                # a few of the thousands of windows of 5 random values are narrower than that: those values alone (each a row and a
                # column) are left to cms_sliding at this window and to the window of 301; every segment and every tile stays compared
                assert held.all() or (win == 5 and mode == "cmvn_sliding" and held.mean() > 0.999)
                assert all(h.any(1).all() for h in b.cut(held)), "no row of any segment leaves the comparison"
            _assert_close(f"{mode} win {win}", got[held], want[held], b.scale)
            if mode == "stg":
                for s, g in zip(b.segments, b.cut(got)):
                    c, w = nfn.warp_counts(s, win)
                    assert numpy.array_equal(numpy.round(ndtr(g.astype(numpy.float64)) * w - 0.5).astype(numpy.int64), c), "exact ranks"


def test_offsets_must_cover_every_row_and_the_table_modes_ignore_the_window(gpu, batches):
    """a row outside every segment would be written by no kernel; ``win`` means nothing to cms / cmvn"""
    import torch
    from sidekit_amd import features_server as fs
    b = batches[1]
    x, off = torch.as_tensor(b.x).to(gpu), torch.as_tensor(b.off).to(gpu)
    for bad in (off[2:], off[:-1], b.off[:-1], b.off[:1], torch.flip(off, [0])):
        for call in (lambda: fs.rasta_device(x, bad), lambda: fs.delta_device(x, bad), lambda: fs.normalise_device(x, bad, "stg"),
                     lambda: fs.segment_moments_device(x, bad), lambda: fs.post_process_device(x, bad, rasta=True)):
            with pytest.raises(AssertionError, match="from 0 to N"):
                call()
    for norm in ("cms", "cmvn"):
        assert _same(fs.normalise_device(x, off, norm, win=300), fs.normalise_device(x, off, norm, win=301))
        assert _same(fs.post_process_device(x, off, feat_norm=norm, win=4000)[0], fs.post_process_device(x, off, feat_norm=norm)[0])
    with pytest.raises(ValueError, match="sc_feat_norm"):
        fs.normalise_device(x, off, "cms_sliding", win=300)


def _post(fs, b, gpu, x=None, off=None, lab=None, **kw):
    import torch
    x, off, lab = (b.x if x is None else x), (b.off if off is None else off), (b.lab if lab is None else lab)
    return fs.post_process_device(torch.as_tensor(x).to(gpu), torch.as_tensor(off).to(gpu), torch.as_tensor(lab).to(gpu), **kw)


@pytest.mark.parametrize("norm", NORMS + [None])
def test_post_process_device_against_the_restatement(gpu, batches, norm):
    import torch
    from sidekit_amd import features_server as fs
    b = batches[0]
    opts = dict(rasta_on=True, delta_on=True, double_delta=True, feat_norm=norm)
    for keep in (True, False):
        want = b.ref(f"post {norm} {keep}", lambda s, l: nfn.post_process(s, l, keep_all=keep, **opts))
        out, labels, off = _post(fs, b, gpu, rasta=True, delta=True, double_delta=True, feat_norm=norm, keep_all_features=keep)
        assert out.is_cuda and out.dtype == torch.float32 and labels.dtype == torch.bool and off.dtype == torch.int64
        assert numpy.array_equal(_np(off), numpy.concatenate(([0], numpy.cumsum([w[0].shape[0] for w in want]))))
        assert numpy.array_equal(_np(labels), numpy.concatenate([w[1] for w in want]))
        _assert_close(f"post {norm} keep {keep}", _np(out), numpy.concatenate([w[0] for w in want]), b.scale)
        if norm == "stg":
            before = b.ref("post None True", lambda s, l: nfn.post_process(s, l, rasta_on=True, delta_on=True, double_delta=True))
            got = _np(out)
            for i, (pre, lab) in enumerate(before):
                rows = got[int(_np(off)[i]):int(_np(off)[i + 1])]
                rows = rows[lab] if keep else rows
                c, w = nfn.warp_counts(pre[lab], 301)
                assert numpy.array_equal(numpy.round(ndtr(rows.astype(numpy.float64)) * w - 0.5).astype(numpy.int64), c), "exact ranks on every labelled row"
    # a mask, global vectors, another window and no RASTA
    gm, gs = numpy.linspace(-1, 1, 4), numpy.linspace(0.5, 2, 4)
    for kw, rkw in ((dict(mask=[0, 2, 3, 9], feat_norm="cmvn", global_mean=gm, global_std=gs, delta=True),
                     dict(mask=[0, 2, 3, 9], feat_norm="cmvn", global_mean=gm, global_std=gs, delta_on=True)),
                    (dict(mask=[0, 2, 3, 9], feat_norm="cms", global_mean=gm, delta=True), dict(mask=[0, 2, 3, 9], feat_norm="cms", global_mean=gm, delta_on=True)),
                    (dict(feat_norm="cmvn_sliding", win=5), dict(feat_norm="cmvn_sliding", win=5)),
                    (dict(feat_norm="stg", win=5, keep_all_features=False), dict(feat_norm="stg", win=5, keep_all=False))):
        if norm is not None:
            break
        want = [nfn.post_process(s, l, **rkw) for s, l in zip(b.segments, b.labels)]
        out, labels, off = _post(fs, b, gpu, **kw)
        _assert_close(f"post {sorted(kw)}", _np(out), numpy.concatenate([w[0] for w in want]), b.scale)


def test_unlabelled_rows_keep_their_bits_and_frames_are_not_written(gpu, batches):
    import torch
    from sidekit_amd import features_server as fs
    b = batches[0]
    x = torch.as_tensor(b.x).to(gpu)
    keep = x.clone()
    counts = numpy.array([int(l.sum()) for l in b.labels])
    for norm in ("cms_sliding", "cmvn_sliding", "stg"):
        out, labels, off = fs.post_process_device(x, torch.as_tensor(b.off).to(gpu), torch.as_tensor(b.lab).to(gpu), feat_norm=norm)
        assert torch.equal(x, keep), "the caller's frames are never written"
        got = _np(out)
        for i, (g, s, l) in enumerate(zip(b.cut(got), b.segments, b.labels)):
            windowed = norm == "stg" or counts[i] > 301
            assert numpy.array_equal(g[~l], s[~l]) == (windowed or counts[i] == 0 or not (~l).any()), (norm, i, counts[i])
            if counts[i] == 0:
                assert numpy.array_equal(g, s), "a segment without a labelled row is left unchanged"
    assert (counts > 301).sum() >= 3 and (counts == 0).sum() >= 1 and ((counts > 0) & (counts <= 301)).sum() >= 10


def _same(p, q):
    """the same bits, a NaN (a single row divided by its zero deviation) being equal to a NaN"""
    import torch
    return p.shape == q.shape and torch.equal(torch.isnan(p), torch.isnan(q)) and torch.equal(p.nan_to_num(), q.nan_to_num())


def _ops(fs):
    ops = {"rasta": lambda x, off: fs.rasta_device(x, off), "delta": lambda x, off: fs.delta_device(x, off),
           "mean": lambda x, off: fs.segment_moments_device(x, off)[0], "std": lambda x, off: fs.segment_moments_device(x, off)[1]}
    for mode in NORMS:
        for win in (301, 5):
            ops[f"{mode} {win}"] = lambda x, off, mode=mode, win=win: fs.normalise_device(x, off, mode=mode, win=win)
    return ops


def test_a_segment_has_the_same_bits_alone_and_anywhere_in_the_batch(gpu, batches):
    import torch
    from sidekit_amd import features_server as fs
    for b in batches:
        S = len(b.segments)
        x, off = torch.as_tensor(b.x).to(gpu), torch.as_tensor(b.off).to(gpu)
        back = Batch(b.segments[::-1], b.labels[::-1])
        xb, offb = torch.as_tensor(back.x).to(gpu), torch.as_tensor(back.off).to(gpu)
        for name, op in _ops(fs).items():
            whole, again, mirrored = op(x, off), op(x, off), op(xb, offb)
            assert _same(whole, again), f"{name}: two runs differ"
            per_segment = name in ("mean", "std")
            for i in range(S):
                a0, a1 = int(b.off[i]), int(b.off[i + 1])
                alone = op(x[a0:a1].clone(), None)
                j = S - 1 - i
                if per_segment:
                    inside, elsewhere = whole[i:i + 1], mirrored[j:j + 1]
                else:
                    inside, elsewhere = whole[a0:a1], mirrored[int(back.off[j]):int(back.off[j + 1])]
                assert _same(alone, inside) and _same(alone, elsewhere), f"{name}: segment {i} ({a1 - a0} rows) differs from itself alone"
    b = batches[0]
    for norm in NORMS:
        kw = dict(rasta=True, delta=True, double_delta=True, feat_norm=norm, keep_all_features=False)
        out, labels, off = _post(fs, b, gpu, **kw)
        again = _post(fs, b, gpu, **kw)[0]
        assert _same(out, again), "two runs of the batch give the same bits"
        off = _np(off)
        for i in (0, 3, len(b.segments) - 1, int(numpy.argmax([s.shape[0] for s in b.segments]))):
            s, l = b.segments[i], b.labels[i]
            alone = _post(fs, b, gpu, x=s, off=numpy.array([0, s.shape[0]]), lab=l, **kw)[0] if s.shape[0] else out[:0]
            assert _same(alone, out[int(off[i]):int(off[i + 1])]), f"post {norm}: segment {i}"


# ---- segments longer than one round of the tile lanes ----------------------------------------------------------------------------------
def long_segments():
    """The third batch (D = 5): 2048 rows (one full round of the FZ = 8 tile lanes, no second pass), an empty segment, 2049 rows, a short
    one, 2048 + 256 + 150 + 1 rows (the second pass's window of 301 reaches into rows of the first round) and 2 * 2048 + 7 rows (a third
    pass); and one of D = 17 with 2049 rows.  Every row is labelled but five of the longest segment, two of them either side of row 2048:
    4098 speech rows, still three passes."""
    rs = numpy.random.RandomState(78)
    out = []
    for lengths, d in ((LONG, 5), (LONG_WIDE, 17)):
        segs, labs = [], []
        for n in lengths:
            x, _ = _draw(rs, n, d)
            lab = numpy.ones(n, dtype=bool)
            if n == 2 * PASS + 7:
                lab[[10, 1000, PASS - 1, PASS, 3000]] = False
            segs.append(x)
            labs.append(lab)
        out.append(Batch(segs, labs))
    return tuple(out)


@pytest.fixture(scope="module")
def long_batches():
    narrow, wide = long_segments()
    assert st.FZ * st.SC_FEAT_TILE == PASS == 2048 and TILE == st.SC_FEAT_TILE
    assert max(s.shape[0] for s in narrow.segments) > 2 * PASS and max(s.shape[0] for s in wide.segments) > PASS   # a third pass; a second one
    assert int(narrow.labels[-1].sum()) > 2 * PASS
    return narrow, wide


def test_long_segments_delta_and_moments_against_the_restatement(gpu, long_batches):
    """feat_delta_kernel's second and third ``t0 += FZ * FT`` pass (a segment longer than FZ * FT = 2048 rows): RASTA, every filter and
    the moments on the third batch, every row compared, under the criteria of the first two batches."""
    test_rasta_delta_and_moments_against_the_restatement(gpu, long_batches)


@pytest.mark.parametrize("win", [301, 5])
def test_long_segments_normalisations_against_the_restatement(gpu, long_batches, win):
    """feat_norm_kernel<MODE> past FZ * FT = 2048 rows: the barrier between two tiles of one workgroup and the staging window
    ``slo..shi`` counted from a later tile, all five modes, warp ranks exact.  The restatement is of every row (100 % compared; at
    window 5 cmvn_sliding leaves out what the first two batches leave out, windows narrower than 0.1, under 0.1 % of the values)."""
    test_normalisations_against_the_restatement(gpu, long_batches, win)


def test_long_segments_post_process_with_warping(gpu, long_batches):
    """``post_process_device`` (RASTA, deltas, double deltas, feature warping over the labelled rows) on the third batch."""
    test_post_process_device_against_the_restatement(gpu, long_batches, "stg")


def test_long_segments_have_the_same_bits_alone_and_anywhere_in_the_batch(gpu, long_batches):
    """A segment of two or three passes alone, inside the batch and inside the mirrored batch: the same bits, every operation."""
    test_a_segment_has_the_same_bits_alone_and_anywhere_in_the_batch(gpu, long_batches)


def _close_to_golden(what, got, want, extra=1e-6):
    got, want = numpy.asarray(got, dtype=numpy.float64), numpy.asarray(want, dtype=numpy.float64)
    got = got[:, :want.shape[1]]
    assert got.shape == want.shape, what
    finite = numpy.isfinite(want)
    assert numpy.array_equal(finite, numpy.isfinite(got)), what
    excess = numpy.abs(got - want)[finite] - (2.0 ** -23 * numpy.abs(want[finite]) + extra)
    assert excess.size == 0 or excess.max() <= 0, f"{what}: exceeds the bound by {excess.max():.3e}"


def _warp_close_to_golden(what, got, want, x_speech, win):
    """float32 device values against the reference's float64 ones at 2^-23 |g| + 1e-6 wherever a frame's value is the only one of its
    kind in its window; elsewhere (the duplicated frame of an even short stream, the rows RASTA makes equal) against the rule's own
    value, which the reference's is one tie order away from (tests/test_features_reference_cpu.py)"""
    from scipy.special import ndtri
    c, w = nfn.warp_counts(x_speech, win)
    e = nfn.warp_ties(x_speech, win)[:, :want.shape[1]]
    rule = ndtri((c + 0.5) / w)[:, :want.shape[1]]
    _close_to_golden(what, got, numpy.where(e > 1, rule, want))


def test_numpy_surface_against_the_reference(gpu, fx):
    from sidekit_amd.frontend import normfeat
    from sidekit_amd.frontend.features import compute_delta
    gm, gs = fx["gmean"], fx["gstd"]
    seen = 0
    for k in KEYS:
        x, lab = fx["x_" + k], fx["lab_" + k]
        scale = float(numpy.abs(x).max())
        r = normfeat.rasta_filt(x.astype(numpy.float64))
        assert r.dtype == numpy.float64
        _close_to_golden("rasta " + k, r, fx["rasta_" + k])
        d = compute_delta(x.astype(numpy.float64))
        assert d.dtype == numpy.float32 and d.shape == x.shape
        _close_to_golden("delta " + k, d, fx["delta_" + k], extra=1e-6 * scale)
        _close_to_golden("delta of delta " + k, compute_delta(d), fx["ddelta_" + k], extra=1e-6 * scale)
        for key in sorted(fx):
            parts = key.split("_")
            if parts[-1] != k or parts[0] not in ("cms", "cmvn", "slc", "slcr", "stg"):
                continue
            seen += 1
            a = x.astype(numpy.float64)
            if parts[0] in ("cms", "cmvn"):
                args = (lab.copy(),) if parts[1] == "lab" else ((lab.copy(), gm) if parts[0] == "cms" else (lab.copy(), gm, gs))
                getattr(normfeat, parts[0])(a, *args)
                _close_to_golden(key, a, fx[key])
                continue
            win, label = int(parts[1]), (lab.copy() if parts[2] == "lab" else None)
            if parts[0] == "stg":
                normfeat.stg(a, label=label, win=win)
                speech = numpy.ones(x.shape[0], dtype=bool) if label is None else lab
                assert numpy.array_equal(a[~speech], x[~speech].astype(numpy.float64))
                _warp_close_to_golden(key, a[speech], fx[key][speech], x[speech].astype(numpy.float64), win)
            else:
                normfeat.cep_sliding_norm(a, win=win, label=label, center=True, reduce=parts[0] == "slcr")
                _close_to_golden(key, a, fx[key])
    assert seen == 9 * 4 + 3 * 39
    untouched = fx["x_650"].astype(numpy.float64)
    normfeat.cep_sliding_norm(untouched, win=301, center=False, reduce=True)
    assert numpy.array_equal(untouched, fx["x_650"].astype(numpy.float64)), "nothing happens without center when the window applies"
    f32 = fx["x_9"].copy()
    normfeat.cmvn(f32)
    assert f32.dtype == numpy.float32 and numpy.abs(f32.mean(0)).max() < 1e-6
    numpy.testing.assert_array_equal(compute_delta(fx["x_9"], win=1, method='diff'), compute_delta(fx["x_9"], win=1, filt=[-1, 0, 1]))


def test_features_server_post_processing_against_the_reference(gpu, fx):
    from sidekit_amd.features_server import FeaturesServer
    for k in ("9", "s301", "s302"):
        x, lab = fx["x_" + k][:, :1], fx["lab_" + k]
        scale = float(numpy.abs(x).max())
        for norm in NORMS:
            for tag, keep in (("keep", True), ("drop", False)):
                server = FeaturesServer(feat_norm=norm, delta=True, double_delta=True, rasta=True, keep_all_features=keep)
                label = lab.copy()
                feat, out_label = server.post_processing(x.astype(numpy.float64), label)
                want = fx[f"post_{norm}_{tag}_{k}"]
                assert feat.dtype == numpy.float64 and numpy.array_equal(out_label, fx[f"postlab_{norm}_{tag}_{k}"])
                if norm == "stg":
                    before, speech = nfn.post_process(x, lab, rasta_on=True, delta_on=True, double_delta=True)
                    rows = speech if keep else numpy.ones(feat.shape[0], dtype=bool)
                    _warp_close_to_golden(f"post stg {tag} {k}", feat[rows], want[rows], before[speech], 301)
                    if keep:
                        _close_to_golden(f"post stg {tag} {k} unlabelled", feat[~speech], want[~speech], extra=2e-6 * scale)
                else:
                    # the reference keeps RASTA in float64 and rounds its deltas to float32; here every stage is float32: 1e-6 max|x|
                    # per stage, carried through a division by a standard deviation of order 1
                    _close_to_golden(f"post {norm} {tag} {k}", feat, want, extra=4e-6 * scale)
    plain = FeaturesServer(feat_norm="cms", mask="[0,2-3]")
    feat, _ = plain.post_processing(fx["x_9"].copy(), None)
    assert feat.dtype == numpy.float32 and feat.shape == (9, 3)
    two = numpy.array([True, True])
    _, fused = FeaturesServer().post_processing(fx["x_9"][:2], two)
    assert not fused.any() and not two.any(), "the reference's label_fusion turns a two-frame [True, True] into [False, False]"


class Source:
    """an in-memory features extractor: show 'u<i>' is segment i"""
    def __init__(self, segments, labels):
        self.segments, self.labels = segments, labels

    def extract(self, show, channel, input_audio_filename=None):
        i = int(show[1:])
        return self.segments[i], self.labels[i]


def test_server_feeds_the_mixture_and_the_statistics_as_the_resident_path_does(gpu, fx):
    import torch
    from sidekit_amd.features_server import FeaturesServer
    from sidekit_amd.mixture import Mixture, em_split_device
    from sidekit_amd.statserver import StatServer
    keys = ["9", "299", "s301", "s302", "650"]
    segments, labels = [fx["x_" + k][:, :3] for k in keys], [fx["lab_" + k] for k in keys]
    shows = [f"u{i}" for i in range(len(keys))]
    opts = dict(feat_norm="cmvn_sliding", delta=True, rasta=True)
    server = FeaturesServer(features_extractor=Source(segments, labels), keep_all_features=False, **opts)
    stacked = server.stack_features(shows)
    frames, off = server.stack_features_device(shows)
    assert frames.is_cuda and frames.dtype == torch.float32 and isinstance(off, numpy.ndarray) and off.dtype == numpy.int64
    assert stacked.dtype == numpy.float64 and numpy.array_equal(stacked, _np(frames).astype(numpy.float64)), "a show's rows are the bits load() returns"
    assert off.tolist() == numpy.concatenate(([0], numpy.cumsum([int(l.sum()) for l in _fused(labels)]))).tolist()
    feat, lab = server.load("u1", start=-2, stop=310)
    assert feat.shape == (int(_fused([numpy.pad(labels[1], (2, 11), mode='edge')])[0].sum()), 6) and lab.all(), "start / stop reach beyond the stream"
    by_server = Mixture()
    llk = by_server.EM_split(server, shows, 2, iterations=(1,))
    resident, llk_dev = em_split_device(frames, 2, iterations=(1,))
    rel = lambda a, b: numpy.abs(numpy.asarray(a) - numpy.asarray(b)).max() / numpy.abs(numpy.asarray(b)).max()   # noqa: E731
    assert rel(llk, llk_dev) < 1e-9     # tests/test_gpu_mixture.py's bound for float64 quantities
    for k in ("w", "mu", "invcov", "cov_var_ctl"):
        assert rel(getattr(by_server, k), getattr(resident, k)) < 1e-9, k
    names = numpy.array(shows, dtype="|O")
    host = StatServer()
    host.modelset, host.segset = names, names.copy()
    host.start, host.stop = numpy.empty(len(shows), dtype="|O"), numpy.empty(len(shows), dtype="|O")
    all_rows = FeaturesServer(features_extractor=Source(segments, labels), keep_all_features=True, **opts)
    host.accumulate_stat(resident, all_rows)
    dev = StatServer()
    dev.modelset, dev.segset, dev.start, dev.stop = names, names.copy(), host.start, host.stop
    dev.accumulate_stat_device(resident, frames, off)
    assert host.validate() and rel(host.stat0, dev.stat0) < 1e-9 and rel(host.stat1, dev.stat1) < 1e-9
    assert abs(host.stat0.sum() - off[-1]) < 1e-6 * off[-1]


def _fused(labels):
    """the labels after RASTA: frames 0-1 take the label of frame 2"""
    out = []
    for l in labels:
        l = l.copy()
        l[:2] = l[2]
        out.append(l)
    return out
