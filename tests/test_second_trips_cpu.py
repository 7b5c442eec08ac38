"""The tests of second trips (a persistent workgroup's second tile, a launcher's second row block, a pass loop's second pass) without a
GPU: the thresholds the GPU cases' shapes rest on, read out of the sources, and, for every GPU case, a numpy emulation of the launch
structure that passes the case's own criterion on the case's own data -- and fails it once the second trip is made wrong in the way
such code goes wrong.  The emulations and the data are those of tests/tools/second_trips.py; the criteria are imported from the GPU
test modules themselves."""
import os
import sys

import numpy
import pytest
import scipy.ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))

import second_trips as st  # noqa: E402
import vad_numpy as vn  # noqa: E402
import test_gpu_features as feat  # noqa: E402
import test_gpu_hist_norm as cos_hist  # noqa: E402
import test_gpu_plda_hist as plda_hist  # noqa: E402
from sidekit_amd import iv_scoring  # noqa: E402


# ---- the thresholds ------------------------------------------------------------------------------------------------------------------
def test_the_sources_state_the_thresholds_the_shapes_assume():
    src = st.read_sources()
    assumed = {k: getattr(st, k) for k in src}
    assert src == assumed, "a threshold moved: move the shapes of the second-trip tests (tests/tools/second_trips.py) with it"
    # what the GPU cases derive from them
    assert st.hist_side(st.CUS, st.HT) == (4099, 17) and st.hist_side(st.CUS, st.PT) == (2051, 17)
    assert st.hist_side(st.CUS - 1, st.HT) == (3843, 16) and 16 * 16 > st.CUS - 1              # the smallest t, not a larger one
    n = st.ROWS + st.COHORT_EXTRA
    assert n > st.ROWS and st.COHORT_R + n <= st.COHORT_M and st.ROWS - 128 == 32640
    assert st.slab_rule(st.COHORT_M) == (258, 5, 52)
    assert st.SLAB_M == (16384, 16485) and st.slab_rule(16384) == (128, 2, 64) and st.slab_rule(16485) == (129, 3, 43)
    assert all(0 <= a < b <= st.ROWS - 128 for a, b in st.first_block_samples())
    assert feat.PASS == st.FZ * st.SC_FEAT_TILE == 2048 and feat.TILE == st.SC_FEAT_TILE
    assert sorted(feat.LONG) == [0, 7, 2048, 2049, 2455, 4103] and feat.LONG_WIDE == [0, 2049]
    assert st.VAD_WINDOWS[-1] == st.VAD_MAX_WIN and [st.vad_lengths(w // 2)[2] for w in st.VAD_WINDOWS] == [2053, 2109, 2557]
    assert st.vad_lengths(1)[3] > 2 * st.VAD_TILE
    # the flush of the LDS counters stays out of reach: a workgroup would have to take this many tiles
    assert st.HIST_FLUSH == {"cosine": 1 << 15, "plda": 1 << 17}


# ---- 1. histogram kernels that walk more than one tile ------------------------------------------------------------------------------
def _stats(cs, topk):
    if topk is None:
        return cs.mean(1), cs.std(1)
    best = numpy.sort(cs, axis=1)[:, -topk:]
    return best.mean(1), best.std(1, ddof=1)


def _walk_case(H, tile, s, term, stats, kind, lab, dtype):
    """One histogram case: ``s`` the (n, n) cross terms, ``term`` the per-row term added on both sides (None: cosine), ``stats`` the
    (mean, std) per row.  -> (reference counts of the whole normalised matrix, a function variant -> counts of the tile walk)."""
    n = s.shape[0]
    half = dtype(0.5)

    def value(v, me, se, mt, sd):
        if kind == "z":
            return (v - me[:, None]) / se[:, None]
        if kind == "t":
            return (v - mt[None, :]) / sd[None, :]
        if kind == "s":
            return half * ((v - me[:, None]) / se[:, None]) + half * ((v - mt[None, :]) / sd[None, :])
        return v

    mean, std = stats
    zero = numpy.zeros(n, dtype=dtype) if term is None else term
    whole = value(s + zero[:, None] + zero[None, :], mean, std, mean, std)
    off = ~numpy.eye(n, dtype=bool)
    lo, hi = H._range(whole[off])
    tar = lab[:, None] == lab[None, :]
    bins = H._bins(whole, lo, hi)
    ref = (H._count(bins, tar & off), H._count(bins, ~tar & off))

    def block(m0, n0, s0):
        rows, cols = numpy.arange(m0, min(m0 + tile, n)), numpy.arange(n0, min(n0 + tile, n))
        nr, nc = rows.shape[0], cols.shape[0]
        v = s[m0:m0 + nr, n0:n0 + nc]
        if term is not None:
            v = v + st.staged(term, s0[0], tile, 0)[:nr, None] + st.staged(term, s0[1], tile, 0)[None, :nc]
        v = value(v, st.staged(mean, s0[0], tile, 0)[:nr], st.staged(std, s0[0], tile, 1)[:nr], st.staged(mean, s0[1], tile, 0)[:nc],
                  st.staged(std, s0[1], tile, 1)[:nc])
        b, t, keep = H._bins(v, lo, hi), tar[m0:m0 + nr, n0:n0 + nc], rows[:, None] != cols[None, :]
        return H._count(b, t & keep), H._count(b, ~t & keep)

    return ref, lambda variant: st.walk_tiles(n, n, tile, st.CUS, block, variant)


def _check_walk(ref, walk, variants):
    got = walk(None)
    assert numpy.array_equal(got[0], ref[0]) and numpy.array_equal(got[1], ref[1]), "the tile walk as the kernels do it"
    for variant in variants:
        bad = walk(variant)
        assert not (numpy.array_equal(bad[0], ref[0]) and numpy.array_equal(bad[1], ref[1])), f"{variant}: the case's criterion does not notice"
        if variant == "dropped":
            assert int(bad[0].sum() + bad[1].sum()) < int(ref[0].sum() + ref[1].sum())    # the total N^2 - N alone shows it


@pytest.mark.parametrize("name", ["plain"] + list(cos_hist.KINDS))
def test_cosine_histogram_cases_notice_a_wrong_second_tile(name):
    n, t = st.hist_side(st.CUS, st.HT)
    x, lab = st.cosine_corpus(n)
    c, _ = st.cosine_corpus(300, seed=26)
    kind, topk = cos_hist.KINDS.get(name, (None, None))
    stats = _stats(x @ c.T, topk) if kind else (numpy.zeros(n, dtype=numpy.float32), numpy.ones(n, dtype=numpy.float32))
    stats = tuple(v.astype(numpy.float32) for v in stats)
    ref, walk = _walk_case(cos_hist, st.HT, x @ x.T, None, stats, kind, lab, numpy.float32)
    assert int(ref[0].sum() + ref[1].sum()) == n * n - n and t * t - st.CUS == 33         # 33 workgroups take a second tile
    _check_walk(ref, walk, ("dropped", "stale") if kind else ("dropped",))


@pytest.mark.parametrize("name", ["plain"] + list(cos_hist.KINDS))
def test_plda_histogram_cases_notice_a_wrong_second_tile(name, golden_dir):
    n, t = st.hist_side(st.CUS, st.PT)
    model = st.plda_model(golden_dir, 10)
    x, lab = st.plda_corpus(model, n)
    c = st.plda_corpus(model, 300, seed=27, n_spk=60)[0]
    Phi, Psi, cst = iv_scoring.plda_parameters(*model)
    xc, cc = x - model[0], c - model[0]
    quad = lambda v: 0.5 * numpy.einsum("ik,kl,il->i", v, Phi, v)                          # noqa: E731
    term = quad(xc) + 0.5 * cst                                                            # cst rides on the two terms, half each
    kind, topk = cos_hist.KINDS.get(name, (None, None))
    cohort = xc @ Psi @ cc.T + quad(xc)[:, None] + quad(cc)[None, :] + cst
    stats = _stats(cohort, topk) if kind else (numpy.zeros(n), numpy.ones(n))
    ref, walk = _walk_case(plda_hist, st.PT, xc @ Psi @ xc.T, term, stats, kind, lab, numpy.float64)
    assert int(ref[0].sum() + ref[1].sum()) == n * n - n
    _check_walk(ref, walk, ("dropped", "stale"))                                          # plain: `term` alone is stale


# ---- 2. cohort moments past the row block and the slab limit ------------------------------------------------------------------------
def _cohort_case(kind, golden_dir, m=st.COHORT_M):
    """-> (scores_of for X = C[r:], the case's own comparison of a statistic with float64 numpy's)"""
    if kind.startswith("cosine"):
        c = st.cohort_cosine()[:m].astype(numpy.float64)
        if kind == "cosine":                                                               # test_cohort_moments_ragged_shapes' bound
            return (lambda rows, terms: c[st.COHORT_R + rows] @ c.T), lambda got, want: numpy.abs(got - want).max() <= 2e-6
        rs = numpy.random.RandomState(24)                                                  # the col_shift / col_scale of the GPU case
        shift, scale = (0.1 * rs.randn(st.COHORT_M)).astype(numpy.float32)[:m], rs.uniform(0.5, 20.0, st.COHORT_M).astype(numpy.float32)[:m]
        scores = lambda rows, terms: (c[st.COHORT_R + rows] @ c.T - shift.astype(numpy.float64)) * scale.astype(numpy.float64)   # noqa: E731
        return scores, lambda got, want: numpy.allclose(got, want, rtol=1.2e-7, atol=1e-9)   # test_cohort_moments_col_shift_and_scale's
    model = st.plda_model(golden_dir, 5)
    cc = st.plda_corpus(model, st.COHORT_M, seed=25 + 5)[0][:m] - model[0]
    Phi, Psi, cst = iv_scoring.plda_parameters(*model)
    quad = 0.5 * numpy.einsum("ik,kl,il->i", cc, Phi, cc)
    scores = lambda rows, terms: (cc[st.COHORT_R + rows] @ Psi) @ cc.T + quad[st.COHORT_R + terms][:, None] + quad[None, :] + cst   # noqa: E731
    bound = 1e-9 * float(numpy.abs(scores(numpy.arange(64), numpy.arange(64))).max())     # this module's 1e-9 of the largest score
    return scores, lambda got, want: numpy.abs(got - want).max() <= bound


def _moments_criteria(scores, close, n, m, ranges, tail, variant):
    """The two criteria of the GPU cases on the emulated launcher's output: (a) the rows ``tail`` against float64 numpy under ``close``;
    (b) every range of ``ranges`` against a call of its own on those rows alone, exactly.  -> the list of what failed."""
    r = st.COHORT_R
    rows = numpy.unique(numpy.concatenate([numpy.arange(a, b) for a, b in ranges]))
    mean, std = st.moments_launcher(scores, n, m, r, rows, variant)
    failed = []
    t = numpy.arange(*tail)
    want_mean, want_std = st.kept_moments(scores(t, t), t + r)
    if not (close(mean[t], want_mean) and close(std[t], want_std)):
        failed.append("a")
    for a0, a1 in ranges:
        own = numpy.arange(a1 - a0)
        alone = st.moments_launcher(lambda rr, tt: scores(rr + a0, tt + a0), a1 - a0, m, r + a0, own, "slab" if variant == "slab" else None)
        if not (numpy.array_equal(alone[0], mean[a0:a1]) and numpy.array_equal(alone[1], std[a0:a1])):
            failed.append(("b", a0))
    return failed


@pytest.mark.parametrize("kind", ["cosine", "cosine affine", "plda"])
def test_cohort_moment_cases_notice_a_wrong_second_row_block(kind, golden_dir):
    scores, close = _cohort_case(kind, golden_dir)
    n, m = st.ROWS + st.COHORT_EXTRA, st.COHORT_M
    ranges = st.first_block_samples() + [(st.ROWS - 128, n)]
    tail = (st.ROWS - 2, n)
    assert _moments_criteria(scores, close, n, m, ranges, tail, None) == []
    # a dropped self-pair moves a cosine mean by about (1 - mean) / M = 3e-5, fifteen times the bound; a PLDA mean by far more
    for variant in ("self_off", "out", "x") + (("xterm",) if kind == "plda" else ()):
        failed = _moments_criteria(scores, close, n, m, ranges, tail, variant)
        assert "a" in failed and ("b", st.ROWS - 128) in failed, (variant, failed)
        if variant == "out":
            assert ("b", 0) in failed, "the second block's output lands on the first block's first rows"
    failed = _moments_criteria(scores, close, n, m, ranges, tail, "slab")
    assert "a" in failed, "a slab join that stops at two tiles per slab: criterion (a) sees it (b compares like with like)"


@pytest.mark.parametrize("kind", ["cosine", "plda"])
def test_slab_cases_notice_a_join_that_stops_at_two_tiles(kind, golden_dir):
    old, new = st.SLAB_M
    for m in st.SLAB_M:
        scores, close = _cohort_case(kind, golden_dir, m)
        n = st.COHORT_EXTRA
        assert _moments_criteria(scores, close, n, m, [(0, n), (77, n)], (0, n), None) == []
        failed = _moments_criteria(scores, close, n, m, [(0, n), (77, n)], (0, n), "slab")
        assert failed == ([] if m == old else ["a"]), (m, failed)            # 16 384: two tiles ARE the slab, the old path is pinned as it is


# ---- 3. feature post-processing on segments longer than 2048 rows -------------------------------------------------------------------
def _per_pass(fn, x):
    """``fn`` applied to every FZ * FT rows on their own: what a window (or a filter) clamped to the pass computes."""
    return numpy.concatenate([fn(x[a:a + feat.PASS]) for a in range(0, max(x.shape[0], 1), feat.PASS)])


@pytest.mark.parametrize("what", ["delta", "cms_sliding 301", "cmvn_sliding 301", "stg 301", "cms_sliding 5", "cmvn_sliding 5", "stg 5"])
def test_feature_cases_notice_a_window_clamped_to_the_pass(what):
    if what == "delta":
        fn = lambda s: feat.nfn.delta(s)                                                  # noqa: E731
    else:
        mode, win = what.split()
        fn = lambda s: feat.nfn.normalise(s, mode, int(win))                              # noqa: E731
    for b in feat.long_segments():
        want = [fn(s.astype(numpy.float64)) for s in b.segments]
        stored = [w.astype(numpy.float32) for w in want]                                 # the restatement as the device stores it
        feat._assert_close(what, numpy.concatenate(stored), numpy.concatenate(want), b.scale)
        long = [i for i, s in enumerate(b.segments) if s.shape[0] > feat.PASS]
        assert long
        for i in long:
            bad = _per_pass(fn, b.segments[i].astype(numpy.float64))
            assert bad.shape == want[i].shape
            with numpy.errstate(all="ignore"), pytest.raises(AssertionError):
                feat._assert_close(what, bad.astype(numpy.float32), want[i], b.scale)
            # and a second pass that is not made at all leaves the rows from 2048 on as they were
            unwritten = stored[i].copy()
            unwritten[feat.PASS:] = -7.0
            with pytest.raises(AssertionError):
                feat._assert_close(what, unwritten, want[i], b.scale)


# ---- 4. VAD label fusion past one tile -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", st.VAD_WINDOWS)
def test_vad_cases_notice_a_fusion_without_its_halo(win):
    patterns = st.vad_patterns(win)
    le, nf = st.vad_log_energies(patterns)
    caught = {}
    for b, p in enumerate(patterns):
        n = p.shape[0]
        if n > 1:                                                                        # the two levels give the designed raw labels
            raw = vn.vad_energy(le[b, :n], 8, fusion_win=0, **st.VAD_KW)[0]
            assert numpy.array_equal(raw, p.astype(bool)), b
        want = scipy.ndimage.grey_opening(scipy.ndimage.grey_closing(p, size=win), size=win).astype(bool)
        assert want.any() or n == 1
        assert numpy.array_equal(vn.label_fusion(p, win), want)                           # the unmodified restatement
        for variant in ("reflect", "no_halo"):
            same = numpy.array_equal(st.fuse_per_tile(p, win, variant), want)
            assert same or n > st.VAD_TILE, "one tile: nothing to get wrong"
            if n > st.VAD_TILE:
                caught.setdefault((n, variant), []).append(not same)
    assert len(caught) == 6                                                             # three lengths past one tile, two variants
    for key, hits in caught.items():
        assert sum(hits) >= 4, (key, sum(hits))                                          # each on several of the 24 patterns
