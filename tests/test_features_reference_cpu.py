"""The float64 numpy restatement of the feature post-processing (tests/tools/normfeat_numpy.py) against what the reference computes
(tests/golden/features.npz, written by make_features_golden.py from the imported reference modules).  No GPU, no library.

Bounds: 1e-10 absolute for RASTA and the normalisers (float64 against float64; pandas' rolling moments are online sums, the
restatement's direct ones); 1e-6 max|x| for the deltas, which the reference stores in float32.  Feature warping of an even number of
frames below the window: every frame but the last real one at 1e-10; that one frame of the fixture must be normcdfinv((c + 0.5) / w) or
normcdfinv((c + 1.5) / w) -- the reference's duplicated frame ties with it and numpy's argsort orders the tie either way -- and the
restatement gives the first.  The same holds, for the same reason, for the rows RASTA makes equal at the head of a stream (zeros in rows
0-3, rows 0-1 copied from row 2) when ``post_processing`` warps them: e equal values in a window have e accepted ranks in the
reference's output, c in the restatement's; every other frame of the fixture has one.
"""
import os
import sys

import numpy
import pytest
from scipy.special import ndtri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import normfeat_numpy as nfn  # noqa: E402

TOL = 1e-10
LENGTHS = [3, 4, 5, 6, 7, 8, 9, 299, 300, 301, 302, 303, 650, 900]
KEYS = [str(n) for n in LENGTHS] + ["s301", "s302"]
NORMS = ["cms", "cmvn", "cms_sliding", "cmvn_sliding", "stg"]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(numpy.load(os.path.join(golden_dir, "features.npz")))


def cut(fx, got, want):
    """the fixture keeps the first columns only of a long stream"""
    return got[:, :want.shape[1]]


def check(fx, name, got, tol=TOL):
    want = fx[name]
    got = cut(fx, got, want)
    assert got.shape == want.shape, name
    err = numpy.abs(got - want).max() if want.size else 0.0
    assert err <= tol, f"{name}: differs by {err:.3e} (bound {tol:.1e})"


def test_fixture_is_the_set_its_generator_describes(fx):
    assert sorted(k[2:] for k in fx if k.startswith("x_")) == sorted(KEYS)
    for k in KEYS:
        x = fx["x_" + k]
        assert x.dtype == numpy.float32 and x.shape[1] == 5 and fx["lab_" + k].shape == (x.shape[0],)
        assert all(numpy.unique(x[:, c]).shape[0] == x.shape[0] for c in range(5)), "tie-free"
    assert fx["lab_s301"].sum() == 301 and fx["lab_s302"].sum() == 302 and int(fx["cols_big"]) == 1
    assert fx["delta_650"].dtype == numpy.float32 and fx["rasta_650"].dtype == numpy.float64


def test_rasta(fx):
    for k in KEYS:
        check(fx, "rasta_" + k, nfn.rasta(fx["x_" + k]))


def test_deltas(fx):
    for k in KEYS:
        x = fx["x_" + k].astype(numpy.float64)
        d = nfn.delta(x)
        check(fx, "delta_" + k, d, 1e-6 * numpy.abs(x).max())
        d32 = d.astype(numpy.float32).astype(numpy.float64)
        check(fx, "ddelta_" + k, nfn.delta(d32), 1e-6 * numpy.abs(x).max())


def test_centring_with_labels_and_with_global_vectors(fx):
    seen = 0
    for k in KEYS:
        if "cms_lab_" + k not in fx:
            continue
        seen += 1
        x, lab = fx["x_" + k], fx["lab_" + k]
        for norm in ("cms", "cmvn"):
            check(fx, f"{norm}_lab_{k}", nfn.post_process(x, lab, feat_norm=norm, round32=False)[0])
            check(fx, f"{norm}_glob_{k}", nfn.post_process(x, lab, feat_norm=norm, global_mean=fx["gmean"], global_std=fx["gstd"], round32=False)[0])
    assert seen == 9


def _windowed(fx, mode, name):
    """every recorded stream of one windowed mode -> [(key, win, labelled, got, want)]"""
    cases = []
    for key in sorted(fx):
        if not key.startswith(name + "_"):
            continue
        _, win, tag, k = key.split("_")
        lab = fx["lab_" + k] if tag == "lab" else None
        got = nfn.post_process(fx["x_" + k], lab, feat_norm=mode, win=int(win), round32=False)[0]
        cases.append((key, k, int(win), lab, got, fx[key]))
    return cases


def test_sliding_norms(fx):
    for mode, name in (("cms_sliding", "slc"), ("cmvn_sliding", "slcr")):
        cases = _windowed(fx, mode, name)
        assert len(cases) == 14 + 10 + 8 + 7      # win 301: 14 without labels, 7 + 3 with; win 5: 7 + 1 without, 7 with
        for key, k, win, lab, got, want in cases:
            finite = numpy.isfinite(want)
            assert numpy.array_equal(finite, numpy.isfinite(cut(fx, got, want))), key
            err = numpy.abs(cut(fx, got, want) - want)[finite].max()
            assert err <= TOL, f"{key}: differs by {err:.3e}"
    for k in ("s301", "s302"):     # the switch: 301 labelled frames are the fallback and touch every frame, 302 only the labelled ones
        got = nfn.post_process(fx["x_" + k], fx["lab_" + k], feat_norm="cms_sliding", round32=False)[0]
        untouched = numpy.array_equal(got[~fx["lab_" + k]], fx["x_" + k][~fx["lab_" + k]].astype(numpy.float64))
        assert untouched == (k == "s302")
        want = fx["slc_301_lab_" + k]
        assert numpy.array_equal(want[~fx["lab_" + k]], fx["x_" + k][~fx["lab_" + k], :1].astype(numpy.float64)) == (k == "s302")


def assert_warp(key, x_speech, win, got, want):
    """``got`` (the restatement's) is normcdfinv((c + 0.5) / w) everywhere; ``want`` (the reference's) too wherever a frame's value is
    the only one of its kind in its window, and normcdfinv((c + j + 0.5) / w) with 0 <= j < e where e window values are equal to it (the
    reference ranks its first and last window by a double argsort, which orders equal values either way).  -> e"""
    c, w = nfn.warp_counts(x_speech, win)
    e = nfn.warp_ties(x_speech, win)
    c, e = c[:, :want.shape[1]], e[:, :want.shape[1]]
    err = numpy.abs(got - ndtri((c + 0.5) / w)).max()
    assert err <= TOL, f"{key}: the restatement differs from its own rule by {err:.3e}"
    best = numpy.full(want.shape, numpy.inf)
    for j in range(int(e.max())):
        best = numpy.where(j < e, numpy.minimum(best, numpy.abs(want - ndtri((c + j + 0.5) / w))), best)
    assert best.max() <= TOL, f"{key}: differs by {best.max():.3e}"
    return e


def test_feature_warping(fx):
    even_short = 0
    for key, k, win, lab, got, want in _windowed(fx, "stg", "stg"):
        x = fx["x_" + k].astype(numpy.float64)
        speech = numpy.ones(x.shape[0], dtype=bool) if lab is None else lab
        n = int(speech.sum())
        got = cut(fx, got, want)
        assert numpy.array_equal(got[~speech], x[~speech, :want.shape[1]]) and numpy.array_equal(want[~speech], x[~speech, :want.shape[1]])
        e = assert_warp(key, x[speech], win, got[speech], want[speech])
        if n < win and n % 2 == 0:     # the duplicated frame ties with the last real one: the one frame with two accepted values
            even_short += 1
            assert numpy.all(e[-1] == 2) and numpy.all(e[:-1] == 1)
        else:
            assert numpy.all(e == 1)
    assert even_short >= 4      # 4, 6, 8 and 300 frames at win 301 at least


def test_post_processing(fx):
    """RASTA leaves a stream's rows 0-3 equal in its first column (zeros, rows 0-1 copied from row 2) and their deltas partly so: the
    only ties of this set, and with the even short case the only frames with more than one accepted value under ``stg``."""
    for k in ("9", "s301", "s302"):
        x, lab = fx["x_" + k][:, :1], fx["lab_" + k]
        scale = numpy.abs(x).max()
        for norm in NORMS:
            for tag, keep in (("keep", True), ("drop", False)):
                got, labels = nfn.post_process(x, lab, rasta_on=True, delta_on=True, double_delta=True, feat_norm=norm, keep_all=keep, round32='delta')
                want = fx[f"post_{norm}_{tag}_{k}"]
                assert numpy.array_equal(labels, fx[f"postlab_{norm}_{tag}_{k}"])
                assert got.shape == want.shape
                if norm == "stg":
                    before, speech = nfn.post_process(x, lab, rasta_on=True, delta_on=True, double_delta=True, round32='delta')
                    rows = speech if keep else numpy.ones(got.shape[0], dtype=bool)
                    e = assert_warp(f"post stg {tag} {k}", before[speech], 301, got[rows], want[rows])
                    tied = numpy.flatnonzero((e > 1).any(1))
                    n = int(speech.sum())
                    allowed = set(range(int(speech[:4].sum()))) | ({n - 1} if n < 301 and n % 2 == 0 else set())
                    assert set(tied.tolist()) <= allowed, (k, tied)
                    if keep:
                        assert numpy.array_equal(got[~speech], before[~speech]) and numpy.abs(want[~speech] - before[~speech]).max() <= 1e-6 * scale
                    continue
                # the reference rounds its deltas to float32 (1e-6 max|x| on those columns); the normalisers carry that through
                # divided by a standard deviation of order 1
                bound = 4e-6 * scale
                err = numpy.abs(got - want).max()
                assert err <= bound, f"post {norm} {tag} {k}: differs by {err:.3e} (bound {bound:.1e})"
