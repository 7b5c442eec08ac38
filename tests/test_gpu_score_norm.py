"""Cohort score normalisation on the GPU: sc_cohort_moments / sc_norm_apply / sc_matrix_moments and the Python surface over them
(sidekit_amd.score_normalization), against the reference's golden results and float64 numpy.  Where a statistic is held to the device's
own cohort scores, sc_cosine is the root of trust: tests/test_gpu_scoring_kernels.py is where sc_cosine itself (and sc_topk_stats) is judged
against float64."""
import ctypes
import os
import sys

import numpy
import pytest
import torch

from sidekit_amd import _lib
from sidekit_amd import score_normalization as sn
from sidekit_amd.bosaris import Scores

from test_gpu_plda_norm import _Spy

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import second_trips as st  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = dict(rtol=5e-5, atol=5e-5)      # normalised scores: the tolerance of the asnorm tests (same arithmetic, same 1 / std amplification)


def _st(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _unit(rs, n, d):
    x = rs.randn(n, d).astype(numpy.float32)
    return x / numpy.linalg.norm(x, axis=1, keepdims=True)


def _cosine(x, c):
    """float32 products of sc_cosine, as float64 numpy"""
    out = torch.empty((x.shape[0], c.shape[0]), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().sc_cosine(x.data_ptr(), x.shape[0], c.data_ptr(), c.shape[0], x.shape[1], out.data_ptr(), _st(x.device)))
    return out.cpu().numpy().astype(numpy.float64)


def _moments(x, c, shift=None, scale=None, self_offset=-1):
    mean = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    std = torch.empty_like(mean)
    _lib.check(_lib.lib().sc_cohort_moments(x.data_ptr(), x.shape[0], c.data_ptr(), c.shape[0], x.shape[1],
                                            None if shift is None else shift.data_ptr(), None if scale is None else scale.data_ptr(),
                                            self_offset, mean.data_ptr(), std.data_ptr(), _st(x.device)))
    return mean, std


def _ids(prefix, n):
    return numpy.array([f"{prefix}{i:04d}" for i in range(n)], dtype="|O")


def _scores(models, segs, mat, cls=Scores):
    s = cls()
    s.modelset, s.segset, s.scoremat, s.scoremask = models, segs, numpy.array(mat, dtype=numpy.float64), numpy.ones(mat.shape, dtype="bool")
    return s


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(numpy.load(os.path.join(golden_dir, "score_norm.npz")))


def test_golden_tnorm_znorm_asnorm(gpu, fx, golden_dir):
    e, t, c = (torch.from_numpy(fx[k]).to(gpu) for k in ("enrol", "test", "cohort"))
    s = torch.from_numpy(_cosine(e, t).astype(numpy.float32)).to(gpu)
    got = sn.tnorm_device(s.clone(), t, c)
    assert got.dtype == torch.float32 and got.is_cuda
    numpy.testing.assert_allclose(got.cpu().numpy(), fx["tnorm"], **TOL)
    numpy.testing.assert_allclose(sn.znorm_device(s.clone(), e, c).cpu().numpy(), fx["znorm"], **TOL)
    # Scores level, from host matrices whose models / segments arrive unsorted
    e64, t64, c64 = (fx[k].astype(numpy.float64) for k in ("enrol", "test", "cohort"))
    rs = numpy.random.RandomState(1)
    pe, pt, pc = rs.permutation(37), rs.permutation(53), rs.permutation(301)
    em, ts, cm = _ids("enr", 37), _ids("tst", 53), _ids("imp", 301)
    enrol_test = _scores(em[pe], ts[pt], (e64 @ t64.T)[pe][:, pt])
    before = enrol_test.scoremat.copy()
    tn = sn.tnorm(enrol_test, _scores(cm[pc], ts, (c64 @ t64.T)[pc]))
    assert list(tn.modelset) == list(em) and list(tn.segset) == list(ts) and tn.scoremat.dtype == numpy.float64
    numpy.testing.assert_allclose(tn.scoremat, fx["tnorm"], **TOL)
    zn = sn.znorm(enrol_test, _scores(em, cm[pc], (e64 @ c64.T)[:, pc]))
    assert list(zn.modelset) == list(em) and list(zn.segset) == list(ts)
    numpy.testing.assert_allclose(zn.scoremat, fx["znorm"], **TOL)
    numpy.testing.assert_array_equal(enrol_test.scoremat, before)                    # deep copy: the argument keeps its order and values
    # the adaptive coincidence case: enrolment against itself is the reference's asnorm
    ax = numpy.load(os.path.join(golden_dir, "asnorm.npz"))
    en = torch.from_numpy(ax["enrol"]).to(gpu)
    got = sn.asnorm_trials(en, en, torch.from_numpy(ax["cohort"]).to(gpu))
    assert got.shape == (64, 64) and got.is_cuda
    numpy.testing.assert_allclose(got.cpu().numpy(), ax["snorm"], **TOL)
    numpy.testing.assert_allclose(got.cpu().numpy(), sn.asnorm(ax["enrol"], ax["cohort"]), **TOL)


@pytest.mark.parametrize("N,M,D", [(1, 1, 4), (1, 257, 8), (255, 1, 256), (257, 513, 256), (300, 255, 132)])
def test_cohort_moments_ragged_shapes(gpu, N, M, D):
    """Shapes that straddle every tile edge, against float64 numpy on the float32 products of sc_cosine: 2e-6 absolute, the agreement
    test_cosine_scoring_golden asks of the products themselves."""
    rs = numpy.random.RandomState(N + M + D)
    x, c = torch.from_numpy(_unit(rs, N, D)).to(gpu), torch.from_numpy(_unit(rs, M, D)).to(gpu)
    mean, std = _moments(x, c)
    s = _cosine(x, c)
    numpy.testing.assert_allclose(mean.cpu().numpy(), s.mean(1), rtol=0, atol=2e-6)
    numpy.testing.assert_allclose(std.cpu().numpy(), s.std(1), rtol=0, atol=2e-6)
    if M == 1:
        assert (std == 0).all()
    m2, s2 = sn.cohort_stats_device(x, c)                                              # the Python entry: the same call
    assert torch.equal(m2, mean) and torch.equal(s2, std)


@pytest.mark.parametrize("r", [0, 255, 256])
def test_cohort_moments_self_offset(gpu, r):
    """X = rows [r, r + 300) of a 600-row cohort: the statistics of the explicit matrix with the pairs j == i + r masked out."""
    n, M = 300, 600
    c = torch.from_numpy(_unit(numpy.random.RandomState(5), M, 256)).to(gpu)
    x = c[r:r + n].contiguous()
    mean, std = _moments(x, c, self_offset=r)
    s = _cosine(x, c)
    keep = numpy.ones((n, M), dtype=bool)
    keep[numpy.arange(n), numpy.arange(n) + r] = False
    kept = s[keep].reshape(n, M - 1)
    assert numpy.all(s[~keep] > 0.999)                                                 # the masked pairs are the self-scores
    numpy.testing.assert_allclose(mean.cpu().numpy(), kept.mean(1), rtol=0, atol=2e-6)
    numpy.testing.assert_allclose(std.cpu().numpy(), kept.std(1), rtol=0, atol=2e-6)


def test_cohort_moments_col_shift_and_scale(gpu):
    """The statistics of (S - shift) * scale formed explicitly in float64.  The kernel evaluates the same float64 expression on the same
    float32 products; what is left is the order of float64 sums (1e-13 here) and the rounding of the two float32 results: 2^-23."""
    rs = numpy.random.RandomState(6)
    x, c = torch.from_numpy(_unit(rs, 257, 256)).to(gpu), torch.from_numpy(_unit(rs, 513, 256)).to(gpu)
    shift = (0.1 * rs.randn(513)).astype(numpy.float32)
    scale = rs.uniform(0.5, 20.0, 513).astype(numpy.float32)
    mean, std = _moments(x, c, torch.from_numpy(shift).to(gpu), torch.from_numpy(scale).to(gpu))
    v = (_cosine(x, c) - shift.astype(numpy.float64)) * scale.astype(numpy.float64)
    numpy.testing.assert_allclose(mean.cpu().numpy(), v.mean(1), rtol=1.2e-7, atol=1e-9)
    numpy.testing.assert_allclose(std.cpu().numpy(), v.std(1), rtol=1.2e-7, atol=1e-9)
    m2, s2 = sn.cohort_stats_device(x, c, col_shift=torch.from_numpy(shift).to(gpu), col_scale=torch.from_numpy(scale).to(gpu))
    assert torch.equal(m2, mean) and torch.equal(s2, std)


def test_identical_cohort_rows_give_a_tiny_finite_std(gpu):
    """64 identical cohort rows: the variance is a difference of two float64 roundings of a sum of 64 squares no larger than 1."""
    rs = numpy.random.RandomState(7)
    x = torch.from_numpy(_unit(rs, 130, 256)).to(gpu)
    c = torch.from_numpy(numpy.repeat(_unit(rs, 1, 256), 64, axis=0)).to(gpu)
    mean, std = _moments(x, c)
    assert torch.isfinite(std).all() and (std >= 0).all() and (std <= 1e-6).all(), std.max()
    numpy.testing.assert_allclose(mean.cpu().numpy(), _cosine(x, c)[:, 0], rtol=0, atol=2e-6)


def test_cohort_moments_bits_do_not_depend_on_stream_or_on_n(gpu):
    rs = numpy.random.RandomState(8)
    c = torch.from_numpy(_unit(rs, 600, 256)).to(gpu)
    x = c[100:400].contiguous()
    whole = _moments(x, c, self_offset=100)
    torch.cuda.synchronize()
    for _ in range(2):
        stream = torch.cuda.Stream(device=gpu)
        with torch.cuda.stream(stream):
            again = _moments(x, c, self_offset=100)
        stream.synchronize()
        assert torch.equal(again[0], whole[0]) and torch.equal(again[1], whole[1])
    lo, hi = _moments(x[:150].contiguous(), c, self_offset=100), _moments(x[150:].contiguous(), c, self_offset=250)
    assert torch.equal(torch.cat((lo[0], hi[0])), whole[0]) and torch.equal(torch.cat((lo[1], hi[1])), whole[1])
    odd = _moments(x[77:].contiguous(), c, self_offset=177)                            # another place in the tile, the same bits
    assert torch.equal(odd[0], whole[0][77:]) and torch.equal(odd[1], whole[1][77:])


@pytest.fixture(scope="module")
def long_cohort(gpu):
    """33 000 unit rows of D = 4 (tests/tools/second_trips.py): 258 cohort tiles, and room for X = C[100 : 100 + 32 768 + 130]."""
    return torch.from_numpy(st.cohort_cosine()).to(gpu)


@pytest.mark.parametrize("affine", [False, True])
def test_cohort_moments_past_the_row_block(gpu, long_cohort, affine, monkeypatch):
    """sc_cohort_moments launches ROWS = 32 768 rows of X at a time and gives a slab more than two cohort tiles once M > 16 384
    (``tiles_m > 128``).  X = C[r : r + N] with N = 32 768 + 130, M = 33 000 and self_offset = r crosses both in one call: the second
    launch reads ``d_X + r0 * D``, drops the pair ``i + self_offset + r0``, writes ``d_mean + r0`` and reuses the first launch's workspace;
    a slab holds 5 tiles and 52 partials are joined.  With and without col_shift / col_scale.  (a) Rows [32 766, N), either side of the
    block edge, against float64 numpy on sc_cosine's products of those rows: 2e-6 absolute (test_cohort_moments_ragged_shapes), with the
    affine form the bound of test_cohort_moments_col_shift_and_scale.  (b) The same rows, and four ranges of the first block, against
    calls of their own on those rows alone: bit for bit, the property the kernel documents (a row's additions depend on M alone)."""
    M, r, N = st.COHORT_M, st.COHORT_R, st.ROWS + st.COHORT_EXTRA
    tiles_m, per, slabs = st.slab_rule(M)
    assert N > st.ROWS and M > st.SLAB_TILES * st.COHORT_TILE and tiles_m > st.SLAB_TILES and per > st.MIN_PER and r + N <= M
    c = long_cohort
    x = c[r:r + N].contiguous()
    shift = scale = None
    if affine:
        rs = numpy.random.RandomState(24)
        shift = torch.from_numpy((0.1 * rs.randn(M)).astype(numpy.float32)).to(gpu)
        scale = torch.from_numpy(rs.uniform(0.5, 20.0, M).astype(numpy.float32)).to(gpu)
    mean, std = _moments(x, c, shift, scale, self_offset=r)
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(std).all()) and float(std.min()) > 0.0
    reached, lib = [], _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: _Spy(lib, reached))
    m2, s2 = sn.cohort_stats_device(x, c, self_offset=r, col_shift=shift, col_scale=scale)      # the Python entry: ONE call carries the whole N
    monkeypatch.undo()
    assert reached.count("sc_cohort_moments") == 1 and m2.shape == (N,) and torch.equal(m2, mean) and torch.equal(s2, std)
    # (a) float64 numpy on the rows around the block edge
    a = st.ROWS - 2
    s = _cosine(x[a:].contiguous(), c)
    drop = numpy.arange(a, N) + r
    assert numpy.all(s[numpy.arange(N - a), drop] > 0.999)                             # the dropped pairs are the self-scores
    if affine:
        s = (s - shift.cpu().numpy().astype(numpy.float64)) * scale.cpu().numpy().astype(numpy.float64)
    want_mean, want_std = st.kept_moments(s, drop)
    tol = dict(rtol=1.2e-7, atol=1e-9) if affine else dict(rtol=0, atol=2e-6)
    got_mean, got_std = mean[a:].cpu().numpy(), std[a:].cpu().numpy()
    print(f"affine {affine}: mean off by {numpy.abs(got_mean - want_mean).max():.2e}, std by {numpy.abs(got_std - want_std).max():.2e}")
    numpy.testing.assert_allclose(got_mean, want_mean, **tol)
    numpy.testing.assert_allclose(got_std, want_std, **tol)
    # (b) the same bits as calls of their own
    for a0, a1 in st.first_block_samples() + [(st.ROWS - 128, N)]:
        part = _moments(x[a0:a1].contiguous(), c, shift, scale, self_offset=r + a0)
        assert torch.equal(part[0], mean[a0:a1]) and torch.equal(part[1], std[a0:a1]), (a0, a1)


@pytest.mark.parametrize("M", st.SLAB_M)
def test_cohort_moments_at_and_past_the_slab_limit(gpu, long_cohort, M):
    """M = 16 384 is the last cohort whose slabs hold two tiles (``tiles_m > 128`` is false: 64 slabs of 2); M = 16 385 + 100 gives 129
    tiles, 3 to a slab, 43 partials.  N = 130 rows, X = C[100 : 230] with its self-pairs dropped: float64 numpy on sc_cosine's products
    at 2e-6 absolute, and the bits of a call on the last 53 rows alone."""
    tiles_m, per, slabs = st.slab_rule(M)
    assert (tiles_m, per, slabs) == ((128, 2, 64) if M == st.SLAB_TILES * st.COHORT_TILE else (129, 3, 43))
    r, n = st.COHORT_R, st.COHORT_EXTRA
    c = long_cohort[:M].contiguous()
    x = c[r:r + n].contiguous()
    mean, std = _moments(x, c, self_offset=r)
    want_mean, want_std = st.kept_moments(_cosine(x, c), numpy.arange(n) + r)
    numpy.testing.assert_allclose(mean.cpu().numpy(), want_mean, rtol=0, atol=2e-6)
    numpy.testing.assert_allclose(std.cpu().numpy(), want_std, rtol=0, atol=2e-6)
    part = _moments(x[77:].contiguous(), c, self_offset=r + 77)
    assert torch.equal(part[0], mean[77:]) and torch.equal(part[1], std[77:])


def test_norm_apply(gpu):
    """Both pairs: the bits of sc_snorm_apply.  One pair: one float32 subtraction and one division, both correctly rounded, so numpy's
    float32 result to one unit in the last place; a zero std gives numpy's inf / NaN."""
    lib = _lib.lib()
    rs = numpy.random.RandomState(9)
    ne, nt = 37, 53
    S = rs.randn(ne, nt).astype(numpy.float32)
    me, se = rs.randn(ne).astype(numpy.float32), rs.uniform(0.1, 2, ne).astype(numpy.float32)
    mt, sd = rs.randn(nt).astype(numpy.float32), rs.uniform(0.1, 2, nt).astype(numpy.float32)
    se[3] = 0.0
    sd[5] = 0.0
    S[3, 0] = me[3]                                                                    # 0 / 0
    S[1, 5] = mt[5]
    d = {k: torch.from_numpy(v).to(gpu) for k, v in dict(me=me, se=se, mt=mt, sd=sd).items()}

    def apply(fn, *ptrs):
        s = torch.from_numpy(S).to(gpu)
        _lib.check(fn(s.data_ptr(), ne, nt, *[None if p is None else p.data_ptr() for p in ptrs], _st(gpu)))
        return s.cpu().numpy()

    both = apply(lib.sc_norm_apply, d["me"], d["se"], d["mt"], d["sd"])
    numpy.testing.assert_array_equal(both.view(numpy.uint32), apply(lib.sc_snorm_apply, d["me"], d["se"], d["mt"], d["sd"]).view(numpy.uint32))
    with numpy.errstate(divide="ignore", invalid="ignore"):
        want_z, want_t = (S - me[:, None]) / se[:, None], (S - mt) / sd
    z = apply(lib.sc_norm_apply, d["me"], d["se"], None, None)
    t = apply(lib.sc_norm_apply, None, None, d["mt"], d["sd"])
    assert numpy.isnan(z[3, 0]) and numpy.isinf(z[3, 1:]).all() and numpy.isnan(t[1, 5]) and numpy.isinf(t[0, 5])
    numpy.testing.assert_allclose(z, want_z, rtol=1.2e-7, atol=0)
    numpy.testing.assert_allclose(t, want_t, rtol=1.2e-7, atol=0)
    s = torch.from_numpy(S).to(gpu)
    assert lib.sc_norm_apply(s.data_ptr(), ne, nt, None, None, None, None, _st(gpu)) == _lib.SK_EARG


@pytest.mark.parametrize("rows,cols", [(37, 53), (129, 129)])
def test_matrix_moments(gpu, rows, cols):
    """float64 numpy on the same float32 values; what is left is the rounding of the float32 results."""
    S = (0.3 * numpy.random.RandomState(rows).randn(rows, cols)).astype(numpy.float32)
    s64 = S.astype(numpy.float64)
    for axis in (0, 1):
        mean, std = sn.matrix_moments_device(torch.from_numpy(S).to(gpu), axis)
        numpy.testing.assert_allclose(mean.cpu().numpy(), s64.mean(axis), rtol=1.2e-7, atol=1e-9)
        numpy.testing.assert_allclose(std.cpu().numpy(), s64.std(axis), rtol=1.2e-7, atol=1e-9)
        if rows != cols:
            with pytest.raises(ValueError):
                sn.matrix_moments_device(torch.from_numpy(S).to(gpu), axis, skip_diag=True)
            continue
        off = s64[~numpy.eye(rows, dtype=bool)].reshape(rows, rows - 1) if axis == 1 else s64.T[~numpy.eye(rows, dtype=bool)].reshape(rows, rows - 1)
        mean, std = sn.matrix_moments_device(torch.from_numpy(S).to(gpu), axis, skip_diag=True)
        numpy.testing.assert_allclose(mean.cpu().numpy(), off.mean(1), rtol=1.2e-7, atol=1e-9)
        numpy.testing.assert_allclose(std.cpu().numpy(), off.std(1), rtol=1.2e-7, atol=1e-9)


def test_ztnorm_device_against_scores_level_and_float64(gpu, fx):
    """zt-norm with (Ne, Nt, M) = (37, 53, 301).  UNPINNED by the reference: its znorm cannot normalise a non-square matrix
    (score_normalization.py:70) and its sym=True statistics omit the square root (:64-66), so the yardstick is the float64 restatement
    below of the definition DESIGN.md states, which the device form and the Scores-level form must both meet."""
    e, t, c = (torch.from_numpy(fx[k]).to(gpu) for k in ("enrol", "test", "cohort"))
    s, ei, it, ii = _cosine(e, t), _cosine(e, c), _cosine(c, t), _cosine(c, c)
    M = 301
    off = ~numpy.eye(M, dtype=bool)
    z_s = (s - ei.mean(1)[:, None]) / ei.std(1)[:, None]
    m_c = (ii * off).sum(1) / (M - 1)
    sd_c = numpy.sqrt((((ii - m_c[:, None]) ** 2) * off).sum(1) / (M - 1))
    z_it = (it - m_c[:, None]) / sd_c[:, None]
    want = (z_s - z_it.mean(0)) / z_it.std(0)
    got = sn.ztnorm_device(torch.from_numpy(s.astype(numpy.float32)).to(gpu), e, t, c)
    numpy.testing.assert_allclose(got.cpu().numpy(), want, **TOL)
    em, ts, cm = _ids("enr", 37), _ids("tst", 53), _ids("imp", M)
    host = sn.ztnorm(_scores(em, ts, s), _scores(em, cm, ei), _scores(cm, ts, it), _scores(cm, cm, ii))
    assert list(host.modelset) == list(em) and list(host.segset) == list(ts)
    numpy.testing.assert_allclose(host.scoremat, want, **TOL)
    numpy.testing.assert_allclose(host.scoremat, got.cpu().numpy(), **TOL)
    plain = sn.snorm_device(torch.from_numpy(s.astype(numpy.float32)).to(gpu), e, t, c)          # whole-cohort s-norm, while the matrices are here
    numpy.testing.assert_allclose(plain.cpu().numpy(), 0.5 * ((s - ei.mean(1)[:, None]) / ei.std(1)[:, None] + (s - it.mean(0)) / it.std(0)), **TOL)


def test_adaptive_statistics_in_bounded_memory(gpu):
    N, M, k, ws = 4096, 2048, 20, 1 << 20
    rs = numpy.random.RandomState(10)
    x, c = torch.from_numpy(_unit(rs, N, 256)).to(gpu), torch.from_numpy(_unit(rs, M, 256)).to(gpu)
    whole = sn.cohort_stats_device(x, c, topk=k)
    del whole
    whole = sn.cohort_stats_device(x, c, topk=k)                                       # (N, M) scores in one block
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(gpu)
    base = torch.cuda.memory_allocated(gpu)
    blocked = sn.cohort_stats_device(x, c, topk=k, max_workspace_bytes=ws)             # 128 rows at a time
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(gpu) - base
    assert rise <= ws + 2 * N * 4 + (1 << 20), rise
    assert torch.equal(blocked[0], whole[0]) and torch.equal(blocked[1], whole[1])
    torch.cuda.reset_peak_memory_stats(gpu)
    base = torch.cuda.memory_allocated(gpu)
    sn.cohort_stats_device(x, c)                                                       # whole-cohort statistics: no score buffer at all
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated(gpu) - base <= 2 * N * 4 + (1 << 20)
    with pytest.raises(ValueError):
        sn.cohort_stats_device(x[:4], c[:10], topk=20)


def test_one_object_on_both_sides_shares_the_statistics(gpu, monkeypatch):
    """Cosine scores are symmetric: ``test_xv is enroll_xv`` computes the cohort moments once, an equal tensor of its own twice, same bits."""
    rs = numpy.random.RandomState(13)
    x, c = (torch.from_numpy(_unit(rs, n, 36)).to(gpu) for n in (65, 33))
    mat = torch.from_numpy(_cosine(x, x).astype(numpy.float32)).to(gpu)
    reached, lib = [], _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: _Spy(lib, reached))
    shared = sn.snorm_device(mat.clone(), x, x, c)
    assert reached.count("sc_cohort_moments") == 1, reached
    del reached[:]
    apart = sn.snorm_device(mat.clone(), x, x.clone(), c)
    assert reached.count("sc_cohort_moments") == 2, reached
    monkeypatch.undo()
    assert shared.shape == (65, 65) and torch.equal(shared, apart) and not torch.equal(shared, mat)


def test_drop_in_names_after_install_as_sidekit(gpu, fx):
    import sidekit_amd
    saved = {k: v for k, v in sys.modules.items() if k == "sidekit" or k.startswith("sidekit.")}
    try:
        sidekit_amd.install_as_sidekit()
        import sidekit
        from sidekit.score_normalization import tnorm, znorm, ztnorm
        assert sidekit.tnorm is tnorm and sidekit.znorm is znorm and sidekit.ztnorm is ztnorm
        e64, t64, c64 = (fx[k].astype(numpy.float64) for k in ("enrol", "test", "cohort"))
        em, ts, cm = _ids("enr", 37), _ids("tst", 53), _ids("imp", 301)
        mk = lambda models, segs, mat: _scores(models, segs, mat, sidekit.bosaris.Scores)
        tn = sidekit.score_normalization.tnorm(mk(em, ts, e64 @ t64.T), mk(cm, ts, c64 @ t64.T))
        numpy.testing.assert_allclose(tn.scoremat, fx["tnorm"], **TOL)
        zn = sidekit.score_normalization.znorm(mk(em, ts, e64 @ t64.T), mk(em, cm, e64 @ c64.T))
        numpy.testing.assert_allclose(zn.scoremat, fx["znorm"], **TOL)
        zt = sidekit.score_normalization.ztnorm(mk(em, ts, e64 @ t64.T), mk(em, cm, e64 @ c64.T), mk(cm, ts, c64 @ t64.T), mk(cm, cm, c64 @ c64.T))
        assert isinstance(zt, sidekit.bosaris.Scores) and zt.validate() and zt.scoremat.shape == (37, 53) and numpy.isfinite(zt.scoremat).all()
    finally:
        for k in [k for k in sys.modules if k == "sidekit" or k.startswith("sidekit.")]:
            del sys.modules[k]
        sys.modules.update(saved)
