"""Trial scoring one kernel at a time: sc_cosine (and the zero-padding branch of cosine_matrix_device), sc_normalize_rows, sc_cosine_trials,
sc_topk_stats / sc_topk_stats_f64 and the k-tail of the cosine histograms, each against a float64 evaluation of the SAME operands
(tests/tools/scoring_f64.py, where the criteria are stated).  tests/test_scoring_reference_cpu.py shows on these operands that float32
evaluations of the formulas pass the criteria and that the wrong kernels listed there do not.  This is where sc_cosine itself is judged:
the cohort statistics and the histograms of tests/test_gpu_score_norm.py, test_gpu_hist_norm.py and test_gpu_hist_bins.py are held to
sc_cosine's own products.

Operands are rows of randn x 2^uniform(-6, 6), each row its own scale, not unit vectors (the histogram test, whose range is [-1, 1), says
where it uses unit rows).  The entry points are called through _lib.launch / _lib.lib(); every output is a view between two sentinel rows
(or before a sentinel element) of a larger buffer whose border must be intact afterwards.  A HIP error ends the session (returncode 3):
nothing more is started on the device.  Every comparison prints the largest share of its bound it used; DESIGN.md section 4g has the table.
"""
import contextlib
import ctypes
import os
import sys

import numpy
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import scoring_f64 as sf  # noqa: E402

from sidekit_amd import _lib, iv_scoring  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = -1.5e30


def _say(capsys, text):
    with capsys.disabled():
        print(f"  [{text}]", end="")


@contextlib.contextmanager
def device(what):
    """a HIP error inside (at the launch or at the synchronisation that follows): nothing more is started on this device"""
    try:
        yield
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what} failed on the device: {e}", returncode=3)


def bits(a, b):
    """the same bytes (a NaN equals only the same NaN)"""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def framed(gpu, rows, cols, dtype=torch.float32):
    """(frame, the view of its rows 1 .. rows): an output between two sentinel rows"""
    frame = torch.full((rows + 2, cols), SENTINEL, dtype=dtype, device=gpu)
    return frame, frame[1:rows + 1]


def intact(frame):
    return bool((frame[0] == SENTINEL).all()) and bool((frame[-1] == SENTINEL).all())


def _stream(gpu):
    return ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)


# ---- sc_cosine --------------------------------------------------------------------------------------------------------------------------
def _cosine(gpu, E, T):
    """one sc_cosine call on (host or device) float32 operands -> the (Ne, Nt) matrix on the host"""
    e, t = E.to(gpu).contiguous(), T.to(gpu).contiguous()
    frame, out = framed(gpu, e.shape[0], t.shape[0])
    with device(f"sc_cosine{e.shape[0], t.shape[0], e.shape[1]}"):
        _lib.launch("sc_cosine", gpu, e, e.shape[0], t, t.shape[0], e.shape[1], out, exc=AssertionError)
    assert intact(frame), "the border around the output is intact"
    return out.cpu()


@pytest.mark.parametrize("shape", sf.COSINE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cosine_against_float64(gpu, capsys, shape):
    """The smallest problem; exactly one tile and one k-tile; one row past a tile, one column short and a k-tail of 4; less than one k-tile
    and three column tiles; ragged in both directions; long K; the smallest 128-tile launch and a ragged one."""
    ne, nt, d = shape
    assert (ne >= sf.BIG_M and nt >= sf.BIG_N) == (shape in sf.COSINE_SHAPES[-2:])
    E, T = sf.cosine_operands(ne, nt, d)
    got = _cosine(gpu, E, T)
    err, err32, share = sf.check_cosine(f"sc_cosine{shape}", got, E, T)
    _say(capsys, f"{shape}: {share:.3f} of 2 K u S; norm-relative {err:.1e}, torch float32 {err32:.1e}")
    assert bits(_cosine(gpu, E, T), got), "two runs give the same bits"
    # a row alone and inside the batch: the first row, the last row of one 64-row tile and the first of the next, the last row
    for i in sorted({0, sf.TILE - 1, sf.TILE, ne - 1}):
        if i < ne:
            assert bits(_cosine(gpu, E[i:i + 1], T)[0], got[i]), f"row {i} alone and inside the batch"
    # one NaN and one +inf in single elements of E and of T: exactly their rows and columns are not finite, the rest keeps its bits
    E2, T2 = E.clone(), T.clone()
    rows, cols = (0, ne - 1), (nt // 2, nt - 1)
    E2[rows[0], d - 1], E2[rows[1], 0] = float("nan"), float("inf")
    T2[cols[0], 0], T2[cols[1], d - 1] = float("nan"), float("inf")
    dirty = _cosine(gpu, E2, T2)
    hit = torch.zeros(ne, nt, dtype=torch.bool)
    hit[list(rows)] = True
    hit[:, list(cols)] = True
    assert not bool(torch.isfinite(dirty[hit]).any()), "a NaN or an infinity in a row reaches every score of the row"
    assert bool(torch.isnan(dirty[rows[0]]).all()) and bool(torch.isnan(dirty[:, cols[0]]).all())
    assert bits(dirty[~hit], got[~hit]), "a NaN or an infinity reaches no other row or column"


@pytest.mark.parametrize("d", sf.PAD_D)
def test_cosine_padding_branch(gpu, capsys, d):
    """cosine_matrix_device on D % 4 != 0 (LDA to 150 dimensions): judged on the unpadded operands with K = D, bit-equal to the result on
    operands the test pads with zeros, the caller's tensors unchanged."""
    worst = 0.0
    for ne, nt in sf.PAD_SHAPES:
        E, T = sf.cosine_operands(ne, nt, d)
        e, t = E.to(gpu), T.to(gpu)
        with device(f"cosine_matrix_device{ne, nt, d}"):
            got = iv_scoring.cosine_matrix_device(e, t)
            own = iv_scoring.cosine_matrix_device(sf.padded(E).to(gpu), sf.padded(T).to(gpu))
        assert got.shape == (ne, nt) and got.dtype == torch.float32
        assert e.shape == (ne, d) and t.shape == (nt, d) and torch.equal(e.cpu(), E) and torch.equal(t.cpu(), T), "the caller's tensors are unchanged"
        worst = max(worst, sf.check_cosine(f"cosine_matrix_device{ne, nt, d}", got.cpu(), E, T)[2])
        assert bits(got, own), "the bits of the zero-padded operands"
    _say(capsys, f"D = {d}: {worst:.3f} of 2 D u S")


# ---- sc_normalize_rows ------------------------------------------------------------------------------------------------------------------
def _normalize(gpu, x):
    xd = x.to(gpu).contiguous()
    frame, out = framed(gpu, *xd.shape)
    with device(f"sc_normalize_rows{tuple(xd.shape)}"):
        _lib.launch("sc_normalize_rows", gpu, xd, xd.shape[0], xd.shape[1], out, exc=AssertionError)
    assert intact(frame), "the border around the output is intact"
    return out.cpu()


@pytest.mark.parametrize("d", sf.NORM_D)
def test_normalize_rows_against_float64(gpu, capsys, d):
    """40 rows of magnitude 2^uniform(-20, 20), a zero row, a row of norm 1e-15 < eps; D on both sides of the 256-column stride and past two of them."""
    x = sf.normalize_operands(d)
    got = _normalize(gpu, x)
    share = sf.check_normalize(f"sc_normalize_rows D = {d}", got, x)
    _say(capsys, f"D = {d}: {share:.3f} of (D + 4) u |r|")
    assert bool((got[sf.NORM_ZERO_ROW] == 0).all())
    tiny = x[sf.NORM_TINY_ROW].double() / 1e-12
    assert float((got[sf.NORM_TINY_ROW].double() - tiny).abs().max()) <= (d + 4) * sf.U32 * float(tiny.abs().max()), "below eps: x / eps"
    for i in (0, sf.NORM_ZERO_ROW, sf.NORM_TINY_ROW, sf.NORM_ROWS - 1):
        assert bits(_normalize(gpu, x[i:i + 1])[0], got[i]), f"row {i} alone and inside the batch"


# ---- sc_cosine_trials -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", sf.TRIAL_D)
def test_cosine_trials_against_float64(gpu, capsys, d):
    """D around a wave's 64 lanes and past eight strides of them; n around the four trials of a workgroup and 1001; repeats, the first and
    last rows of E and T, and one trial that names a zero vector: NaN there and nowhere else (check_trials)."""
    worst = 0.0
    for n in sf.TRIAL_N:
        E, T, ei, ti = sf.trials_operands(d, n)
        out = torch.full((n + 1,), SENTINEL, dtype=torch.float64, device=gpu)
        with device(f"sc_cosine_trials(D = {d}, n = {n})"):
            _lib.launch("sc_cosine_trials", gpu, E.to(gpu), T.to(gpu), d, torch.from_numpy(ei).to(gpu), torch.from_numpy(ti).to(gpu), n, out[:n])
        assert float(out[n]) == SENTINEL, "the element after out[n - 1] is intact"
        worst = max(worst, sf.check_trials(f"sc_cosine_trials(D = {d}, n = {n})", out[:n].cpu().numpy(), E, T, ei, ti))
    _say(capsys, f"D = {d}: {worst:.3f} of 2 (D + 6) 2^-53 S / (|e| |t|)")


# ---- sc_topk_stats / sc_topk_stats_f64 --------------------------------------------------------------------------------------------------
def _topk(gpu, x, k):
    """one call on the rows x (numpy) -> (rc, mean, std); the outputs lie between sentinel elements"""
    xd = torch.from_numpy(x).to(gpu)
    n = x.shape[0]
    frame = torch.full((2, n + 2), SENTINEL, dtype=xd.dtype, device=gpu)
    name = "sc_topk_stats" if x.dtype == numpy.float32 else "sc_topk_stats_f64"
    with device(f"{name}{x.shape}, k = {k}"):
        rc = getattr(_lib.lib(), name)(xd.data_ptr(), n, x.shape[1], k, frame[0, 1:].data_ptr(), frame[1, 1:].data_ptr(), _stream(gpu))
    assert bool((frame[:, 0] == SENTINEL).all()) and bool((frame[:, -1] == SENTINEL).all()), "the border around the outputs is intact"
    return rc, frame[0, 1:n + 1].cpu().numpy(), frame[1, 1:n + 1].cpu().numpy()


@pytest.mark.parametrize("dtype,family", [(t, f) for t in ("float32", "float64") for f in sf.TOPK_FAMILIES[t]])
def test_topk_stats_against_float64(gpu, capsys, dtype, family):
    """Mean and unbiased std of the k largest values against numpy.longdouble at every (ncols, k) of scoring_f64.topk_cases(): five rows of
    the family -- (a) 0.3 N(0, 1) + U(-1, 1) per row, (b) -600 + N(0, 1), (c) 1e4 + 1e-2 N(0, 1) -- and the constructed rows of
    scoring_f64.topk_rows.  The std bound (u_T + (k + 8) 2^-52) r has no conditioning term.

    Measured on one MI355X with the one-pass variance (sum v^2 - k m^2) / (k - 1) this kernel had before: float32 passed; float64 used up to
    1.4e7 (a), 5.8e9 (b) and 1.5e13 (c) times the std bound, and k equal values of -598.0 had a std of 8.0e-6.  With the centred second
    pass: 0.159 (a), 0.215 (b), 0.055 (c) of the bound."""
    worst_m, worst_s, failures = 0.0, 0.0, []
    for ncols, k in sf.topk_cases():
        x, names = sf.topk_rows(ncols, k, family, dtype)
        rc, mean, std = _topk(gpu, x, k)
        assert rc == _lib.SK_OK, _lib.last_error()
        ms, ss = sf.topk_shares(mean, std, x, k)
        worst_m, worst_s = max(worst_m, float(ms.max())), max(worst_s, float(ss.max()))
        if not ((ms <= 1).all() and (ss <= 1).all()):
            i = int(numpy.argmax(numpy.maximum(ms, ss)))
            failures.append(f"({ncols}, {k}) row {i} ({names[i]}): mean {float(ms[i]):.3g}, std {float(ss[i]):.3g} of its bound")
        eq = names.index("equal")             # k equal values: exactly 0 in float32, at most the mean's last-place error in float64
        cap = 0.0 if dtype == "float32" else 4 * 2.0 ** -52 * abs(float(x[eq].max()))
        if not 0.0 <= std[eq] <= cap:
            failures.append(f"({ncols}, {k}) row {eq} (equal): std {std[eq]:.3g} on {k} copies of {float(x[eq].max())!r}, allowed {cap:.3g}")
        rc2, mean2, std2 = _topk(gpu, x, k)
        assert rc2 == _lib.SK_OK and numpy.array_equal(mean2.view(numpy.uint8), mean.view(numpy.uint8)) and numpy.array_equal(
            std2.view(numpy.uint8), std.view(numpy.uint8)), "two runs give the same bits"
        for i in range(len(names)):
            _, m1, s1 = _topk(gpu, x[i:i + 1], k)
            assert m1.tobytes() == mean[i:i + 1].tobytes() and s1.tobytes() == std[i:i + 1].tobytes(), f"({ncols}, {k}) row {i} alone and inside the batch"
    _say(capsys, f"{dtype} ({family}): mean {worst_m:.3g} of u_T |r| + (k + 2) 2^-53 A, std {worst_s:.3g} of (u_T + (k + 8) 2^-52) r")
    assert not failures, f"{len(failures)} rows outside their bounds (the worst of each of the {len(sf.topk_cases())} cases): " + "; ".join(failures)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_topk_stats_refuse_k_outside_the_row(gpu, dtype):
    """k = 1 (no unbiased std) and k = ncols + 1 return SK_EARG with nothing launched: the outputs keep what they held."""
    x = sf.topk_rows(119, 7, "a", dtype)[0]
    for k in (1, 120, 0, -3):
        rc, mean, std = _topk(gpu, x, k)
        assert rc == _lib.SK_EARG and "1 < k <= n_cols" in _lib.last_error()
        assert (mean == SENTINEL).all() and (std == SENTINEL).all()


# ---- cosine histograms with a k-tail ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", sf.HIST_D)
def test_cosine_histograms_with_a_k_tail(gpu, d):
    """cosine_hist_kernel has k < D guards of its own: D = 36 and 132 (a 4-wide tail after one and after four k-tiles), N = 300 (two ragged
    256-tiles).  The counts are those of binning sc_cosine's matrix (judged above), by the expression of
    tests/test_gpu_scoring.py::test_cosine_histograms_match_the_score_matrix.  UNIT rows here: the histogram's range is [-1, 1)."""
    n = sf.HIST_N
    rs = numpy.random.RandomState(d)
    lab = rs.randint(0, 12, n).astype(numpy.int32)
    X = torch.nn.functional.normalize(torch.from_numpy(rs.randn(12, d)[lab] + 1.3 * rs.randn(n, d)).float(), dim=1).to(gpu)
    S = _cosine(gpu, X, X).numpy()
    nb = iv_scoring.HIST_BINS
    b = numpy.clip(numpy.floor((S - numpy.float32(-1.0)) * numpy.float32(nb / 2.0)).astype(numpy.int64), 0, nb - 1)
    tar, off = lab[:, None] == lab[None, :], ~numpy.eye(n, dtype=bool)
    with device(f"cosine_histograms(N = {n}, D = {d})"):
        ht, hn = iv_scoring.cosine_histograms(X, X, lab, lab, self_offset=0)
        lo, hi = 100, 250
        ht2, hn2 = iv_scoring.cosine_histograms(X[lo:hi], X, lab[lo:hi], lab, self_offset=lo)
    assert int(ht.sum() + hn.sum()) == n * n - n and len(numpy.unique(b)) > 100
    assert numpy.array_equal(ht, numpy.bincount(b[tar & off], minlength=nb)) and numpy.array_equal(hn, numpy.bincount(b[~tar], minlength=nb))
    assert numpy.array_equal(ht2, numpy.bincount(b[lo:hi][(tar & off)[lo:hi]], minlength=nb))
    assert numpy.array_equal(hn2, numpy.bincount(b[lo:hi][~tar[lo:hi]], minlength=nb))


# ---- 16-byte alignment ------------------------------------------------------------------------------------------------------------------
def test_operands_off_a_16_byte_boundary(gpu):
    """sc_cosine, sc_cosine_hist, sc_cosine_hist_norm and sc_cohort_moments read rows with 16-byte loads: a view that starts 4 bytes into a
    buffer is refused (SK_EARG before anything is enqueued: the outputs keep what they held), and the Python layer hands over an aligned
    copy of it.  No kernel ever runs on a misaligned pointer."""
    ne, nt, d = 70, 33, 36
    E, T = (torch.nn.functional.normalize(x, dim=1) for x in sf.cosine_operands(ne, nt, d))
    flat = torch.cat([torch.zeros(1), E.reshape(-1), T.reshape(-1)]).to(gpu)
    e, t = flat[1:1 + ne * d].view(ne, d), flat[1 + ne * d:].view(nt, d)
    ok_e, ok_t = e.clone(), t.clone()
    assert e.data_ptr() % 16 == 4 and t.data_ptr() % 16 == 4 and ok_e.data_ptr() % 16 == 0 and ok_t.data_ptr() % 16 == 0 and e.is_contiguous()
    lib, st = _lib.lib(), _stream(gpu)
    le, lt = (torch.arange(n, dtype=torch.int32, device=gpu) % 5 for n in (ne, nt))
    out = torch.full((ne, nt), SENTINEL, device=gpu)
    hists = torch.full((2, iv_scoring.HIST_BINS), 7, dtype=torch.int64, device=gpu)
    stats = torch.full((4, ne), SENTINEL, device=gpu)
    ones = torch.ones(max(ne, nt), device=gpu)
    for a, b in ((e, ok_t), (ok_e, t)):
        calls = {
            "sc_cosine": lambda: lib.sc_cosine(a.data_ptr(), ne, b.data_ptr(), nt, d, out.data_ptr(), st),
            "sc_cosine_hist": lambda: lib.sc_cosine_hist(a.data_ptr(), ne, b.data_ptr(), nt, d, le.data_ptr(), lt.data_ptr(), -1, -1.0, 1.0,
                                                         iv_scoring.HIST_BINS, hists[0].data_ptr(), hists[1].data_ptr(), st),
            "sc_cosine_hist_norm": lambda: lib.sc_cosine_hist_norm(a.data_ptr(), ne, b.data_ptr(), nt, d, le.data_ptr(), lt.data_ptr(), -1, ones.data_ptr(),
                                                                   ones.data_ptr(), None, None, -4.0, 4.0, iv_scoring.HIST_BINS,
                                                                   hists[0].data_ptr(), hists[1].data_ptr(), st),
            "sc_cohort_moments": lambda: lib.sc_cohort_moments(a.data_ptr(), ne, b.data_ptr(), nt, d, None, None, -1, stats[0].data_ptr(),
                                                               stats[1].data_ptr(), st),
        }
        for name, call in calls.items():
            assert call() == _lib.SK_EARG and f"{name}: operands must be 16-byte aligned" in _lib.last_error(), name
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((hists == 7).all()) and bool((stats == SENTINEL).all()), "nothing was enqueued"
    with device("the Python route on an offset view"):
        got, want = iv_scoring.cosine_matrix_device(e, t), iv_scoring.cosine_matrix_device(ok_e, ok_t)
        h, hw = iv_scoring.cosine_histograms(e, t, le, lt), iv_scoring.cosine_histograms(ok_e, ok_t, le, lt)
    assert bits(got, want) and bits(want.cpu(), _cosine(gpu, ok_e, ok_t))
    assert all(numpy.array_equal(x, y) for x, y in zip(h, hw)) and int(h[0].sum() + h[1].sum()) == ne * nt
    assert e.data_ptr() % 16 == 4 and torch.equal(e, ok_e) and torch.equal(t, ok_t), "the caller's views are unchanged"
