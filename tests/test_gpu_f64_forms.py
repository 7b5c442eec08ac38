"""The float64 back end one entry point at a time: the TN, NN and gathered-centre forms of csrc/dgemm_tile.h behind sc_gemm_tn,
sc_scatter_within, sc_class_scatter, sc_tv_gram, sc_dgemm_nn and sc_gauss_loglik, and sc_whiten_rows' tile on the same loaders, each against a
numpy.longdouble evaluation of the SAME operands under a per-element bound (tests/tools/f64_forms.py, where operands, references, criteria
and shapes are stated).  tests/test_f64_forms_reference_cpu.py shows on these operands that float64 numpy passes every criterion and that
the wrong kernels listed there do not.

The entry points are called through _lib.lib() on device buffers the test made; every output is a view between two sentinel rows of a larger
buffer whose border must be intact afterwards, and the inputs must hold what they held.  A HIP error ends the session (returncode 3):
nothing more is started on the device.  Every comparison prints the largest share of its bound it used; DESIGN.md section 4h has the table.
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
import f64_forms as ff  # noqa: E402

from sidekit_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = ff.SENTINEL
XT = {"float32": _lib.XT_F32, "float64": _lib.XT_F64}


def ids(s):
    return "x".join(ids(v) if isinstance(v, tuple) else str(v) for v in s) if isinstance(s, tuple) else str(s)


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


def _ok(rc, what):
    if rc == _lib.SK_EHIP:
        pytest.exit(f"{what} failed on the device: {_lib.last_error()}", returncode=3)
    assert rc == _lib.SK_OK, f"{what}: {_lib.last_error()}"


def same_bits(a, b):
    """the same bytes (a NaN equals only the same NaN)"""
    a, b = numpy.ascontiguousarray(a), numpy.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def framed(gpu, rows, cols, dtype=torch.float64):
    """(frame, the view of its rows 1 .. rows): an output between two sentinel rows"""
    frame = torch.full((rows + 2, cols), SENTINEL, dtype=dtype, device=gpu)
    return frame, frame[1:rows + 1]


def intact(frame):
    return bool((frame[0] == SENTINEL).all()) and bool((frame[-1] == SENTINEL).all())


def _stream(gpu):
    return ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)


class Inputs:
    """device copies of numpy operands; a name in ``shift`` starts one element (8 bytes of float64, 4 of float32) into a larger buffer, off
    the boundary a pair load needs.  unchanged(): every copy still holds its operand."""

    def __init__(self, gpu, shift=(), **arrays):
        self.host, self.dev = arrays, {}
        assert set(shift) <= set(arrays)
        for name, x in arrays.items():
            if x is None:
                self.dev[name] = None
                continue
            t = torch.from_numpy(numpy.ascontiguousarray(x))
            if name in shift:
                buf = torch.zeros(t.numel() + 3, dtype=t.dtype, device=gpu)
                d = buf[1:1 + t.numel()].view(t.shape)
                d.copy_(t)
                assert d.data_ptr() % (2 * t.element_size()) == t.element_size() and d.is_contiguous()
            else:
                d = t.to(gpu)
                assert d.data_ptr() % 16 == 0
            self.dev[name] = d

    def ptr(self, name):
        return None if self.dev[name] is None else self.dev[name].data_ptr()

    def unchanged(self):
        return all(d is None or same_bits(d.cpu().numpy(), self.host[n]) for n, d in self.dev.items())


# ---- one call of each entry point on numpy operands -> the output on the host -------------------------------------------------------------
def gemm_tn(gpu, A, B, w=None, ca=None, cb=None, shift=(), same=False):
    """``same``: B is A's buffer"""
    (K, M), N = A.shape, B.shape[1]
    ins = Inputs(gpu, shift, A=A, B=None if same else B, w=w, ca=ca, cb=cb)
    frame, out = framed(gpu, M, N)
    what = f"sc_gemm_tn{K, M, N}"
    with device(what):
        _ok(_lib.lib().sc_gemm_tn(ins.ptr("A"), ins.ptr("A" if same else "B"), XT[str(A.dtype)], K, M, N, ins.ptr("w"), ins.ptr("ca"), ins.ptr("cb"),
                                  out.data_ptr(), _stream(gpu)), what)
    assert intact(frame), f"{what}: the border around the output is intact"
    assert ins.unchanged(), f"{what}: the operands are unchanged"
    return out.cpu().numpy()


def scatter_within(gpu, X, cls, Mc, w, C, shift=()):
    N, D = X.shape
    ins = Inputs(gpu, shift, X=X, cls=cls, Mc=Mc, w=w)
    frame, out = framed(gpu, D, D)
    what = f"sc_scatter_within{N, D}"
    with device(what):
        _ok(_lib.lib().sc_scatter_within(ins.ptr("X"), XT[str(X.dtype)], N, D, ins.ptr("cls"), ins.ptr("Mc"), ins.ptr("w"), C, out.data_ptr(), _stream(gpu)), what)
    assert intact(frame), f"{what}: the border around the output is intact"
    assert ins.unchanged(), f"{what}: the operands are unchanged"
    return out.cpu().numpy()


def class_scatter(gpu, X, off, Mc, shift=()):
    (N, D), C = X.shape, len(Mc)
    ins = Inputs(gpu, shift, X=X, off=off, Mc=Mc)
    frame, out = framed(gpu, C * D, D)
    what = f"sc_class_scatter{tuple(int(v) for v in numpy.diff(off)), D}"
    with device(what):
        _ok(_lib.lib().sc_class_scatter(ins.ptr("X"), XT[str(X.dtype)], N, D, ins.ptr("off"), ins.ptr("Mc"), C, int(numpy.diff(off).max()), out.data_ptr(),
                                        _stream(gpu)), what)
    assert intact(frame), f"{what}: the border around the output is intact"
    assert ins.unchanged(), f"{what}: the operands are unchanged"
    return out.cpu().numpy().reshape(C, D, D)


def tv_gram(gpu, F, shift=()):
    """[C][R (R + 1) / 2]: one call for all components into a buffer with a sentinel element before and after"""
    C, D, R = F.shape
    P = R * (R + 1) // 2
    ins = Inputs(gpu, shift, F=F)
    buf = torch.full((C * P + 2,), SENTINEL, dtype=torch.float64, device=gpu)
    what = f"sc_tv_gram{C, D, R}"
    with device(what):
        _ok(_lib.lib().sc_tv_gram(ins.ptr("F"), C, D, R, buf[1:].data_ptr(), _stream(gpu)), what)
    assert float(buf[0]) == SENTINEL and float(buf[-1]) == SENTINEL, f"{what}: the elements around the output are intact"
    assert ins.unchanged(), f"{what}: the operand is unchanged"
    return buf[1:-1].cpu().numpy().reshape(C, P)


def dgemm_nn(gpu, A, B, alpha, rowv, colv, epi, shift=()):
    (M, K), N = A.shape, B.shape[1]
    ins = Inputs(gpu, shift, A=A, B=B, rowv=rowv, colv=colv)
    frame, out = framed(gpu, M, N)
    what = f"sc_dgemm_nn{M, N, K}"
    with device(what):
        _ok(_lib.lib().sc_dgemm_nn(ins.ptr("A"), ins.ptr("B"), M, N, K, alpha, ins.ptr("rowv"), ins.ptr("colv"), epi, out.data_ptr(), _stream(gpu)), what)
    assert intact(frame), f"{what}: the border around the output is intact"
    assert ins.unchanged(), f"{what}: the operands are unchanged"
    return out.cpu().numpy()


def whiten_rows(gpu, X, mu, R, normalize, ytype="float64", shift=()):
    (N, D), P = X.shape, R.shape[1]
    ins = Inputs(gpu, shift, X=X, mu=mu, R=R)
    frame, out = framed(gpu, N, P, torch.float32 if ytype == "float32" else torch.float64)
    what = f"sc_whiten_rows{N, D, P}"
    with device(what):
        _ok(_lib.lib().sc_whiten_rows(ins.ptr("X"), XT[str(X.dtype)], N, D, ins.ptr("mu"), ins.ptr("R"), P, normalize, out.data_ptr(), XT[ytype], _stream(gpu)), what)
    assert intact(frame), f"{what}: the border around the output is intact"
    assert ins.unchanged(), f"{what}: the operands are unchanged"
    return out.cpu().numpy()


def gauss_loglik(gpu, X, means, W, cst):
    """[C][N]"""
    (N, D), C = X.shape, len(means)
    ins = Inputs(gpu, (), X=X, means=means, W=W, cst=cst)
    frame, out = framed(gpu, C, N)
    what = f"sc_gauss_loglik{N, D, C}"
    with device(what):
        _ok(_lib.lib().sc_gauss_loglik(ins.ptr("X"), N, D, ins.ptr("means"), ins.ptr("W"), ins.ptr("cst"), C, out.data_ptr(), _stream(gpu)), what)
    assert intact(frame), f"{what}: the border around the output is intact"
    assert ins.unchanged(), f"{what}: the operands are unchanged"
    return out.cpu().numpy()


def _rows_of(n, edge=64):
    """the first row, the last of one tile and the first of the next, the last row"""
    return sorted({i for i in (0, edge - 1, edge, n - 1) if 0 <= i < n})


# ---- sc_gemm_tn ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ff.DTYPES)
@pytest.mark.parametrize("shape", ff.TN_SHAPES, ids=ids)
def test_gemm_tn_against_longdouble(gpu, capsys, shape, dtype):
    """The smallest problem; one tile and one k-tile; one past and one short (odd: scalar loads); less than one k-tile with pair loads and three
    column tiles; the first second slab; the smallest 128-tile launch, just below it on either side, and a ragged one of nine slabs -- plain,
    weighted, with ca alone and with w, ca and cb."""
    worst = {}
    for form in ff.TN_FORMS:
        case, r, bound = ff.tn(shape, form, dtype)
        got = gemm_tn(gpu, **case)
        worst[form] = ff.check(f"sc_gemm_tn{shape} {form} {dtype}", got, r, bound)
    assert same_bits(gemm_tn(gpu, **case), got), "two runs give the same bits"
    _say(capsys, f"{shape} {dtype}: " + ", ".join(f"{f} {s:.3f}" for f, s in worst.items()) + " of (K + 8) u S")


@pytest.mark.parametrize("dtype", ff.DTYPES)
def test_gemm_tn_rows_past_k_add_exact_zeros_beside_large_centres(gpu, capsys, dtype):
    """K = 17 leaves 15 zero-filled rows in the second k-tile.  With centres of 1e6 each of them would add (0 - ca)(0 - cb) = 1e12 unless its
    weight is an exact 0; the bound is taken after centring and is that of the case without the shift."""
    shape = (17, 65, 63)
    case, _, small = ff.tn(shape, "w+ca+cb", dtype)
    big = dict(case, A=(case["A"].astype(numpy.float64) + 1e6).astype(dtype), B=(case["B"].astype(numpy.float64) + 1e6).astype(dtype),
               ca=case["ca"] + 1e6, cb=case["cb"] + 1e6)
    r, bound = ff.tn_ref(**big)
    assert shape[0] % ff.DK != 0
    if dtype == "float64":               # float32 operands near 1e6 are multiples of 1/16: their centred values are other numbers, not larger bounds
        assert float((bound / small).max()) < 4.0, "the bound does not grow with the centres"
    share = ff.check(f"sc_gemm_tn{shape} centres of 1e6 {dtype}", gemm_tn(gpu, **big), r, bound)
    _say(capsys, f"{dtype}: {share:.3f} of (K + 8) u S")


@pytest.mark.parametrize("shape", [s for s in ff.TN_SHAPES if s[0] <= ff.SLAB_K and s[1] > 1], ids=ids)
def test_gemm_tn_row_alone_and_inside_the_batch(gpu, shape):
    """One slab (K <= 512): row m of G has the bits of the product on column m of A alone."""
    for form, dtype in (("w+ca+cb", "float64"), ("plain", "float32")):
        case = ff.tn(shape, form, dtype)[0]
        G = gemm_tn(gpu, **case)
        for m in _rows_of(shape[1]):
            one = dict(case, A=numpy.ascontiguousarray(case["A"][:, m:m + 1]), ca=None if case["ca"] is None else case["ca"][m:m + 1])
            assert same_bits(gemm_tn(gpu, **one)[0], G[m]), f"row {m} alone and inside the batch ({form}, {dtype})"


@pytest.mark.parametrize("dtype", ff.DTYPES)
@pytest.mark.parametrize("shape", [(17, 65, 63), (513, 6, 5), (4097, 129, 130)], ids=ids)
def test_gemm_tn_with_b_equal_to_a_is_symmetric(gpu, capsys, shape, dtype):
    """B = A's buffer, cb = ca: G and its transpose have the same bits (a product commutes and both elements add the same products in the
    same order).  With a weight the two factors of a product are w a[m] and a[n], rounded differently from w a[n] and a[m]: there the two
    elements agree within twice their bound, and how many differ in bits is printed, not asserted."""
    for form in ("plain", "ca"):
        case = ff.tn(shape, form, dtype)[0]
        G = gemm_tn(gpu, case["A"], case["A"], None, case["ca"], case["ca"], same=True)
        assert same_bits(G, G.T), f"B = A gives a symmetric matrix bit for bit ({form})"
    case = ff.tn(shape, "w+ca+cb", dtype)[0]
    G = gemm_tn(gpu, case["A"], case["A"], case["w"], case["ca"], case["ca"], same=True)
    r, bound = ff.tn_ref(case["A"], case["A"], case["w"], case["ca"], case["ca"])
    ff.check("weighted, B = A", G, r, bound)
    ff.check("weighted, B = A, transposed", G.T, r, bound)
    _say(capsys, f"{shape} {dtype}: weighted, {int((G != G.T).sum())} of {G.size} elements differ from their mirror image in bits")


@pytest.mark.parametrize("dtype", ff.DTYPES)
@pytest.mark.parametrize("shape", [(17, 65, 63), (513, 6, 5)], ids=ids)
def test_gemm_tn_a_nan_stays_in_its_row(gpu, shape, dtype):
    """One NaN in A[k][m] makes exactly row m of G non-finite; with B = A's buffer, row and column m.  Every other element keeps its bits."""
    K, M, _ = shape
    case = ff.tn(shape, "w+ca+cb", dtype)[0]
    clean = gemm_tn(gpu, **case)
    for k, m in ((K - 1, 0), (0, M - 1), (K // 2, M // 2)):
        A = case["A"].copy()
        A[k, m] = numpy.nan
        dirty = gemm_tn(gpu, **dict(case, A=A))
        assert numpy.isnan(dirty[m]).all(), f"a NaN in A[{k}][{m}] reaches every element of row {m}"
        keep = numpy.arange(M) != m
        assert same_bits(dirty[keep], clean[keep]), f"a NaN in A[{k}][{m}] reaches no other row"
    sym = gemm_tn(gpu, case["A"], case["A"], case["w"], case["ca"], case["ca"], same=True)
    dirty = gemm_tn(gpu, A, A, case["w"], case["ca"], case["ca"], same=True)
    hit = numpy.zeros((M, M), dtype=bool)
    hit[m], hit[:, m] = True, True
    assert numpy.isnan(dirty[hit]).all() and same_bits(dirty[~hit], sym[~hit]), "B = A: exactly row and column m"


# ---- sc_scatter_within: the gathered centre -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ff.DTYPES)
@pytest.mark.parametrize("shape", ff.GATHERED_SHAPES, ids=ids)
def test_scatter_within_against_longdouble(gpu, capsys, shape, dtype):
    """One row that is its class's mean (exactly 0); one tile; odd; two slabs; the 128-tile form, whole and ragged.  From N = 16 on one class
    holds a single row that is its mean, cls[1] = -1 and cls[N - 2] = C + 5."""
    worst = {}
    for weighted in (False, True):
        case, r, bound = ff.gathered(shape, weighted, dtype)
        got = scatter_within(gpu, **case)
        worst[weighted] = ff.check(f"sc_scatter_within{shape} w={weighted} {dtype}", got, r, bound)
        if not weighted:
            assert same_bits(got, got.T), "B = A gives a symmetric matrix bit for bit"
    assert same_bits(scatter_within(gpu, **case), got), "two runs give the same bits"
    if shape[0] > 1:
        C, single = case["C"], shape[0] // 2
        assert case["cls"][single] == C - 1
        w = case["w"].copy()
        w[C - 1] = 1e300
        assert same_bits(scatter_within(gpu, **dict(case, w=w)), got), "a single-row class adds exact zeros whatever its weight"
        X = case["X"].copy()
        X[1], X[shape[0] - 2] = numpy.nan, numpy.inf
        assert same_bits(scatter_within(gpu, **dict(case, X=X)), got), "a row whose class number is out of range is not read"
        Mc = case["Mc"].copy()
        X = case["X"].copy()
        X[single, 0] = numpy.nan
        dirty = scatter_within(gpu, **dict(case, X=X))
        assert numpy.isnan(dirty[0]).all() and numpy.isnan(dirty[:, 0]).all() and same_bits(dirty[1:, 1:], got[1:, 1:]), "a NaN reaches row and column 0 only"
        assert same_bits(Mc, case["Mc"])
    _say(capsys, f"{shape} {dtype}: plain {worst[False]:.3f}, weighted {worst[True]:.3f} of (K + 8) u S")


# ---- sc_class_scatter -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ff.DTYPES)
@pytest.mark.parametrize("counts,D", ff.CLASS_SHAPES, ids=ids)
def test_class_scatter_against_longdouble(gpu, capsys, counts, D, dtype):
    """Classes of 1, 15, 16, 17 and 600 rows (two slabs; four classes end before the second one and store zeros there); D = 65 with a class
    of one row; the 128-tile form with eight slabs beside a class of one row.  K is each class's own count."""
    case, r, bound = ff.classes(counts, D, dtype)
    X, off, Mc = case["X"], case["off"], case["Mc"]
    got = class_scatter(gpu, X, off, Mc)
    share = ff.check(f"sc_class_scatter{counts, D} {dtype}", got, r, bound)
    assert same_bits(class_scatter(gpu, X, off, Mc), got), "two runs give the same bits"
    slab = ff.tn_cut(max(counts), D, D, len(counts))[3]
    for c, n in enumerate(counts):
        assert same_bits(got[c], got[c].T), f"class {c}: a symmetric matrix bit for bit"
        if n <= slab:                    # no row in a second slab: its partial tiles past the first are zeros, the join adds them exactly
            assert ff.tn_cut(n, D, D)[2] == 1
            alone = class_scatter(gpu, numpy.ascontiguousarray(X[off[c]:off[c + 1]]), numpy.array([0, n], dtype=numpy.int32), Mc[c:c + 1])
            assert same_bits(alone[0], got[c]), f"class {c} alone (one slab) and inside the batch"
    _say(capsys, f"{counts, D} {dtype}: {share:.3f} of (count + 8) u S")


# ---- sc_tv_gram -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ff.GRAM_SHAPES, ids=ids)
def test_tv_gram_against_longdouble(gpu, capsys, shape):
    """R = 2 (D = 1), one tile, one past it with D one past a k-tile, three column tiles with pair loads, three whole tiles at the largest
    rank.  A sentinel element follows each component's triangle: every component is also computed alone into a buffer of its own."""
    C, D, R = shape
    case, r, bound = ff.gram(shape)
    got = tv_gram(gpu, case["F"])
    share = ff.check(f"sc_tv_gram{shape}", got, r, bound)
    assert same_bits(tv_gram(gpu, case["F"]), got), "two runs give the same bits"
    for c in range(C):
        assert same_bits(tv_gram(gpu, case["F"][c:c + 1])[0], got[c]), f"component {c} alone, a sentinel after its triangle, and inside the batch"
    F = case["F"].copy()
    F[C - 1, D - 1, R - 1] = numpy.nan
    dirty = tv_gram(gpu, F)
    iu = numpy.triu_indices(R)
    hit = numpy.zeros((C, len(iu[0])), dtype=bool)
    hit[C - 1] = iu[1] == R - 1                        # the upper triangle holds column R - 1 of row R - 1's mirror image
    assert numpy.isnan(dirty[hit]).all() and same_bits(dirty[~hit], got[~hit]), "a NaN in column R - 1 of one component reaches that column alone"
    _say(capsys, f"{shape}: {share:.3f} of (D + 8) u S")


# ---- sc_dgemm_nn ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ff.NN_SHAPES, ids=ids)
def test_dgemm_nn_against_longdouble(gpu, capsys, shape):
    """The plain form and both epilogues at the smallest problem, one tile and one k-tile, one past and one short (K and N odd: scalar loads),
    three column tiles with pair loads, three row tiles with four whole k-tiles."""
    M, N, K = shape
    worst = {}
    for epi in ff.NN_EPILOGUES:
        case, r, bound = ff.nn(shape, epi)
        got = dgemm_nn(gpu, **case)
        worst[epi] = ff.check(f"sc_dgemm_nn{shape} {epi}", got, r, bound)
        assert same_bits(dgemm_nn(gpu, **case), got), "two runs give the same bits"
        vec = lambda v, s: None if v is None else numpy.ascontiguousarray(v[s])  # noqa: E731
        for i in _rows_of(M):
            one = dict(case, A=numpy.ascontiguousarray(case["A"][i:i + 1]), rowv=vec(case["rowv"], slice(i, i + 1)))
            assert same_bits(dgemm_nn(gpu, **one)[0], got[i]), f"row {i} of A alone and inside the batch ({epi})"
        for j in _rows_of(N):
            one = dict(case, B=numpy.ascontiguousarray(case["B"][:, j:j + 1]), colv=vec(case["colv"], slice(j, j + 1)))
            assert same_bits(dgemm_nn(gpu, **one)[:, 0], got[:, j]), f"column {j} of B alone and inside the batch ({epi})"
        B = case["B"].copy()
        j = N // 2
        B[K - 1, j] = numpy.nan
        dirty = dgemm_nn(gpu, **dict(case, B=B))
        keep = numpy.arange(N) != j
        assert numpy.isnan(dirty[:, j]).all() and same_bits(dirty[:, keep], got[:, keep]), f"a NaN in B[{K - 1}][{j}] reaches column {j} alone ({epi})"
    _say(capsys, f"{shape}: plain {worst['plain']:.3f} and rank-one {worst['rank1']:.3f} of (K + 4) u (|alpha| S + |rowv colv|), "
                 f"posterior {worst['posterior']:.3f} of (K + 6) u |alpha| S / (1 + t)")


# ---- sc_whiten_rows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ff.DTYPES)
@pytest.mark.parametrize("shape", ff.WHITEN_SHAPES, ids=ids)
def test_whiten_rows_against_longdouble(gpu, capsys, shape, dtype):
    """64, 128 and 256 columns per workgroup at their last column and one past it; 257 columns: the two-pass form when normalising.  With
    and without mu, with and without normalising; the float32 output is the float64 output rounded once (bits)."""
    N, D, P = shape
    worst = {}
    for centred in (False, True):
        for normalize in (0, 1):
            case, r, bound = ff.whiten(shape, centred, dtype, normalize)
            X, mu, R = case["X"], case["mu"], case["R"]
            got = whiten_rows(gpu, X, mu, R, normalize)
            key = ("mu, " if centred else "") + ("normalised" if normalize else "plain")
            worst[key] = ff.check(f"sc_whiten_rows{shape} {key} {dtype}", got, r, bound)
            assert same_bits(whiten_rows(gpu, X, mu, R, normalize, "float32"), got.astype(numpy.float32)), "float32 output: the float64 result rounded once"
            if N >= ff.WHITEN_ROWS:
                assert (got[ff.WHITEN_ZERO_ROW] == 0).all(), "a row equal to mu gives exact zeros"
            if case["tiny"] is not None and normalize:
                plain = ff.whiten(shape, centred, dtype, 0)[1][case["tiny"]]
                assert 0 < float(numpy.sqrt((plain * plain).sum())) < ff.EPS_LEN / 2
                assert float(ff.shares(got[case["tiny"]], plain / ff.LD(ff.EPS_LEN), bound[case["tiny"]]).max()) <= 1, "a row shorter than 1e-8 gives v / 1e-8"
            for i in _rows_of(N, ff.WHITEN_ROWS):
                assert same_bits(whiten_rows(gpu, X[i:i + 1], mu, R, normalize)[0], got[i]), f"row {i} alone and inside the batch ({key})"
    case = ff.whiten(shape, True, dtype, 1)[0]
    clean = whiten_rows(gpu, case["X"], case["mu"], case["R"], 1)
    assert same_bits(clean, got), "two runs give the same bits"
    X = case["X"].copy()
    i = N - 1
    X[i, D // 2] = numpy.nan
    dirty = whiten_rows(gpu, X, case["mu"], case["R"], 1)
    keep = numpy.arange(N) != i
    assert numpy.isnan(dirty[i]).all() and same_bits(dirty[keep], clean[keep]), f"a NaN in row {i} of X reaches that row alone"
    _say(capsys, f"{shape} {dtype}: " + ", ".join(f"{k} {s:.3f}" for k, s in worst.items()))


# ---- sc_gauss_loglik ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ff.LOGLIK_SHAPES, ids=ids)
def test_gauss_loglik_against_longdouble(gpu, capsys, shape):
    """The smallest problem; a second column tile one column wide; three column tiles with pair loads; the 128-row form with one row and with a
    second, ragged row tile."""
    N, D, C = shape
    case, r, bound = ff.loglik(shape)
    X, means, W, cst = case["X"], case["means"], case["W"], case["cst"]
    got = gauss_loglik(gpu, X, means, W, cst)
    share = ff.check(f"sc_gauss_loglik{shape}", got, r, bound)
    assert same_bits(gauss_loglik(gpu, X, means, W, cst), got), "two runs give the same bits"
    for n in _rows_of(N):
        assert same_bits(gauss_loglik(gpu, X[n:n + 1], means, W, cst)[:, 0], got[:, n]), f"row {n} alone and inside the batch"
    for c in sorted({0, C // 2, C - 1}):
        assert same_bits(gauss_loglik(gpu, X, means[c:c + 1], W[c:c + 1], cst[c:c + 1])[0], got[c]), f"class {c} alone and inside the batch"
    Xn = X.copy()
    n = N // 2
    Xn[n, D - 1] = numpy.nan
    dirty = gauss_loglik(gpu, Xn, means, W, cst)
    keep = numpy.arange(N) != n
    assert numpy.isnan(dirty[:, n]).all() and same_bits(dirty[:, keep], got[:, keep]), f"a NaN in row {n} of X reaches column {n} alone"
    _say(capsys, f"{shape}: {share:.3f} of sum |y| dy + (P + 4) u q / 2 + u (|cst| + |r|)")


# ---- views off the pair-load boundary -------------------------------------------------------------------------------------------------------
def test_views_off_the_pair_load_boundary(gpu):
    """Every pair load of these paths sits behind a predicate on its row length and its base pointer (vec_a, vec_b, vec_c in dgemm_tile.h;
    vec_x, vec_mu, vec_r in whiten_rows_kernel); w, cs, rowv, colv, cst and V are read one element at a time and every store is a single
    element.  Here the row lengths are even, so an aligned base takes the pair loads, and each operand in turn starts 8 bytes (float64) or
    4 bytes (float32) into a larger buffer and takes the scalar fall-back: the bits are those of the aligned copies (the callers in this file
    also check that the operands are unchanged)."""
    for dtype in ff.DTYPES:
        case = ff.tn((15, 66, 130), "w+ca+cb", dtype)[0]
        want = gemm_tn(gpu, **case)
        for shift in (("A",), ("B",), ("w",), ("ca",), ("cb",), ("A", "B", "w", "ca", "cb")):
            assert same_bits(gemm_tn(gpu, shift=shift, **case), want), f"sc_gemm_tn {dtype}: {shift} off the boundary"
        want = gemm_tn(gpu, case["A"], case["A"], None, case["ca"], case["ca"], same=True)
        assert same_bits(gemm_tn(gpu, case["A"], case["A"], None, case["ca"], case["ca"], shift=("A",), same=True), want), f"sc_gemm_tn {dtype}, B = A off the boundary"
        case = ff.gathered((16, 64), True, dtype)[0]
        want = scatter_within(gpu, **case)
        for shift in (("X",), ("Mc",), ("w",), ("X", "Mc", "w")):
            assert same_bits(scatter_within(gpu, shift=shift, **case), want), f"sc_scatter_within {dtype}: {shift} off the boundary"
        case = ff.classes((1, 15, 16, 17, 600), 6, dtype)[0]
        want = class_scatter(gpu, case["X"], case["off"], case["Mc"])
        for shift in (("X",), ("Mc",), ("X", "Mc")):
            assert same_bits(class_scatter(gpu, case["X"], case["off"], case["Mc"], shift=shift), want), f"sc_class_scatter {dtype}: {shift} off the boundary"
        for shape in ((70, 36, 128), (66, 40, 256)):
            case = ff.whiten(shape, True, dtype, 1)[0]
            want = whiten_rows(gpu, case["X"], case["mu"], case["R"], 1)
            for shift in (("X",), ("mu",), ("R",), ("X", "mu", "R")):
                assert same_bits(whiten_rows(gpu, case["X"], case["mu"], case["R"], 1, shift=shift), want), f"sc_whiten_rows{shape} {dtype}: {shift} off the boundary"
    case = ff.nn((33, 130, 28), "rank1")[0]
    want = dgemm_nn(gpu, **case)
    for shift in (("A",), ("B",), ("rowv",), ("colv",), ("A", "B", "rowv", "colv")):
        assert same_bits(dgemm_nn(gpu, shift=shift, **case), want), f"sc_dgemm_nn: {shift} off the boundary"
    case = ff.gram((2, 16, 64))[0]
    assert same_bits(tv_gram(gpu, case["F"], shift=("F",)), tv_gram(gpu, case["F"])), "sc_tv_gram: F off the boundary"


# ---- argument errors ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched(gpu):
    """rowv without colv, the posterior epilogue without both, an unknown dtype, Y aliasing X: SK_EARG before anything is enqueued."""
    lib, st = _lib.lib(), _stream(gpu)
    case = ff.nn((33, 130, 28), "rank1")[0]
    M, N, K = 33, 130, 28
    ins = Inputs(gpu, (), **{k: case[k] for k in ("A", "B", "rowv", "colv")})
    frame, out = framed(gpu, M, N)
    a, b, rv, cv = (ins.ptr(k) for k in ("A", "B", "rowv", "colv"))
    assert lib.sc_dgemm_nn(a, b, M, N, K, 0.7, rv, None, _lib.SC_EPI_RANK1, out.data_ptr(), st) == _lib.SK_EARG and "come together" in _lib.last_error()
    assert lib.sc_dgemm_nn(a, b, M, N, K, 0.7, None, cv, _lib.SC_EPI_RANK1, out.data_ptr(), st) == _lib.SK_EARG
    assert lib.sc_dgemm_nn(a, b, M, N, K, 0.7, None, None, _lib.SC_EPI_POSTERIOR, out.data_ptr(), st) == _lib.SK_EARG
    assert lib.sc_dgemm_nn(a, b, M, N, K, 0.7, rv, cv, 2, out.data_ptr(), st) == _lib.SK_EARG and "unknown epilogue" in _lib.last_error()
    tn = ff.tn((15, 66, 130), "plain", "float64")[0]
    tin = Inputs(gpu, (), A=tn["A"], B=tn["B"])
    g_frame, g = framed(gpu, 66, 130)
    for bad in (_lib.XT_BF16, _lib.XT_I64, 7):
        assert lib.sc_gemm_tn(tin.ptr("A"), tin.ptr("B"), bad, 15, 66, 130, None, None, None, g.data_ptr(), st) == _lib.SK_EARG and "XT_F32 or XT_F64" in _lib.last_error()
    wc = ff.whiten((64, 16, 64), True, "float64", 0)[0]
    # X lives inside a framed buffer as wide as Y (D = 16 of P = 64 columns' worth of bytes per row do not matter: the ranges overlap)
    win = Inputs(gpu, (), mu=wc["mu"], R=wc["R"])
    y_frame, y = framed(gpu, 64, 64)
    x_inside = y.reshape(-1)[:64 * 16]
    for bad in (_lib.XT_BF16, 7):
        xin = Inputs(gpu, (), X=wc["X"])
        assert lib.sc_whiten_rows(xin.ptr("X"), bad, 64, 16, win.ptr("mu"), win.ptr("R"), 64, 0, y.data_ptr(), _lib.XT_F64, st) == _lib.SK_EARG
        assert lib.sc_whiten_rows(xin.ptr("X"), _lib.XT_F64, 64, 16, win.ptr("mu"), win.ptr("R"), 64, 0, y.data_ptr(), bad, st) == _lib.SK_EARG
    assert lib.sc_whiten_rows(x_inside.data_ptr(), _lib.XT_F64, 64, 16, win.ptr("mu"), win.ptr("R"), 64, 0, y.data_ptr(), _lib.XT_F64, st) == _lib.SK_EARG
    assert "Y may not alias X" in _lib.last_error()
    last = y.reshape(-1)[64 * 64 - 1:]                   # X begins at Y's last element
    assert lib.sc_whiten_rows(last.data_ptr(), _lib.XT_F64, 64, 16, win.ptr("mu"), win.ptr("R"), 64, 0, y.data_ptr(), _lib.XT_F64, st) == _lib.SK_EARG
    torch.cuda.synchronize()
    for f in (frame, g_frame, y_frame):
        assert bool((f == SENTINEL).all()), "nothing was enqueued: the framed outputs keep what they held"
    assert ins.unchanged() and tin.unchanged() and win.unchanged()
