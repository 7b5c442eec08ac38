"""Joint factor analysis on the GPU (sidekit_amd/jfa_scoring.py, csrc/jfa.hip, the JFA methods of sidekit_amd/statserver.py) against
numpy on the two kernels' own formulas, the reference's own output (tests/golden/jfa.npz, written by make_jfa_golden.py from the imported
reference module) and the float64 numpy restatement (tests/tools/jfa_numpy.py, held to 1e-12 against the fixture by
tests/test_jfa_cpu.py).

TOL = 1e-9 relative max-norm, this project's bound for float64 quantities: every inverted or solved matrix of the fixture has
``cond <= 1e3`` / ``1e4`` (asserted by its generator, measured 31 and 12), and the generator measured that statistics moved by 1e-13
relative move no recorded output by more than 1.9e-12 relative, so nine EM iterations amplify a rounding error of 2^-52 by less than
twenty.  The kernels' own tests sum at most 192 products per element.  Every comparison prints the error it measured.  The bitwise tests
are exact: no floating-point atomics, every sum in a fixed order.
"""
import copy
import os
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ivector_numpy as ivn  # noqa: E402
import jfa_numpy as jfn  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9
C, D, RANK_F, RANK_G = 6, 5, 4, 3
SENTINEL = -7.25e11


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(numpy.load(os.path.join(golden_dir, "jfa.npz")))


def _check(errs):
    print({k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < TOL, f"{k} differs by {v:.3e} (relative max-norm, bound {TOL})"


def _np(t):
    return t if isinstance(t, numpy.ndarray) else t.cpu().numpy()


def _dev(gpu, a):
    import torch
    return torch.as_tensor(numpy.ascontiguousarray(a)).to(gpu)


def _ubm(fx):
    from sidekit_amd.mixture import Mixture
    m = Mixture()
    m.w, m.mu, m.invcov = (numpy.array(fx[k], dtype=numpy.float64) for k in ("w", "mu", "invcov"))
    m.cov_var_ctl = 1.0 / m.invcov
    m.cst, m.det = numpy.zeros(m.w.shape), numpy.zeros(m.w.shape)
    m._compute_all()
    return m


def _server(models, segments, stat0, stat1):
    from sidekit_amd.statserver import StatServer
    s = StatServer()
    s.modelset, s.segset = numpy.array(models, dtype="|O"), numpy.array(segments, dtype="|O")
    s.start, s.stop = numpy.empty(len(models), dtype="|O"), numpy.empty(len(models), dtype="|O")
    s.stat0, s.stat1 = numpy.array(stat0, dtype=numpy.float64), numpy.array(stat1, dtype=numpy.float64)
    return s


def _training_server(fx):
    n = fx["stat0"].shape[0]
    return _server([f"spk{s:02d}" for s in fx["speaker_of"]], [f"sess{i:02d}" for i in range(n)], fx["stat0"], fx["stat1"])


def _model(fx):
    return fx["mu"].reshape(-1), 1.0 / fx["invcov"].reshape(-1), fx["F"], fx["G"], fx["H"]


# ---- sc_jfa_shift -----------------------------------------------------------------------------------------------------------------------

def _shift(gpu, stat0, stat1, W, H, rows, mean, scale, in_place=False):
    """one sc_jfa_shift call whose output lies between two sentinel rows -> the output (device); the dense layout has no padding between
    the columns of consecutive rows, so a write past a row's end lands in the next row or in the border"""
    import torch
    from sidekit_amd import _lib
    n, cd = stat1.shape
    frame = torch.full((n + 2, cd), SENTINEL, dtype=torch.float64, device=gpu)
    out = frame[1:n + 1]
    s1 = _dev(gpu, stat1)
    if in_place:
        out.copy_(s1)
        s1 = out
    rank = 0 if W is None else W.shape[1]
    args = [None if a is None else _dev(gpu, a) for a in (W, H, None if rows is None else numpy.asarray(rows, dtype=numpy.int32), mean, scale)]
    _lib.launch("sc_jfa_shift", gpu, s1, _dev(gpu, stat0), n, stat0.shape[1], cd // stat0.shape[1], args[0], args[1],
                0 if H is None else H.shape[0], rank, args[2], args[3], args[4], out)
    assert bool((frame[0] == SENTINEL).all()) and bool((frame[n + 1] == SENTINEL).all()), "the border around the output is intact"
    return out.clone()


SHIFT_SHAPES = [(1, 1, 1, 1, 1), (5, 3, 7, 3, 2), (63, 7, 5, 16, 9), (65, 3, 23, 17, 65), (130, 5, 27, 36, 12), (33, 2, 60, 192, 33), (70, 4, 9, 0, 0)]


@pytest.mark.parametrize("with_mean,with_scale", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("shape", SHIFT_SHAPES)
def test_shift_against_numpy_and_its_bitwise_properties(gpu, shape, with_mean, with_scale):
    """One session and one column; fewer rows of H than sessions; 63 and 65 sessions (R one k-tile, and one more than it); the
    128-tile crossed in both directions with odd D and R = 2 k-tiles and a tail of 4; the rank cap; R = 0 (the plain whitening)"""
    import torch
    n, c, d, r, nh = shape
    rs = numpy.random.RandomState(1000 * n + r)
    stat0 = 5.0 * rs.rand(n, c)
    stat0[n // 2, c // 2] = 0.0
    stat1 = stat0.repeat(d, axis=1) * rs.randn(n, c * d) + rs.randn(n, c * d)
    W = rs.randn(c * d, r) / numpy.sqrt(max(r, 1)) if r else None
    H = rs.randn(nh, r) if r else None
    mean = rs.randn(c * d) if with_mean else None
    scale = 0.5 + rs.rand(c * d) if with_scale else None
    rows = None
    if r:   # non-monotonic, with repeats, and (from three sessions on) one index below and one above the rows of H
        rows = rs.randint(0, nh, n)
        rows[0] = rows[-1]
        if n >= 3:
            rows[1], rows[n - 2] = -1, nh
    errs = {}
    plain = _shift(gpu, stat0, stat1, W, H, rows, mean, scale)
    errs["gathered rows" if r else "no shift"] = jfn.rel(_np(plain), jfn.shift(stat0, stat1, W, H, rows, mean, scale))
    if r:
        own = _shift(gpu, stat0, stat1, W, H, None, mean, scale)
        errs["own rows"] = jfn.rel(_np(own), jfn.shift(stat0, stat1, W, H, None, mean, scale))
        if nh < n:
            untouched = (stat1[nh:] - stat0[nh:].repeat(d, axis=1) * (0.0 if mean is None else mean)) * (1.0 if scale is None else scale)
            assert numpy.array_equal(_np(own)[nh:], untouched), "without rows, the sessions beyond the rows of H get a zero factor"
        if n >= 3:
            zero = (stat1[1] - stat0[1].repeat(d) * (0.0 if mean is None else mean)) * (1.0 if scale is None else scale)
            assert numpy.array_equal(_np(plain)[1], zero), "a row index outside [0, Nh) is a zero factor"
    _check(errs)
    assert torch.equal(_shift(gpu, stat0, stat1, W, H, rows, mean, scale, in_place=True), plain), "in place gives the same bits"
    assert torch.equal(_shift(gpu, stat0, stat1, W, H, rows, mean, scale), plain), "two runs give the same bits"
    i = n - 1
    alone = _shift(gpu, stat0[i:i + 1], stat1[i:i + 1], W, H, None if rows is None else rows[i:i + 1], mean, scale)
    assert torch.equal(alone[0], plain[i]), "a session alone and the same session inside the batch"


def test_jfa_shift_device_checks_and_defaults(gpu):
    import torch
    from sidekit_amd.jfa_scoring import jfa_shift_device
    rs = numpy.random.RandomState(4)
    stat0, stat1, W, H = 3.0 * rs.rand(9, 3), rs.randn(9, 12), rs.randn(12, 5), rs.randn(4, 5)
    rows = numpy.array([3, 0, 0, 2, 1, 3, 3, 0, 2])
    s0, s1 = _dev(gpu, stat0), _dev(gpu, stat1)
    keep = s1.clone()
    out = jfa_shift_device(s0, s1, W, H, rows, rs.rand(12), None)
    assert out is not s1 and torch.equal(s1, keep) and out.dtype == torch.float64
    same = jfa_shift_device(s0, s1, _dev(gpu, W), _dev(gpu, H), torch.as_tensor(rows).to(gpu))
    _check({"host and device arguments": jfn.rel(_np(same), jfn.shift(stat0, stat1, W, H, rows))})
    assert jfa_shift_device(s0, s1, W, H, rows, out=s1) is s1 and torch.equal(s1, same)
    empty = jfa_shift_device(s0, keep, numpy.zeros((12, 0)), numpy.zeros((9, 0)))
    assert torch.equal(empty, keep), "a loading matrix without columns: nothing is subtracted"
    with pytest.raises(ValueError, match="192"):
        jfa_shift_device(s0, keep, numpy.zeros((12, 193)), numpy.zeros((9, 193)))


# ---- sc_jfa_map_acc ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1, 1), (7, 3, 5), (257, 6, 5), (1000, 2, 33)])
def test_map_accumulators_against_numpy(gpu, shape):
    """One model; fewer than a slab; one row more than a slab; four slabs and columns that end inside a block of 256"""
    import torch
    from sidekit_amd.jfa_scoring import jfa_map_acc_device
    m, c, d = shape
    rs = numpy.random.RandomState(m)
    stat0 = 40.0 * rs.rand(m, c)
    if m > 1:
        stat0[m // 3] = 0.0       # a model without frames
        stat0[:, c - 1] = 0.0     # a component without frames
    stat1 = numpy.sqrt(stat0).repeat(d, axis=1) * rs.randn(m, c * d)
    Dv, sigma = 0.1 + rs.rand(c * d), 0.5 + rs.rand(c * d)
    A, Cacc = jfa_map_acc_device(_dev(gpu, stat0), _dev(gpu, stat1), Dv, sigma)
    want_a, want_c = jfn.map_acc(stat0, stat1, Dv, sigma)
    _check({"_A": jfn.rel(_np(A), want_a), "_C": jfn.rel(_np(Cacc), want_c)})
    if m > 1:
        assert not _np(A)[(c - 1) * d:].any() and not _np(Cacc)[(c - 1) * d:].any(), "a component without frames accumulates nothing"
    A2, C2 = jfa_map_acc_device(_dev(gpu, stat0), _dev(gpu, stat1), _dev(gpu, Dv), _dev(gpu, sigma))
    assert torch.equal(A, A2) and torch.equal(Cacc, C2), "two runs give the same bits"


# ---- the hidden variables against the fixture ------------------------------------------------------------------------------------------

CASES = {"v": (True, False, False), "u": (False, True, False), "vu": (True, True, False), "vud": (True, True, True)}


@pytest.mark.parametrize("tag", list(CASES))
def test_estimate_hidden_against_the_fixture(gpu, fx, tag):
    import torch
    from sidekit_amd.jfa_scoring import estimate_hidden_device
    mean, sigma, F, G, H = _model(fx)
    V, U, Dm = (m if use else None for m, use in zip((F, G, H), CASES[tag]))
    s0, s1 = _dev(gpu, fx["stat0"]), _dev(gpu, fx["stat1"])
    keep = s1.clone()
    y, x, z = estimate_hidden_device(s0, s1, mean, sigma, V, U, Dm)
    assert torch.equal(s1, keep) and y.is_cuda and y.dtype == torch.float64 and (z is None) == (Dm is None)
    assert y.shape == fx[f"hid_{tag}_y"].shape and x.shape == fx[f"hid_{tag}_x"].shape
    errs = {}
    if V is not None:
        errs["y"] = jfn.rel(_np(y), fx[f"hid_{tag}_y"])
    if U is not None:
        errs["x"] = jfn.rel(_np(x), fx[f"hid_{tag}_x"])
    if Dm is not None:
        errs["z"] = jfn.rel(_np(z), fx[f"hid_{tag}_z"])
    rank = y.shape[1] + x.shape[1]
    per = 8 * (rank * (rank + 1) // 2 + C * D + C + 2 * rank)
    y2, x2, z2 = estimate_hidden_device(s0, s1.view(-1, C, D), mean, sigma, V, U, Dm, max_workspace_bytes=5 * per)
    assert torch.equal(y, y2) and torch.equal(x, x2) and (z is None or torch.equal(z, z2)), "nine batches give the bits of one"
    server = _training_server(fx)
    ys, xs, zs = server.estimate_hidden(mean, sigma, V, U, Dm, batch_size=7, num_thread=3)
    numpy.testing.assert_array_equal(server.stat1, fx["stat1"])
    assert numpy.array_equal(ys.stat1, _np(y)) and numpy.array_equal(xs.stat1, _np(x)) and numpy.array_equal(ys.segset, server.segset)
    assert numpy.array_equal(ys.stat0, numpy.ones((server.segset.shape[0], 1))) and ys.modelset is not server.modelset
    if Dm is None:
        assert zs.stat1.size == 0 and zs.modelset.size == 0
    else:
        assert numpy.array_equal(zs.stat1, _np(z)) and numpy.array_equal(zs.modelset, server.modelset)
    _check(errs)


# ---- training against the fixture -------------------------------------------------------------------------------------------------------

def test_first_iteration_accumulators_against_the_fixture(gpu, fx):
    import torch
    from sidekit_amd import jfa_scoring as js
    from sidekit_amd.factor_analyser import ClassIndex, class_sums_device
    mean, sigma, F, G, H = _model(fx)
    s0, s1 = _dev(gpu, fx["stat0"]), _dev(gpu, fx["stat1"])
    index = ClassIndex(fx["speaker_of"])
    m0, m1 = class_sums_device(s0, index)[0], class_sums_device(s1, index)[0]
    mean_d, sigma_d = _dev(gpu, mean), _dev(gpu, sigma)
    scale = 1.0 / torch.sqrt(sigma_d)
    hrows = torch.as_tensor(index.inverse.astype(numpy.int32)).to(gpu)
    n_models, n = m0.shape[0], s0.shape[0]
    _A, _C, _R = js._e_step(torch, m0, m1, fx["F_init"], mean_d, scale, 16)
    errs = {"between: _A": jfn.rel(ivn.unpack(_A, RANK_F), fx["A_F"]), "between: _C": jfn.rel(_C, fx["C_F"]),
            "between: _R": jfn.rel(ivn.unpack(_R, RANK_F) / n_models, fx["R_F"])}
    y = js.estimate_hidden_device(m0, m1, mean, sigma, F)[0]
    _A, _C, _R = js._e_step(torch, s0, s1, fx["G_init"], mean_d, scale, 16, _dev(gpu, F), y, hrows)
    errs.update({"within: _A": jfn.rel(ivn.unpack(_A, RANK_G), fx["A_G"]), "within: _C": jfn.rel(_C, fx["C_G"]),
                 "within: _R": jfn.rel(ivn.unpack(_R, RANK_G) / n, fx["R_G"])})
    sums = js._map_statistics(torch, s0, s1, index, mean_d, scale, _dev(gpu, F), y, hrows, _dev(gpu, G), 1 << 30)
    A, Cacc = js.jfa_map_acc_device(m0, sums, fx["H_init"], sigma)
    errs.update({"map: _A": jfn.rel(_np(A), fx["A_H"]), "map: _C": jfn.rel(_np(Cacc), fx["C_H"]), "map: H after one iteration": jfn.rel(_np(Cacc / A), fx["H_it0"])})
    _check(errs)


def test_factor_analysis_every_stage_against_the_fixture(gpu, fx):
    import torch
    from sidekit_amd.jfa_scoring import factor_analysis_device
    ubm = _ubm(fx)
    init = (fx["F_init"], fx["G_init"], fx["H_init"])
    it_nb, batch = tuple(int(i) for i in fx["it_nb"]), int(fx["batch_size"])
    s0, s1 = _dev(gpu, fx["stat0"]), _dev(gpu, fx["stat1"])
    keep0, keep1 = s0.clone(), s1.clone()
    mean, F, G, H, sigma = factor_analysis_device(s0, s1.view(-1, C, D), fx["speaker_of"], ubm, RANK_F, RANK_G, True, it_nb, True, init)
    assert torch.equal(s0, keep0) and torch.equal(s1, keep1) and all(isinstance(a, numpy.ndarray) and a.dtype == numpy.float64 for a in (mean, F, G, H, sigma))
    assert numpy.array_equal(mean, fx["mu"].reshape(-1)) and numpy.array_equal(sigma, fx["sigma"])
    errs = {"device: F": jfn.rel(F, fx["F"]), "device: G": jfn.rel(G, fx["G"]), "device: H": jfn.rel(H, fx["H"])}
    # the stages one after the other: F alone is the first stage's matrix after each of its iterations, H after one iteration
    for i in range(it_nb[0]):
        only_f = factor_analysis_device(s0, s1, fx["speaker_of"], ubm, RANK_F, RANK_G, True, (i + 1, 0, 0), True, init)
        errs[f"F after iteration {i}"] = jfn.rel(only_f[1], fx[f"F_it{i}"])
        assert numpy.array_equal(only_f[2], fx["G_init"]) and numpy.array_equal(only_f[3], fx["H_init"]), "it_nb[2] == 0 skips G and H"
    one = factor_analysis_device(s0, s1, torch.as_tensor(fx["speaker_of"]).to(gpu), ubm, RANK_F, RANK_G, True, (it_nb[0], it_nb[1], 1), True, init)
    errs["H after one iteration"] = jfn.rel(one[3], fx["H_it0"])
    assert numpy.array_equal(one[1], F) and numpy.array_equal(one[2], G)
    # a workspace of five sessions per batch against one batch
    per = 8 * (RANK_F * (RANK_F + 1) // 2 + C * D + C + 2 * RANK_F)
    small = factor_analysis_device(s0, s1, fx["speaker_of"], ubm, RANK_F, RANK_G, True, it_nb, True, init, max_workspace_bytes=5 * per)
    errs.update({"small workspace: F": jfn.rel(small[1], F), "small workspace: G": jfn.rel(small[2], G), "small workspace: H": jfn.rel(small[3], H)})
    # the StatServer method
    server = _training_server(fx)
    got = server.factor_analysis(RANK_F, RANK_G, True, False, it_nb, True, ubm, batch, 1, False, tuple(m.copy() for m in init))
    numpy.testing.assert_array_equal(server.stat1, fx["stat1"])
    errs.update({"method: F": jfn.rel(got[1], fx["F"]), "method: G": jfn.rel(got[2], fx["G"]), "method: H": jfn.rel(got[3], fx["H"])})
    assert numpy.array_equal(got[0], mean) and numpy.array_equal(got[4], sigma)
    _check(errs)


def test_the_three_estimations_as_methods(gpu, fx):
    """estimate_between_class, estimate_within_class and estimate_map on the shifts the reference's factor_analysis hands them, built
    here from the fixture's y and x"""
    mean, sigma, F, G, H = _model(fx)
    server = _training_server(fx)
    n = server.segset.shape[0]
    V, sig = server.estimate_between_class(3, fx["F_init"].copy(), mean, sigma, 16)
    errs = {"between": jfn.rel(V, fx["F"])}
    assert sig is sigma
    _, inverse, m0, m1 = jfn.model_sums(fx["stat0"], fx["stat1"], fx["speaker_of"])
    y = jfn.hidden(m0, m1, mean, sigma, F)[0]
    Vy = _training_server(fx)
    Vy.stat1 = y[inverse].dot(F.T)
    errs["within"] = jfn.rel(server.estimate_within_class(3, fx["G_init"].copy(), mean, sigma, 16, Vy), fx["G"])
    x = jfn.hidden(fx["stat0"], jfn.shift(fx["stat0"], fx["stat1"], F, y, inverse), mean, sigma, None, G)[1]
    Ux = _training_server(fx)
    Ux.stat1 = x.dot(G.T)
    errs["map"] = jfn.rel(server.estimate_map(3, fx["H_init"].copy(), mean, sigma, Vy, Ux), fx["H"])
    errs["map, one iteration"] = jfn.rel(server.estimate_map(1, fx["H_init"].copy(), mean, sigma, Vy, Ux), fx["H_it0"])
    numpy.testing.assert_array_equal(server.stat1, fx["stat1"])
    assert n == fx["stat0"].shape[0]
    _check(errs)


def test_missing_start_matrices_are_drawn_in_the_reference_order(gpu, fx):
    from sidekit_amd.jfa_scoring import factor_analysis_device
    ubm = _ubm(fx)
    s0, s1 = _dev(gpu, fx["stat0"]), _dev(gpu, fx["stat1"])
    numpy.random.seed(11)
    F0 = numpy.random.randn(C * D, RANK_F)
    G0 = numpy.random.randn(C * D, RANK_G)
    H0 = numpy.random.randn(C * D) * (1.0 / fx["invcov"]).mean()
    numpy.random.seed(11)
    drawn = factor_analysis_device(s0, s1, fx["speaker_of"], ubm, RANK_F, RANK_G, True, (1, 1, 0))
    given = factor_analysis_device(s0, s1, fx["speaker_of"], ubm, RANK_F, RANK_G, True, (1, 1, 0), True, (F0, G0, H0))
    for a, b in zip(drawn, given):
        numpy.testing.assert_array_equal(a, b)
    numpy.testing.assert_array_equal(drawn[2], G0)
    numpy.testing.assert_array_equal(drawn[3], H0)
    assert factor_analysis_device(s0, s1, fx["speaker_of"], ubm, RANK_F, RANK_G, None, (0, 0, 0))[3].shape == (0,)


# ---- scoring against the fixture --------------------------------------------------------------------------------------------------------

def _scoring_set(fx):
    from sidekit_amd.bosaris import Ndx
    enroll = _server([f"m{s}" for s in fx["enroll_of"]], [f"e{i}" for i in range(6)], fx["enroll_stat0"], fx["enroll_stat1"])
    test = _server([f"t{i}" for i in range(9)], [f"t{i}" for i in range(9)], fx["test_stat0"], fx["test_stat1"])
    ndx = Ndx()
    ndx.modelset = numpy.array(["m0", "m1", "m2", "m3", "m_missing"], dtype="|O")
    ndx.segset = numpy.array([f"t{i}" for i in range(9)] + ["t_missing"], dtype="|O")
    ndx.trialmask = fx["ndx_mask"].copy()
    exact = Ndx()
    exact.modelset, exact.segset, exact.trialmask = ndx.modelset[:4].copy(), ndx.segset[:9].copy(), fx["ndx_mask"][:4, :9].copy()
    return enroll, test, ndx, exact


def test_jfa_scoring_against_the_fixture(gpu, fx, monkeypatch):
    import torch
    from sidekit_amd import jfa_scoring as js
    ubm = _ubm(fx)
    mean, sigma, F, G, H = _model(fx)
    enroll, test, ndx, exact = _scoring_set(fx)
    before = copy.deepcopy((enroll, test, ndx))
    checked = js.jfa_scoring(ubm, enroll, test, ndx, mean, sigma, F, G, H)
    summed = js.jfa_scoring(ubm, enroll, test, exact, mean, sigma, F, G, H, check_missing=False)
    for got in (checked, summed):
        assert list(got.modelset) == ["m0", "m1", "m2", "m3"] and list(got.segset) == [f"t{i}" for i in range(9)]
        assert numpy.array_equal(got.scoremask, fx["ndx_mask"][:4, :9]) and got.scoremat.dtype == numpy.float64
    _check({"the missing model and segment dropped (a model's first session is what is left of it)": jfn.rel(checked.scoremat, fx["scores_checked"]),
            "multi-session enrolment summed": jfn.rel(summed.scoremat, fx["scores_unchecked"])})
    for kept, orig in zip((enroll, test), before[:2]):
        for name in ("modelset", "segset", "stat0", "stat1"):
            numpy.testing.assert_array_equal(getattr(kept, name), getattr(orig, name))
    numpy.testing.assert_array_equal(ndx.trialmask, before[2].trialmask)
    assert numpy.array_equal(js.jfa_scoring(ubm, enroll, test, exact, mean, sigma, F, G, H, batch_size=2, num_thread=5, check_missing=False).scoremat,
                             summed.scoremat), "batch_size changes no bit"
    per_model = copy.deepcopy(enroll).sum_stat_per_model()[0]   # sc_class_sums, as inside jfa_scoring
    args = (_dev(gpu, per_model.stat0), _dev(gpu, per_model.stat1), _dev(gpu, fx["test_stat0"]), _dev(gpu, fx["test_stat1"]).view(-1, C, D))
    keep = [a.clone() for a in args]
    device = js.jfa_score_device(ubm, *args, mean, sigma, F, G, H)
    assert device.is_cuda and device.dtype == torch.float64 and all(torch.equal(a, k) for a, k in zip(args, keep))
    assert numpy.array_equal(_np(device), summed.scoremat), "jfa_score_device on the per-model sums gives the bits of jfa_scoring"
    rank = RANK_F + RANK_G
    monkeypatch.setattr(js, "SCORING_BYTES", 4 * 8 * (rank * (rank + 1) // 2 + C * D + C + 2 * rank))   # two sessions per batch
    assert torch.equal(js.jfa_score_device(ubm, *args, mean, sigma, F, G, H), device), "five batches of segments give the bits of one"
    assert numpy.array_equal(js.jfa_scoring(ubm, enroll, test, ndx, mean, sigma, F, G, H).scoremat, checked.scoremat)
