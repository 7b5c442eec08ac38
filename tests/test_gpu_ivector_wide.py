"""Total variability at ranks above 192 on the GPU (sidekit_amd/factor_analyser_wide.py, csrc/ivector_wide.hip) against
``numpy.linalg.inv`` on inputs whose conditioning the tests assert, LAPACK's own Cholesky inverse on an ill-conditioned one, the
reference's own output (tests/golden/ivector.npz) and the float64 numpy restatement (tests/tools/ivector_numpy.py, held to 1e-12 against
the fixture by tests/test_ivector_cpu.py, and independent of the rank).

TOL = 1e-9 relative max-norm as in tests/test_gpu_ivector.py: the compared inputs have ``cond <= 1e3`` (1e4 for the M-step's matrices),
asserted, so the bound keeps more than an order of margin over ``cond R 2^-52`` at R = 1024.  Every comparison prints the error it
measured.  The bitwise tests are exact: one workgroup per session on its own scratch, every sum in a fixed order.
"""
import os
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ivector_numpy as ivn  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9
C, D, R, N = 6, 5, 7, 40


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(numpy.load(os.path.join(golden_dir, "ivector.npz")))


def _check(errs, tol=TOL):
    print({k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < tol, f"{k} differs by {v:.3e} (relative max-norm, bound {tol})"


def _np(t):
    return t if isinstance(t, numpy.ndarray) else t.cpu().numpy()


def _ubm(mu, invcov):
    from sidekit_amd.mixture import Mixture
    m = Mixture()
    m.mu, m.invcov = numpy.array(mu, dtype=numpy.float64), numpy.array(invcov, dtype=numpy.float64)
    m.w = numpy.full(m.mu.shape[0], 1.0 / m.mu.shape[0])
    m.cov_var_ctl = 1.0 / m.invcov
    m.cst, m.det = numpy.zeros(m.w.shape), numpy.zeros(m.w.shape)
    m._compute_all()
    return m


def _server(stat0, stat1):
    from sidekit_amd.statserver import StatServer
    names = numpy.array([f"s{i:03d}" for i in range(stat0.shape[0])], dtype="|O")
    s = StatServer()
    s.modelset, s.segset = names.copy(), names.copy()
    s.start, s.stop = numpy.empty(names.shape[0], dtype="|O"), numpy.empty(names.shape[0], dtype="|O")
    s.stat0, s.stat1 = stat0.copy(), stat1.copy()
    return s


# ---- sc_tvw_gram ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 3, 193), (1, 7, 257), (2, 23, 64)])
def test_gram_against_einsum(gpu, shape):
    import torch
    from sidekit_amd.factor_analyser_wide import tv_gram_wide_device
    c, d, r = shape
    F = numpy.random.RandomState(c * 1000 + r).randn(c * d, r)
    G = tv_gram_wide_device(torch.as_tensor(F).to(gpu), c)
    assert G.shape == (c, r * (r + 1) // 2) and G.dtype == torch.float64
    Fc = F.reshape(c, d, r)
    _check({f"gram {shape}": ivn.rel(_np(G), ivn.pack(numpy.einsum("cdi,cdj->cij", Fc, Fc)))})


def test_gram_has_the_bits_of_the_narrow_entry(gpu):
    import torch
    from sidekit_amd.factor_analyser import tv_gram_device
    from sidekit_amd.factor_analyser_wide import tv_gram_wide_device
    F = torch.as_tensor(numpy.random.RandomState(5064).randn(5 * 7, 64)).to(gpu)
    assert torch.equal(tv_gram_wide_device(F, 5), tv_gram_device(F, 5))


# ---- sc_tvw_posterior -------------------------------------------------------------------------------------------------------------------

def _posterior(gpu, Lp, B, packed=True, diag=True, alias=False, shift=1.0):
    """one sc_tvw_posterior call on host arrays -> (e_h or None, E_hh or None, diag or None) device tensors"""
    import torch
    from sidekit_amd import _lib
    from sidekit_amd.factor_analyser_wide import workspace_bytes
    lp = torch.as_tensor(numpy.ascontiguousarray(Lp)).to(gpu)
    n = lp.shape[0]
    rank = int(round((numpy.sqrt(8 * lp.shape[1] + 1) - 1) / 2))
    b = None if B is None else torch.as_tensor(numpy.ascontiguousarray(B)).to(gpu)
    e_h = None if b is None else torch.empty_like(b)
    e_hh = (lp if alias else torch.empty_like(lp)) if packed else None
    dg = torch.empty((n, rank), dtype=torch.float64, device=gpu) if diag else None
    need = workspace_bytes(n, rank)
    work = torch.empty(need // 8, dtype=torch.float64, device=gpu)
    _lib.launch("sc_tvw_posterior", gpu, lp, b, n, rank, float(shift), e_h, e_hh, dg, work, need)
    return e_h, e_hh, dg


def _sessions(rank, n=5, zero=2):
    """``_sessions`` of tests/test_gpu_ivector.py: n sessions of packed sums W' diag(counts) W (K = rank + 3 rows of W, counts of order
    1; session `zero` has none) and projections"""
    rs = numpy.random.RandomState(100 + rank)
    K = rank + 3
    W = rs.randn(K, rank) / numpy.sqrt(K)
    counts = 3.0 * rs.rand(n, K)
    counts[zero] = 0.0
    full = numpy.einsum("ki,nk,kj->nij", W, counts, W)
    return ivn.pack(full), rs.randn(n, rank)


def _expected(Lp, B, rank):
    lam = numpy.eye(rank)[None] + ivn.unpack(Lp, rank)
    cond = numpy.linalg.cond(lam).max()
    inv = numpy.linalg.inv(lam)
    want_eh = numpy.einsum("nij,nj->ni", inv, B)
    return cond, want_eh, ivn.pack(inv + want_eh[:, :, None] * want_eh[:, None, :])


@pytest.mark.parametrize("rank", [1, 63, 64, 65, 128, 129, 193, 257, 400])
def test_posterior_against_numpy_inverse_and_its_bitwise_properties(gpu, rank):
    """one tile with and without padding, tile edges, two and more block rows, the old cap + 1, and a rank in use"""
    import torch
    Lp, B = _sessions(rank)
    cond, want_eh, want_ehh = _expected(Lp, B, rank)
    print(f"rank {rank}: worst cond(Lambda) {cond:.3g}")
    assert cond <= 1e3
    e_h, e_hh, dg = _posterior(gpu, Lp, B)
    errs = {"e_h": ivn.rel(_np(e_h), want_eh), "E_hh": ivn.rel(_np(e_hh), want_ehh)}
    if rank <= 192:   # the narrow kernel on the same sessions: close, not the same bits
        from sidekit_amd import _lib
        lp, b = torch.as_tensor(numpy.ascontiguousarray(Lp)).to(gpu), torch.as_tensor(B).to(gpu)
        n_h, n_hh = torch.empty_like(b), torch.empty_like(lp)
        _lib.launch("sc_tv_posterior", gpu, lp, b, b.shape[0], rank, n_h, n_hh, None)
        errs.update({"e_h against sc_tv_posterior": ivn.rel(_np(e_h), _np(n_h)), "E_hh against sc_tv_posterior": ivn.rel(_np(e_hh), _np(n_hh))})
    _check(errs)
    diag_at = [ivn.packed_index(i, i, rank) for i in range(rank)]
    assert torch.equal(dg, e_hh[:, diag_at]), "d_diag is the diagonal of the packed output, bit for bit"
    assert numpy.array_equal(_np(e_h)[2], B[2]), "all-zero counts: Lambda = I and e_h = b, bit for bit"
    a_h, a_hh, a_dg = _posterior(gpu, Lp, B, alias=True)
    assert torch.equal(a_h, e_h) and torch.equal(a_hh, e_hh) and torch.equal(a_dg, dg), "d_Ehh aliased onto d_Lp gives the same bits"
    d_h, none, d_dg = _posterior(gpu, Lp, B, packed=False)
    assert none is None and torch.equal(d_h, e_h) and torch.equal(d_dg, dg), "the diagonal alone gives the same bits"
    p_h, p_hh, none = _posterior(gpu, Lp, B, diag=False)
    assert none is None and torch.equal(p_h, e_h) and torch.equal(p_hh, e_hh), "the packed output alone gives the same bits"
    s_h, s_hh, s_dg = _posterior(gpu, Lp[3:4], B[3:4])
    assert torch.equal(s_h[0], e_h[3]) and torch.equal(s_hh[0], e_hh[3]) and torch.equal(s_dg[0], dg[3]), "a session alone and at position 3 of 5"
    again = _posterior(gpu, Lp, B)
    assert all(torch.equal(x, y) for x, y in zip(again, (e_h, e_hh, dg))), "two runs give the same bits"


@pytest.mark.parametrize("rank", [600, 1024])
def test_posterior_at_the_ranks_in_use_and_at_the_cap(gpu, rank):
    import torch
    Lp, B = _sessions(rank, n=2, zero=1)
    cond, want_eh, want_ehh = _expected(Lp, B, rank)
    print(f"rank {rank}: worst cond(Lambda) {cond:.3g}")
    assert cond <= 1e3
    e_h, e_hh, dg = _posterior(gpu, Lp, B)
    _check({"e_h": ivn.rel(_np(e_h), want_eh), "E_hh": ivn.rel(_np(e_hh), want_ehh)})
    again = _posterior(gpu, Lp, B)
    assert all(torch.equal(x, y) for x, y in zip(again, (e_h, e_hh, dg))), "two runs give the same bits"


def _potri(lam):
    """LAPACK's Cholesky inverse: dpotrf, then dpotri, the upper triangle mirrored"""
    from scipy.linalg.lapack import dpotrf, dpotri
    c, info = dpotrf(lam, lower=0)
    assert info == 0
    x, info = dpotri(c, lower=0)
    assert info == 0
    x = numpy.triu(x)
    return x + numpy.triu(x, 1).T


@pytest.mark.parametrize("rank", [65, 193, 400])
def test_posterior_ill_conditioned_session_by_residual(gpu, rank):
    """The construction of tests/test_gpu_ivector.py: counts of order 1e5 on K = rank // 2 directions, so that Lambda has eigenvalue 1 on
    the other half and ~1e7 and more on these.  Judged by the residual max|Lambda X - I| (formed in extended precision) against the one
    LAPACK's own Cholesky inverse (dpotrf + dpotri) leaves on the same matrix: the same algorithm with another blocking and summation
    order, and 4 x is the margin this project gives between two backward-stable evaluations.  With b = 0 the packed output is
    inv_lambda itself.  Measured ratios on an MI355X: see DESIGN.md, section 4."""
    rs = numpy.random.RandomState(rank)
    K = rank // 2
    W = rs.randn(K, rank)
    counts = 4e5 * (0.5 + rs.rand(K))
    Lp = numpy.stack([ivn.pack((W.T * counts).dot(W)), numpy.zeros(rank * (rank + 1) // 2)])
    lam = numpy.eye(rank) + ivn.unpack(Lp[0], rank)     # the matrix the kernel forms: 1 added to the packed diagonal
    cond = numpy.linalg.cond(lam)
    assert cond >= 1e7
    e_h, e_hh, _ = _posterior(gpu, Lp, numpy.zeros((2, rank)))
    assert not _np(e_h).any()
    X = ivn.unpack(_np(e_hh)[0], rank)
    assert numpy.array_equal(ivn.unpack(_np(e_hh)[1], rank), numpy.eye(rank)), "the well-conditioned neighbour returns the identity"
    wide, eye = lam.astype(numpy.longdouble), numpy.eye(rank, dtype=numpy.longdouble)
    ours = float(numpy.abs(wide.dot(X.astype(numpy.longdouble)) - eye).max())
    potri = float(numpy.abs(wide.dot(_potri(lam).astype(numpy.longdouble)) - eye).max())
    print(f"rank {rank}: cond {cond:.3g}, residual {ours:.3e}, dpotrf + dpotri leave {potri:.3e}, ratio {ours / potri:.2f}")
    assert ours <= 4 * potri


def test_posterior_non_finite_session_stays_alone(gpu):
    Lp, B = _sessions(193)
    e_h, e_hh, dg = _posterior(gpu, Lp, B)
    bad = Lp.copy()
    bad[1, 5] = numpy.nan
    n_h, n_hh, n_dg = _posterior(gpu, bad, B)
    keep = [0, 2, 3, 4]
    assert all(numpy.array_equal(_np(x)[keep], _np(y)[keep]) for x, y in ((n_h, e_h), (n_hh, e_hh), (n_dg, dg)))
    assert numpy.isnan(_np(n_h)[1]).any()


@pytest.mark.parametrize("size", [65, 200])
def test_inverse_alone_with_no_shift_and_no_right_hand_side(gpu, size):
    """shift = 0, d_B null: what the device M-step asks for"""
    import torch
    from sidekit_amd.factor_analyser_wide import tv_inverse_wide_device
    rs = numpy.random.RandomState(size)
    M = rs.randn(3, size + 40, size)
    spd = numpy.einsum("nki,nkj->nij", M, M) / (size + 40) + 0.05 * numpy.eye(size)
    cond = numpy.linalg.cond(spd).max()
    print(f"size {size}: worst cond {cond:.3g}")
    assert cond <= 1e4
    none, inv, dg = _posterior(gpu, ivn.pack(spd), None, shift=0.0)
    assert none is None
    want = numpy.linalg.inv(spd)
    _check({"inverse": ivn.rel(_np(inv), ivn.pack(want)), "its diagonal": ivn.rel(_np(dg), numpy.einsum("nii->ni", want))})
    ap = torch.as_tensor(numpy.ascontiguousarray(ivn.pack(spd))).to(gpu)
    keep = ap.clone()
    assert torch.equal(tv_inverse_wide_device(ap), inv) and torch.equal(ap, keep), "the module's wrapper: the same bits, its input left alone"


# ---- against the reference's own numbers (R = 7) ----------------------------------------------------------------------------------------

def _fx_ubm(fx):
    return _ubm(fx["mu"], fx["invcov"])


def test_first_e_step_against_the_fixture(gpu, fx):
    import torch
    from sidekit_amd import factor_analyser as fa, factor_analyser_wide as faw
    s0, s1 = fx["stat0"], fx["stat1"]
    sw = ivn.whiten(s0, s1, fx["mu"], fx["invcov"])
    dev = lambda a: torch.as_tensor(numpy.ascontiguousarray(a)).to(gpu)   # noqa: E731
    e_h, e_hh = faw.tv_posterior_wide_device(dev(s0), dev(sw), dev(fx["tv_init"]))
    errs = {"e_h": ivn.rel(_np(e_h), fx["e_h"]), "e_hh": ivn.rel(_np(e_hh), fx["e_hh"])}
    _A, _C, _R = fa._tv_e_step(torch, dev(s0), dev(s1), fa._whitener(torch, _fx_ubm(fx), gpu), dev(fx["tv_init"]), 16,
                               faw.tv_posterior_wide_device, faw.tv_gram_wide_device)
    errs.update({"_A": ivn.rel(_A, fx["A"]), "_C": ivn.rel(_C, fx["C"]), "_R": ivn.rel(_R, fx["R"])})
    _check(errs)


@pytest.mark.parametrize("m_step", ["device", "host"])
@pytest.mark.parametrize("tag,min_div", [("md", True), ("nomd", False)])
def test_total_variability_wide_device_every_recorded_iteration(gpu, fx, tag, min_div, m_step):
    import torch
    from sidekit_amd.factor_analyser_wide import total_variability_wide_device
    s0, s1 = torch.as_tensor(fx["stat0"]).to(gpu), torch.as_tensor(fx["stat1"]).to(gpu)
    keep0, keep1 = s0.clone(), s1.clone()
    trace = []
    F = total_variability_wide_device(s0, s1, _fx_ubm(fx), R, nb_iter=3, min_div=min_div, tv_init=fx["tv_init"],
                                      after_iteration=lambda it, F: trace.append(F.copy()), m_step=m_step)
    assert len(trace) == 3 and numpy.array_equal(F, trace[-1]) and torch.equal(s0, keep0) and torch.equal(s1, keep1)
    _check({f"F it{i}": ivn.rel(trace[i], fx[f"F_{tag}_it{i}"]) for i in range(3)})


def test_extraction_and_the_class_against_the_fixture(gpu, fx, tmp_path):
    import torch
    from sidekit_amd.factor_analyser import FactorAnalyser
    from sidekit_amd.factor_analyser_wide import WideFactorAnalyser, extract_ivectors_wide_device
    ubm = _fx_ubm(fx)
    s0, s1 = torch.as_tensor(fx["stat0"]).to(gpu), torch.as_tensor(fx["stat1"]).to(gpu)
    iv, sigma = extract_ivectors_wide_device(s0, s1, ubm, fx["F_md_it2"], uncertainty=True)
    assert iv.is_cuda and iv.dtype == torch.float64 and torch.equal(extract_ivectors_wide_device(s0, s1, ubm, fx["F_md_it2"]), iv)
    errs = {"device: iv": ivn.rel(_np(iv), fx["iv"]), "device: iv_sigma": ivn.rel(_np(sigma), fx["iv_sigma"])}
    # through a StatServer, as the narrow end-to-end test does: training from a file, extraction from an object and from a file
    path, out = str(tmp_path / "stats.h5"), str(tmp_path / "tv")
    _server(fx["stat0"], fx["stat1"]).write(path)
    wide = WideFactorAnalyser()
    wide.total_variability(path, ubm, R, nb_iter=3, min_div=True, tv_init=fx["tv_init"].copy(), batch_size=16, output_file_name=out)
    assert not wide.mean.any() and wide.mean.shape == wide.Sigma.shape == (C * D,)
    errs.update({"class: F": ivn.rel(wide.F, fx["F_md_it2"]), "class: saved F": ivn.rel(FactorAnalyser.read(out + ".h5").F, fx["F_md_it2"])})
    server = _server(fx["stat0"], fx["stat1"])
    single, single_sigma = wide.extract_ivectors_single(ubm, server, uncertainty=True)
    from_file, file_sigma = wide.extract_ivectors(ubm, path, uncertainty=True)
    errs.update({"single: iv": ivn.rel(single.stat1, fx["iv"]), "single: iv_sigma": ivn.rel(single_sigma, fx["iv_sigma"]),
                 "single: the caller's statistics are left whitened": ivn.rel(server.stat1, fx["stat1_whitened"]),
                 "file: iv": ivn.rel(from_file.stat1, fx["iv"]), "file: iv_sigma": ivn.rel(file_sigma, fx["iv_sigma"])})
    assert single.validate() and numpy.array_equal(single.stat0, numpy.ones((N, 1))) and numpy.array_equal(single.segset, server.segset)
    # the same i-vector StatServer as the narrow class (other bits in stat1)
    narrow = FactorAnalyser(F=wide.F).extract_ivectors(ubm, path)
    for name in ("modelset", "segset", "stat0"):
        numpy.testing.assert_array_equal(getattr(from_file, name), getattr(narrow, name))
    errs["file: iv against FactorAnalyser"] = ivn.rel(from_file.stat1, narrow.stat1)
    _check(errs)


# ---- above the old cap end to end -------------------------------------------------------------------------------------------------------

WC, WD, WR, WN = 8, 26, 200, 260


@pytest.fixture(scope="module")
def wide_set():
    """Synthetic statistics drawn like the fixture's (make_ivector_golden.py: frame counts ``50 (0.5 + rand)`` spread by a Dirichlet
    draw, a low-rank shift of the means and noise ``sqrt(stat0)``) at C = 8, D = 26, R = 200, N = 260, with the restatement's two
    iterations and i-vectors computed once.  Seed 200 with a shift and a start of scale 0.05 was chosen on the CPU: the restatement
    alone has cond(Lambda) <= 40 and cond(A_c) <= 35 in both iterations and the extraction."""
    rs = numpy.random.RandomState(200)
    mu = 2 * rs.randn(WC, WD)
    invcov = 1.0 / (0.5 + rs.rand(WC, WD))
    frames = 50 * (0.5 + rs.rand(WN))
    stat0 = frames[:, None] * rs.dirichlet(3 * numpy.ones(WC), WN)
    sigma = numpy.sqrt(1.0 / invcov)
    shift = (0.05 * rs.randn(WC * WD, WR)).dot(rs.randn(WR, WN)).T.reshape(WN, WC, WD)
    stat1 = stat0[:, :, None] * (mu[None] + sigma[None] * shift) + numpy.sqrt(stat0)[:, :, None] * sigma[None] * rs.randn(WN, WC, WD)
    stat1 = stat1.reshape(WN, WC * WD)
    tv_init = 0.05 * rs.randn(WC * WD, WR)
    batches, F, trace, accs, cond_lam, cond_a = [numpy.arange(WN)], tv_init, [], [], 0.0, 0.0
    for _ in range(2):
        cond_lam = max(cond_lam, numpy.linalg.cond(numpy.eye(WR)[None] + ivn.unpack(stat0.dot(ivn.gram(F, WC, WD)), WR)).max())
        F, acc, _, _ = ivn.em_iteration(stat0, stat1, mu, invcov, F, batches, True)
        cond_a = max(cond_a, numpy.linalg.cond(ivn.unpack(acc[0], WR)).max())
        trace.append(F)
        accs.append(acc)
    cond_lam = max(cond_lam, numpy.linalg.cond(numpy.eye(WR)[None] + ivn.unpack(stat0.dot(ivn.gram(F, WC, WD)), WR)).max())
    iv, iv_sigma = ivn.extract(stat0, stat1, mu, invcov, F)
    return {"mu": mu, "invcov": invcov, "stat0": stat0, "stat1": stat1, "tv_init": tv_init, "F": trace, "acc": accs, "iv": iv,
            "iv_sigma": iv_sigma, "cond_lam": cond_lam, "cond_a": cond_a}


def test_rank_200_training_and_extraction_against_the_restatement(gpu, wide_set):
    import torch
    from sidekit_amd import factor_analyser as fa, factor_analyser_wide as faw
    ws = wide_set
    print(f"worst cond(Lambda) {ws['cond_lam']:.3g}, worst cond(A_c) {ws['cond_a']:.3g}")
    assert ws["cond_lam"] <= 1e3 and ws["cond_a"] <= 1e4
    ubm = _ubm(ws["mu"], ws["invcov"])
    s0, s1 = torch.as_tensor(ws["stat0"]).to(gpu), torch.as_tensor(ws["stat1"]).to(gpu)
    with pytest.raises(ValueError, match="192"):
        fa.total_variability_device(s0, s1, ubm, WR, nb_iter=1, tv_init=ws["tv_init"])
    trace = []
    F = faw.total_variability_wide_device(s0, s1, ubm, WR, nb_iter=2, tv_init=ws["tv_init"], after_iteration=lambda it, F: trace.append(F.copy()))
    errs = {f"F it{i}": ivn.rel(trace[i], ws["F"][i]) for i in range(2)}
    # the M-step alone on the restatement's accumulators: device against host and against the restatement
    _A, _C, _R = (torch.as_tensor(numpy.ascontiguousarray(a)).to(gpu) for a in ws["acc"][1])
    F_dev = _np(faw.tv_m_step_device(_A, _C, _R, WN, True))
    F_host = fa.tv_m_step(*ws["acc"][1], WN, True)
    errs.update({"M-step: device against host": ivn.rel(F_dev, F_host), "M-step: device against the restatement": ivn.rel(F_dev, ws["F"][1])})
    # three batches against one
    per = faw._session_bytes(WC, WD, WR)
    assert faw._batch_rows(WN, WC, WD, WR, 100 * per) == 100
    small = faw.total_variability_wide_device(s0, s1, ubm, WR, nb_iter=2, tv_init=ws["tv_init"], max_workspace_bytes=100 * per)
    errs["F, three batches against one"] = ivn.rel(small, F)
    iv, sigma = faw.extract_ivectors_wide_device(s0, s1, ubm, ws["F"][1], uncertainty=True)
    iv3, sigma3 = faw.extract_ivectors_wide_device(s0, s1, ubm, ws["F"][1], uncertainty=True, max_workspace_bytes=100 * per)
    errs.update({"iv": ivn.rel(_np(iv), ws["iv"]), "iv_sigma": ivn.rel(_np(sigma), ws["iv_sigma"])})
    _check(errs)
    assert torch.equal(iv3, iv) and torch.equal(sigma3, sigma), "a session's i-vector has the same bits whatever the batch"
    assert numpy.isfinite(F).all()


def test_rank_400_through_the_class_gives_finite_ivectors(gpu, wide_set):
    from sidekit_amd.factor_analyser_wide import WideFactorAnalyser
    ws = wide_set
    ubm, server = _ubm(ws["mu"], ws["invcov"]), _server(ws["stat0"][:48], ws["stat1"][:48])
    wide = WideFactorAnalyser()
    wide.total_variability(server, ubm, 400, nb_iter=1, tv_init=0.05 * numpy.random.RandomState(400).randn(WC * WD, 400))
    iv = wide.extract_ivectors(ubm, server)
    assert wide.F.shape == (WC * WD, 400) and iv.stat1.shape == (48, 400) and numpy.isfinite(wide.F).all() and numpy.isfinite(iv.stat1).all()


def test_the_count_weighted_sums_beyond_one_product(gpu):
    """C = 2 048 components at rank 512: C P is just above what one sc_gemm_tn call takes, so the accumulator ``_A`` is formed in two
    blocks of components; at rank 600, where trainings run, it is 3.7e8.  Three sessions keep the product itself small."""
    import torch
    from sidekit_amd import factor_analyser as fa
    c, p = 2048, fa.packed_size(512)
    assert c * p > fa.GEMM_TN_MAX_OUTPUT >= (c // 2) * p
    g = torch.Generator(device=gpu).manual_seed(3)
    s0 = torch.rand((3, c), dtype=torch.float64, device=gpu, generator=g)
    e_hh = torch.randn((3, p), dtype=torch.float64, device=gpu, generator=g)
    got = fa._count_weighted_sums(s0, e_hh)
    want = s0.t().matmul(e_hh)
    assert got.shape == (c, p)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"two blocks of components against one matmul: {err:.2e}")
    assert err < TOL
    with pytest.raises(ValueError, match="sc_gemm_tn"):
        fa.gemm_tn_device(s0, e_hh)
