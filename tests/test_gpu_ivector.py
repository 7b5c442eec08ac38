"""Total variability on the GPU (sidekit_amd/factor_analyser.py, csrc/ivector.hip) against the reference's own output
(tests/golden/ivector.npz, written by make_ivector_golden.py from the imported reference module), ``numpy.linalg.inv`` on inputs whose
conditioning the tests assert, and the float64 numpy restatement (tests/tools/ivector_numpy.py, held to 1e-12 against the fixture by
tests/test_ivector_cpu.py).

TOL = 1e-9 relative max-norm, this project's bound for float64 quantities: the compared inputs have ``cond <= 1e3`` (asserted), so the
bound has three orders of margin over ``cond R 2^-52`` at R = 192.  Every comparison prints the error it measured.  The bitwise tests are
exact: no floating-point atomics, one workgroup per session, every sum in a fixed order.
"""
import os
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ivector_numpy as ivn  # noqa: E402
import mixture_numpy as mxn  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9
C, D, R, N = 6, 5, 7, 40


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(numpy.load(os.path.join(golden_dir, "ivector.npz")))


def _check(errs):
    print({k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < TOL, f"{k} differs by {v:.3e} (relative max-norm, bound {TOL})"


def _np(t):
    return t if isinstance(t, numpy.ndarray) else t.cpu().numpy()


def _ubm(fx):
    from sidekit_amd.mixture import Mixture
    m = Mixture()
    m.w, m.mu, m.invcov = (numpy.array(fx[k], dtype=numpy.float64) for k in ("w", "mu", "invcov"))
    m.cov_var_ctl = 1.0 / m.invcov
    m.cst, m.det = numpy.zeros(m.w.shape), numpy.zeros(m.w.shape)
    m._compute_all()
    return m


def _server(fx, rows=slice(None)):
    from sidekit_amd.statserver import StatServer
    names = numpy.array([f"s{i:02d}" for i in range(N)], dtype="|O")[rows]
    s = StatServer()
    s.modelset, s.segset = names.copy(), names.copy()
    s.start, s.stop = numpy.empty(names.shape[0], dtype="|O"), numpy.empty(names.shape[0], dtype="|O")
    s.stat0, s.stat1 = fx["stat0"][rows].copy(), fx["stat1"][rows].copy()
    return s


# ---- sc_tv_gram -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(3, 5, 1), (2, 23, 17), (5, 7, 64), (2, 3, 65), (1, 60, 192)])
def test_gram_against_einsum(gpu, shape):
    """K = D shorter than a k-tile (16) and with a tail, rank one below and one above a tile edge (64), and the cap"""
    import torch
    from sidekit_amd.factor_analyser import tv_gram_device
    c, d, r = shape
    F = numpy.random.RandomState(c * 1000 + r).randn(c * d, r)
    G = tv_gram_device(torch.as_tensor(F).to(gpu), c)
    assert G.shape == (c, r * (r + 1) // 2) and G.dtype == torch.float64
    Fc = F.reshape(c, d, r)
    _check({f"gram {shape}": ivn.rel(_np(G), ivn.pack(numpy.einsum("cdi,cdj->cij", Fc, Fc)))})
    assert torch.equal(G, tv_gram_device(torch.as_tensor(F).to(gpu), c)), "two runs give the same bits"


# ---- sc_tv_posterior --------------------------------------------------------------------------------------------------------------------

def _posterior(gpu, Lp, B, packed=True, diag=True, alias=False):
    """one sc_tv_posterior call on host arrays -> (e_h, E_hh or None, diag or None) device tensors"""
    import torch
    from sidekit_amd import _lib
    lp, b = torch.as_tensor(numpy.ascontiguousarray(Lp)).to(gpu), torch.as_tensor(numpy.ascontiguousarray(B)).to(gpu)
    e_h = torch.empty_like(b)
    e_hh = (lp if alias else torch.empty_like(lp)) if packed else None
    dg = torch.empty_like(b) if diag else None
    _lib.launch("sc_tv_posterior", gpu, lp, b, b.shape[0], b.shape[1], e_h, e_hh, dg)
    return e_h, e_hh, dg


def _sessions(rank, n=5, zero=2):
    """n sessions of packed sums W' diag(counts) W (K = rank + 3 rows of W, counts of order 1; session `zero` has none) and projections"""
    rs = numpy.random.RandomState(100 + rank)
    K = rank + 3
    W = rs.randn(K, rank) / numpy.sqrt(K)
    counts = 3.0 * rs.rand(n, K)
    counts[zero] = 0.0
    full = numpy.einsum("ki,nk,kj->nij", W, counts, W)
    return ivn.pack(full), rs.randn(n, rank)


@pytest.mark.parametrize("rank", [1, 2, 17, 64, 65, 191, 192])
def test_posterior_against_numpy_inverse_and_its_bitwise_properties(gpu, rank):
    import torch
    Lp, B = _sessions(rank)
    lam = numpy.eye(rank)[None] + ivn.unpack(Lp, rank)
    cond = max(numpy.linalg.cond(m) for m in lam)
    print(f"rank {rank}: worst cond(Lambda) {cond:.3g}")
    assert cond <= 1e3
    inv = numpy.linalg.inv(lam)
    want_eh = numpy.einsum("nij,nj->ni", inv, B)
    want_ehh = ivn.pack(inv + want_eh[:, :, None] * want_eh[:, None, :])
    e_h, e_hh, dg = _posterior(gpu, Lp, B)
    _check({"e_h": ivn.rel(_np(e_h), want_eh), "E_hh": ivn.rel(_np(e_hh), want_ehh)})
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


@pytest.mark.parametrize("rank", [17, 192])
def test_posterior_ill_conditioned_session_by_residual(gpu, rank):
    """Counts of order 1e5 on K = rank // 2 directions: Lambda has eigenvalue 1 on the other half and ~1e7 on these.  Judged by the
    residual max|Lambda X - I| (formed in extended precision) against the one ``numpy.linalg.inv`` (LU) leaves on the same matrix: both
    are backward stable with different constants, 4 x covers the difference.  With b = 0 the packed output is inv_lambda itself."""
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
    assert numpy.array_equal(ivn.unpack(_np(e_hh)[1], rank), numpy.eye(rank)), "the well-conditioned neighbour is not affected"
    wide, eye = lam.astype(numpy.longdouble), numpy.eye(rank, dtype=numpy.longdouble)
    ours = float(numpy.abs(wide.dot(X.astype(numpy.longdouble)) - eye).max())
    lu = float(numpy.abs(wide.dot(numpy.linalg.inv(lam).astype(numpy.longdouble)) - eye).max())
    print(f"rank {rank}: cond {cond:.3g}, residual {ours:.3e}, numpy.linalg.inv leaves {lu:.3e}, ratio {ours / lu:.2f}")
    assert ours <= 4 * lu


def test_posterior_non_finite_session_stays_alone(gpu):
    Lp, B = _sessions(17)
    e_h, e_hh, dg = _posterior(gpu, Lp, B)
    bad = Lp.copy()
    bad[1, 5] = numpy.nan
    n_h, n_hh, n_dg = _posterior(gpu, bad, B)
    keep = [0, 2, 3, 4]
    assert all(numpy.array_equal(_np(x)[keep], _np(y)[keep]) for x, y in ((n_h, e_h), (n_hh, e_hh), (n_dg, dg)))
    assert numpy.isnan(_np(n_h)[1]).any()


# ---- end to end against the fixture -----------------------------------------------------------------------------------------------------

def test_first_e_step_against_the_fixture(gpu, fx):
    import torch
    from sidekit_amd import factor_analyser as fa
    s0, s1 = fx["stat0"], fx["stat1"]
    sw = ivn.whiten(s0, s1, fx["mu"], fx["invcov"])
    dev = lambda a: torch.as_tensor(numpy.ascontiguousarray(a)).to(gpu)   # noqa: E731
    e_h, e_hh = fa.tv_posterior_device(dev(s0), dev(sw), dev(fx["tv_init"]))
    errs = {"e_h": ivn.rel(_np(e_h), fx["e_h"]), "e_hh": ivn.rel(_np(e_hh), fx["e_hh"])}
    _A, _C, _R = fa._tv_e_step(torch, dev(s0), dev(s1), fa._whitener(torch, _ubm(fx), gpu), dev(fx["tv_init"]), 16)
    errs.update({"_A": ivn.rel(_A, fx["A"]), "_C": ivn.rel(_C, fx["C"]), "_R": ivn.rel(_R, fx["R"])})
    _check(errs)


@pytest.mark.parametrize("tag,min_div", [("md", True), ("nomd", False)])
def test_total_variability_device_every_recorded_iteration(gpu, fx, tag, min_div):
    import torch
    from sidekit_amd.factor_analyser import total_variability_device
    s0, s1 = torch.as_tensor(fx["stat0"]).to(gpu), torch.as_tensor(fx["stat1"]).to(gpu)
    keep0, keep1 = s0.clone(), s1.clone()
    trace = []
    F = total_variability_device(s0, s1, _ubm(fx), R, nb_iter=3, min_div=min_div, tv_init=fx["tv_init"], after_iteration=lambda it, F: trace.append(F.copy()))
    assert len(trace) == 3 and numpy.array_equal(F, trace[-1]) and torch.equal(s0, keep0) and torch.equal(s1, keep1)
    errs = {f"F it{i}": ivn.rel(trace[i], fx[f"F_{tag}_it{i}"]) for i in range(3)}
    # one batch against several: 3 sessions per batch gives 14 batches
    per = 8 * (R * (R + 1) // 2 + C * D + C + 2 * R)
    small = total_variability_device(s0, s1.view(N, C, D), _ubm(fx), R, nb_iter=3, min_div=min_div,
                                     tv_init=fx["tv_init"], max_workspace_bytes=3 * per)
    errs["F, 14 batches against one"] = ivn.rel(small, F)
    _check(errs)


def test_total_variability_from_files_and_a_seeded_start(gpu, fx, tmp_path):
    from sidekit_amd.factor_analyser import FactorAnalyser
    from sidekit_amd.statserver import StatServer
    ubm = _ubm(fx)
    whole, first, second = (str(tmp_path / n) for n in ("all.h5", "first.h5", "second.h5"))
    _server(fx).write(whole)
    _server(fx, slice(0, 23)).write(first)
    _server(fx, slice(23, None)).write(second)
    numpy.testing.assert_array_equal(StatServer.read(whole).stat1, fx["stat1"])
    out = str(tmp_path / "tv")
    one = FactorAnalyser()
    one.total_variability(whole, ubm, R, nb_iter=3, min_div=True, tv_init=fx["tv_init"].copy(), batch_size=16, save_init=True, output_file_name=out)
    assert not one.mean.any() and not one.Sigma.any() and one.mean.shape == one.Sigma.shape == (C * D,)
    two = FactorAnalyser()
    two.total_variability([first, second], ubm, R, nb_iter=3, min_div=True, tv_init=fx["tv_init"].copy(), num_thread=4)
    obj = FactorAnalyser()
    obj.total_variability_single(_server(fx), ubm, R, nb_iter=3, min_div=False, tv_init=fx["tv_init"].copy())
    errs = {"F from one file": ivn.rel(one.F, fx["F_md_it2"]), "F from two files": ivn.rel(two.F, fx["F_md_it2"]),
            "F from a StatServer, no min_div": ivn.rel(obj.F, fx["F_nomd_it2"])}
    for name, want in (("_init", fx["tv_init"]), ("_it-0", fx["F_md_it0"]), ("_it-1", fx["F_md_it1"]), ("", fx["F_md_it2"])):
        saved = FactorAnalyser.read(out + name + ".h5")
        errs[f"saved tv{name}.h5"] = ivn.rel(saved.F, want)
        assert saved.G is None and saved.H is None and saved.mean.shape == (C * D,)
    assert not os.path.exists(out + "_it-2.h5")
    _check(errs)
    # tv_init=None draws numpy.random.randn(sv_size, tv_rank) as the reference does
    numpy.random.seed(5)
    start = numpy.random.randn(C * D, R)
    numpy.random.seed(5)
    drawn = FactorAnalyser()
    drawn.total_variability(whole, ubm, R, nb_iter=1)
    given = FactorAnalyser()
    given.total_variability(whole, ubm, R, nb_iter=1, tv_init=start)
    numpy.testing.assert_array_equal(drawn.F, given.F)


def test_extract_ivectors_against_the_fixture(gpu, fx, tmp_path):
    import torch
    from sidekit_amd.factor_analyser import FactorAnalyser, extract_ivectors_device
    ubm = _ubm(fx)
    fa = FactorAnalyser(F=fx["F_md_it2"])
    server = _server(fx)
    iv, sigma = fa.extract_ivectors_single(ubm, server, uncertainty=True)
    errs = {"single: iv": ivn.rel(iv.stat1, fx["iv"]), "single: iv_sigma": ivn.rel(sigma, fx["iv_sigma"]),
            "single: the caller's statistics are left whitened": ivn.rel(server.stat1, fx["stat1_whitened"])}
    assert numpy.array_equal(iv.stat0, numpy.ones((N, 1))) and numpy.array_equal(iv.segset, server.segset) and iv.modelset is not server.modelset
    assert iv.start.shape == (N,) and iv.validate()
    plain = fa.extract_ivectors_single(ubm, _server(fx))
    assert numpy.array_equal(plain.stat1, iv.stat1)
    path = str(tmp_path / "stats.h5")
    _server(fx).write(path, prefix="tv/")
    from_file, file_sigma = fa.extract_ivectors(ubm, path, prefix="tv/", uncertainty=True, batch_size=7, num_thread=3)
    untouched = _server(fx)
    from_object = fa.extract_ivectors(ubm, untouched)
    numpy.testing.assert_array_equal(untouched.stat1, fx["stat1"])
    errs.update({"file: iv": ivn.rel(from_file.stat1, fx["iv"]), "file: iv_sigma": ivn.rel(file_sigma, fx["iv_sigma"]),
                 "object: iv": ivn.rel(from_object.stat1, fx["iv"])})
    assert numpy.array_equal(from_file.segset, server.segset) and from_file.stat0.shape == (N, 1) and all(v is None for v in from_file.start)
    # one batch against several
    s0, s1 = torch.as_tensor(fx["stat0"]).to(gpu), torch.as_tensor(fx["stat1"]).to(gpu)
    per = 8 * (R * (R + 1) // 2 + C * D + C + 2 * R)
    big, big_sigma = extract_ivectors_device(s0, s1, ubm, fa.F, uncertainty=True)
    small, small_sigma = extract_ivectors_device(s0, s1, ubm, fa.F, uncertainty=True, max_workspace_bytes=7 * per)
    only = extract_ivectors_device(s0, s1, ubm, fa.F)
    assert big.is_cuda and big.dtype == torch.float64 and torch.equal(only, big)
    errs.update({"device: iv": ivn.rel(_np(big), fx["iv"]), "6 batches against one: iv": ivn.rel(_np(small), _np(big)),
                 "6 batches against one: iv_sigma": ivn.rel(_np(small_sigma), _np(big_sigma))})
    _check(errs)


# ---- chain: frames -> statistics -> i-vectors without a host copy ---------------------------------------------------------------------------

def test_statistics_of_resident_frames_feed_the_extraction(gpu, golden_dir):
    import torch
    from sidekit_amd.factor_analyser import extract_ivectors_device
    from sidekit_amd.mixture import Mixture, gmm_stats_device
    mx = dict(numpy.load(os.path.join(golden_dir, "mixture.npz")))
    keys = ("w", "mu", "invcov", "cov_var_ctl")
    ubm = Mixture()
    ubm.w, ubm.mu, ubm.invcov, ubm.cov_var_ctl = (numpy.array(mx[f"split4_{k}"], dtype=numpy.float64) for k in keys)
    ubm.cst, ubm.det = numpy.zeros(ubm.w.shape), numpy.zeros(ubm.w.shape)
    ubm._compute_all()
    F = 0.1 * numpy.random.RandomState(3).randn(ubm.sv_size(), 5)
    stat0, stat1, _, _ = gmm_stats_device(ubm, torch.as_tensor(mx["X"]).to(gpu), mx["seg_off"], order=1)
    assert stat0.is_cuda and stat1.dim() == 3
    iv, sigma = extract_ivectors_device(stat0, stat1, ubm, F, uncertainty=True)
    assert iv.is_cuda and iv.shape == (8, 5)
    h0, h1 = _np(stat0), _np(stat1).reshape(8, -1)
    lam = numpy.eye(5)[None] + ivn.unpack(h0.dot(ivn.gram(F, 8, 23)), 5)
    assert max(numpy.linalg.cond(m) for m in lam) <= 1e3
    want_iv, want_sigma = ivn.extract(h0, h1, ubm.mu, ubm.invcov, F)
    _check({"iv": ivn.rel(_np(iv), want_iv), "iv_sigma": ivn.rel(_np(sigma), want_sigma), "stat0 vs fixture": mxn.rel(h0, mx["acc_stat0"])})
    assert numpy.array_equal(_np(sigma)[2], numpy.ones(5)) and not _np(iv)[2].any(), "the empty segment: Lambda = I, b = 0"
