"""Back-end normalisation on the GPU (sidekit_amd/backend.py, the StatServer methods, csrc/plda_train.hip ``sc_scatter_within``,
csrc/backend.hip ``sc_whiten_rows``) against the reference's own output (tests/golden/backend.npz) and against the float64 numpy
restatement that tests/test_backend_cpu.py pins to it.

Tolerances: 1e-9 relative (max-norm) for every float64 quantity, the project's bound for them; the consumers' score
matrices by the bounds of their own fixture tests (float32 cosine 2e-6 absolute, float64 1e-9); the kernels alone 1e-12 against
``numpy.einsum`` / ``numpy.dot`` in float64 (the bound of ``test_tn_product``).  float32 input is compared with the restatement run on
the SAME float32 values widened to float64.  From the second iteration of spectral normalisation on, everything lives in a basis fixed
by eigenvector signs (``whiten_stat1`` multiplies by ``V diag(lambda^-1/2)``), so iterations 2 and 3 are compared by what sign flips
leave invariant: sorted eigenvalues of each covariance, the length of each mean, the Gram matrix of the transformed rows.  The LDA
matrix is compared only where the test has first shown, on the restatement's spectrum, that the eigenvalue gaps condition it.
"""
import json
import os
import sys

import numpy
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import backend_numpy as bn  # noqa: E402
import plda_bits  # noqa: E402
import plda_em_numpy as pen  # noqa: E402

from sidekit_amd import backend  # noqa: E402
from sidekit_amd import factor_analyser as fa  # noqa: E402
from sidekit_amd import iv_scoring  # noqa: E402
from sidekit_amd.bosaris import Ndx  # noqa: E402
from sidekit_amd.statserver import StatServer  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _check(errs, tol, what):
    print(what, {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < tol, f"{what}: {k} differs by {v:.3e} (relative max-norm, bound {tol})"


def _stat_server(ids, X):
    return StatServer.from_arrays(ids, numpy.array([f"seg{i:04d}" for i in range(X.shape[0])], dtype="|O"), X)


def _invariants(means, covs, rows, ref_means, ref_covs, ref_rows, sel):
    """what eigenvector sign flips leave alone, iterations 2.. (and the Gram matrix of the rows `sel`)"""
    errs = {}
    for i in range(1, len(means)):
        errs[f"eig(covs[{i}])"] = pen.rel(bn.sorted_eigenvalues(covs[i]), bn.sorted_eigenvalues(ref_covs[i]))
        errs[f"|means[{i}]|"] = abs(numpy.linalg.norm(means[i]) / numpy.linalg.norm(ref_means[i]) - 1)
    errs["Gram"] = pen.rel(rows[sel].dot(rows[sel].T), ref_rows[sel].dot(ref_rows[sel].T))
    return errs


# ---- 1. the reference's fixture, through the StatServer methods ------------------------------------------------------------------

@pytest.fixture(scope="module")
def fx(golden_dir):
    return numpy.load(os.path.join(golden_dir, "backend.npz"))


def test_fixture_matrices_through_the_stat_server(gpu, fx):
    X, ids, rank = fx["X"], fx["modelset"].astype("|O"), int(fx["rank"])
    s = _stat_server(ids, X)
    L = s.get_lda_matrix_stat1(rank)
    assert L.shape == (X.shape[1], rank)
    wccn = s.get_wccn_choleski_stat1()
    numpy.testing.assert_array_equal(wccn, numpy.tril(wccn))
    errs = {"within": pen.rel(s.get_within_covariance_stat1(), fx["within"]), "between": pen.rel(s.get_between_covariance_stat1(), fx["between"]),
            "total": pen.rel(backend.covariances_device(torch.as_tensor(X).to(gpu), ids)[3], fx["total"]),
            "total (host method)": pen.rel(s.get_total_covariance_stat1(), fx["total"]),
            "wccn": pen.rel(wccn, fx["wccn"]), "mahalanobis": pen.rel(s.get_mahalanobis_matrix_stat1(), fx["mahalanobis"]),
            "LL'": pen.rel(L.dot(L.T), fx["L"].dot(fx["L"].T)), "L": pen.rel(pen.sign_align(L, fx["L"]), fx["L"])}
    _check(errs, TOL, "fixture")
    numpy.testing.assert_array_equal(s.stat1, X)                      # none of these touches the statistics


def test_fixture_branches_no_estimate_reaches(gpu, fx):
    """whiten_cholesky_stat1 with a full and a diagonal covariance, spectral_norm_stat1 with a diagonal covariance and with
    is_sqr_inv_sigma=True: each against the rows the reference produced (every row_step-th is stored)"""
    X, ids, mu, step = fx["X"], fx["modelset"].astype("|O"), fx["mean"], int(fx["row_step"])
    diag = numpy.diag(fx["total"]).copy()
    errs = {}
    for key, call in (("chol_stat1", lambda t: t.whiten_cholesky_stat1(mu, fx["total"])),
                      ("chol_diag_stat1", lambda t: t.whiten_cholesky_stat1(mu, diag)),
                      ("diag_stat1", lambda t: t.spectral_norm_stat1([mu], [diag])),
                      ("sqrinv_stat1", lambda t: t.spectral_norm_stat1([mu, 0.1 * mu], [fx["wccn"], fx["mahalanobis"]], True))):
        t = _stat_server(ids, X)
        call(t)
        assert t.stat1.shape == X.shape
        errs[key] = pen.rel(t.stat1[::step], fx[key])
    _check(errs, TOL, "fixture")


@pytest.mark.parametrize("mode", ["efr", "sphNorm"])
def test_fixture_spectral_normalisation(gpu, fx, mode):
    X, ids, it, step = fx["X"], fx["modelset"].astype("|O"), int(fx["it"]), int(fx["row_step"])
    ref_means, ref_covs, ref_rows = fx[f"{mode}_means"], fx[f"{mode}_covs"], fx[f"{mode}_stat1"]     # every step-th transformed row
    s = _stat_server(ids, X)
    s.spectral_norm_stat1(list(ref_means), list(ref_covs))            # with the fixture's lists: deterministic given (mu, cov)
    errs = {"apply": pen.rel(s.stat1[::step], ref_rows)}
    s = _stat_server(ids, X)
    means, covs = s.estimate_spectral_norm_stat1(it, mode)
    numpy.testing.assert_array_equal(s.stat1, X)                      # the estimate leaves stat1 untouched
    assert len(means) == len(covs) == it
    errs.update({"means[0]": pen.rel(means[0], ref_means[0]), "covs[0]": pen.rel(covs[0], ref_covs[0])})
    s.spectral_norm_stat1(means, covs)
    errs.update(_invariants(means, covs, s.stat1[::step], ref_means, ref_covs, ref_rows, slice(None)))
    _check(errs, TOL, f"fixture {mode}")
    m2, c2, rows = backend.spectral_norm_estimate_device(torch.as_tensor(X).to(gpu), ids, it, mode)
    assert rows.is_cuda and rows.dtype == torch.float64
    numpy.testing.assert_array_equal(rows.cpu().numpy(), s.stat1)     # the rows the estimate keeps are the rows apply gives
    for a, b in zip(m2 + c2, means + covs):
        numpy.testing.assert_array_equal(a, b)


def test_fixture_consumers_scored_with_the_produced_matrices(gpu, fx):
    """producer -> consumer: the matrices come from the GPU methods, the scores are compared with the reference's, which used its own"""
    X, ids = fx["X"], fx["modelset"].astype("|O")
    ne, nt = int(fx["n_enrol"]), int(fx["n_test"])
    s = _stat_server(ids, X)
    wccn, maha = s.get_wccn_choleski_stat1(), s.get_mahalanobis_matrix_stat1()
    W, B = s.get_within_covariance_stat1(), s.get_between_covariance_stat1()
    segs = numpy.array([f"seg{i:04d}" for i in range(X.shape[0])], dtype="|O")
    enr_ids, tst_ids = segs[:ne], segs[ne:ne + nt]
    enroll, test = StatServer.from_arrays(enr_ids, enr_ids, X[:ne]), StatServer.from_arrays(tst_ids, tst_ids, X[ne:ne + nt])
    mm, ss = numpy.meshgrid(numpy.arange(ne), numpy.arange(nt), indexing="ij")
    ndx = Ndx(models=enr_ids[mm.ravel()], testsegs=tst_ids[ss.ravel()])
    cos = iv_scoring.cosine_scoring(enroll, test, ndx, wccn=wccn)
    assert list(cos.modelset) == list(enr_ids) and list(cos.segset) == list(tst_ids)
    print("cosine(wccn) max abs", numpy.abs(cos.scoremat - fx["cos_wccn_scoremat"]).max())
    numpy.testing.assert_allclose(cos.scoremat, fx["cos_wccn_scoremat"], atol=2e-6)
    errs = {"mahalanobis scores": pen.rel(iv_scoring.mahalanobis_scoring(enroll, test, ndx, maha).scoremat, fx["maha_scoremat"]),
            "two-covariance scores": pen.rel(iv_scoring.two_covariance_scoring(enroll, test, ndx, W, B).scoremat, fx["twocov_scoremat"])}
    _check(errs, TOL, "consumers")


# ---- 2. the shapes of test_shapes_against_the_restatement -------------------------------------------------------------------------

def _synthetic(seed, D, counts, dtype):
    """class centres + within-class noise around a common offset, rows shuffled; integer labels that are not 0..C-1
    (tests/test_gpu_plda_train.py's corpus)"""
    rs = numpy.random.RandomState(seed)
    lab = numpy.repeat(numpy.arange(len(counts)), counts)
    centres = rs.randn(len(counts), D)
    X = 0.3 + centres[lab] + 1.5 * rs.randn(lab.shape[0], D)
    p = rs.permutation(X.shape[0])
    p = p[:p.shape[0] - (p.shape[0] - 37) % 64]        # N = 37 mod 64: no multiple of any tile or slab
    return X[p].astype(dtype), 7 + 3 * lab[p]


_COUNTS = {"half": lambda: numpy.concatenate(([619], numpy.random.RandomState(3).randint(1, 30, 40))),       # one class holds half the rows
           "3000": lambda: numpy.random.RandomState(4).randint(1, 41, 3000)}                                  # 3 000 classes of 1-40 sessions
LDA_RANK = 10     # seed 7: smallest gap among the top 11 eigenvalues 2.7e-3 ("half", D 50) and 1.9e-3 ("3000", D 256) of the largest


@pytest.mark.parametrize("layout,D", [("half", 50), ("3000", 256)])
@pytest.mark.parametrize("dtype", [numpy.float32, numpy.float64])
def test_shapes_against_the_restatement(gpu, layout, D, dtype):
    X, lab = _synthetic(7, D, _COUNTS[layout](), dtype)
    assert X.shape[0] % 64 == 37 and X.dtype == dtype
    X64 = X.astype(numpy.float64)                                      # float32 input: the same values, widened
    xv = torch.as_tensor(X).to(gpu)
    what = f"{layout} D={D} {numpy.dtype(dtype).name} N={X.shape[0]}"
    mu, within, between, total = backend.covariances_device(xv, lab)
    mu_r, within_r, between_r, total_r = bn.covariances(X64, lab)
    errs = {"mean": pen.rel(mu, mu_r), "within": pen.rel(within, within_r), "between": pen.rel(between, between_r), "total": pen.rel(total, total_r),
            "within + between = total": pen.rel(within + between, total_r),
            "wccn": pen.rel(backend.wccn_device(xv, lab), bn.wccn(X64, lab)),
            "mahalanobis": pen.rel(backend.mahalanobis_device(xv, torch.as_tensor(lab).to(gpu)), bn.mahalanobis(X64, lab))}
    # LDA: eigenvector error is perturbation / eigenvalue gap, so the comparison is conditioned on the restatement's spectrum
    gap = bn.top_gap(bn.lda_spectrum(X64, lab)[0], LDA_RANK)
    print(what, f"LDA rank {LDA_RANK}: smallest gap among the top {LDA_RANK + 1} eigenvalues / largest = {gap:.2e}")
    assert gap >= 1e-4, "pick a rank and a seed whose eigenvalue gaps condition the comparison"
    L, L_r = backend.lda_device(xv, lab, LDA_RANK), bn.lda(X64, lab, LDA_RANK)
    errs.update({"LL'": pen.rel(L.dot(L.T), L_r.dot(L_r.T)), "L": pen.rel(pen.sign_align(L, L_r), L_r)})
    sel = numpy.arange(0, X.shape[0], max(1, X.shape[0] // 700))       # the Gram matrix of every ~N/700-th row
    for mode in ("efr", "sphNorm"):
        means_r, covs_r, rows_r = bn.spectral_norm_estimate(X64, lab, 2, mode)
        means, covs, rows = backend.spectral_norm_estimate_device(xv, lab, 2, mode)
        assert rows.is_cuda and rows.shape == xv.shape
        errs.update({f"{mode} means[0]": pen.rel(means[0], means_r[0]), f"{mode} covs[0]": pen.rel(covs[0], covs_r[0])})
        errs.update({f"{mode} {k}": v for k, v in _invariants(means, covs, rows.cpu().numpy(), means_r, covs_r, rows_r, sel).items()})
        applied = backend.spectral_norm_apply_device(xv, means_r, covs_r)             # the restatement's lists: deterministic
        errs[f"{mode} apply"] = pen.rel(applied.cpu().numpy(), rows_r)
    _check(errs, TOL, what)


# ---- 3. the kernels alone ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 777, 100003])
@pytest.mark.parametrize("D", [37, 256])
@pytest.mark.parametrize("dtype", [numpy.float32, numpy.float64])
def test_scatter_within(gpu, N, D, dtype):
    rs = numpy.random.RandomState(N % 1000 + D)
    C = max(1, min(N // 3, 900))
    cls = rs.randint(0, C, N).astype(numpy.int32)
    if N > 1:
        cls[cls == 1] = 0
        cls[N // 2] = 1                                                # class 1: a single row, which contributes exactly zero
    X = (0.4 + rs.randn(C, D)[cls] + 0.5 * rs.randn(N, D)).astype(dtype)
    X64 = X.astype(numpy.float64)
    counts = numpy.maximum(numpy.bincount(cls, minlength=C), 1)
    Mc = numpy.zeros((C, D))
    numpy.add.at(Mc, cls, X64)
    Mc /= counts[:, None]
    w = rs.uniform(0.05, 3.0, C)
    xv = torch.as_tensor(X).to(gpu)
    for tag, wv in (("plain", None), ("weights", w)):
        Z = X64 - Mc[cls]
        want = numpy.einsum("k,km,kn->mn", numpy.ones(N) if wv is None else wv[cls], Z, Z)
        got = backend.scatter_within_device(xv, cls, Mc, wv).cpu().numpy()
        if N == 1:                                                     # one row, its own mean: zero, exactly
            assert not got.any() and not want.any()
            continue
        err = pen.rel(got, want)
        print(f"scatter_within N={N} D={D} {numpy.dtype(dtype).name} {tag}: {err:.2e}")
        assert err < 1e-12, (tag, err)
    if N > 1:
        # the single-row class contributes exactly zero whatever its weight; an out-of-range class number is skipped
        w_big = w.copy()
        w_big[1] = 1e30
        a = backend.scatter_within_device(xv, cls, Mc, w).cpu().numpy()
        numpy.testing.assert_array_equal(backend.scatter_within_device(xv, cls, Mc, w_big).cpu().numpy(), a)
        bad = cls.copy()
        bad[N // 2] = C + 5
        bad[0] = -1
        keep = numpy.ones(N, dtype=bool)
        keep[[0, N // 2]] = False
        Z = X64[keep] - Mc[cls[keep]]
        assert pen.rel(backend.scatter_within_device(xv, bad, Mc, None).cpu().numpy(), Z.T.dot(Z)) < 1e-12


@pytest.mark.parametrize("N,D", [(777, 37), (100003, 256)])
def test_scatter_within_when_the_class_means_dwarf_the_spread(gpu, N, D):
    """Class means 1e4 times the within-class spread, float64 input: the direct form holds 1e-12 of the within scatter (numpy's own
    class-centred product: 7e-14).  The by-difference form (total scatter minus between scatter, both from sc_gemm_tn) is printed
    beside it: its error is eps x |total| / |within|, which is why the kernel exists."""
    rs = numpy.random.RandomState(D)
    C = max(2, N // 40)
    cls = rs.randint(0, C, N).astype(numpy.int32)
    X = 1e4 * rs.randn(C, D)[cls] + rs.randn(N, D)
    counts = numpy.maximum(numpy.bincount(cls, minlength=C), 1).astype(numpy.float64)
    S = numpy.zeros((C, D))
    numpy.add.at(S, cls, X)
    Mc = S / counts[:, None]
    # the yardstick, free of cancellation: centre in extended precision, then accumulate in float64
    Z = (X.astype(numpy.longdouble) - Mc.astype(numpy.longdouble)[cls]).astype(numpy.float64)
    want = Z.T.dot(Z)
    xv = torch.as_tensor(X).to(gpu)
    direct = pen.rel(backend.scatter_within_device(xv, cls, Mc).cpu().numpy(), want)
    mu = X.mean(axis=0)
    total = fa.gemm_tn_device(xv, None, None, mu, mu).cpu().numpy()
    between = fa.gemm_tn_device(torch.as_tensor(Mc).to(gpu), None, counts, mu, mu).cpu().numpy()
    print(f"ill-conditioned N={N} D={D}: direct {direct:.2e}, by difference {pen.rel(total - between, want):.2e}, "
          f"|total| / |within| = {numpy.abs(total).max() / numpy.abs(want).max():.1e}")
    assert direct < 1e-12


@pytest.mark.parametrize("N,D,P", [(1, 37, 37), (100003, 50, 10), (5000, 256, 256), (777, 256, 129), (333, 40, 300)])
@pytest.mark.parametrize("dtype", [numpy.float32, numpy.float64])
def test_whiten_rows(gpu, N, D, P, dtype):
    """(333, 40, 300): more than 256 columns, where a normalising call goes through the two-pass form"""
    rs = numpy.random.RandomState(N % 1000 + P)
    X = (0.3 + rs.randn(N, D)).astype(dtype)
    mu = X.astype(numpy.float64).mean(axis=0) + 0.1 if N > 1 else 0.1 * rs.randn(D)
    if N > 2:
        mu = X[2].astype(numpy.float64)                                # row 2 equals mu: zeros out, finite
    R = rs.randn(D, P) / numpy.sqrt(D)
    xv = torch.as_tensor(X).to(gpu)
    for use_mu in (True, False):
        for normalize in (False, True):
            want = bn.whiten_rows(X.astype(numpy.float64), mu if use_mu else None, R, normalize)
            got = backend.whiten_rows_device(xv, mu if use_mu else None, R, normalize)
            assert got.dtype == torch.float64 and got.shape == (N, P)
            g = got.cpu().numpy()
            assert numpy.isfinite(g).all()
            err = pen.rel(g, want)
            print(f"whiten_rows N={N} D={D} P={P} {numpy.dtype(dtype).name} mu={use_mu} normalize={normalize}: {err:.2e}")
            assert err < 1e-12, (use_mu, normalize, err)
            if use_mu and N > 2:
                assert not g[2].any()
            if normalize:
                lengths = numpy.linalg.norm(numpy.delete(g, 2, axis=0) if use_mu and N > 2 else g, axis=1)
                numpy.testing.assert_allclose(lengths, 1.0, rtol=1e-14)
            g32 = backend.whiten_rows_device(xv, mu if use_mu else None, R, normalize, torch.float32)
            assert g32.dtype == torch.float32
            numpy.testing.assert_array_equal(g32.cpu().numpy(), g.astype(numpy.float32))       # the float64 result rounded once


def test_argument_errors_are_reported_before_anything_is_enqueued(gpu):
    x = torch.zeros((8, 6), dtype=torch.float64, device=gpu)
    from sidekit_amd import _lib
    R = torch.eye(6, dtype=torch.float64, device=gpu)
    with pytest.raises(ValueError, match="may not alias"):
        _lib.check(_lib.lib().sc_whiten_rows(x.data_ptr(), _lib.XT_F64, 8, 6, None, R.data_ptr(), 6, 0, x.data_ptr(), _lib.XT_F64, None))
    with pytest.raises(ValueError, match="null argument"):
        _lib.check(_lib.lib().sc_whiten_rows(x.data_ptr(), _lib.XT_F64, 8, 6, None, None, 6, 0, x.data_ptr(), _lib.XT_F64, None))
    with pytest.raises(ValueError, match="bad sizes"):
        _lib.check(_lib.lib().sc_scatter_within(x.data_ptr(), _lib.XT_F64, 0, 6, x.data_ptr(), x.data_ptr(), None, 1, x.data_ptr(), None))
    with pytest.raises(ValueError, match="XT_F32 or XT_F64"):
        _lib.check(_lib.lib().sc_scatter_within(x.data_ptr(), _lib.XT_BF16, 8, 6, x.data_ptr(), x.data_ptr(), None, 1, x.data_ptr(), None))


# ---- 4. bits -------------------------------------------------------------------------------------------------------------------------

def _every_function(xv, lab):
    out = list(backend.covariances_device(xv, lab))
    out += [backend.lda_device(xv, lab, 32), backend.wccn_device(xv, lab), backend.mahalanobis_device(xv, lab)]
    for mode in ("efr", "sphNorm"):
        means, covs, rows = backend.spectral_norm_estimate_device(xv, lab, 2, mode)
        out += means + covs + [rows.cpu().numpy(), backend.spectral_norm_apply_device(xv, means, covs, out_dtype=torch.float32).cpu().numpy()]
    out.append(backend.whiten_rows_device(xv, out[0], out[4], True).cpu().numpy())
    return out


def test_two_runs_and_a_side_stream_give_identical_bits(gpu):
    X, lab = _synthetic(10, 256, _COUNTS["3000"](), numpy.float32)
    xv = torch.as_tensor(X).to(gpu)
    first = _every_function(xv, lab)
    second = _every_function(xv, lab)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        third = _every_function(xv, lab)
    side.synchronize()
    assert len(first) == len(second) == len(third)
    for x, y, z in zip(first, second, third):
        numpy.testing.assert_array_equal(x, y)
        numpy.testing.assert_array_equal(x, z)


def test_the_existing_entry_points_give_the_bits_they_gave(gpu, golden_dir):
    """sc_plda_fast / sc_gemm_tn / sc_dgemm_nn on fixed inputs against the digests recorded on the commit before dgemm_tile gained the
    gathered-centre operand form (tests/tools/plda_bits.py)."""
    with open(os.path.join(golden_dir, "plda_bits.json")) as f:
        recorded = json.load(f)
    now = plda_bits.digests(gpu)
    assert sorted(now) == sorted(recorded)
    changed = [k for k in recorded if now[k] != recorded[k]]
    assert not changed, f"bits changed: {changed}"


def test_the_f64_tile_users_give_the_bits_they_gave(gpu, golden_dir):
    """Every other user of csrc/dgemm_tile.h (the scatters, the Gram, the whitening, the log-likelihoods, the JFA shift, the PLDA histograms
    and cohort moments) on fixed inputs against the digests recorded with the library of the commit before the tile's loaders, lane map and
    tile store were consolidated (tests/tools/plda_bits.py, tile_digests).  A digest that differs is a changed kernel, not a fixture to
    record again."""
    with open(os.path.join(golden_dir, "f64_tile_bits.json")) as f:
        recorded = json.load(f)
    now = plda_bits.tile_digests(gpu)
    assert sorted(now) == sorted(recorded)
    changed = [k for k in recorded if now[k] != recorded[k]]
    assert not changed, f"bits changed: {changed}"


# ---- 5. the driver -------------------------------------------------------------------------------------------------------------------

def test_driver_applies_lda_and_sphnorm_on_the_device(gpu, capsys):
    from sidekit_amd.bin import shard_extract_score as drv
    n = 400
    args = ["--utterances", "2048", "--batch", "256", "--seconds", "1", "--trials", str(n), "--speakers", "40", "--plda-rank", "32",
            "--plda-train", "em", "--lda", "64", "--sphnorm", "2"]
    keep = {}
    out = drv.main(args, keep=keep)
    capsys.readouterr()
    xv, labels = keep["xv"], keep["labels"]
    assert xv.is_cuda and xv.dtype == torch.float32
    assert out["backend_normalisation"]["lda_rank"] == 64 and out["backend_normalisation"]["sphnorm_iterations"] == 2
    assert out["backend_normalisation"]["dimension"] == 64
    L = backend.lda_device(xv[2 * n:], labels[2 * n:], 64)
    numpy.testing.assert_array_equal(keep["transforms"]["lda"], L)
    projected = backend.whiten_rows_device(xv, None, L)
    means, covs, _ = backend.spectral_norm_estimate_device(projected[2 * n:], labels[2 * n:], 2, "sphNorm")
    for a, b in zip(keep["transforms"]["sphnorm"][0] + keep["transforms"]["sphnorm"][1], means + covs):
        numpy.testing.assert_array_equal(a, b)
    rows = backend.spectral_norm_apply_device(projected, means, covs)
    E, T, train = keep["plda_rows"]
    for t in (E, T, train):
        assert t.is_cuda and t.dtype == torch.float64 and t.shape[1] == 64      # the x-vectors stay on the device throughout
    assert torch.equal(torch.cat((E, T, train)), rows)
    for x, y in zip(keep["plda"], fa.plda_device(train, labels[2 * n:], 32)):
        assert numpy.isfinite(x).all()
        numpy.testing.assert_array_equal(x, y)
    for name in ("cosine_eer", "plda_eer"):
        assert numpy.isfinite(out[name]) and 0.0 <= out[name] <= 0.5
