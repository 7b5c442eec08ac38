"""The Gaussian back-end on the GPU (sidekit_amd/lid_utils.py; csrc/gaussian_backend.hip ``sc_class_scatter``, ``sc_gauss_loglik``,
``sc_closed_set_llr``) against the reference's own output (tests/golden/gaussian_backend.npz) and against the float64 numpy
restatement that tests/test_gaussian_backend_cpu.py pins to it.

Tolerances: 1e-9 relative (max-norm) for parameters and score matrices, the project's bound for float64 quantities (``TOL`` of
test_gpu_backend.py and the fast-PLDA fixtures); ``sc_class_scatter`` and ``sc_closed_set_llr`` alone 1e-12 against numpy in float64
(the bound of ``test_tn_product``); float32 input against the restatement run on the SAME float32 values widened.  Where the
documentation promises equal bits (a row of ``sc_gauss_loglik`` whatever N, its place, the tile edge or the stream; the tied route and
``sc_plda_fast`` by hand; in place and out of place) the comparison is ``array_equal``.

Shapes beyond the fixture are the smallest that reach another path: classes longer than 512 rows (k-slabs, with a class that leaves its
later slabs empty), D >= 128 with a class of 4096 rows or more (the 128 tile of ``sc_class_scatter``), D = 150 (three 64-column tiles, the
last one partial; two 128-column ones) and N large enough for ``cdiv(N, 128) * C >= 512`` (the 128 tile of ``sc_gauss_loglik``).
"""
import os
import sys

import numpy
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gaussian_backend_numpy as gbn  # noqa: E402
import plda_em_numpy as pen  # noqa: E402

from sidekit_amd import iv_scoring, lid_utils  # noqa: E402
from sidekit_amd.bosaris import Scores  # noqa: E402
from sidekit_amd.statserver import StatServer  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-9
KERNEL_TOL = 1e-12


def _check(errs, tol, what):
    print(what, {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < tol, f"{what}: {k} differs by {v:.3e} (relative max-norm, bound {tol})"


def _stat_server(ids, X):
    return StatServer.from_arrays(ids, numpy.array([f"seg{i:04d}" for i in range(X.shape[0])], dtype="|O"), X)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return numpy.load(os.path.join(golden_dir, "gaussian_backend.npz"))


def _dev(a, gpu, dtype=torch.float64):
    return torch.as_tensor(numpy.ascontiguousarray(a)).to(device=gpu, dtype=dtype)


# ---- 1. the reference's fixture ------------------------------------------------------------------------------------------------------

def test_fixture_through_the_stat_server_functions(gpu, fx):
    train = _stat_server(fx["modelset"].astype("|O"), fx["X"])
    test = _stat_server(numpy.array([f"class{c}" for c in fx["test_classes"]], dtype="|O"), fx["T"])
    tied = lid_utils.gaussian_backend_train(train)
    hetero = lid_utils.gaussian_backend_train_hetero(train, float(fx["alpha"]))
    for params in (tied, hetero):
        assert isinstance(params[0], StatServer) and list(params[0].modelset) == list(fx["classes"])
    assert isinstance(tied[1], numpy.ndarray) and isinstance(tied[2], float)
    assert isinstance(hetero[1], list) and isinstance(hetero[2], list) and len(hetero[1]) == len(hetero[2]) == 7
    assert all(isinstance(c, float) for c in hetero[2]) and all(s.shape == (45, 45) for s in hetero[1])
    by_label = lid_utils._gaussian_backend_train(fx["X"], fx["modelset"].astype("|O"))
    errs = {"means": pen.rel(tied[0].stat1, fx["means"]), "hetero means": pen.rel(hetero[0].stat1, fx["means"]),
            "tied sigma": pen.rel(tied[1], fx["tied_sigma"]), "tied cst": pen.rel(tied[2], fx["tied_cst"]),
            "hetero sigma": pen.rel(numpy.array(hetero[1]), fx["hetero_sigma"]), "hetero cst": pen.rel(numpy.array(hetero[2]), fx["hetero_cst"]),
            "_gaussian_backend_train sigma": pen.rel(by_label[1], fx["tied_sigma"]), "_gaussian_backend_train cst": pen.rel(by_label[2], fx["tied_cst"])}
    scores = {"tied_ll": lid_utils.gaussian_backend_test(test, tied, compute_llr=False), "tied_llr": lid_utils.gaussian_backend_test(test, tied),
              "hetero_ll": lid_utils.gaussian_backend_test_hetero(test, hetero, compute_llr=False),
              "hetero_llr": lid_utils.gaussian_backend_test_hetero(test, hetero)}
    for key, s in scores.items():
        assert isinstance(s, Scores) and s.validate() and s.scoremask.all() and s.scoremask.dtype == bool
        assert list(s.modelset) == list(fx["classes"]) and list(s.segset) == list(test.segset) and s.scoremat.shape == (7, 301)
        errs[key] = pen.rel(s.scoremat, fx[key])
    _check(errs, TOL, "fixture, StatServer functions")
    numpy.testing.assert_array_equal(train.stat1, fx["X"])
    # the reference's compute_log_likelihood_ratio by its own name, on host matrices
    errs = {"tied": pen.rel(lid_utils.compute_log_likelihood_ratio(fx["tied_ll"]), fx["tied_llr"]),
            "hand": pen.rel(lid_utils.compute_log_likelihood_ratio(fx["hand"], float(fx["p_tar_hand"])), fx["hand_llr"])}
    _check(errs, KERNEL_TOL, "compute_log_likelihood_ratio")


def test_fixture_through_the_device_functions(gpu, fx):
    xv, tv, ids = _dev(fx["X"], gpu), _dev(fx["T"], gpu), fx["modelset"].astype("|O")
    means, sigma, cst = lid_utils.gaussian_backend_device(xv, ids)
    hmeans, sigmas, csts = lid_utils.gaussian_backend_hetero_device(xv, ids, float(fx["alpha"]))
    assert means.is_cuda and hmeans.is_cuda and sigmas.shape == (7, 45, 45) and csts.shape == (7,)
    tied_ll = lid_utils.gaussian_loglik_device(tv, means, sigma, cst)
    hetero_ll = lid_utils.gaussian_loglik_device(tv, hmeans, sigmas, csts)
    tied_llr, hetero_llr = lid_utils.closed_set_llr_device(tied_ll), lid_utils.closed_set_llr_device(hetero_ll)
    assert all(t.is_cuda and t.dtype == torch.float64 and t.shape == (7, 301) for t in (tied_ll, hetero_ll, tied_llr, hetero_llr))
    errs = {"means": pen.rel(means.cpu().numpy(), fx["means"]), "hetero means": pen.rel(hmeans.cpu().numpy(), fx["means"]),
            "tied sigma": pen.rel(sigma, fx["tied_sigma"]), "tied cst": pen.rel(cst, fx["tied_cst"]),
            "hetero sigma": pen.rel(sigmas, fx["hetero_sigma"]), "hetero cst": pen.rel(csts, fx["hetero_cst"]),
            "tied_ll": pen.rel(tied_ll.cpu().numpy(), fx["tied_ll"]), "hetero_ll": pen.rel(hetero_ll.cpu().numpy(), fx["hetero_ll"]),
            "tied_llr": pen.rel(tied_llr.cpu().numpy(), fx["tied_llr"]), "hetero_llr": pen.rel(hetero_llr.cpu().numpy(), fx["hetero_llr"])}
    # the fixture's own parameters through the scoring kernels alone, and a list of covariances as the reference hands them over
    errs["hetero_ll, fixture parameters"] = pen.rel(
        lid_utils.gaussian_loglik_device(tv, fx["means"], list(fx["hetero_sigma"]), list(fx["hetero_cst"])).cpu().numpy(), fx["hetero_ll"])
    errs["tied_ll, fixture parameters"] = pen.rel(
        lid_utils.gaussian_loglik_device(tv, fx["means"], fx["tied_sigma"], float(fx["tied_cst"])).cpu().numpy(), fx["tied_ll"])
    _check(errs, TOL, "fixture, device functions")
    # end to end: the class the LLRs name is the class the log-likelihoods name
    numpy.testing.assert_array_equal(hetero_llr.argmax(dim=0).cpu().numpy(), fx["hetero_ll"].argmax(axis=0))
    numpy.testing.assert_array_equal(hetero_llr.argmax(dim=0).cpu().numpy(), hetero_ll.argmax(dim=0).cpu().numpy())


# ---- 2. sc_class_scatter -------------------------------------------------------------------------------------------------------------

def _scatter_errs(S, X, ids):
    ref = gbn.class_scatters(X, ids)
    assert S.shape == ref.shape
    counts = numpy.unique(ids, return_counts=True)[1]
    errs = {}
    for c in range(ref.shape[0]):
        if counts[c] == 1:
            numpy.testing.assert_array_equal(S[c], numpy.zeros_like(S[c]))     # a class of one row: exact zeros
        else:
            errs[f"class {c} ({counts[c]} rows)"] = pen.rel(S[c], ref[c])
    return errs


def test_class_scatter_on_the_fixture_with_a_class_of_one(gpu, fx):
    X = numpy.concatenate((fx["X"][:100], fx["X"][7:8] * 1.5, fx["X"][100:]))
    ids = numpy.concatenate((fx["modelset"][:100], ["solo"], fx["modelset"][100:])).astype("|O")
    S, means = lid_utils.class_scatter_device(_dev(X, gpu), ids)
    assert S.shape == (8, 45, 45) and S.dtype == torch.float64 and means.shape == (8, 45)
    errs = _scatter_errs(S.cpu().numpy(), X, ids)
    assert len(errs) == 7 and "class 0 (3 rows)" in errs
    errs["means"] = pen.rel(means.cpu().numpy(), gbn.class_means(X, ids)[3])
    _check(errs, KERNEL_TOL, "sc_class_scatter, float64")
    X32 = X.astype(numpy.float32)
    S32, _ = lid_utils.class_scatter_device(_dev(X32, gpu, torch.float32), ids)
    _check(_scatter_errs(S32.cpu().numpy(), X32.astype(numpy.float64), ids), KERNEL_TOL, "sc_class_scatter, float32 rows widened")


@pytest.mark.parametrize("counts,dim", [((1100, 3, 600, 1), 45), ((4100, 7), 130)], ids=["k-slabs", "128-tile"])
def test_class_scatter_long_classes(gpu, counts, dim):
    """(1100, 3, 600, 1) x 45: three slabs of 368 rows (tn_cut), the class of 600 leaves its third slab empty, the short ones two;
    (4100, 7) x 130: the 128 x 128 tile (D >= 128, a class of 4096 rows or more), a partial second tile, nine slabs."""
    rs = numpy.random.RandomState(11)
    cls = rs.permutation(numpy.repeat(numpy.arange(len(counts)), counts))
    X = 0.4 * rs.randn(len(counts), dim)[cls] + 0.5 * rs.randn(cls.shape[0], dim) + 0.2
    S, _ = lid_utils.class_scatter_device(_dev(X, gpu), cls)
    _check(_scatter_errs(S.cpu().numpy(), X, cls), KERNEL_TOL, f"sc_class_scatter {counts} x {dim}")


# ---- 3. sc_gauss_loglik ----------------------------------------------------------------------------------------------------------------

def test_gauss_loglik_bits_do_not_depend_on_rows_tile_or_stream(gpu, fx):
    tv, means, sigmas, csts = _dev(fx["T"], gpu), fx["means"], fx["hetero_sigma"], fx["hetero_cst"]
    full = lid_utils.gaussian_loglik_device(tv, means, sigmas, csts).cpu().numpy()
    one = lid_utils.gaussian_loglik_device(tv[5:6], means, sigmas, csts).cpu().numpy()
    numpy.testing.assert_array_equal(one[:, 0], full[:, 5])
    shifted = lid_utils.gaussian_loglik_device(tv[3:200], means, sigmas, csts).cpu().numpy()
    numpy.testing.assert_array_equal(shifted, full[:, 3:200])
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        other = lid_utils.gaussian_loglik_device(tv, means, sigmas, csts)
    side.synchronize()
    numpy.testing.assert_array_equal(other.cpu().numpy(), full)
    # 32 copies of the rows: cdiv(9632, 128) * 7 = 532 >= 512 workgroups, the 128-row tile
    big = lid_utils.gaussian_loglik_device(tv.repeat(32, 1), means, sigmas, csts).cpu().numpy()
    assert big.shape == (7, 9632)
    numpy.testing.assert_array_equal(big, numpy.tile(full, (1, 32)))


@pytest.fixture(scope="module")
def wide():
    """3 classes, D = 150: three 64-column tiles (the last partial) or two 128-column ones per workgroup"""
    rs = numpy.random.RandomState(12)
    C, D, N = 3, 150, 200
    means = 0.6 * rs.randn(C, D)
    sigmas = numpy.stack([(lambda A: A.dot(A.T) / D + 0.2 * numpy.eye(D))(rs.randn(D, D)) for _ in range(C)])
    csts = numpy.array([gbn.constant(s) for s in sigmas])
    T = means[rs.randint(0, C, N)] + 0.5 * rs.randn(N, D) + 0.2
    return T, means, sigmas, csts, gbn.loglik(T, means, sigmas, csts)


def test_gauss_loglik_several_column_tiles(gpu, wide):
    T, means, sigmas, csts, ref = wide
    tv = _dev(T, gpu)
    small = lid_utils.gaussian_loglik_device(tv, means, sigmas, csts).cpu().numpy()
    _check({"64 tile": pen.rel(small, ref)}, TOL, "sc_gauss_loglik, D = 150")
    # 110 copies: cdiv(22000, 128) * 3 = 516 >= 512, the 128 tile: the same bits, row for row
    big = lid_utils.gaussian_loglik_device(tv.repeat(110, 1), means, sigmas, csts).cpu().numpy()
    numpy.testing.assert_array_equal(big, numpy.tile(small, (1, 110)))
    # float32 rows are widened once, as float64 rows of the same values
    t32 = _dev(T.astype(numpy.float32), gpu, torch.float32)
    numpy.testing.assert_array_equal(lid_utils.gaussian_loglik_device(t32, means, sigmas, csts).cpu().numpy(),
                                     lid_utils.gaussian_loglik_device(t32.double(), means, sigmas, csts).cpu().numpy())


def test_tied_route_is_sc_plda_fast(gpu, fx):
    tv = _dev(fx["T"], gpu)
    P = numpy.linalg.inv(fx["tied_sigma"])
    by_hand = iv_scoring.plda_matrix_device(fx["means"], tv, -P, P, float(fx["tied_cst"]))
    got = lid_utils.gaussian_loglik_device(tv, fx["means"], fx["tied_sigma"], float(fx["tied_cst"]))
    assert got.shape == (7, 301)
    numpy.testing.assert_array_equal(got.cpu().numpy(), by_hand.cpu().numpy())


# ---- 4. sc_closed_set_llr ------------------------------------------------------------------------------------------------------------

def test_closed_set_llr_hand_made_matrix(gpu, fx):
    """one class leading by 800 nats, an exact tie of the two largest, all equal, values near -1e4"""
    got = lid_utils.closed_set_llr_device(_dev(fx["hand"], gpu), float(fx["p_tar_hand"])).cpu().numpy()
    assert numpy.all(numpy.isfinite(got))
    _check({"hand-made": pen.rel(got, fx["hand_llr"])}, KERNEL_TOL, "sc_closed_set_llr")


@pytest.mark.parametrize("C,N,p_tar", [(2, 37, 0.5), (2, 37, 0.03), (300, 1000, 0.5), (300, 1000, 0.9)])
def test_closed_set_llr_against_the_restatement(gpu, C, N, p_tar):
    rs = numpy.random.RandomState(C + N)
    M = -80.0 + 30.0 * rs.randn(C, N)
    M[rs.randint(0, C, N // 4), numpy.arange(N // 4)] += 900.0        # a quarter of the columns: one class dominates
    M[1, N // 2:N // 2 + 5] = M[0, N // 2:N // 2 + 5] = 40.0          # exact ties of the two largest
    m = _dev(M, gpu)
    out = lid_utils.closed_set_llr_device(m, p_tar)
    got = out.cpu().numpy()
    assert numpy.all(numpy.isfinite(got))
    numpy.testing.assert_array_equal(m.cpu().numpy(), M)                                # out of place leaves M alone
    _check({f"C={C}": pen.rel(got, gbn.closed_set_llr(M, p_tar))}, KERNEL_TOL, "sc_closed_set_llr")
    same = lid_utils.closed_set_llr_device(m, p_tar, out=m)
    assert same is m
    numpy.testing.assert_array_equal(m.cpu().numpy(), got)                              # in place equals out of place
    if C == 2:   # two classes: the leave-one-out sum is the other class
        other = M[::-1]
        _check({"C=2 closed form": pen.rel(got, numpy.log(p_tar) + M - other - numpy.log(1 - p_tar))}, KERNEL_TOL, "sc_closed_set_llr")
