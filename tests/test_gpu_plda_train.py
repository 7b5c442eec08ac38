"""PLDA training on the GPU (sidekit_amd/factor_analyser.py, csrc/plda_train.hip) against the reference's own output and against the
float64 numpy restatement that tests/test_plda_train_cpu.py pins to it.

Tolerances: 1e-9 relative (max-norm) for every float64 PLDA quantity, the project's bound for them; a different
summation order in float64 sits five orders below it.  ``F`` is compared as ``F F'`` and, column signs aligned, directly.  float32
input is compared with the restatement run on the SAME float32 values widened to float64, never with a float64 fixture.  The kernels
alone: class sums and mean 1e-13, the TN product 1e-12 against ``numpy.einsum`` in float64.
"""
import os
import sys

import numpy
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plda_em_numpy as pen  # noqa: E402

from sidekit_amd import factor_analyser as fa  # noqa: E402
from sidekit_amd import iv_scoring  # noqa: E402
from sidekit_amd.bosaris import Key, Ndx, rocch, rocch2eer  # noqa: E402
from sidekit_amd.statserver import StatServer  # noqa: E402

pytestmark = pytest.mark.gpu


def _assert_model(got, want, tol, what):
    mu, F, Sigma = got
    mu_r, F_r, Sigma_r = want
    errs = {"mu": numpy.abs(mu - mu_r).max() / numpy.abs(mu_r).max(), "Sigma": pen.rel(Sigma, Sigma_r),
            "FF'": pen.rel(F.dot(F.T), F_r.dot(F_r.T)), "F": pen.rel(pen.sign_align(F, F_r), F_r)}
    print(what, {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < tol, f"{what}: {k} differs by {v:.3e} (relative max-norm, bound {tol})"


def _stat_server(ids, X):
    return StatServer.from_arrays(ids, numpy.array([f"seg{i:06d}" for i in range(X.shape[0])], dtype="|O"), X)


def test_config5_training_set_reproduces_the_reference_model_and_its_scores(gpu, golden_dir):
    """The training set config5.npz's (mu, F, Sigma) came from, through FactorAnalyser.plda; then the config-5 trial set scored with the
    TRAINED parameters against the fixture's scores (tolerances of test_config5_pinned_by_the_reference_at_full_size)."""
    sys.path.insert(0, golden_dir)
    import config5_inputs as c5
    fx = numpy.load(os.path.join(golden_dir, "config5.npz"))
    X, lab = c5.plda_training_set()
    numpy.testing.assert_array_equal(c5.digest(X), fx["X_digest"])
    plda = fa.FactorAnalyser()
    plda.plda(_stat_server(numpy.array([f"spk{l:04d}" for l in lab], dtype="|O"), X), rank_f=c5.PLDA_RANK, nb_iter=10, save_final=False)
    assert plda.G is None and plda.H is None and plda.F.shape == (c5.D, c5.PLDA_RANK)
    _assert_model((plda.mean, plda.F, plda.Sigma), (fx["mu"], fx["F"], fx["Sigma"]), 1e-9, "config5 on the GPU vs the reference")
    E, T, spk_e, spk_t = c5.trial_set()
    numpy.testing.assert_array_equal(c5.digest(E), fx["E_digest"])
    numpy.testing.assert_array_equal(c5.digest(T), fx["T_digest"])
    enr_ids, tst_ids = c5.ids("enr", c5.NE), c5.ids("tst", c5.NT)
    enroll, test = StatServer.from_arrays(enr_ids, enr_ids, E), StatServer.from_arrays(tst_ids, tst_ids, T)
    mm, ss = numpy.meshgrid(numpy.arange(c5.NE), numpy.arange(c5.NT), indexing="ij")
    models, segs = enr_ids[mm.ravel()], tst_ids[ss.ravel()]
    tar_mask = spk_e[:, None] == spk_t[None, :]
    ndx = Ndx(models=models, testsegs=segs)
    key = Key(models=models, testsegs=segs, trials=numpy.where(tar_mask.ravel(), "target", "nontarget").astype(object))
    sc = iv_scoring.fast_PLDA_scoring(enroll, test, ndx, plda.mean, plda.F, plda.Sigma)
    m = sc.scoremat
    scale = numpy.abs(fx["plda_sample"]).max()
    print("plda_sample", numpy.abs(m[::7, ::11] - fx["plda_sample"]).max() / scale)
    assert numpy.abs(m[::7, ::11] - fx["plda_sample"]).max() / scale < 1e-9
    numpy.testing.assert_allclose(m.sum(axis=1), fx["plda_row_sums"], rtol=1e-9, atol=1e-6)
    numpy.testing.assert_allclose(m.sum(axis=0), fx["plda_col_sums"], rtol=1e-9, atol=1e-6)
    tar, non = sc.get_tar_non(key)
    pmiss, pfa = rocch(tar.astype(float), non.astype(float))
    assert abs(rocch2eer(pmiss, pfa) - float(fx["plda_eer"])) < 1e-9


@pytest.mark.parametrize("k", [0, 1])
def test_ragged_fixture_trained_by_the_reference(gpu, golden_dir, k):
    """plda_train.npz: string model ids, shuffled rows, a class of one session, scaling_factor 1.0 and 0.7."""
    fx = numpy.load(os.path.join(golden_dir, "plda_train.npz"))
    ids = fx["modelset"].astype("|O")
    assert numpy.unique(ids, return_counts=True)[1].min() == 1
    plda = fa.FactorAnalyser()
    plda.plda(_stat_server(ids, fx["X"]), rank_f=int(fx["rank"]), nb_iter=int(fx["nb_iter"]), scaling_factor=float(fx["scalings"][k]), save_final=False)
    _assert_model((plda.mean, plda.F, plda.Sigma), (fx[f"mean_{k}"], fx[f"F_{k}"], fx[f"Sigma_{k}"]), 1e-9, f"ragged scaling={fx['scalings'][k]}")


def _synthetic(seed, D, counts, dtype):
    """class centres + within-class noise around a common offset, rows shuffled; integer labels that are not 0..C-1"""
    rs = numpy.random.RandomState(seed)
    lab = numpy.repeat(numpy.arange(len(counts)), counts)
    centres = rs.randn(len(counts), D)
    X = 0.3 + centres[lab] + 1.5 * rs.randn(lab.shape[0], D)
    p = rs.permutation(X.shape[0])
    p = p[:p.shape[0] - (p.shape[0] - 37) % 64]        # N = 37 mod 64: no multiple of any tile or slab
    return X[p].astype(dtype), 7 + 3 * lab[p]


_COUNTS = {"half": lambda: numpy.concatenate(([619], numpy.random.RandomState(3).randint(1, 30, 40))),       # one class holds half the rows
           "3000": lambda: numpy.random.RandomState(4).randint(1, 41, 3000)}                                  # 3 000 classes of 1-40 sessions


@pytest.mark.parametrize("layout,D,rank,dtype,nb_iter", [("half", 50, 10, numpy.float64, 5), ("half", 50, 50, numpy.float32, 5),
                                                         ("3000", 256, 10, numpy.float32, 3), ("3000", 256, 256, numpy.float64, 3)])
def test_shapes_against_the_restatement(gpu, layout, D, rank, dtype, nb_iter):
    X, lab = _synthetic(7, D, _COUNTS[layout](), dtype)
    assert X.shape[0] % 64 == 37 and X.dtype == dtype
    got = fa.plda_device(torch.as_tensor(X).to(gpu), lab, rank, nb_iter)
    want = pen.em(X.astype(numpy.float64), lab, rank, nb_iter)      # float32 input: the same values, widened
    _assert_model(got, want, 1e-9, f"{layout} D={D} rank={rank} {numpy.dtype(dtype).name} N={X.shape[0]}")


def test_plda_device_and_plda_on_a_stat_server_are_the_same_code(gpu):
    X, lab = _synthetic(8, 50, _COUNTS["half"](), numpy.float64)
    a = fa.plda_device(torch.as_tensor(X).to(gpu), torch.as_tensor(lab).to(gpu), 10, 4, 0.7)
    plda = fa.FactorAnalyser()
    plda.plda(_stat_server(numpy.array([f"{l:05d}" for l in lab], dtype="|O"), X), 10, 4, 0.7, save_final=False, num_thread=8)
    for x, y in zip(a, (plda.mean, plda.F, plda.Sigma)):
        numpy.testing.assert_array_equal(x, y)


def test_plda_saves_when_the_reference_does(gpu, tmp_path):
    X, ids = pen.ragged_set()
    plda = fa.FactorAnalyser()
    plda.plda(_stat_server(ids, X), 8, 3, output_file_name=str(tmp_path / "m"), save_partial=True)
    assert sorted(os.listdir(tmp_path)) == ["m.h5", "m_it-0.h5", "m_it-1.h5"]
    back = fa.FactorAnalyser.read(str(tmp_path / "m.h5"))
    numpy.testing.assert_array_equal(back.F, plda.F)
    numpy.testing.assert_array_equal(back.Sigma, plda.Sigma)
    assert back.G is None and back.H is None


@pytest.mark.parametrize("dtype", [numpy.float32, numpy.float64])
def test_class_sums_and_mean(gpu, dtype):
    X, lab = _synthetic(9, 256, _COUNTS["3000"](), dtype)
    S, colsum = fa.class_sums_device(torch.as_tensor(X).to(gpu), lab)
    ids, _, counts, want = pen.class_sums(X, lab)
    err_s = pen.rel(S.cpu().numpy(), want)
    err_m = pen.rel(colsum.cpu().numpy() / X.shape[0], X.astype(numpy.float64).mean(axis=0))
    print("class sums", err_s, "mean", err_m)
    assert err_s < 1e-13 and err_m < 1e-13
    out, sessions = _stat_server(numpy.array([f"{l:05d}" for l in lab], dtype="|O"), X.astype(numpy.float64)).sum_stat_per_model()
    assert pen.rel(out.stat1, want) < 1e-13
    numpy.testing.assert_array_equal(sessions, counts)
    numpy.testing.assert_array_equal(out.stat0[:, 0], counts)


@pytest.mark.parametrize("K,M,Nn", [(1, 37, 51), (100003, 37, 51), (5000, 256, 256), (777, 129, 64)])
@pytest.mark.parametrize("dtype", [numpy.float32, numpy.float64])
def test_tn_product(gpu, K, M, Nn, dtype):
    rs = numpy.random.RandomState(K % 1000)
    A = (0.5 + rs.randn(K, M)).astype(dtype)
    B = (A.astype(numpy.float64)[:, numpy.arange(Nn) % M] + 0.5 * rs.randn(K, Nn) - 0.25).astype(dtype)
    w, a, b = rs.uniform(0.5, 12.0, K), A.astype(numpy.float64).mean(axis=0), B.astype(numpy.float64).mean(axis=0)
    Ad, Bd, A64, B64 = torch.as_tensor(A).to(gpu), torch.as_tensor(B).to(gpu), A.astype(numpy.float64), B.astype(numpy.float64)
    for tag, (wv, av, bv) in {"plain": (None, None, None), "weights": (w, None, None), "centred": (None, a + 0.1, b - 0.1),
                              "weights + centred": (w, a + 0.1, b - 0.1)}.items():
        want = numpy.einsum("k,km,kn->mn", numpy.ones(K) if wv is None else wv, A64 - (0 if av is None else av), B64 - (0 if bv is None else bv))
        err = pen.rel(fa.gemm_tn_device(Ad, Bd, wv, av, bv).cpu().numpy(), want)
        print(f"TN K={K} M={M} Nn={Nn} {numpy.dtype(dtype).name} {tag}: {err:.2e}")
        assert err < 1e-12, (tag, err)
    c = a + 0.1                                                        # off the mean: at K = 1 the centred row would be all zeros
    G = fa.gemm_tn_device(Ad, None, None, c, c).cpu().numpy()          # the total scatter's form: B = A
    assert pen.rel(G, (A64 - c).T.dot(A64 - c)) < 1e-12
    numpy.testing.assert_array_equal(G, G.T)


def test_nn_product_epilogues(gpu):
    rs = numpy.random.RandomState(11)
    A, B, r, c = rs.randn(333, 77), rs.randn(77, 45), rs.uniform(1, 9, 333), rs.uniform(0.1, 5, 45)
    Ad = torch.as_tensor(A).to(gpu)
    from sidekit_amd import _lib
    assert pen.rel(fa.dgemm_nn_device(Ad, B).cpu().numpy(), A.dot(B)) < 1e-13
    assert pen.rel(fa.dgemm_nn_device(Ad, B, 0.7, r, c, _lib.SC_EPI_RANK1).cpu().numpy(), 0.7 * A.dot(B) - numpy.outer(r, c)) < 1e-13
    assert pen.rel(fa.dgemm_nn_device(Ad, B, 1.0, r, c, _lib.SC_EPI_POSTERIOR).cpu().numpy(), A.dot(B) / (1 + numpy.outer(r, c))) < 1e-13


def test_two_runs_and_a_side_stream_give_identical_bits(gpu):
    X, lab = _synthetic(10, 256, _COUNTS["3000"](), numpy.float32)
    xv = torch.as_tensor(X).to(gpu)
    first = fa.plda_device(xv, lab, 32, 3)
    second = fa.plda_device(xv, lab, 32, 3)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        third = fa.plda_device(xv, lab, 32, 3)
    side.synchronize()
    for x, y, z in zip(first, second, third):
        numpy.testing.assert_array_equal(x, y)
        numpy.testing.assert_array_equal(x, z)


def test_driver_trains_on_the_gathered_device_tensor(gpu, capsys):
    """shard_extract_score --plda-train em: its PLDA parameters are plda_device's on the gathered x-vectors; without the flag the
    driver's outputs are what they were: the moment estimate of the same x-vectors and the scores that follow from it."""
    from sidekit_amd.bin import shard_extract_score as drv
    args = ["--utterances", "2048", "--batch", "256", "--seconds", "1", "--trials", "400", "--speakers", "40", "--plda-rank", "32"]
    n = 400
    keep_em, keep_mo = {}, {}
    out_em = drv.main(args + ["--plda-train", "em"], keep=keep_em)
    out_mo = drv.main(args, keep=keep_mo)
    capsys.readouterr()
    assert torch.equal(keep_em["xv"], keep_mo["xv"]) and keep_em["xv"].is_cuda and keep_em["xv"].dtype == torch.float32
    assert out_em["plda"] == "EM on the device" and out_mo["plda"] == "moment estimate"
    want = fa.plda_device(keep_em["xv"][2 * n:], keep_em["labels"][2 * n:], 32)
    for x, y in zip(keep_em["plda"], want):
        assert numpy.isfinite(x).all()
        numpy.testing.assert_array_equal(x, y)
    assert 0.0 <= out_em["plda_eer"] < 0.3
    xv = keep_mo["xv"]
    mu, F, Sigma = drv.plda_moments(xv[2 * n:].cpu().numpy(), keep_mo["labels"][2 * n:], 32)
    for x, y in zip(keep_mo["plda"], (mu, F, Sigma)):
        numpy.testing.assert_array_equal(x, y)
    Phi, Psi, cst = iv_scoring.plda_parameters(mu, F, Sigma)
    mu_d = torch.as_tensor(mu, device=gpu)
    scores = iv_scoring.plda_matrix_device(xv[:n].double() - mu_d, xv[n:2 * n].double() - mu_d, Phi, Psi, cst, 1.0, gpu).cpu().numpy()
    numpy.testing.assert_array_equal(keep_mo["plda_scores"], scores)
    numpy.testing.assert_array_equal(keep_mo["cosine_scores"], keep_em["cosine_scores"])
