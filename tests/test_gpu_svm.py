"""The SVM back end on the GPU (sidekit_amd/svm_training.py, svm_scoring.py, the SVM methods of StatServer, csrc/svm.hip) against libsvm
and the reference's own modules (tests/golden/svm.npz, make_svm_golden.py).

A model's bar on ``W`` and ``b`` at ``eps = 1e-12`` is ``max(10 d, 1e-12)`` with the ``d`` the generator measured between the numpy
restatement and libsvm on that model (tests/tools/svm_fixture.py).  At libsvm's default ``eps = 1e-3`` two correct solvers differ by
1e-3 in ``w`` (the result depends on the path), so there the returned coefficients are checked for what they must satisfy instead.

Measured on one MI355X (printed by the tests; DESIGN.md section 4 "SVM back end"): the kernel makes the restatement's number of
iterations on every problem and ``w`` lands at ``d`` itself, a tenth of the bar (5.7e-13 to 3.7e-12; 2.4e-17 and 9.4e-17 on ``n2`` and
``nofree``), ``b`` within 1.4e-13; the scores through files within 9.2e-13 against bars of 1.4e-12 to 1.3e-11.
"""
import logging
import os
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import svm_fixture as sfx  # noqa: E402
import svm_numpy as svn  # noqa: E402

from sidekit_amd import _lib, sv_utils, svm_scoring, svm_training  # noqa: E402
from sidekit_amd.bosaris import Ndx  # noqa: E402
from sidekit_amd.statserver import StatServer  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden_dir):
    return sfx.load(golden_dir)


def _server(models, segs, stat1):
    s = StatServer()
    s.modelset, s.segset = numpy.array(models, dtype="|O"), numpy.array(segs, dtype="|O")
    s.start, s.stop = numpy.empty(len(segs), dtype="|O"), numpy.empty(len(segs), dtype="|O")
    s.stat0, s.stat1 = numpy.ones((len(segs), 1)), numpy.array(stat1, dtype=numpy.float64)
    assert s.validate()
    return s


@pytest.mark.parametrize("tag", sfx.SETS)
def test_tight_tolerance_matches_libsvm(gpu, fx, tag):
    p = sfx.problem(fx, tag)
    c = p["c"] if tag == "nofree" else None    # everywhere else the default cost is the reference's, and the fixture's
    W, b, info = svm_training.svm_train_device(p["bg"], p["en"], p["model_of"], c=c, eps=1e-12)
    assert numpy.all(info["status"] == _lib.SC_SVM_CONVERGED) and numpy.all(info["gap"] < 1e-12)
    assert numpy.array_equal(info["n"], p["bg"].shape[0] + numpy.bincount(p["model_of"]))
    assert numpy.abs(info["c"] - p["c"]).max() <= info["n"].max() * 2.0 ** -52 * p["c"].max(), "the cost: a sum of n terms in another order"
    print(tag, "iterations", info["iterations"].tolist(), "the restatement's", fx[f"{tag}_iterations"].tolist())
    sfx.assert_within_bars(tag, p, W, b)


@pytest.mark.parametrize("tag", ("eq3", "batch7", "n257", "dup", "twin", "nofree"))
def test_default_tolerance_solves_the_dual(gpu, fx, tag):
    p = sfx.problem(fx, tag)
    B = p["bg"].shape[0]
    W, b, info = svm_training.svm_train_device(p["bg"], p["en"], p["model_of"], c=p["c"])
    assert numpy.all(info["status"] == _lib.SC_SVM_CONVERGED) and numpy.all(info["gap"] < 1e-3)
    for m in range(len(p["names"])):
        own = p["en"][p["model_of"] == m]
        n = B + own.shape[0]
        assert numpy.all(info["coef"][m, n:] == 0)
        sfx.assert_solves(svn.gram(p["bg"], own), B, info["coef"][m, :n], b[m], p["c"][m], 1e-3, int(info["iterations"][m]))
        w, _ = svn.weights(p["bg"], own, info["coef"][m, :n], b[m])
        assert numpy.abs(W[m] - w).max() <= 1e-12 * numpy.abs(w).max(), "W is -X' coef of the returned coefficients"


def test_a_problem_beyond_64_kib_of_lds(gpu):
    """2700 points need 65824 bytes of LDS, past what a kernel may use without asking: checked for what a solution must satisfy"""
    rng = numpy.random.default_rng(7)
    bg, own = rng.standard_normal((2698, 32)), rng.standard_normal((2, 32)) + 0.5
    W, b, info = svm_training.svm_train_device(bg, own, numpy.zeros(2, dtype=int))
    assert info["status"][0] == _lib.SC_SVM_CONVERGED
    print("iterations", info["iterations"][0], "gap", info["gap"][0])
    sfx.assert_solves(svn.gram(bg, own), 2698, info["coef"][0], b[0], info["c"][0], 1e-3, int(info["iterations"][0]))


def test_max_iter_is_a_status_and_a_warning(gpu, fx, caplog):
    p = sfx.problem(fx, "n257")
    with caplog.at_level(logging.WARNING):
        W, b, info = svm_training.svm_train_device(p["bg"], p["en"], p["model_of"], max_iter=3)
    assert info["status"].tolist() == [_lib.SC_SVM_MAX_ITER] and info["iterations"].tolist() == [3] and info["gap"][0] >= 1e-3
    assert any("max number of iterations" in r.getMessage() for r in caplog.records)
    _, _, want = svn.train(p["bg"], p["en"], p["c"][0], max_iter=3)
    assert numpy.abs(info["coef"][0] - want["coef"]).max() <= 1e-12 * numpy.abs(want["coef"]).max() and numpy.isfinite(W).all()


def _gram_blocks(torch, gpu, p):
    """the Gram blocks of a problem set, model by model: k_bb, [k_eb rows of model m], [k_ee block of model m]"""
    bg = torch.as_tensor(p["bg"]).to(gpu)
    k_bb = torch.matmul(bg, bg.t())
    k_eb, k_ee = [], []
    for m in range(len(p["names"])):
        e = torch.as_tensor(p["en"][p["model_of"] == m]).to(gpu)
        k_eb.append(torch.matmul(e, bg.t()))
        k_ee.append(torch.matmul(e, e.t()).reshape(-1))
    return k_bb, k_eb, k_ee


def _solve(torch, gpu, k_bb, k_eb, k_ee, c, models, eps=1e-3):
    """``svm_solve_device`` on the models ``models`` in that order -> per model (coef of its n points, rho, iterations, gap, status)"""
    rows = numpy.array([k_eb[m].shape[0] for m in models])
    en_off = numpy.concatenate(([0], numpy.cumsum(rows)))
    ee_off = numpy.concatenate(([0], numpy.cumsum(rows * rows)))[:-1]
    out = svm_training.svm_solve_device(k_bb, torch.cat([k_eb[m] for m in models]).contiguous(), torch.cat([k_ee[m] for m in models]).contiguous(),
                                        en_off, ee_off, torch.as_tensor(c[list(models)]).to(gpu), eps)
    coef, rho, iters, gap, status = (t.cpu().numpy() for t in out)
    B = k_bb.shape[0]
    return {m: (coef[i, :B + rows[i]].copy(), rho[i], iters[i], gap[i], status[i]) for i, m in enumerate(models)}


def _same_bits(a, b):
    return all(numpy.array_equal(numpy.asarray(x), numpy.asarray(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("eps", (1e-3, 1e-12))
def test_results_are_the_same_bits(gpu, fx, eps):
    import torch
    p = sfx.problem(fx, "batch7")
    k_bb, k_eb, k_ee = _gram_blocks(torch, gpu, p)
    batch = _solve(torch, gpu, k_bb, k_eb, k_ee, p["c"], range(7), eps)
    again = _solve(torch, gpu, k_bb, k_eb, k_ee, p["c"], range(7), eps)
    backwards = _solve(torch, gpu, k_bb, k_eb, k_ee, p["c"], range(6, -1, -1), eps)
    for m in range(7):
        assert _same_bits(batch[m], again[m]), f"model {m}: one run against another"
        assert _same_bits(batch[m], backwards[m]), f"model {m}: the batch in reversed model order"
        assert _same_bits(batch[m], _solve(torch, gpu, k_bb, k_eb, k_ee, p["c"], [m], eps)[m]), f"model {m}: alone against inside the batch"
    first = svm_training.svm_train_device(p["bg"], p["en"], p["model_of"], eps=eps)
    second = svm_training.svm_train_device(p["bg"], p["en"], p["model_of"], eps=eps)
    assert numpy.array_equal(first[0], second[0]) and numpy.array_equal(first[1], second[1]), "W and b, one run against another"
    assert all(numpy.array_equal(first[2][k], second[2][k]) for k in first[2])


@pytest.mark.parametrize("tag", ("eq3", "batch7"))
def test_training_then_scoring_through_files(gpu, fx, tag, tmp_path, monkeypatch):
    """``svm_training`` into a directory, ``svm_scoring`` from it, against the reference's ``Scores`` of libsvm's models; trained at
    the fixture's tolerance (``svm_training`` takes none: it trains at the module's ``EPS``, libsvm's default)"""
    monkeypatch.setattr(svm_training, "EPS", 1e-12)
    p = sfx.problem(fx, tag)
    background = _server([f"bg{i}" for i in range(len(p["bg"]))], [f"bgseg{i}" for i in range(len(p["bg"]))], p["bg"])
    enroll = _server([p["names"][m] for m in p["model_of"]], [f"{tag}_s{i}" for i in range(len(p["en"]))], p["en"])
    svm_dir = str(tmp_path / "svm")
    svm_training.svm_training(svm_dir, background, enroll, num_thread=3)
    structure = os.path.join(svm_dir, "{}.svm")
    assert sorted(os.listdir(svm_dir)) == sorted(n + ".svm" for n in p["names"])
    W = numpy.stack([sv_utils.read_svm(structure.format(n))[0] for n in p["names"]])
    b = numpy.array([sv_utils.read_svm(structure.format(n))[1] for n in p["names"]])
    sfx.assert_within_bars(tag, p, W, b)
    test = fx[f"{tag}_test"] / sfx.SCALE
    test_sv = _server(list(fx[f"{tag}_test_segset"]), list(fx[f"{tag}_test_segset"]), test)
    ndx = Ndx()
    ndx.modelset, ndx.segset = fx[f"{tag}_ndx_modelset"].astype("|O"), fx[f"{tag}_ndx_segset"].astype("|O")
    ndx.trialmask = fx[f"{tag}_ndx_trialmask"].copy()
    scores = svm_scoring.svm_scoring(structure, test_sv, ndx, num_thread=2)
    assert list(scores.modelset) == list(fx[f"{tag}_score_modelset"]) and list(scores.segset) == list(fx[f"{tag}_score_segset"])
    assert numpy.array_equal(scores.scoremask, fx[f"{tag}_scoremask"]) and numpy.all(scores.scoremat[~scores.scoremask] == 0)
    for i, name in enumerate(scores.modelset):
        m = p["names"].index(name)
        bar = max(p["bar_w"][m], p["bar_b"][m]) * numpy.abs(test @ p["W"][m]).max()
        err = numpy.abs(scores.scoremat[i] - fx[f"{tag}_scoremat"][i]).max()
        print(f"{name}: scores differ by {err:.2e} (bar {bar:.1e})")
        assert err <= bar


def test_score_device_and_the_statserver_methods(gpu, fx):
    import torch
    p = sfx.problem(fx, "eq3")
    test = fx["eq3_test"] / sfx.SCALE
    want = svn.scores(p["W"], p["b"], test)
    got = svm_scoring.svm_score_device(p["W"], p["b"], test)
    assert isinstance(got, numpy.ndarray) and numpy.abs(got - want).max() <= 1e-12 * numpy.abs(want).max()
    resident = svm_scoring.svm_score_device(torch.as_tensor(p["W"]).to(gpu), torch.as_tensor(p["b"]).to(gpu), torch.as_tensor(test).to(gpu))
    assert resident.is_cuda and numpy.array_equal(resident.cpu().numpy(), got)
    s = _server(["x"] * 20, [f"nap{i}" for i in range(20)], fx["nap_q"] / sfx.SCALE)
    K = s.precompute_svm_kernel_stat1()
    assert numpy.abs(K - s.stat1 @ s.stat1.T).max() <= 1e-12 * numpy.abs(K).max()
    N = s.get_nap_matrix_stat1(3)
    sign = numpy.sign((N * fx["nap_N"]).sum(axis=0))
    assert N.shape == (12, 3) and numpy.abs(N * sign - fx["nap_N"]).max() <= 1e-10 * numpy.abs(fx["nap_N"]).max()
    assert numpy.abs(N @ N.T - fx["nap_N"] @ fx["nap_N"].T).max() <= 1e-10 * numpy.abs(fx["nap_N"] @ fx["nap_N"].T).max()


def test_a_problem_beyond_the_cap_is_refused_before_any_launch(gpu):
    import torch
    bg = torch.zeros((svm_training.MAX_N, 2), dtype=torch.float64, device=gpu)
    with pytest.raises(ValueError, match="never split"):
        svm_training.svm_train_device(bg, torch.ones((1, 2), dtype=torch.float64, device=gpu), numpy.zeros(1, dtype=int))
    with pytest.raises(ValueError, match="never split"):   # the entry point's own check, with nothing enqueued
        _lib.launch("sc_svm_train", gpu, bg, svm_training.MAX_N, bg, 1, bg, 1, bg, bg, 1, 1, bg, 1e-3, 10, bg, bg, bg, bg, bg)
    ok = svm_training.svm_train_device(torch.ones((3, 2), dtype=torch.float64, device=gpu), -torch.ones((1, 2), dtype=torch.float64, device=gpu),
                                       numpy.zeros(1, dtype=int))
    assert ok[0].is_cuda and ok[2]["status"].cpu().tolist() == [_lib.SC_SVM_CONVERGED], "tensors in, tensors out"
