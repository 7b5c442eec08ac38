"""Writes tests/golden/backend.npz: the ragged set of plda_train.npz shifted off-centre and what the REFERENCE's ``StatServer`` computes
on it -- within / between / total covariance, the LDA matrix (rank 10), the WCCN factor, the Mahalanobis matrix, three iterations of
spectral normalisation in both modes (means, covariances, every eighth transformed row), ``whiten_cholesky_stat1`` with a full and with a
diagonal covariance, ``spectral_norm_stat1`` with a diagonal covariance and with ``is_sqr_inv_sigma=True`` -- and the reference's ``cosine_scoring(wccn=)``,
``mahalanobis_scoring`` and ``two_covariance_scoring`` of a small enrol / test split of the set, scored with the matrices just produced.

The reference's modules are imported with the stand-in recipe of make_golden.py (no reference text is copied).  Before writing, the
tests' numpy restatement (tests/tools/backend_numpy.py) is asserted against the reference: 1e-12 for everything that does not depend
on eigenvector signs; iterations 2 and 3 of spectral normalisation by what sign flips leave invariant (eigenvalues, |mean|, Gram matrix).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_backend_golden.py
"""
import contextlib
import copy
import io
import os
import sys

import numpy
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

import make_golden  # noqa: E402
import backend_numpy as bn  # noqa: E402
import plda_em_numpy as pen  # noqa: E402

RANK, IT, SHIFT, N_ENROL, N_TEST, ROW_STEP = 10, 3, 0.2, 24, 30, 8     # transformed rows: every ROW_STEP-th is stored


def main():
    mods = make_golden.import_reference()
    sts_mod, ivs, bos = mods["sidekit.statserver"], mods["sidekit.iv_scoring"], mods["sidekit.bosaris"]
    X, ids = pen.ragged_set()
    X = X + SHIFT
    segs = numpy.array([f"seg{i:04d}" for i in range(X.shape[0])], dtype="|O")

    def make_sts(models, segments, rows):
        s = sts_mod.StatServer()
        s.modelset, s.segset = numpy.array(models, dtype="|O"), numpy.array(segments, dtype="|O")
        s.start, s.stop = numpy.empty(len(segments), dtype="|O"), numpy.empty(len(segments), dtype="|O")
        s.stat0, s.stat1 = numpy.ones((len(segments), 1)), numpy.array(rows, dtype=numpy.float64)
        return s

    full = {}      # the reference's transformed rows, whole, for the assertions below
    fx = {"X": X, "modelset": ids.astype("U"), "rank": RANK, "it": IT, "row_step": ROW_STEP}
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        s = make_sts(ids, segs, X)
        fx.update(mean=s.get_mean_stat1(), within=s.get_within_covariance_stat1(), between=s.get_between_covariance_stat1(),
                  total=s.get_total_covariance_stat1(), L=s.get_lda_matrix_stat1(RANK), wccn=s.get_wccn_choleski_stat1(),
                  mahalanobis=s.get_mahalanobis_matrix_stat1())
        for mode in ("efr", "sphNorm"):
            means, covs = s.estimate_spectral_norm_stat1(IT, mode)
            t = copy.deepcopy(s)
            t.spectral_norm_stat1(means, covs)
            full[mode] = t.stat1
            fx.update({f"{mode}_means": numpy.array(means), f"{mode}_covs": numpy.array(covs), f"{mode}_stat1": t.stat1[::ROW_STEP]})
        numpy.testing.assert_array_equal(s.stat1, X)
        # the branches no estimate reaches: Cholesky whitening (full and diagonal covariance), a diagonal covariance in whiten_stat1,
        # and lists that already hold the matrices to multiply by (any two matrices serve: the WCCN factor and the Mahalanobis matrix)
        diag = numpy.diag(fx["total"]).copy()
        for key, call in (("chol_stat1", lambda t: t.whiten_cholesky_stat1(fx["mean"], fx["total"])),
                          ("chol_diag_stat1", lambda t: t.whiten_cholesky_stat1(fx["mean"], diag)),
                          ("diag_stat1", lambda t: t.spectral_norm_stat1([fx["mean"]], [diag])),
                          ("sqrinv_stat1", lambda t: t.spectral_norm_stat1([fx["mean"], 0.1 * fx["mean"]], [fx["wccn"], fx["mahalanobis"]], True))):
            t = copy.deepcopy(s)
            call(t)
            full[key] = t.stat1
            fx[key] = t.stat1[::ROW_STEP]
    # restatement against the reference
    mu, within, between, total = bn.covariances(X, ids)
    errs = {"mean": pen.rel(mu, fx["mean"]), "within": pen.rel(within, fx["within"]), "between": pen.rel(between, fx["between"]),
            "total": pen.rel(total, fx["total"]), "wccn": pen.rel(bn.wccn(X, ids), fx["wccn"]),
            "mahalanobis": pen.rel(bn.mahalanobis(X, ids), fx["mahalanobis"])}
    L = bn.lda(X, ids, RANK)
    errs["LL'"] = pen.rel(L.dot(L.T), fx["L"].dot(fx["L"].T))
    errs["L"] = pen.rel(pen.sign_align(L, fx["L"]), fx["L"])
    gap = bn.top_gap(bn.lda_spectrum(X, ids)[0], RANK)
    print(f"LDA: smallest gap among the top {RANK + 1} eigenvalues / largest = {gap:.3e}")
    assert gap > 1e-4
    for mode in ("efr", "sphNorm"):
        means, covs, Y = bn.spectral_norm_estimate(X, ids, IT, mode)
        errs[f"{mode} means[0]"] = pen.rel(means[0], fx[f"{mode}_means"][0])
        errs[f"{mode} covs[0]"] = pen.rel(covs[0], fx[f"{mode}_covs"][0])
        errs[f"{mode} apply"] = pen.rel(bn.spectral_norm_apply(X, fx[f"{mode}_means"], fx[f"{mode}_covs"]), full[mode])
        for i in range(1, IT):
            errs[f"{mode} eig(covs[{i}])"] = pen.rel(bn.sorted_eigenvalues(covs[i]), bn.sorted_eigenvalues(fx[f"{mode}_covs"][i]))
            errs[f"{mode} |means[{i}]|"] = abs(numpy.linalg.norm(means[i]) / numpy.linalg.norm(fx[f"{mode}_means"][i]) - 1)
        errs[f"{mode} Gram"] = pen.rel(Y.dot(Y.T), full[mode].dot(full[mode].T))
    diag = numpy.diag(fx["total"]).copy()
    errs["whiten_cholesky"] = pen.rel(bn.whiten_rows(X, fx["mean"], bn.cholesky_transform(fx["total"]), False), full["chol_stat1"])
    errs["whiten_cholesky diagonal"] = pen.rel(bn.whiten_rows(X, fx["mean"], bn.cholesky_transform(diag), False), full["chol_diag_stat1"])
    errs["diagonal covariance"] = pen.rel(bn.spectral_norm_apply(X, [fx["mean"]], [diag]), full["diag_stat1"])
    errs["is_sqr_inv_sigma"] = pen.rel(bn.spectral_norm_apply(X, [fx["mean"], 0.1 * fx["mean"]], [fx["wccn"], fx["mahalanobis"]], True), full["sqrinv_stat1"])
    for k, v in errs.items():
        print(f"restatement vs reference  {k}: {v:.1e}")
    assert max(errs.values()) < 1e-12, errs
    # producer -> consumer: a small enrol / test split scored by the reference with the matrices it has just produced
    E, T = X[:N_ENROL], X[N_ENROL:N_ENROL + N_TEST]
    enr_ids, tst_ids = segs[:N_ENROL], segs[N_ENROL:N_ENROL + N_TEST]
    mm, ss = numpy.meshgrid(numpy.arange(N_ENROL), numpy.arange(N_TEST), indexing="ij")
    ndx = bos.Ndx(models=enr_ids[mm.ravel()], testsegs=tst_ids[ss.ravel()])
    cos = ivs.cosine_scoring(make_sts(enr_ids, enr_ids, E), make_sts(tst_ids, tst_ids, T), ndx, wccn=fx["wccn"], check_missing=True,
                             device=torch.device("cpu"))
    mah = ivs.mahalanobis_scoring(make_sts(enr_ids, enr_ids, E), make_sts(tst_ids, tst_ids, T), ndx, fx["mahalanobis"])
    two = ivs.two_covariance_scoring(make_sts(enr_ids, enr_ids, E), make_sts(tst_ids, tst_ids, T), ndx, fx["within"], fx["between"])
    assert list(cos.modelset) == list(enr_ids) and list(cos.segset) == list(tst_ids)
    assert list(mah.modelset) == list(enr_ids) and list(two.segset) == list(tst_ids)
    fx.update(n_enrol=N_ENROL, n_test=N_TEST, cos_wccn_scoremat=numpy.asarray(cos.scoremat), maha_scoremat=mah.scoremat,
              twocov_scoremat=two.scoremat)
    path = os.path.join(HERE, "backend.npz")
    numpy.savez_compressed(path, **fx)
    print("backend.npz", os.path.getsize(path), "bytes", {k: getattr(v, "shape", v) for k, v in fx.items()})


if __name__ == "__main__":
    main()
