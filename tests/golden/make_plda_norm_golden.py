"""Writes tests/golden/plda_norm.npz: seeded x-vectors (enrolment 37 x 48, test 53 x 48, cohort 301 x 48), a seeded two-covariance PLDA
model ``(mu, F, Sigma)`` and what the REFERENCE's ``sidekit.score_normalization.tnorm`` makes of the REFERENCE's own
``sidekit.iv_scoring.fast_PLDA_scoring`` scores of them:

  tnorm        tnorm(enrolment x test, cohort x test)                                  (37 x 53)
  znorm        tnorm((enrolment x test)', (enrolment x cohort)') transposed             (37 x 53)

The second is the z-norm pin, as in make_score_norm_golden.py: per-model statistics of the model's impostor scores ``s(e_i, c_j)``, applied
along the model's row, is the reference's own ``tnorm`` of the transposed problem.  The raw enrolment x test scores are stored as well.

The reference's modules are imported with the stand-in recipe of make_golden.py (no reference text is copied).  Every cohort std that
enters a stored result is asserted to be above 1e-3, so that the 1 / std amplification of the comparison stays bounded.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_plda_norm_golden.py
"""
import importlib
import os
import sys

import numpy

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

SEED, NE, NT, NC, D, RANK, NSPK = 53, 37, 53, 301, 48, 10, 9


def ids(prefix, n):
    return numpy.array([f"{prefix}{i:04d}" for i in range(n)], dtype="|O")


def main():
    mods = make_golden.import_reference()
    ivs, sts_mod, bos = mods["sidekit.iv_scoring"], mods["sidekit.statserver"], mods["sidekit.bosaris"]
    sn = importlib.import_module("sidekit.score_normalization")
    rs = numpy.random.RandomState(SEED)
    mu = 0.3 * rs.randn(D)
    F = rs.randn(D, RANK) / numpy.sqrt(D)
    A = rs.randn(D, D) / numpy.sqrt(D)
    Sigma = 0.4 * (A @ A.T) + 0.3 * numpy.eye(D)
    spk = rs.randn(NSPK, RANK) @ F.T
    mk = lambda n: mu + spk[rs.randint(0, NSPK, n)] + rs.multivariate_normal(numpy.zeros(D), Sigma, n)
    enrol, test, cohort = mk(NE), mk(NT), mk(NC)

    def sts(names, X):
        s = sts_mod.StatServer()
        s.modelset, s.segset = names.copy(), names.copy()
        s.start, s.stop = numpy.empty(len(names), dtype="|O"), numpy.empty(len(names), dtype="|O")
        s.stat0, s.stat1 = numpy.ones((len(names), 1)), numpy.array(X, dtype=numpy.float64)
        return s

    def plda(models, X, segs, Y):
        """The reference's scores of every (model, segment) pair, in the order of `models` x `segs`."""
        mm, ss = numpy.meshgrid(numpy.arange(len(models)), numpy.arange(len(segs)), indexing="ij")
        ndx = bos.Ndx(models=models[mm.ravel()], testsegs=segs[ss.ravel()])
        sc = ivs.fast_PLDA_scoring(sts(models, X), sts(segs, Y), ndx, mu, F, Sigma)
        assert sc.scoremask.all()
        rows = [list(sc.modelset).index(m) for m in models]
        cols = [list(sc.segset).index(s) for s in segs]
        return sc.scoremat[numpy.ix_(rows, cols)]

    def scores(models, segs, mat):
        s = bos.Scores()
        s.modelset, s.segset, s.scoremat, s.scoremask = models, segs, mat.copy(), numpy.ones(mat.shape, dtype="bool")
        assert s.validate()
        return s

    em, ts, cm = ids("enr", NE), ids("tst", NT), ids("imp", NC)
    enrol_test, imp_test, enrol_imp = plda(em, enrol, ts, test), plda(cm, cohort, ts, test), plda(em, enrol, cm, cohort)
    assert imp_test.std(0).min() > 1e-3 and enrol_imp.std(1).min() > 1e-3, "a cohort std below 1e-3: the comparison would be ill-conditioned"
    tn = sn.tnorm(scores(em, ts, enrol_test), scores(cm, ts, imp_test))
    zn = sn.tnorm(scores(ts, em, enrol_test.T), scores(cm, em, enrol_imp.T))
    assert list(tn.modelset) == list(em) and list(tn.segset) == list(ts) and list(zn.modelset) == list(ts) and list(zn.segset) == list(em)
    fx = {"seed": SEED, "enrol": enrol, "test": test, "cohort": cohort, "mu": mu, "F": F, "Sigma": Sigma, "scores": enrol_test,
          "tnorm": tn.scoremat, "znorm": zn.scoremat.T.copy(), "min_cohort_std": min(imp_test.std(0).min(), enrol_imp.std(1).min())}
    path = os.path.join(HERE, "plda_norm.npz")
    numpy.savez_compressed(path, **fx)
    print("plda_norm.npz", os.path.getsize(path), "bytes", {k: getattr(v, "shape", v) for k, v in fx.items()})


if __name__ == "__main__":
    main()
