"""Writes tests/golden/score_norm.npz: seeded unit-norm x-vectors (enrolment 37 x 256, test 53 x 256, cohort 301 x 256) and what the
REFERENCE's ``sidekit.score_normalization.tnorm`` makes of their cosine scores (float64 products of the stored float32 rows):

  tnorm        tnorm(enrolment x test, cohort x test)                                  (37 x 53)
  znorm        tnorm(test x enrolment, cohort x enrolment) transposed                   (37 x 53)

The second is the z-norm pin: z-norm by definition -- per-model statistics of the model's impostor scores, applied along the model's row --
is the reference's own ``tnorm`` of the transposed problem.  (The reference's ``znorm`` itself broadcasts the per-model vectors along the
segment axis, score_normalization.py:70: on this 37 x 53 matrix it raises, which the script checks.)  The adaptive case reuses asnorm.npz.

The reference's modules are imported with the stand-in recipe of make_golden.py (no reference text is copied).  Every cohort std that
enters a stored result is asserted to be above 1e-3, so that the 1 / std amplification of the comparison stays bounded.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_score_norm_golden.py
"""
import importlib
import os
import sys

import numpy
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

SEED, NE, NT, NC, D = 47, 37, 53, 301, 256


def vectors():
    g = torch.Generator().manual_seed(SEED)
    common = torch.randn(D, generator=g)                      # a shared direction: cohort means away from zero
    mk = lambda n: torch.nn.functional.normalize(torch.randn(n, D, generator=g) + 1.5 * common, dim=1).numpy()
    return mk(NE), mk(NT), mk(NC)


def ids(prefix, n):
    return numpy.array([f"{prefix}{i:04d}" for i in range(n)], dtype="|O")


def main():
    mods = make_golden.import_reference()
    Scores = mods["sidekit.bosaris"].Scores
    sn = importlib.import_module("sidekit.score_normalization")
    enrol, test, cohort = vectors()
    e64, t64, c64 = enrol.astype(numpy.float64), test.astype(numpy.float64), cohort.astype(numpy.float64)

    def scores(models, segs, mat):
        s = Scores()
        s.modelset, s.segset, s.scoremat, s.scoremask = models, segs, mat.copy(), numpy.ones(mat.shape, dtype="bool")
        assert s.validate()
        return s

    em, ts, cm = ids("enr", NE), ids("tst", NT), ids("imp", NC)
    enrol_test, imp_test, enrol_imp = e64 @ t64.T, c64 @ t64.T, e64 @ c64.T
    assert imp_test.std(0).min() > 1e-3 and enrol_imp.std(1).min() > 1e-3, "a cohort std below 1e-3: the comparison would be ill-conditioned"
    tn = sn.tnorm(scores(em, ts, enrol_test), scores(cm, ts, imp_test))
    zn = sn.tnorm(scores(ts, em, enrol_test.T), scores(cm, em, enrol_imp.T))
    assert list(tn.modelset) == list(em) and list(tn.segset) == list(ts) and list(zn.modelset) == list(ts) and list(zn.segset) == list(em)
    try:
        sn.znorm(scores(em, ts, enrol_test), scores(em, cm, enrol_imp))
        raise AssertionError("the reference's znorm was expected to fail to broadcast on a non-square matrix")
    except ValueError:
        pass
    fx = {"seed": SEED, "enrol": enrol, "test": test, "cohort": cohort, "tnorm": tn.scoremat, "znorm": zn.scoremat.T.copy(),
          "min_cohort_std": min(imp_test.std(0).min(), enrol_imp.std(1).min())}
    path = os.path.join(HERE, "score_norm.npz")
    numpy.savez_compressed(path, **fx)
    print("score_norm.npz", os.path.getsize(path), "bytes", {k: getattr(v, "shape", v) for k, v in fx.items()})


if __name__ == "__main__":
    main()
