"""Writes tests/golden/plda_train.npz: a ragged PLDA training set and what the REFERENCE's ``FactorAnalyser.plda`` trains on it.

The reference's ``sidekit.factor_analyser`` / ``sidekit.statserver`` are imported with the stand-in recipe of make_golden.py (no
reference text is copied).  The set (tests/tools/plda_em_numpy.ragged_set): 60 classes of 1-12 sessions, D = 48, rows shuffled,
string model ids; trained with rank 16, 5 iterations, ``scaling_factor`` 1.0 and 0.7.  Stored: the inputs and both
``(mean, F, Sigma)``.  Before writing, the tests' numpy restatement is asserted against the reference at 1e-12 (both E-step forms).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_plda_train_golden.py
"""
import contextlib
import importlib
import io
import os
import sys

import numpy

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

import make_golden  # noqa: E402
import plda_em_numpy as pen  # noqa: E402

RANK, NB_ITER, SCALINGS = 16, 5, (1.0, 0.7)


def main():
    mods = make_golden.import_reference()
    sts_mod = mods["sidekit.statserver"]
    fa_mod = importlib.import_module("sidekit.factor_analyser")
    X, ids = pen.ragged_set()
    counts = numpy.unique(ids, return_counts=True)[1]
    assert counts.min() == 1 and counts.max() == 12 and counts.shape[0] == 60
    fx = {"X": X, "modelset": ids.astype("U"), "rank": RANK, "nb_iter": NB_ITER, "scalings": numpy.array(SCALINGS)}
    for k, sf in enumerate(SCALINGS):
        s = sts_mod.StatServer()
        s.modelset = ids.copy()
        s.segset = numpy.array([f"seg{i:04d}" for i in range(X.shape[0])], dtype="|O")
        s.start, s.stop = numpy.empty(X.shape[0], dtype="|O"), numpy.empty(X.shape[0], dtype="|O")
        s.stat0, s.stat1 = numpy.ones((X.shape[0], 1)), X.copy()
        plda = fa_mod.FactorAnalyser()
        with contextlib.redirect_stdout(io.StringIO()):
            plda.plda(s, rank_f=RANK, nb_iter=NB_ITER, scaling_factor=sf, save_final=False)
        for form in (False, True):
            mu, F, Sigma = pen.em(X, ids, RANK, NB_ITER, sf, eigen_form=form)
            errs = (numpy.abs(mu - plda.mean).max(), pen.rel(Sigma, plda.Sigma), pen.rel(F.dot(F.T), plda.F.dot(plda.F.T)),
                    pen.rel(pen.sign_align(F, plda.F), plda.F))
            print(f"scaling {sf} eigen_form {form}: mu {errs[0]:.1e} Sigma {errs[1]:.1e} FF' {errs[2]:.1e} F {errs[3]:.1e}")
            assert max(errs) < 1e-12, errs
        fx.update({f"mean_{k}": plda.mean, f"F_{k}": plda.F, f"Sigma_{k}": plda.Sigma})
    numpy.savez_compressed(os.path.join(HERE, "plda_train.npz"), **fx)
    print("plda_train.npz", {k: getattr(v, "shape", v) for k, v in fx.items()})


if __name__ == "__main__":
    main()
