"""Writes tests/golden/gaussian_backend.npz: a small off-centre closed set and what the REFERENCE's ``sidekit.lid_utils`` computes on it --
``gaussian_backend_train`` and ``gaussian_backend_train_hetero`` (alpha = 0.1) parameters, the log-likelihood matrices of
``gaussian_backend_test`` / ``gaussian_backend_test_hetero`` (``compute_llr=False``), their closed-set LLRs, and
``compute_log_likelihood_ratio`` with ``p_tar = 0.1`` on a hand-made 5 x 4 matrix (one class leading by 800 nats, an exact tie of the two
largest, all equal, values near -1e4).

The set, from ``RandomState(3)`` in draw order: 7 classes of [3, 40, 17, 130, 5, 64, 29] rows, D = 45; ``centres = 0.6 randn(C, D)``; per
class ``A_c = I + 0.3 randn(D, D)``; per class its training rows ``centres[c] + 0.5 A_c randn(D) + 0.2`` (one ``randn(n_c, D)`` draw); one
permutation that shuffles the rows; the classes of 301 test rows, ``randint(0, C, 301)``; then the test rows, one ``randn(D)`` at a time.
D = 45 leaves an odd k tail and a partial column tile, 301 rows a ragged row tile, the class of 3 is shorter than a k-tile and the class
of 130 longer than a 128 tile.

The reference's module is imported with the stand-in recipe of make_golden.py plus empty stand-ins for the three GMM-era modules
``lid_utils`` imports and never uses on the ``diag=False`` path (no reference text is copied).  Before writing, the tests' numpy
restatement (tests/tools/gaussian_backend_numpy.py) is asserted against the reference at 1e-12.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_gaussian_backend_golden.py
"""
import contextlib
import importlib
import io
import os
import sys
import types

import numpy

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

import make_golden  # noqa: E402
import gaussian_backend_numpy as gbn  # noqa: E402

COUNTS, DIM, N_TEST, ALPHA, P_TAR_HAND = [3, 40, 17, 130, 5, 64, 29], 45, 301, 0.1, 0.1


def import_lid_utils():
    mods = make_golden.import_reference()
    pkg = sys.modules["sidekit"]
    for name in ("mixture", "sv_utils", "frontend"):
        sys.modules["sidekit." + name] = types.ModuleType("sidekit." + name)
        setattr(pkg, name, sys.modules["sidekit." + name])
    sys.modules["sidekit.mixture"].Mixture = type("Mixture", (), {})
    pkg.Scores = mods["sidekit.bosaris"].Scores
    return mods, importlib.import_module("sidekit.lid_utils")


def closed_set():
    """-> training rows, their class numbers, test rows, their class numbers"""
    rs = numpy.random.RandomState(3)
    C = len(COUNTS)
    centres = 0.6 * rs.randn(C, DIM)
    A = [numpy.eye(DIM) + 0.3 * rs.randn(DIM, DIM) for _ in range(C)]
    rows = numpy.concatenate([centres[c] + 0.5 * rs.randn(n, DIM).dot(A[c].T) + 0.2 for c, n in enumerate(COUNTS)])
    cls = numpy.repeat(numpy.arange(C), COUNTS)
    order = rs.permutation(rows.shape[0])
    test_cls = rs.randint(0, C, N_TEST)
    test = numpy.stack([centres[c] + 0.5 * A[c].dot(rs.randn(DIM)) + 0.2 for c in test_cls])
    return rows[order], cls[order], test, test_cls


def hand_made():
    """5 classes x 4 segments: one class leading by 800 nats, an exact tie of the two largest, all equal, values near -1e4"""
    return numpy.array([[-40.0, -3.5, -7.25, -10000.5],
                        [761.0, -1.25, -7.25, -10003.0],
                        [-41.5, -1.25, -7.25, -9998.75],
                        [-39.0, -6.0, -7.25, -10001.25],
                        [-44.0, -2.0, -7.25, -10000.0]])


def main():
    mods, lid = import_lid_utils()
    sts_mod = mods["sidekit.statserver"]
    X, cls, T, test_cls = closed_set()
    labels = numpy.array([f"class{c}" for c in cls], dtype="|O")

    def make_sts(models, rows):
        s = sts_mod.StatServer()
        s.modelset = numpy.array(models, dtype="|O")
        s.segset = numpy.array([f"seg{i:04d}" for i in range(len(models))], dtype="|O")
        s.start, s.stop = numpy.empty(len(models), dtype="|O"), numpy.empty(len(models), dtype="|O")
        s.stat0, s.stat1 = numpy.ones((len(models), 1)), numpy.array(rows, dtype=numpy.float64)
        return s

    train = make_sts(labels, X)
    test = make_sts([f"class{c}" for c in test_cls], T)
    fx = {"X": X, "modelset": labels.astype("U"), "T": T, "test_classes": test_cls, "alpha": ALPHA, "p_tar_hand": P_TAR_HAND, "hand": hand_made()}
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        tied = lid.gaussian_backend_train(train)
        hetero = lid.gaussian_backend_train_hetero(train, ALPHA)
        fx.update(classes=tied[0].modelset.astype("U"), means=tied[0].stat1, tied_sigma=tied[1], tied_cst=tied[2],
                  hetero_sigma=numpy.array(hetero[1]), hetero_cst=numpy.array(hetero[2]),
                  tied_ll=lid.gaussian_backend_test(test, tied, compute_llr=False).scoremat,
                  tied_llr=lid.gaussian_backend_test(test, tied).scoremat,
                  hetero_ll=lid.gaussian_backend_test_hetero(test, hetero, compute_llr=False).scoremat,
                  hetero_llr=lid.gaussian_backend_test_hetero(test, hetero).scoremat,
                  hand_llr=lid.compute_log_likelihood_ratio(fx["hand"], P_TAR_HAND))
    numpy.testing.assert_array_equal(hetero[0].stat1, tied[0].stat1)
    assert numpy.all(numpy.isfinite(fx["hand_llr"]))
    conds = [numpy.linalg.cond(s) for s in [fx["tied_sigma"]] + list(fx["hetero_sigma"])]
    print(f"condition numbers <= {max(conds):.1f}; log-likelihoods in [{min(fx['tied_ll'].min(), fx['hetero_ll'].min()):.1f}, "
          f"{max(fx['tied_ll'].max(), fx['hetero_ll'].max()):.1f}]")
    # restatement against the reference
    rel = lambda a, b: numpy.abs(numpy.asarray(a) - numpy.asarray(b)).max() / numpy.abs(b).max()   # noqa: E731
    means, sigma, cst = gbn.train_tied(X, labels)
    hmeans, sigmas, csts = gbn.train_hetero(X, labels, ALPHA)
    errs = {"means": rel(means, fx["means"]), "tied sigma": rel(sigma, fx["tied_sigma"]), "tied cst": rel(cst, fx["tied_cst"]),
            "hetero sigma": rel(sigmas, fx["hetero_sigma"]), "hetero cst": rel(csts, fx["hetero_cst"]),
            "tied ll": rel(gbn.loglik(T, fx["means"], fx["tied_sigma"], fx["tied_cst"]), fx["tied_ll"]),
            "hetero ll": rel(gbn.loglik(T, fx["means"], fx["hetero_sigma"], fx["hetero_cst"]), fx["hetero_ll"]),
            "tied llr": rel(gbn.closed_set_llr(fx["tied_ll"]), fx["tied_llr"]),
            "hetero llr": rel(gbn.closed_set_llr(fx["hetero_ll"]), fx["hetero_llr"]),
            "hand llr": rel(gbn.closed_set_llr(fx["hand"], P_TAR_HAND), fx["hand_llr"])}
    for k, v in errs.items():
        print(f"restatement vs reference  {k}: {v:.1e}")
    assert max(errs.values()) < 1e-12, errs
    path = os.path.join(HERE, "gaussian_backend.npz")
    numpy.savez_compressed(path, **fx)
    print("gaussian_backend.npz", os.path.getsize(path), "bytes", {k: getattr(v, "shape", v) for k, v in fx.items()})


if __name__ == "__main__":
    main()
