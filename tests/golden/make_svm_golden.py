"""Writes tests/golden/svm.npz: the SVM back end's fixture (``sidekit/svm_training.py``, ``sidekit/svm_scoring.py``).

The reference's bundled libsvm binary is not loaded.  The solver's part comes from scikit-learn's libsvm, the same C-SVC:
``sklearn.svm.SVC(kernel='precomputed', C=c, tol=1e-12)`` on the Gram matrix assembled the way ``svm_training_singleThread`` assembles it
(the background block from the reference's ``StatServer.precompute_svm_kernel_stat1``, then the model's columns and their transpose),
with the reference's labels (2 on the background, 1 on the targets), ``sv_coef = dual_coef_``, ``rho = -intercept_``,
``w = -X[support_]' sv_coef``, ``b = rho``.  The reference's ``StatServer`` (``precompute_svm_kernel_stat1``, ``get_nap_matrix_stat1``,
``get_model_segments``, ``get_model_stat1``), ``sv_utils.save_svm`` / ``read_svm`` / ``check_file_list`` and the score assembly of
``svm_scoring_singleThread`` are the imported reference modules (``make_golden.import_reference()``).  No reference text is copied.

Supervectors are stored as int8 ``q``; the vectors are ``q / 16`` (exact in float64, and the file stays small).

Problem sets (``<set>_bg`` (B, D), ``<set>_en`` (Ne, D), ``<set>_model_of`` (Ne,), ``<set>_c`` (M,), ``<set>_W`` (M, D), ``<set>_b`` (M,)):
  eq1, eq3   B = 48, D = 64, three models of 1 and of 3 sessions each: equal session counts, where the reference is well defined
  batch7     seven models over one background of 33 rows (no multiple of a wavefront), csn in {1, 2, 5}, D = 48
  n2         B = 1, csn = 1
  n255, n256, n257   n just below, at and just above the 256 threads of the solver's workgroup (B = 254, 255, 256, csn = 1, D = 288)
  dup        three identical background vectors and two identical targets: curvature 0 between them (identical points of one class
             have identical gradients, so such a pair is never selected: ``dup_tau_steps`` is 0)
  twin       B = 10, csn = 2, the first target equal to the last background vector: that pair has curvature 0 and is the first one
             selected (the first i is the last background point, by the tie rule), the ``tau`` branch
  nofree     B = csn = 4, c = 1e-3 / mean diag: every a equals C, rho is the midpoint of the two bounds
``c`` is the reference's ``1 / mean(diag(gram))`` except in ``nofree``.  Per model the generator records ``<set>_d_w`` and ``<set>_d_b``:
the discrepancy between the tests' numpy restatement (tests/tools/svm_numpy.py, ``eps = 1e-12``) and libsvm, relative max-norm for ``w``
and ``|db| / max(1, |b|)`` for ``b``.  The tests' bar on a model is ``max(10 d, 1e-12)``: ten times ``d`` is the allowance for a second
correct solver of a uniquely determined optimum (libsvm holds its kernel rows in float32, which is what ``d`` consists of), and 1e-12
is the floor the repository sets for float64 algebra restated in another order, needed where ``d`` is zero (``nofree``: every ``a`` is
``C`` in both, so both ``w`` are the same sum).  A problem with ``d > 1e-5`` is refused: it would hide a wrong update behind a loose bar.
Also recorded: the restatement's counts of free and bounded variables and its iterations, the NAP matrix of 20 vectors x 12 at
``co_rank = 3``, a model file written by the reference, and the ``Scores`` of ``eq3`` and ``batch7`` against test supervectors under an
``Ndx`` with a masked trial, a model without a file and a test segment that ``test_sv`` does not hold.

Usage:  PYTHONDONTWRITEBYTECODE=1 PYTHONHASHSEED=0 python tests/golden/make_svm_golden.py
"""
import importlib
import os
import sys
import tempfile

import numpy
from sklearn.svm import SVC

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

import make_golden  # noqa: E402
import svm_numpy as svn  # noqa: E402

REFUSE = 1e-5
SCALE = 16.0


def quantised(rng, shape):
    return rng.integers(-32, 33, size=shape).astype(numpy.int8)


def server(sts_mod, models, segs, stat1):
    s = sts_mod.StatServer()
    s.modelset, s.segset = numpy.array(models, dtype="|O"), numpy.array(segs, dtype="|O")
    s.start, s.stop = numpy.empty(len(segs), dtype="|O"), numpy.empty(len(segs), dtype="|O")
    s.stat0, s.stat1 = numpy.ones((len(segs), 1)), numpy.array(stat1, dtype=numpy.float64)
    assert s.validate()
    return s


def libsvm_model(K_bb, bg_server, en_server, name, c):
    """one model as the reference builds it, libsvm through scikit-learn -> (w, b, gram, c, sv_coef over all points)"""
    bsn = K_bb.shape[0]
    own = en_server.get_model_stat1(name)
    csn = en_server.get_model_segments(name).shape[0]
    assert own.shape[0] == csn
    X = numpy.vstack((bg_server.stat1, own))
    K = numpy.zeros((bsn + csn, bsn + csn))
    K[:bsn, :bsn] = K_bb
    K[:, bsn:] = numpy.dot(X, own.T)
    K[bsn:, :bsn] = K[:bsn, bsn:].T
    if c is None:
        c = 1 / numpy.mean(numpy.diag(K))
    clf = SVC(kernel="precomputed", C=c, tol=1e-12, shrinking=False, cache_size=500)
    clf.fit(K, numpy.array([2] * bsn + [1] * csn))
    sv_coef, rho = clf.dual_coef_[0], -clf.intercept_[0]
    coef = numpy.zeros(bsn + csn)
    coef[clf.support_] = sv_coef
    assert numpy.all(coef[:bsn] >= 0) and numpy.all(coef[bsn:] <= 0), "the background is libsvm's positive class"
    w = -numpy.dot(X[clf.support_].T, sv_coef)
    return w, rho, K, c, coef


def problem_set(fx, tag, sts_mod, bg_q, en_q, model_of, c_of=None):
    bg, en = bg_q / SCALE, en_q / SCALE
    M = int(model_of.max()) + 1
    names = [f"{tag}_m{m}" for m in range(M)]
    bg_server = server(sts_mod, [f"bg{i}" for i in range(len(bg))], [f"bgseg{i}" for i in range(len(bg))], bg)
    en_server = server(sts_mod, [names[m] for m in model_of], [f"{tag}_s{i}" for i in range(len(en))], en)
    K_bb = bg_server.precompute_svm_kernel_stat1()
    W, b, cs, d_w, d_b, free, at_c, iters, taus = [], [], [], [], [], [], [], [], []
    for m, name in enumerate(names):
        w, rho, K, c, coef = libsvm_model(K_bb, bg_server, en_server, name, None if c_of is None else c_of(bg, en[model_of == m]))
        w2, b2, out = svn.train(bg, en[model_of == m], c, eps=1e-12)
        assert out["status"] == svn.CONVERGED
        dw = numpy.abs(w2 - w).max() / numpy.abs(w).max()
        db = abs(b2 - rho) / max(1.0, abs(rho))
        assert dw <= REFUSE and db <= REFUSE, f"{name}: the restatement and libsvm differ by {dw:.2e} / {db:.2e}: refused"
        a = out["a"]   # the restatement's: where points coincide only the sum of their a is determined, and libsvm's split may differ
        assert numpy.abs(numpy.abs(coef).sum() - a.sum()) <= 1e-9 * a.sum()
        W.append(w); b.append(rho); cs.append(c); d_w.append(dw); d_b.append(db); iters.append(out["iterations"]); taus.append(out["tau_steps"])
        free.append(int(((a > 0) & (a < c)).sum())); at_c.append(int((a >= c).sum()))
    print(f"{tag:8s} B={len(bg):4d} D={bg.shape[1]:4d} csn={numpy.bincount(model_of).tolist()} d_w={max(d_w):.1e} d_b={max(d_b):.1e} "
          f"free={free} at C={at_c} iterations={iters} tau steps={taus}")
    fx.update({f"{tag}_bg": bg_q, f"{tag}_en": en_q, f"{tag}_model_of": model_of.astype(numpy.int64), f"{tag}_c": numpy.array(cs),
               f"{tag}_W": numpy.array(W), f"{tag}_b": numpy.array(b), f"{tag}_d_w": numpy.array(d_w), f"{tag}_d_b": numpy.array(d_b),
               f"{tag}_free": numpy.array(free), f"{tag}_at_c": numpy.array(at_c), f"{tag}_iterations": numpy.array(iters),
               f"{tag}_names": numpy.array(names), f"{tag}_tau_steps": numpy.array(taus)})
    return names, en_server


def scored(fx, tag, mods, names, test_q, masked, ghost="ghost", absent="absent"):
    """the reference's svm_scoring, step by step in one process, on model files the reference wrote"""
    sv_utils = importlib.import_module("sidekit.sv_utils")
    scoring = importlib.import_module("sidekit.svm_scoring")
    sts_mod, bosaris = mods["sidekit.statserver"], mods["sidekit.bosaris"]
    test = test_q / SCALE
    segs = [f"{tag}_t{i}" for i in range(len(test))]
    test_sv = server(sts_mod, segs, segs, test)
    all_models, all_segs = names + [ghost], segs[:2] + [absent] + segs[2:]
    ndx = bosaris.Ndx(models=numpy.repeat(numpy.array(all_models, dtype="|O"), len(all_segs)),
                      testsegs=numpy.tile(numpy.array(all_segs, dtype="|O"), len(all_models)))
    mask = numpy.array(ndx.trialmask)
    for mi, si in masked:
        mask[list(ndx.modelset).index(names[mi]), list(ndx.segset).index(segs[si])] = False
    ndx.trialmask = mask
    with tempfile.TemporaryDirectory() as tmp:
        structure = os.path.join(tmp, "{}.svm")
        for m, name in enumerate(names):
            sv_utils.save_svm(structure.format(name), fx[f"{tag}_W"][m][:, None], fx[f"{tag}_b"][m])
        w0, b0 = sv_utils.read_svm(structure.format(names[0]))
        assert numpy.array_equal(w0, fx[f"{tag}_W"][0]) and b0 == fx[f"{tag}_b"][0]
        fx[f"{tag}_ref_svm_file"] = numpy.frombuffer(open(structure.format(names[0]), "rb").read(), dtype=numpy.uint8)
        existing, idx = sv_utils.check_file_list(ndx.modelset, structure)
        assert ghost not in existing and numpy.array_equal(ndx.modelset[idx], existing)
        clean = ndx.filter(existing, test_sv.segset, True)
        assert list(clean.segset) == list(test_sv.segset), "test_sv is aligned with the filtered Ndx, as the reference's row lookup needs"
        score = bosaris.Scores()
        score.scoremat = numpy.zeros(clean.trialmask.shape)
        score.modelset, score.segset, score.scoremask = clean.modelset, clean.segset, clean.trialmask
        scoring.svm_scoring_singleThread(structure, test_sv, clean, score)
    order = [names.index(n) for n in score.modelset]
    want = svn.scores(fx[f"{tag}_W"][order], fx[f"{tag}_b"][order], test, score.scoremask)
    assert numpy.abs(want - score.scoremat).max() <= 1e-12 * numpy.abs(want).max() and numpy.all(score.scoremat[~score.scoremask] == 0)
    assert (~score.scoremask).sum() == len(masked)
    fx.update({f"{tag}_test": test_q, f"{tag}_test_segset": numpy.array(segs), f"{tag}_ndx_modelset": numpy.array(ndx.modelset, dtype="U"),
               f"{tag}_ndx_segset": numpy.array(ndx.segset, dtype="U"), f"{tag}_ndx_trialmask": mask,
               f"{tag}_score_modelset": numpy.array(score.modelset, dtype="U"), f"{tag}_score_segset": numpy.array(score.segset, dtype="U"),
               f"{tag}_scoremask": numpy.array(score.scoremask), f"{tag}_scoremat": numpy.array(score.scoremat)})


def main():
    mods = make_golden.import_reference()
    sts_mod = mods["sidekit.statserver"]
    rng = numpy.random.default_rng(20240611)
    fx = {}
    eq1_bg = quantised(rng, (48, 64))
    names1, _ = problem_set(fx, "eq1", sts_mod, eq1_bg, quantised(rng, (3, 64)) + 8, numpy.arange(3))
    names3, en3 = problem_set(fx, "eq3", sts_mod, eq1_bg, quantised(rng, (9, 64)) + 8, numpy.array([0, 1, 2, 0, 1, 2, 2, 1, 0]))
    fx["eq3_segments_of_m1"] = numpy.array(en3.get_model_segments("eq3_m1"), dtype="U")
    names7, _ = problem_set(fx, "batch7", sts_mod, quantised(rng, (33, 48)), quantised(rng, (18, 48)) + 8,
                            numpy.array([0, 1, 1, 2, 2, 2, 2, 2, 3, 3, 4, 5, 5, 5, 5, 5, 6, 6]))
    problem_set(fx, "n2", sts_mod, quantised(rng, (1, 8)), quantised(rng, (1, 8)) + 8, numpy.zeros(1, dtype=int))
    pool = quantised(rng, (256, 288))
    target = quantised(rng, (1, 288)) + 8
    for B in (254, 255, 256):
        problem_set(fx, f"n{B + 1}", sts_mod, pool[:B], target, numpy.zeros(1, dtype=int))
    dup_bg = quantised(rng, (12, 24))
    dup_bg[1] = dup_bg[2] = dup_bg[0]
    dup_en = numpy.repeat(quantised(rng, (1, 24)) + 8, 2, axis=0)
    problem_set(fx, "dup", sts_mod, dup_bg, dup_en, numpy.zeros(2, dtype=int))
    assert fx["dup_free"][0] > 0
    twin_bg = quantised(rng, (10, 24))
    problem_set(fx, "twin", sts_mod, twin_bg, numpy.vstack((twin_bg[-1:], quantised(rng, (1, 24)) + 8)), numpy.zeros(2, dtype=int))
    assert fx["twin_tau_steps"][0] > 0, "a target equal to a background vector: the pair has curvature 0 and a positive gradient difference"
    problem_set(fx, "nofree", sts_mod, quantised(rng, (4, 16)), quantised(rng, (4, 16)) + 8, numpy.zeros(4, dtype=int),
                c_of=lambda bg, own: 1e-3 / numpy.mean(numpy.diag(svn.gram(bg, own))))
    assert fx["nofree_free"][0] == 0 and fx["nofree_at_c"][0] == 8, "every variable of `nofree` is at C"
    # NAP
    nap = server(sts_mod, [f"n{i % 5}" for i in range(20)], [f"nap{i}" for i in range(20)], quantised(rng, (20, 12)) / SCALE)
    fx["nap_q"] = (nap.stat1 * SCALE).astype(numpy.int8)
    fx["nap_N"] = nap.get_nap_matrix_stat1(3)
    mine = svn.nap_matrix(nap.stat1, 3)
    sign = numpy.sign((mine * fx["nap_N"]).sum(0))
    assert numpy.abs(mine * sign - fx["nap_N"]).max() <= 1e-10 * numpy.abs(fx["nap_N"]).max()
    # scoring
    scored(fx, "eq3", mods, names3, quantised(rng, (5, 64)) + 4, masked=[(1, 3)])
    scored(fx, "batch7", mods, names7, quantised(rng, (4, 48)) + 4, masked=[(2, 0), (6, 3)])
    path = os.path.join(HERE, "svm.npz")
    numpy.savez_compressed(path, **fx)
    print("svm.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
