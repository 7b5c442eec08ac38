"""Writes tests/golden/ivector.npz: a small set of Baum-Welch statistics and what the REFERENCE's ``sidekit.factor_analyser`` computes on
it: ``e_on_batch``, ``total_variability_single`` and ``extract_ivectors_single``.

The set, from ``RandomState(31)`` in draw order: C = 6 components of D = 5, rank R = 7, N = 40 sessions; ``w`` = a Dirichlet draw,
``mu = 2 randn(C, D)``, ``invcov = 1 / (0.5 + rand(C, D))``; per session a frame count ``50 (0.5 + rand)`` spread over the components by
a Dirichlet draw (``stat0``); ``stat1`` from a low-rank shift of the means (``0.3 randn(C D, R)`` times a standard normal factor) and
noise ``sqrt(stat0)``; ``tv_init = 0.1 randn(C D, R)``.  ``stat0`` and ``stat1`` are rounded to float32 values (held as float64), so a
``StatServer`` file, which stores float32, returns them bit for bit.  ``batch_size = 16`` cuts the 40 sessions into three uneven
batches (14, 13, 13).

Recorded: ``F`` after each of 3 iterations with ``min_div`` True and False (taken by wrapping the imported class's ``write``); for the
first iteration the reference's ``e_on_batch`` output of every batch (``e_h``, ``e_hh``) and the accumulators ``_A``, ``_C``, ``_R`` added
over the batches with the reference's own expressions, in its order; ``extract_ivectors_single(..., uncertainty=True)`` with the final
``F`` of the ``min_div`` run.  ``h5py`` is not installed where the fixtures are made: the stand-in module gets a ``File`` over a dict of
numpy arrays (a context manager whose ``__getitem__`` returns the array: ``.shape`` and fancy row indexing are numpy's), which is all
``total_variability_single`` touches.  No reference text is copied.

Asserted before writing: ``cond(Lambda) <= 1e3`` for every session under every ``F`` an E-step used, ``cond <= 1e4`` for every unpacked
``_A[c]`` and ``_R`` of every iteration (with these bounds the project's float64 bound of 1e-9 has two to three orders of margin over
``cond R 2^-52``); the tests' numpy restatement (tests/tools/ivector_numpy.py) against every recorded array at 1e-12.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ivector_golden.py
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
import ivector_numpy as ivn  # noqa: E402

C, D, R, N, BATCH, ITERATIONS = 6, 5, 7, 40, 16, 3
COND_LAMBDA, COND_ACC = 1e3, 1e4


def data():
    rs = numpy.random.RandomState(31)
    w = rs.dirichlet(5 * numpy.ones(C))
    mu = 2 * rs.randn(C, D)
    invcov = 1.0 / (0.5 + rs.rand(C, D))
    frames = 50 * (0.5 + rs.rand(N))
    stat0 = frames[:, None] * rs.dirichlet(3 * numpy.ones(C), N)
    shift = (0.3 * rs.randn(C * D, R)).dot(rs.randn(R, N)).T.reshape(N, C, D)
    sigma = 1.0 / numpy.sqrt(invcov)
    stat1 = stat0[:, :, None] * (mu[None] + sigma[None] * shift) + numpy.sqrt(stat0)[:, :, None] * sigma[None] * rs.randn(N, C, D)
    tv_init = 0.1 * rs.randn(C * D, R)
    f32 = lambda a: a.astype(numpy.float32).astype(numpy.float64)   # noqa: E731
    return w, mu, invcov, f32(stat0), f32(stat1.reshape(N, C * D)), tv_init


class DictFile:
    """what ``total_variability_single`` touches of ``h5py.File``"""
    store = {}

    def __init__(self, name, mode='r'):
        self.data = DictFile.store[name]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def __getitem__(self, key):
        return self.data[key]


def main():
    mods = make_golden.import_reference()
    sys.modules["h5py"].File = DictFile
    mix = importlib.import_module("sidekit.mixture")
    fa_mod = importlib.import_module("sidekit.factor_analyser")
    sts_mod = mods["sidekit.statserver"]
    w, mu, invcov, stat0, stat1, tv_init = data()
    ubm = mix.Mixture()
    ubm.w, ubm.mu, ubm.invcov, ubm.cov_var_ctl = w.copy(), mu.copy(), invcov.copy(), 1.0 / invcov
    ubm.cst, ubm.det = numpy.zeros(C), numpy.zeros(C)
    ubm._compute_all()
    assert ubm.validate()
    names = numpy.array([f"s{i:02d}" for i in range(N)], dtype="|O")
    DictFile.store["stats"] = {"stat0": stat0, "stat1": stat1, "segset": names, "modelset": names}
    batches = numpy.array_split(numpy.arange(N), int(numpy.floor(N / float(BATCH) + 0.999)))
    assert [len(b) for b in batches] == [14, 13, 13]
    fx = {"w": w, "mu": mu, "invcov": invcov, "stat0": stat0, "stat1": stat1, "tv_init": tv_init, "batch_size": numpy.array(BATCH)}

    trace = []
    plain_write = fa_mod.FactorAnalyser.write
    fa_mod.FactorAnalyser.write = lambda self, name: trace.append(numpy.array(self.F, dtype=numpy.float64))
    with contextlib.redirect_stdout(io.StringIO()):
        for tag, min_div in (("md", True), ("nomd", False)):
            del trace[:]
            fa = fa_mod.FactorAnalyser()
            fa.total_variability_single("stats", ubm, R, nb_iter=ITERATIONS, min_div=min_div, tv_init=tv_init.copy(), batch_size=BATCH,
                                        output_file_name="unused")
            assert len(trace) == ITERATIONS and numpy.array_equal(trace[-1], fa.F)
            assert not fa.mean.any() and not fa.Sigma.any() and fa.mean.shape == fa.Sigma.shape == (C * D,)
            for i, F in enumerate(trace):
                fx[f"F_{tag}_it{i}"] = F
    fa_mod.FactorAnalyser.write = plain_write

    # the first iteration's E-step, batch by batch, and its accumulators (the reference's expressions, in its order)
    P = R * (R + 1) // 2
    _A, _C, _R = numpy.zeros((C, P)), numpy.zeros((R, C * D)), numpy.zeros(P)
    ehs, ehhs = [], []
    for idx in batches:
        s0, s1 = stat0[idx, :], stat1[idx, :]
        e_h, e_hh = fa_mod.e_on_batch(s0, s1, ubm, tv_init.copy())   # whitens s1 in place
        _R += numpy.sum(e_hh, axis=0)
        _C += e_h.T.dot(s1)
        _A += s0.T.dot(e_hh)
        ehs.append(e_h)
        ehhs.append(e_hh)
    fx.update(e_h=numpy.concatenate(ehs), e_hh=numpy.concatenate(ehhs), A=_A, C=_C, R=_R)

    # extraction with the final F of the min_div run
    server = sts_mod.StatServer()
    server.modelset, server.segset = names.copy(), names.copy()
    server.start, server.stop = numpy.empty(N, dtype="|O"), numpy.empty(N, dtype="|O")
    server.stat0, server.stat1 = stat0.copy(), stat1.copy()
    fa = fa_mod.FactorAnalyser()
    fa.F = fx[f"F_md_it{ITERATIONS - 1}"].copy()
    iv, iv_sigma = fa.extract_ivectors_single(ubm, server, uncertainty=True)
    assert numpy.array_equal(iv.stat0, numpy.ones((N, 1))) and numpy.array_equal(iv.segset, names)
    fx.update(iv=iv.stat1, iv_sigma=iv_sigma, stat1_whitened=server.stat1)

    # conditioning of everything that is inverted or solved
    worst_lambda, worst_acc = 0.0, 0.0
    for tag, min_div in (("md", True), ("nomd", False)):
        Fs = [tv_init] + [fx[f"F_{tag}_it{i}"] for i in range(ITERATIONS)]
        for F in Fs:   # the last one is the F extraction uses
            lam = numpy.eye(R)[None] + ivn.unpack(stat0.dot(ivn.gram(F, C, D)), R)
            worst_lambda = max(worst_lambda, max(numpy.linalg.cond(m) for m in lam))
        for F in Fs[:-1]:
            _, acc, _, _ = ivn.em_iteration(stat0, stat1, mu, invcov, F, batches, min_div)
            worst_acc = max(worst_acc, max(numpy.linalg.cond(m) for m in ivn.unpack(acc[0], R)), numpy.linalg.cond(ivn.unpack(acc[2] / N, R)))
    print(f"worst cond(Lambda) {worst_lambda:.3g} (bound {COND_LAMBDA:g}); worst cond(_A[c]), cond(_R) {worst_acc:.3g} (bound {COND_ACC:g})")
    assert worst_lambda <= COND_LAMBDA and worst_acc <= COND_ACC

    # restatement against the reference
    errs = {}
    F1, acc, e_h, e_hh = ivn.em_iteration(stat0, stat1, mu, invcov, tv_init, batches, True)
    errs.update({"e_h": ivn.rel(e_h, fx["e_h"]), "e_hh": ivn.rel(e_hh, fx["e_hh"]), "_A": ivn.rel(acc[0], _A), "_C": ivn.rel(acc[1], _C),
                 "_R": ivn.rel(acc[2], _R), "M-step from the recorded accumulators": ivn.rel(ivn.m_step(_A, _C, _R, N, True), fx["F_md_it0"]),
                 "M-step, no min_div": ivn.rel(ivn.m_step(_A, _C, _R, N, False), fx["F_nomd_it0"])})
    for tag, min_div in (("md", True), ("nomd", False)):
        for i, F in enumerate(ivn.train(stat0, stat1, mu, invcov, tv_init, ITERATIONS, batches, min_div)):
            errs[f"F {tag} it{i}"] = ivn.rel(F, fx[f"F_{tag}_it{i}"])
    r_iv, r_sigma = ivn.extract(stat0, stat1, mu, invcov, fx[f"F_md_it{ITERATIONS - 1}"])
    errs.update({"iv": ivn.rel(r_iv, fx["iv"]), "iv_sigma": ivn.rel(r_sigma, fx["iv_sigma"]),
                 "whitened stat1": ivn.rel(ivn.whiten(stat0, stat1, mu, invcov), fx["stat1_whitened"])})
    worst = max(errs, key=errs.get)
    print(f"restatement vs reference: worst {worst} {errs[worst]:.1e}")
    assert errs[worst] < 1e-12, errs
    path = os.path.join(HERE, "ivector.npz")
    numpy.savez_compressed(path, **fx)
    print("ivector.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
