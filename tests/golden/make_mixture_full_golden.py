"""Writes tests/golden/mixture_full.npz: what the REFERENCE's full-covariance ``sidekit.mixture`` computes on the frames of
tests/golden/mixture.npz (``X`` 1260 x 23 in eight segments, make_mixture_golden.py), starting from two of the diagonal states recorded
there: ``split0`` (C = 2) and ``split2`` (C = 4).

Recorded per start ``<s>`` in (``split0``, ``split2``):
  * ``<s>_init_*``: the attributes after ``init_from_diag`` (``w, mu, invcov, invchol, cov_var_ctl, cst, det``);
  * ``<s>_lp0``: ``compute_log_posterior_probabilities_full(X)`` of that diagonal-as-full model;
  * three iterations of ``_expectation`` / ``_maximization`` with the reference's OWN factor (``invchol`` as ``_compute_all`` leaves it:
    the lower one), and after each one ``<s>_it<i>_*``: ``w, mu, invcov, invchol, det, cst``, the accumulators ``acc_w, acc_mu,
    acc_invcov`` and ``llk`` (the E-step's return value);
  * ``<s>_lp1``: the log posteriors under the model after the first iteration.
The reference stays well conditioned on these: asserted before writing, covariance condition numbers at most 100 and the smallest
occupation at least 200.  No iterations are recorded from ``split4`` (C = 8): there the reference's E-step, which does not match its
M-step, degenerates within three iterations.  ``eight_*`` is one 8-component full model for the kernel tests alone: the M-step of this
file's restatement (the transposed factor) from ``split4``, condition at most 300.

Asserted before writing: the tests' numpy restatement (tests/tools/mixture_full_numpy.py, ``reference_factor=True``) against all of it at
1e-12.  No reference text is copied: the imported class is called.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mixture_full_golden.py
"""
import contextlib
import copy
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
import mixture_full_numpy as mfn  # noqa: E402
import mixture_numpy as mxn  # noqa: E402

STARTS, ITERATIONS = ("split0", "split2"), 3
KEYS = ("w", "mu", "invcov", "invchol", "det", "cst")


def main():
    make_golden.import_reference()
    mix = importlib.import_module("sidekit.mixture")
    base = numpy.load(os.path.join(HERE, "mixture.npz"))
    X = base["X"]
    fx, errs, conds, occupations = {}, {}, [], []

    def diagonal(start):
        m = mix.Mixture()
        m.w, m.mu, m.invcov, m.cov_var_ctl = (numpy.array(base[f"{start}_{k}"]) for k in ("w", "mu", "invcov", "cov_var_ctl"))
        m.cst, m.det = numpy.zeros(m.w.shape), numpy.zeros(m.w.shape)
        m._compute_all()
        return m

    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        for start in STARTS:
            full = mix.Mixture()
            full.init_from_diag(diagonal(start))
            for k in KEYS + ("cov_var_ctl",):
                fx[f"{start}_init_{k}"] = numpy.array(getattr(full, k), dtype=numpy.float64)
            fx[f"{start}_lp0"] = full.compute_log_posterior_probabilities_full(X)
            accum = copy.deepcopy(full)
            for it in range(ITERATIONS):
                accum._reset()
                llk = full._expectation(accum, X)
                fx.update({f"{start}_it{it}_acc_w": accum.w.copy(), f"{start}_it{it}_acc_mu": accum.mu.copy(),
                           f"{start}_it{it}_acc_invcov": accum.invcov.copy(), f"{start}_it{it}_llk": numpy.array(llk)})
                occupations.append(accum.w.min())
                full._maximization(accum)
                for k in KEYS:
                    fx[f"{start}_it{it}_{k}"] = numpy.array(getattr(full, k), dtype=numpy.float64)
                conds += [numpy.linalg.cond(ic) for ic in full.invcov]
                if it == 0:
                    fx[f"{start}_lp1"] = full.compute_log_posterior_probabilities_full(X)
    assert max(conds) <= 100 and min(occupations) >= 200, (max(conds), min(occupations))

    # the restatement against the reference, with the reference's factor
    for start in STARTS:
        d = mxn.model(*(base[f"{start}_{k}"] for k in ("w", "mu", "invcov", "cov_var_ctl")))
        m = mfn.init_from_diag(d)
        for k in KEYS + ("cov_var_ctl",):
            errs[f"{start} init {k}"] = mxn.rel(m[k], fx[f"{start}_init_{k}"])
        errs[f"{start} lp0"] = mxn.rel(mfn.log_posteriors(m, X, True), fx[f"{start}_lp0"])
        for it in range(ITERATIONS):
            m, _, (s0, s1, s2, llk) = mfn.em_step(m, X, True)
            for name, got in (("acc_w", s0), ("acc_mu", s1), ("acc_invcov", s2), ("llk", llk)):
                errs[f"{start} it{it} {name}"] = mxn.rel(got, fx[f"{start}_it{it}_{name}"])
            for k in KEYS:
                errs[f"{start} it{it} {k}"] = mxn.rel(m[k], fx[f"{start}_it{it}_{k}"])
            if it == 0:
                errs[f"{start} lp1"] = mxn.rel(mfn.log_posteriors(m, X, True), fx[f"{start}_lp1"])
    worst = max(errs, key=errs.get)
    print(f"restatement vs reference: worst {worst} {errs[worst]:.1e}; condition at most {max(conds):.1f}, smallest occupation {min(occupations):.1f}")
    assert errs[worst] < 1e-12, errs

    # one 8-component full model for the kernel tests
    d8 = mxn.model(*(base[f"split4_{k}"] for k in ("w", "mu", "invcov", "cov_var_ctl")))
    eight = mfn.em_step(mfn.init_from_diag(d8), X, False)[0]
    cond8 = max(numpy.linalg.cond(ic) for ic in eight["invcov"])
    print(f"eight: condition at most {cond8:.1f}, smallest weight {eight['w'].min():.4f}")
    assert cond8 <= 300
    fx.update({f"eight_{k}": eight[k] for k in KEYS})

    path = os.path.join(HERE, "mixture_full.npz")
    numpy.savez_compressed(path, **fx)
    print("mixture_full.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
