"""What the CPU and the GPU tests of the SVM back end share: the problem sets of tests/golden/svm.npz (make_svm_golden.py) as float64
arrays, and the bar of a model."""
import os

import numpy

SETS = ("eq1", "eq3", "batch7", "n2", "n255", "n256", "n257", "dup", "twin", "nofree")
SCALE = 16.0      # supervectors are stored as int8 q, the vectors are q / 16
FLOOR = 1e-12     # the repository's bar for float64 algebra restated in another order; the bar where the generator measured d = 0


def load(golden_dir):
    return dict(numpy.load(os.path.join(golden_dir, "svm.npz")))


def problem(fx, tag):
    """-> dict(bg (B, D), en (Ne, D), model_of, c (M,), W, b, bar_w (M,), bar_b (M,), names)"""
    return {"bg": fx[f"{tag}_bg"] / SCALE, "en": fx[f"{tag}_en"] / SCALE, "model_of": fx[f"{tag}_model_of"], "c": fx[f"{tag}_c"],
            "W": fx[f"{tag}_W"], "b": fx[f"{tag}_b"], "names": [str(n) for n in fx[f"{tag}_names"]],
            "bar_w": numpy.maximum(10 * fx[f"{tag}_d_w"], FLOOR), "bar_b": numpy.maximum(10 * fx[f"{tag}_d_b"], FLOOR)}


def errors(p, W, b):
    """-> (M,) relative max-norm error of each model's w, (M,) |db| / max(1, |b|): the quantities the generator's d is measured in"""
    return (numpy.abs(W - p["W"]).max(axis=1) / numpy.abs(p["W"]).max(axis=1),
            numpy.abs(b - p["b"]) / numpy.maximum(1.0, numpy.abs(p["b"])))


def assert_solves(K, B, coef, rho, C, eps, iterations):
    """What a solver's result at tolerance ``eps`` must satisfy, checked in float64 from the returned coefficients alone: the box, the
    equality constraint, the stopping rule on the gradient recomputed from ``a``, and rho as the rule gives it for this ``a``.
    The recomputed gradient differs from the one the solver carried by rounding only: a gradient entry is a sum of n products of at
    most ``C max|K|`` and has seen two more per update, so it is held to ``(n + 2 iterations) 2^-52 (1 + C max_i sum_j |K_ij|)``."""
    import svm_numpy as svn
    n = K.shape[0]
    y = numpy.where(numpy.arange(n) < B, 1.0, -1.0)
    a = coef * y
    assert numpy.all(a >= 0) and numpy.all(a <= C), "0 <= a <= C"
    assert abs(y @ a) <= 1e-12 * C * n, f"y'a = {y @ a:.3e}"
    gap, _, G = svn.gap_of(K, B, a, C)
    assert gap < eps * (1 + 1e-6), f"recomputed gap {gap:.6e} against eps {eps}"
    tol = (n + 2 * iterations) * 2.0 ** -52 * (1 + C * numpy.abs(K).sum(axis=1).max())
    want = svn.rho_of(y, a, G, C)
    assert abs(want - rho) <= tol, f"rho {rho!r} against the rule's {want!r} (bound {tol:.1e})"


def assert_within_bars(tag, p, W, b):
    e_w, e_b = errors(p, numpy.asarray(W), numpy.asarray(b))
    print(f"{tag}: w {e_w.max():.2e} (bar {p['bar_w'].min():.1e}), b {e_b.max():.2e} (bar {p['bar_b'].min():.1e})")
    assert numpy.all(e_w <= p["bar_w"]), f"{tag}: w differs by {e_w} (relative max-norm), bars {p['bar_w']}"
    assert numpy.all(e_b <= p["bar_b"]), f"{tag}: b differs by {e_b}, bars {p['bar_b']}"
