"""Writes tests/golden/mixture.npz: a small set of frames in eight segments and what the REFERENCE's ``sidekit.mixture`` and
``StatServer.accumulate_stat`` compute on it.

The set, from ``RandomState(11)`` in draw order: D = 23; six centres ``2 randn(6, D)``; scales ``0.5 + rand(6, D)``; segment lengths
[3, 301, 0, 64, 130, 17, 700, 45] (N = 1260); ``cls = randint(0, 6, N)``; ``X = centres[cls] + scales[cls] * randn(N, D) + 0.3``.
D = 23 makes 2 D + 1 = 47 statistics columns (a k tail and a partial column tile), the 3-frame segment is shorter than a k-tile and sits
in front of a long one, one segment is empty and the 700-frame one is long enough to be cut into slabs.

Recorded, after every iteration (``w, mu, invcov, cov_var_ctl`` and ``llk``):
  * ``EM_split(fs, names, 8, iterations=(1, 2, 2))`` with a duck-typed features server of this file (one show per segment);
  * ``EM_uniform(X, 4, iteration_min=3, iteration_max=3, do_init=False)`` from the last 4-component state of that run, and the number
    of iterations ``EM_uniform(..., iteration_min=1, iteration_max=10, llk_gain=G)`` runs from the same state, with G = 0.01 at least a
    factor 3 away from every gain of a ten-iteration run (on this well-separated set EM reaches its fixed point: later gains are 0);
  * the state after ``_init_uniform(X, 5)`` alone (on this set it collapses on its first component: no EM is run from it);
  * for the final 8-component mixture: ``compute_log_posterior_probabilities(X)``, ``sum_log_probabilities`` of it, one ``_expectation``
    accumulator, ``accumulate_stat`` over the eight segments, and the log posteriors with a replaced ``mu``.
Asserted before writing: ``cov / cov_var_ctl`` of every recorded M-step strictly inside (floor, ceil) = (0.01, 10); the tests' numpy
restatement (tests/tools/mixture_numpy.py) against all of it at 1e-12.  The per-iteration states are taken by wrapping the imported
class's ``_maximization``; no reference text is copied.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mixture_golden.py
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
import mixture_numpy as mxn  # noqa: E402

DIM, CENTRES, LENGTHS, FLOOR, CEIL = 23, 6, [3, 301, 0, 64, 130, 17, 700, 45], 1e-2, 10


def frames():
    rs = numpy.random.RandomState(11)
    centres = 2 * rs.randn(CENTRES, DIM)
    scales = 0.5 + rs.rand(CENTRES, DIM)
    n = sum(LENGTHS)
    cls = rs.randint(0, CENTRES, n)
    return centres[cls] + scales[cls] * rs.randn(n, DIM) + 0.3


def state(m):
    return {k: numpy.array(getattr(m, k), dtype=numpy.float64) for k in ("w", "mu", "invcov", "cov_var_ctl")}


def main():
    mods = make_golden.import_reference()
    mix = importlib.import_module("sidekit.mixture")
    sts_mod = mods["sidekit.statserver"]
    X = frames()
    off = numpy.concatenate(([0], numpy.cumsum(LENGTHS)))
    names = [f"show{i}" for i in range(len(LENGTHS))]
    rows = {n: X[off[i]:off[i + 1]] for i, n in enumerate(names)}

    class Server(sts_mod.FeaturesServer):
        """the two calls EM_split and accumulate_stat make"""
        def __init__(self):
            self.features_extractor = None

        def stack_features(self, show_list, start_list=None, stop_list=None):
            return numpy.concatenate([rows[s] for s in show_list])

        def load(self, show, channel=0, start=None, stop=None):
            return rows[show], numpy.ones(rows[show].shape[0], dtype=bool)

    trace, ratios = [], []
    plain = mix.Mixture._maximization

    def recording(self, accum, ceil_cov=10, floor_cov=1e-2):
        mu = accum.mu / accum.w[:, None]
        ratios.append((accum.invcov / accum.w[:, None] - numpy.square(mu)) / self.cov_var_ctl)
        plain(self, accum, ceil_cov, floor_cov)
        trace.append(state(self))

    mix.Mixture._maximization = recording
    fs = Server()
    fx = {"X": X, "seg_off": off, "lengths": numpy.array(LENGTHS)}
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        ubm = mix.Mixture()
        llk = ubm.EM_split(fs, names, 8, iterations=(1, 2, 2))
        split_trace = list(trace)
        assert len(llk) == len(split_trace) == 5 and [t["w"].shape[0] for t in split_trace] == [2, 4, 4, 8, 8]
        for i, t in enumerate(split_trace):
            fx.update({f"split{i}_{k}": v for k, v in t.items()})
        fx["split_llk"] = numpy.array(llk)

        def from_state(t):
            m = mix.Mixture()
            m.w, m.mu, m.invcov, m.cov_var_ctl = (copy.deepcopy(t[k]) for k in ("w", "mu", "invcov", "cov_var_ctl"))
            m.cst, m.det = numpy.zeros(m.w.shape), numpy.zeros(m.w.shape)
            m._compute_all()
            return m

        del trace[:]
        four = from_state(split_trace[2])
        ullk = four.EM_uniform(X, 4, iteration_min=3, iteration_max=3, do_init=False)
        uni_trace = list(trace)
        assert len(ullk) == len(uni_trace) == 3
        for i, t in enumerate(uni_trace):
            fx.update({f"uniform{i}_{k}": v for k, v in t.items()})
        fx["uniform_llk"] = numpy.array(ullk)
        long_llk = numpy.array(from_state(split_trace[2]).EM_uniform(X, 4, iteration_min=10, iteration_max=10, do_init=False))
        gains = numpy.diff(long_llk)
        G = 0.01                                                        # the default; every gain is far above or far below it
        assert numpy.all((gains >= 3 * G) | (gains <= G / 3)) and (gains >= 3 * G).any() and (gains <= G / 3).any(), gains
        early = from_state(split_trace[2]).EM_uniform(X, 4, iteration_min=1, iteration_max=10, llk_gain=G, do_init=False)
        assert 2 <= len(early) < 10, len(early)
        fx.update(early_gain=G, early_iterations=len(early), early_llk=numpy.array(early))
        del trace[:]
        ini = mix.Mixture()
        ini._init_uniform(X, 5)
        fx.update({f"init5_{k}": v for k, v in state(ini).items()})
        fx["init5_A"] = numpy.array(ini.A)
        lp = ubm.compute_log_posterior_probabilities(X)
        pp, total = mix.sum_log_probabilities(lp)
        accum = copy.deepcopy(ubm)
        accum._reset()
        e_llk = ubm._expectation(accum, X)
        server = sts_mod.StatServer()
        server.modelset = numpy.array(names, dtype="|O")
        server.segset = numpy.array(names, dtype="|O")
        server.start, server.stop = numpy.empty(len(names), dtype="|O"), numpy.empty(len(names), dtype="|O")
        server.stat0, server.stat1 = numpy.zeros((0, 8)), numpy.zeros((0, 8 * DIM))
        server.accumulate_stat(ubm, fs)
        new_mu = ubm.mu + 0.25 * numpy.random.RandomState(12).randn(*ubm.mu.shape)
        fx.update(final_A=numpy.array(ubm.A), final_cst=ubm.cst, final_det=ubm.det, lp=lp, pp_sum=pp.sum(0), total_llk=total,
                  accum_w=accum.w, accum_mu=accum.mu, accum_invcov=accum.invcov, accum_llk=e_llk, acc_stat0=server.stat0, acc_stat1=server.stat1,
                  new_mu=new_mu, lp_new_mu=ubm.compute_log_posterior_probabilities(X, new_mu.flatten()))
    mix.Mixture._maximization = plain
    lo, hi = min(r.min() for r in ratios), max(r.max() for r in ratios)
    print(f"cov / cov_var_ctl over {len(ratios)} M-steps in [{lo:.3g}, {hi:.3g}]; smallest final weight {ubm.w.min():.4f}; "
          f"EM_uniform gains {gains}; early stop at gain {G:.3g} after {len(early)} iterations")
    assert FLOOR < lo and hi < CEIL
    # restatement against the reference
    errs = {}
    t = mxn.em_split(X, 8, (1, 2, 2), off)
    for i, (m, l) in enumerate(t):
        for k in ("w", "mu", "invcov", "cov_var_ctl"):
            errs[f"split{i} {k}"] = mxn.rel(m[k], fx[f"split{i}_{k}"])
        errs[f"split{i} llk"] = mxn.rel(l, fx["split_llk"][i])
    four = mxn.model(*(fx[f"split2_{k}"] for k in ("w", "mu", "invcov", "cov_var_ctl")))
    for i, (m, l) in enumerate(mxn.em_uniform(four, X, 3, 3)):
        for k in ("w", "mu", "invcov"):
            errs[f"uniform{i} {k}"] = mxn.rel(m[k], fx[f"uniform{i}_{k}"])
        errs[f"uniform{i} llk"] = mxn.rel(l, fx["uniform_llk"][i])
    assert len(mxn.em_uniform(four, X, 1, 10, G)) == len(early)
    m5 = mxn.init_uniform(X, 5)
    for k in ("w", "mu", "invcov", "cov_var_ctl", "A"):
        errs[f"init5 {k}"] = mxn.rel(m5[k], fx[f"init5_{k}"])
    final = mxn.model(*(fx[f"split4_{k}"] for k in ("w", "mu", "invcov", "cov_var_ctl")))
    s0, s1, s2, sl = mxn.stats(final, X, off)
    errs.update({"A": mxn.rel(final["A"], fx["final_A"]), "lp": mxn.rel(mxn.log_posteriors(final, X), lp),
                 "lp new mu": mxn.rel(mxn.log_posteriors(final, X, new_mu), fx["lp_new_mu"]), "llk": mxn.rel(sl.sum(), total),
                 "accum w": mxn.rel(s0.sum(0), accum.w), "accum mu": mxn.rel(s1.sum(0), accum.mu), "accum invcov": mxn.rel(s2.sum(0), accum.invcov),
                 "stat0": mxn.rel(s0, server.stat0), "stat1": mxn.rel(s1.reshape(len(names), -1), server.stat1)})
    worst = max(errs, key=errs.get)
    print(f"restatement vs reference: worst {worst} {errs[worst]:.1e}")
    assert errs[worst] < 1e-12, errs
    path = os.path.join(HERE, "mixture.npz")
    numpy.savez_compressed(path, **fx)
    print("mixture.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
