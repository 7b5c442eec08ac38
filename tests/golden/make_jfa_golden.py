"""Writes tests/golden/jfa.npz: a small set of Baum-Welch statistics with speakers and sessions and what the REFERENCE's
``StatServer.factor_analysis`` / ``estimate_hidden`` (sidekit/statserver.py) and ``jfa_scoring`` (sidekit/jfa_scoring.py) compute on it.

The set, from ``RandomState(SEED)`` in draw order: C = 6 components of D = 5; 12 speakers with 2 to 5 sessions each, the sessions of
all speakers in one random order (so a speaker's sessions are interleaved with the others'); ``w`` = a Dirichlet draw, ``mu = 2 randn``,
``invcov = 1 / (0.5 + rand)``; per session a frame count ``50 (0.5 + rand)`` spread over the components by a Dirichlet draw; ``stat1``
from a speaker shift of rank 4, a session shift of rank 3 and a small full-rank speaker offset, plus noise ``sqrt(stat0)``; the start
matrices ``F = 0.1 randn``, ``G = 0.1 randn``, ``H = 0.1 (0.5 + rand)``.  A second draw of the same kind gives the scoring set: 4 models,
the first with three enrolment sessions, and 9 test segments; the ``Ndx`` names a fifth model and a tenth segment that do not exist and
its mask has holes.  All statistics are rounded to float32 values (held as float64), so a ``StatServer`` file returns them bit for bit.

Recorded: ``factor_analysis(4, 3, True, it_nb=(3, 3, 3), batch_size=16, init_matrices=...)`` -> ``F``, ``G``, ``H``, ``sigma`` and, by
wrapping the imported class's ``_expectation`` / ``_maximization``, the accumulators ``_A``, ``_C``, ``_R`` of the first iteration of the two
sub-space stages and the matrix after every iteration; a second run with ``it_nb=(3, 3, 1)`` whose ``estimate_map`` frame is read at
its return (``sys.setprofile``) for the MAP accumulators of the first iteration; ``estimate_hidden`` with ``V`` only, ``U`` only, both,
and both with ``D``; ``jfa_scoring`` with ``check_missing`` True (``align_models`` keeps the FIRST enrolment session of a model) and False
(exact ``Ndx``; the three sessions are summed).  No reference text is copied.

Asserted before writing: ``cond(Lambda) <= 1e3`` for every posterior, ``cond <= 1e4`` for every ``_A[c]`` and ``_R``; the numpy
restatement (tests/tools/jfa_numpy.py) against every recorded array at 1e-12; with that restatement, statistics perturbed by 1e-13
relative move every recorded output by less than 1e-10 relative -- which is what lets the project's float64 bound of 1e-9 apply to
quantities that went through nine EM iterations.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_jfa_golden.py
"""
import contextlib
import copy
import importlib
import io
import os
import sys
import warnings

import numpy

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

import make_golden  # noqa: E402
import ivector_numpy as ivn  # noqa: E402
import jfa_numpy as jfn  # noqa: E402

SEED = 47
C, D, SPEAKERS, RANK_F, RANK_G, BATCH, IT_NB = 6, 5, 12, 4, 3, 16, (3, 3, 3)
COND_LAMBDA, COND_ACC = 1e3, 1e4
f32 = lambda a: a.astype(numpy.float32).astype(numpy.float64)   # noqa: E731


def statistics(rs, mu, invcov, speaker_of, Vt, Ut):
    """stat0, stat1 of the sessions whose speakers are `speaker_of` (integers), rounded to float32 values"""
    n, n_spk = speaker_of.shape[0], speaker_of.max() + 1
    frames = 50 * (0.5 + rs.rand(n))
    stat0 = frames[:, None] * rs.dirichlet(3 * numpy.ones(C), n)
    y, x, offset = rs.randn(n_spk, RANK_F), rs.randn(n, RANK_G), 0.1 * rs.randn(n_spk, C * D)
    shift = (y[speaker_of].dot(Vt.T) + x.dot(Ut.T) + offset[speaker_of]).reshape(n, C, D)
    sigma = 1.0 / numpy.sqrt(invcov)
    stat1 = stat0[:, :, None] * (mu[None] + sigma[None] * shift) + numpy.sqrt(stat0)[:, :, None] * sigma[None] * rs.randn(n, C, D)
    return f32(stat0), f32(stat1.reshape(n, C * D))


def data():
    rs = numpy.random.RandomState(SEED)
    w = rs.dirichlet(5 * numpy.ones(C))
    mu = 2 * rs.randn(C, D)
    invcov = 1.0 / (0.5 + rs.rand(C, D))
    speaker_of = rs.permutation(numpy.repeat(numpy.arange(SPEAKERS), rs.randint(2, 6, SPEAKERS)))
    Vt, Ut = 0.3 * rs.randn(C * D, RANK_F), 0.2 * rs.randn(C * D, RANK_G)
    stat0, stat1 = statistics(rs, mu, invcov, speaker_of, Vt, Ut)
    init = (0.1 * rs.randn(C * D, RANK_F), 0.1 * rs.randn(C * D, RANK_G), 0.1 * (0.5 + rs.rand(C * D)))
    enroll_of, test_of = numpy.array([0, 1, 0, 2, 3, 0]), numpy.array([0, 1, 2, 3, 0, 1, 2, 3, 0])
    enroll, test = statistics(rs, mu, invcov, enroll_of, Vt, Ut), statistics(rs, mu, invcov, test_of, Vt, Ut)
    mask = rs.rand(5, 10) < 0.7
    mask[:, 0] = True
    mask[0, :] = True
    return w, mu, invcov, speaker_of, stat0, stat1, init, enroll_of, enroll, test, mask


def server_of(sts_mod, models, segments, stat0, stat1):
    s = sts_mod.StatServer()
    s.modelset, s.segset = numpy.array(models, dtype="|O"), numpy.array(segments, dtype="|O")
    s.start, s.stop = numpy.empty(len(models), dtype="|O"), numpy.empty(len(models), dtype="|O")
    s.stat0, s.stat1 = stat0.copy(), stat1.copy()
    return s


def lambda_cond(stat0, W, sigma):
    """worst cond(I + sum_c n_c W_c' W_c) over the sessions, W whitened by sigma"""
    if W.shape[1] == 0:
        return 1.0
    lam = numpy.eye(W.shape[1])[None] + ivn.unpack(stat0.dot(ivn.gram(W / numpy.sqrt(sigma)[:, None], C, D)), W.shape[1])
    return max(numpy.linalg.cond(m) for m in lam)


def main():
    mods = make_golden.import_reference()
    mix = importlib.import_module("sidekit.mixture")
    jfa_mod = importlib.import_module("sidekit.jfa_scoring")
    sts_mod, bosaris = mods["sidekit.statserver"], mods["sidekit.bosaris"]
    w, mu, invcov, speaker_of, stat0, stat1, init, enroll_of, enroll, test, mask = data()
    n = stat0.shape[0]
    print(f"{n} sessions of {SPEAKERS} speakers, sessions per speaker {numpy.bincount(speaker_of).tolist()}")
    assert 36 <= n <= 48 and numpy.bincount(speaker_of).min() >= 2 and numpy.any(numpy.diff(speaker_of) < 0)
    ubm = mix.Mixture()
    ubm.w, ubm.mu, ubm.invcov, ubm.cov_var_ctl = w.copy(), mu.copy(), invcov.copy(), 1.0 / invcov
    ubm.cst, ubm.det = numpy.zeros(C), numpy.zeros(C)
    ubm._compute_all()
    assert ubm.validate()
    models = [f"spk{s:02d}" for s in speaker_of]
    segments = [f"sess{i:02d}" for i in range(n)]
    fx = {"w": w, "mu": mu, "invcov": invcov, "speaker_of": speaker_of, "stat0": stat0, "stat1": stat1, "F_init": init[0], "G_init": init[1],
          "H_init": init[2], "batch_size": numpy.array(BATCH), "it_nb": numpy.array(IT_NB)}

    # ---- training: the accumulators and the matrix of every iteration through the class's own methods
    expectations, maximizations, map_frames = [], [], []
    plain_e, plain_m = sts_mod.StatServer._expectation, sts_mod.StatServer._maximization

    def traced_e(self, *args, **kwargs):
        out = plain_e(self, *args, **kwargs)
        expectations.append(tuple(numpy.array(a, dtype=numpy.float64) for a in out))
        return out

    def traced_m(self, *args, **kwargs):
        out = plain_m(self, *args, **kwargs)
        maximizations.append(numpy.array(out[0], dtype=numpy.float64))
        return out

    def profile(frame, event, arg):
        if event == "return" and frame.f_code.co_name == "estimate_map":
            map_frames.append({k: numpy.array(frame.f_locals[k], dtype=numpy.float64) for k in ("_A", "_C", "D")})

    def run(it_nb):
        server = server_of(sts_mod, models, segments, stat0, stat1)
        with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = server.factor_analysis(RANK_F, RANK_G, True, False, it_nb, True, ubm, BATCH, 1, False, tuple(m.copy() for m in init))
        assert numpy.array_equal(server.stat1, stat1) and numpy.array_equal(server.stat0, stat0)
        return out

    sts_mod.StatServer._expectation, sts_mod.StatServer._maximization = traced_e, traced_m
    mean, F, G, H, sigma = run(IT_NB)
    assert len(expectations) == len(maximizations) == IT_NB[0] + IT_NB[1]
    assert numpy.array_equal(mean, mu.reshape(-1)) and numpy.array_equal(sigma, 1.0 / invcov.reshape(-1))
    assert numpy.array_equal(maximizations[IT_NB[0] - 1], F) and numpy.array_equal(maximizations[-1], G) and H.shape == (C * D,)
    fx.update(F=F, G=G, H=H, sigma=sigma)
    for tag, first in (("F", 0), ("G", IT_NB[0])):
        fx["A_" + tag], fx["C_" + tag], fx["R_" + tag] = expectations[first]
        for i in range(3):
            fx[f"{tag}_it{i}"] = maximizations[first + i]
    traced = list(expectations)
    sys.setprofile(profile)
    one = run((IT_NB[0], IT_NB[1], 1))
    sys.setprofile(None)
    sts_mod.StatServer._expectation, sts_mod.StatServer._maximization = plain_e, plain_m
    assert len(map_frames) == 1 and numpy.array_equal(one[1], F) and numpy.array_equal(one[2], G)
    fx["A_H"], fx["C_H"], fx["H_it0"] = map_frames[0]["_A"], map_frames[0]["_C"], one[3]
    assert numpy.array_equal(map_frames[0]["D"], one[3])

    # ---- estimate_hidden: V only, U only, both, both with D
    for tag, args in (("v", (F, None, None)), ("u", (None, G, None)), ("vu", (F, G, None)), ("vud", (F, G, H))):
        server = server_of(sts_mod, models, segments, stat0, stat1)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            y, x, z = server.estimate_hidden(mean, sigma, *(None if a is None else a.copy() for a in args), batch_size=BATCH)
        fx[f"hid_{tag}_y"], fx[f"hid_{tag}_x"] = y.stat1, x.stat1
        if args[2] is not None:
            fx[f"hid_{tag}_z"] = z.stat1
    assert fx["hid_v_x"].shape == (n, 0) and fx["hid_u_y"].shape == (n, 0) and fx["hid_vud_z"].shape == (n, C * D)

    # ---- jfa_scoring
    enroll_models = [f"m{s}" for s in enroll_of]
    enroll_segments = [f"e{i}" for i in range(len(enroll_of))]
    test_segments = [f"t{i}" for i in range(test[0].shape[0])]
    ndx = bosaris.Ndx()
    ndx.modelset = numpy.array(["m0", "m1", "m2", "m3", "m_missing"], dtype="|O")
    ndx.segset = numpy.array(test_segments + ["t_missing"], dtype="|O")
    ndx.trialmask = mask.copy()
    assert ndx.validate() and not mask.all()
    exact = bosaris.Ndx()
    exact.modelset, exact.segset, exact.trialmask = ndx.modelset[:4].copy(), ndx.segset[:9].copy(), mask[:4, :9].copy()
    fx.update(enroll_of=enroll_of, enroll_stat0=enroll[0], enroll_stat1=enroll[1], test_stat0=test[0], test_stat1=test[1], ndx_mask=mask)
    for tag, which, check in (("checked", ndx, True), ("unchecked", exact, False)):
        e_srv, t_srv = server_of(sts_mod, enroll_models, enroll_segments, *enroll), server_of(sts_mod, test_segments, test_segments, *test)
        with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sc = jfa_mod.jfa_scoring(ubm, e_srv, t_srv, copy.deepcopy(which), mean, sigma, F.copy(), G.copy(), H.copy(), batch_size=BATCH,
                                     check_missing=check)
        assert list(sc.modelset) == ["m0", "m1", "m2", "m3"] and list(sc.segset) == test_segments
        assert numpy.array_equal(sc.scoremask, mask[:4, :9])
        fx["scores_" + tag] = numpy.array(sc.scoremat, dtype=numpy.float64)
    assert jfn.rel(fx["scores_checked"][0], fx["scores_unchecked"][0]) > 1e-3, "the first model: one session against three"
    assert numpy.array_equal(fx["scores_checked"][1:], fx["scores_unchecked"][1:])

    # ---- conditioning of everything that is inverted or solved
    _, _, m0, _ = jfn.model_sums(stat0, stat1, speaker_of)
    worst_lambda = 0.0
    for phi in [init[0]] + [fx[f"F_it{i}"] for i in range(3)]:   # the E-steps of the first stage and the y that follow it
        worst_lambda = max(worst_lambda, lambda_cond(m0, phi, sigma))
    for phi in [init[1]] + [fx[f"G_it{i}"] for i in range(3)] + [F, numpy.hstack((F, G))]:
        worst_lambda = max(worst_lambda, lambda_cond(stat0, phi, sigma))
    first = numpy.array([list(enroll_of).index(m) for m in range(4)])
    _, _, e0, _ = jfn.model_sums(enroll[0], enroll[1], enroll_of)
    for s0, phi in ((enroll[0][first], numpy.hstack((F, G))), (e0, numpy.hstack((F, G))), (test[0], G)):
        worst_lambda = max(worst_lambda, lambda_cond(s0, phi, sigma))
    worst_acc = max(max(max(numpy.linalg.cond(m) for m in a), numpy.linalg.cond(r)) for a, _, r in traced)
    print(f"worst cond(Lambda) {worst_lambda:.3g} (bound {COND_LAMBDA:g}); worst cond(_A[c]), cond(_R) {worst_acc:.3g} (bound {COND_ACC:g})")
    assert worst_lambda <= COND_LAMBDA and worst_acc <= COND_ACC

    # ---- the restatement against the reference, and how far 1e-13 on the statistics moves it
    ours = jfn.restated(fx)
    errs = {k: jfn.rel(ours[k], fx[k]) for k in jfn.RECORDED if fx[k].size}
    worst = max(errs, key=errs.get)
    print(f"restatement vs reference: worst {worst} {errs[worst]:.1e}")
    assert errs[worst] < 1e-12, errs
    rs = numpy.random.RandomState(SEED + 1)
    moved = dict(fx)
    for k in ("stat0", "stat1", "enroll_stat0", "enroll_stat1", "test_stat0", "test_stat1"):
        moved[k] = fx[k] * (1.0 + 1e-13 * rs.choice([-1.0, 1.0], fx[k].shape))
    theirs = jfn.restated(moved)
    sens = {k: jfn.rel(theirs[k], ours[k]) for k in jfn.RECORDED if fx[k].size}
    worst = max(sens, key=sens.get)
    print(f"statistics moved by 1e-13 relative: worst {worst} {sens[worst]:.1e}")
    assert sens[worst] < 1e-10, sens
    path = os.path.join(HERE, "jfa.npz")
    numpy.savez_compressed(path, **fx)
    print("jfa.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
