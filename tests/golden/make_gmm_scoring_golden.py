"""Writes tests/golden/gmm_scoring.npz: what the REFERENCE's ``StatServer.adapt_mean_map``, ``adapt_mean_map_multisession`` and
``sidekit.gmm_scoring.gmm_scoring`` compute on the set of tests/golden/mixture.npz (its frames ``X`` in eight segments, ``seg_off``, and
the final 8-component mixture ``split4``).

Recorded:
  * ``accumulate_stat`` of the eight segments (shows ``show0`` .. ``show7``) under the model names spk0, spk0, spk1, spk1, ... (two
    sessions each; ``show2`` is empty, so spk1's first session has no occupation at all: the ``0 / 0`` case of the single-session form);
  * ``adapt_mean_map`` with ``r`` in {16, 0.5} and ``norm`` in {False, True}; ``adapt_mean_map_multisession`` at ``r = 16``;
  * ``gmm_scoring`` of the four multi-session models and a fifth, ``ubm``, whose super-vector is the UBM's own means, against the seven
    segments that are not empty (all 35 trials), and the same under a trial mask whose row ``spk1`` and column ``show4`` are empty and
    three more trials are off.  The features server is duck-typed on ``load`` and carries a features extractor without an audio file
    name structure, the one branch in which the reference does not look for feature files.
Asserted before writing: the tests' numpy restatement (tests/tools/gmm_scoring_numpy.py) against all of it at 1e-12; the ``ubm`` row of
the reference's scores is exactly 0.  No reference text is copied.

Per frame and component, ``lp_m - lse_ubm`` of this fixture's five models lies in [-246, 2.2] (printed by this script; the largest |mean llk| is 33.06, the largest |llr| 0.6244): nothing
here is near the range of exp, which tests/test_gpu_gmm_scoring.py covers with a case of its own.

Usage:  PYTHONDONTWRITEBYTECODE=1 PYTHONHASHSEED=0 python tests/golden/make_gmm_scoring_golden.py
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
import gmm_scoring_numpy as gsn  # noqa: E402
import mixture_numpy as mxn  # noqa: E402

KEYS = ("w", "mu", "invcov", "cov_var_ctl")
SETTINGS = ((16, False), (16, True), (0.5, False), (0.5, True))


def tag(r, norm):
    return "map_r{}_{}".format(str(r).replace(".", "p"), "norm" if norm else "plain")


def main():
    mods = make_golden.import_reference()
    mix = importlib.import_module("sidekit.mixture")
    scoring = importlib.import_module("sidekit.gmm_scoring")
    sts_mod, bosaris = mods["sidekit.statserver"], mods["sidekit.bosaris"]
    src = dict(numpy.load(os.path.join(HERE, "mixture.npz")))
    X, off = src["X"], src["seg_off"]
    shows = [f"show{i}" for i in range(len(off) - 1)]
    rows = {n: X[off[i]:off[i + 1]] for i, n in enumerate(shows)}

    class Extractor:
        audio_filename_structure = None

    class Server(scoring.FeaturesServer):
        def __init__(self):
            self.features_extractor = Extractor()

        def load(self, show, channel=0, start=None, stop=None):
            return rows[show], numpy.ones(rows[show].shape[0], dtype=bool)

    ubm = mix.Mixture()
    ubm.w, ubm.mu, ubm.invcov, ubm.cov_var_ctl = (numpy.array(src[f"split4_{k}"], dtype=numpy.float64) for k in KEYS)
    ubm.cst, ubm.det = numpy.zeros(ubm.w.shape), numpy.zeros(ubm.w.shape)
    ubm._compute_all()
    fs = Server()
    fx = {}
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        server = sts_mod.StatServer()
        server.modelset = numpy.array([f"spk{i // 2}" for i in range(len(shows))], dtype="|O")
        server.segset = numpy.array(shows, dtype="|O")
        server.start, server.stop = numpy.empty(len(shows), dtype="|O"), numpy.empty(len(shows), dtype="|O")
        server.stat0, server.stat1 = numpy.zeros((0, 8)), numpy.zeros((0, 8 * X.shape[1]))
        server.accumulate_stat(ubm, fs)
        fx.update(modelset=server.modelset.astype("U"), segset=server.segset.astype("U"), stat0=server.stat0, stat1=server.stat1)
        for r, norm in SETTINGS:
            out = server.adapt_mean_map(ubm, r, norm)
            assert out.stat0.shape == (8, 1) and numpy.all(out.stat0 == 1)
            fx[tag(r, norm)] = out.stat1
        multi = server.adapt_mean_map_multisession(ubm, 16, False)
        fx.update(multi_modelset=multi.modelset.astype("U"), multi_stat1=multi.stat1)
        enroll = sts_mod.StatServer()
        enroll.modelset = numpy.concatenate((multi.modelset, numpy.array(["ubm"], dtype="|O")))
        enroll.segset = enroll.modelset.copy()
        enroll.start, enroll.stop = numpy.empty(5, dtype="|O"), numpy.empty(5, dtype="|O")
        enroll.stat0 = numpy.ones((5, 1))
        enroll.stat1 = numpy.concatenate((multi.stat1, ubm.get_mean_super_vector()[None]))
        tested = [s for s in shows if rows[s].shape[0] > 0]
        ndx = bosaris.Ndx(models=numpy.repeat(enroll.modelset, len(tested)), testsegs=numpy.tile(numpy.array(tested, dtype="|O"), 5))
        assert ndx.trialmask.all() and ndx.trialmask.shape == (5, 7)
        full = scoring.gmm_scoring(ubm, enroll, ndx, fs, num_thread=1)
        masked_ndx = bosaris.Ndx(models=numpy.repeat(enroll.modelset, len(tested)), testsegs=numpy.tile(numpy.array(tested, dtype="|O"), 5))
        mask = numpy.ones((5, 7), dtype=bool)
        mask[list(masked_ndx.modelset).index("spk1"), :] = False
        mask[:, list(masked_ndx.segset).index("show4")] = False
        mask[0, 0] = mask[2, 5] = mask[4, 6] = False
        masked_ndx.trialmask = mask
        part = scoring.gmm_scoring(ubm, enroll, masked_ndx, fs, num_thread=1)
    fx.update(enroll_modelset=enroll.modelset.astype("U"), enroll_stat1=enroll.stat1,
              score_modelset=full.modelset.astype("U"), score_segset=full.segset.astype("U"), scoremat=numpy.array(full.scoremat),
              scoremask=numpy.array(full.scoremask), masked_modelset=part.modelset.astype("U"), masked_segset=part.segset.astype("U"),
              masked_scoremat=numpy.array(part.scoremat), masked_scoremask=numpy.array(part.scoremask))
    # restatement against the reference
    m = mxn.model(*(src[f"split4_{k}"] for k in KEYS))
    errs = {}
    for r, norm in SETTINGS:
        errs[tag(r, norm)] = mxn.rel(gsn.adapt_mean_map(m, fx["stat0"], fx["stat1"], r, norm), fx[tag(r, norm)])
    ids, means = gsn.adapt_mean_map_multisession(m, fx["modelset"], fx["stat0"], fx["stat1"], 16, False)
    assert list(ids) == list(fx["multi_modelset"])
    errs["multisession"] = mxn.rel(means, fx["multi_stat1"])
    seg = [shows.index(s) for s in fx["score_segset"]]
    order = [list(fx["enroll_modelset"]).index(n) for n in fx["score_modelset"]]
    want = gsn.llr(m, fx["enroll_stat1"][order], X, off)[:, seg]
    scale = numpy.abs(gsn.llk(m, fx["enroll_stat1"], X, off)[0][:, seg] / numpy.diff(off)[seg]).max()
    errs["scores (absolute, over the largest mean llk)"] = numpy.abs(want - fx["scoremat"]).max() / scale
    errs["masked scores"] = numpy.abs(numpy.where(fx["masked_scoremask"], want, 0.0) - fx["masked_scoremat"]).max() / scale
    assert list(fx["masked_modelset"]) == list(fx["score_modelset"]) and list(fx["masked_segset"]) == list(fx["score_segset"])
    assert numpy.array_equal(fx["masked_scoremask"], mask) and numpy.all(fx["masked_scoremat"][~mask] == 0)
    assert numpy.all(fx["scoremat"][list(fx["score_modelset"]).index("ubm")] == 0.0), "the reference scores the UBM against itself as exactly 0"
    assert numpy.all(fx["stat0"][2] == 0) and numpy.allclose(fx["map_r16_plain"][2], m["mu"].flatten(), rtol=1e-7, atol=0), \
        "the session without frames: mean 0 / 0 = 0, alpha = eps / (eps + r), so the UBM's means less 7e-9 of them"
    lo, hi = gsn.margin_range(m, fx["enroll_stat1"], X)
    worst = max(errs, key=errs.get)
    print(f"restatement vs reference: worst {worst} {errs[worst]:.1e}; largest |mean llk| {scale:.4g}; largest |llr| {numpy.abs(fx['scoremat']).max():.4g}; "
          f"lp_m - lse_ubm per frame and component in [{lo:.3g}, {hi:.3g}]")
    assert errs[worst] < 1e-12, errs
    path = os.path.join(HERE, "gmm_scoring.npz")
    numpy.savez_compressed(path, **fx)
    print("gmm_scoring.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
