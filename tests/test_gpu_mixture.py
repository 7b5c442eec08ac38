"""The diagonal GMM on the GPU (sidekit_amd/mixture.py, csrc/gmm.hip) against the reference's own output (tests/golden/mixture.npz,
written by make_mixture_golden.py from the imported reference module) and the float64 numpy restatement (tests/tools/mixture_numpy.py,
held to 1e-12 against that fixture by tests/test_mixture_cpu.py).

TOL = 1e-9 relative max-norm, this project's bound for float64 quantities.  Every comparison prints the error it measured.  The bitwise
tests are exact: no floating-point atomics, and the cut of a segment depends on its own length alone.
"""
import os
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import mixture_numpy as mxn  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9
KEYS = ("w", "mu", "invcov", "cov_var_ctl")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(numpy.load(os.path.join(golden_dir, "mixture.npz")))


def _mixture(state):
    from sidekit_amd.mixture import Mixture
    m = Mixture()
    m.w, m.mu, m.invcov, m.cov_var_ctl = (numpy.array(state[k], dtype=numpy.float64) for k in KEYS)
    m.cst, m.det = numpy.zeros(m.w.shape), numpy.zeros(m.w.shape)
    m._compute_all()
    return m


def _state(fx, tag):
    return {k: fx[f"{tag}_{k}"] for k in KEYS}


def _check(errs):
    print({k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < TOL, f"{k} differs by {v:.3e} (relative max-norm, bound {TOL})"


@pytest.fixture(scope="module")
def final(fx):
    """the final 8-component mixture, the restatement's model of it and its statistics of the eight segments (computed once)"""
    state = _state(fx, "split4")
    ref = mxn.model(*(state[k] for k in KEYS))
    return _mixture(state), ref, mxn.stats(ref, fx["X"], fx["seg_off"])


def _np(t):
    return t if isinstance(t, numpy.ndarray) else t.cpu().numpy()


def test_loglik_and_statistics_f64_frames(gpu, fx, final):
    import torch
    from sidekit_amd.mixture import frame_loglik_device, gmm_stats_device
    ubm, ref, (r0, r1, r2, rl) = final
    X, off = fx["X"], fx["seg_off"]
    x = torch.as_tensor(X).to(gpu)
    lse = frame_loglik_device(ubm, x)
    assert lse.is_cuda and lse.dtype == torch.float64
    lp = ubm.compute_log_posterior_probabilities(X)
    s0, s1, s2, llk = gmm_stats_device(ubm, x, off, order=2)
    assert s0.is_cuda and s1.shape == (8, 8, 23) and s2.shape == (8, 8, 23)
    o0, o1, o2, _ = gmm_stats_device(ubm, x, off, order=1)
    assert o2 is None and torch.equal(o0, s0) and torch.equal(o1, s1), "order 1 is order 2 without the second moments"
    ref_lp = mxn.log_posteriors(ref, X)
    _check({"lse vs restatement": mxn.rel(_np(lse), mxn.frame_lse(ref_lp)), "lp vs fixture": mxn.rel(lp, fx["lp"]), "lp vs restatement": mxn.rel(lp, ref_lp),
            "stat0": mxn.rel(_np(s0), r0), "stat1": mxn.rel(_np(s1), r1), "stat2": mxn.rel(_np(s2), r2), "llk": mxn.rel(_np(llk), rl),
            "stat0 vs fixture": mxn.rel(_np(s0), fx["acc_stat0"]), "stat1 vs fixture": mxn.rel(_np(s1).reshape(8, -1), fx["acc_stat1"]),
            "sum stat0 vs fixture": mxn.rel(_np(s0).sum(0), fx["accum_w"]), "sum stat2 vs fixture": mxn.rel(_np(s2).sum(0), fx["accum_invcov"]),
            "total llk vs fixture": mxn.rel(_np(llk).sum(), fx["total_llk"])})
    lp_mu = ubm.compute_log_posterior_probabilities(X, fx["new_mu"].flatten())
    _check({"lp, replaced mu, vs fixture": mxn.rel(lp_mu, fx["lp_new_mu"]),
            "lse, replaced mu": mxn.rel(frame_loglik_device(ubm, X, fx["new_mu"]), mxn.frame_lse(fx["lp_new_mu"]))})
    one = ubm.compute_log_posterior_probabilities(X[5])
    assert one.shape == (1, 8) and mxn.rel(one, fx["lp"][5:6]) < TOL


def test_loglik_and_statistics_f32_frames(gpu, fx, final):
    import torch
    from sidekit_amd.mixture import frame_loglik_device, gmm_stats_device
    ubm, ref, _ = final
    X32, off = fx["X"].astype(numpy.float32), fx["seg_off"]
    wide = X32.astype(numpy.float64)
    x = torch.as_tensor(X32).to(gpu)
    s0, s1, s2, llk = gmm_stats_device(ubm, x, off, order=2)
    r0, r1, r2, rl = mxn.stats(ref, wide, off)
    _check({"lse": mxn.rel(_np(frame_loglik_device(ubm, x)), mxn.frame_lse(mxn.log_posteriors(ref, wide))), "stat0": mxn.rel(_np(s0), r0),
            "stat1": mxn.rel(_np(s1), r1), "stat2": mxn.rel(_np(s2), r2), "llk": mxn.rel(_np(llk), rl)})
    w0, w1, w2, wl = gmm_stats_device(ubm, torch.as_tensor(wide).to(gpu), off, order=2)
    assert torch.equal(w0, s0) and torch.equal(w1, s1) and torch.equal(w2, s2) and torch.equal(wl, llk), "widening in the load is exact"


def test_em_one_step_from_every_recorded_state(gpu, fx):
    """each recorded iteration from the fixture's previous state: split where the reference split, one E and one M step"""
    import copy
    X = fx["X"]
    errs = {}
    prev = None
    for i in range(5):
        if prev is None:
            from sidekit_amd.mixture import Mixture
            m = Mixture()
            m._init_single(X.mean(0), (X ** 2).mean(0))
        else:
            m = _mixture(prev)
        if prev is None or fx[f"split{i}_w"].shape[0] != prev["w"].shape[0]:
            m._split_ditribution()
        accum = copy.deepcopy(m)
        accum._reset()
        llk = m._expectation(accum, X) / numpy.sum(accum.w)
        m._maximization(accum)
        prev = _state(fx, f"split{i}")
        errs.update({f"split{i} {k}": mxn.rel(getattr(m, k), prev[k]) for k in KEYS})
        errs[f"split{i} llk"] = mxn.rel(llk, fx["split_llk"][i])
    prev = _state(fx, "split2")
    for i in range(3):
        m = _mixture(prev)
        llk = m.EM_uniform(X, 4, iteration_min=1, iteration_max=1, do_init=False)
        prev = _state(fx, f"uniform{i}")
        errs.update({f"uniform{i} {k}": mxn.rel(getattr(m, k), prev[k]) for k in KEYS})
        errs[f"uniform{i} llk"] = mxn.rel(llk[0], fx["uniform_llk"][i])
    _check(errs)


def test_em_end_to_end(gpu, fx):
    import torch
    from sidekit_amd.mixture import Mixture, em_split_device
    X = fx["X"]
    seen = []
    ubm, llk = em_split_device(torch.as_tensor(X).to(gpu), 8, iterations=(1, 2, 2), after_iteration=lambda m, v: seen.append((m.distrib_nb(), v)))
    assert [n for n, _ in seen] == [2, 4, 4, 8, 8] and [v for _, v in seen] == llk
    errs = {f"em_split_device {k}": mxn.rel(getattr(ubm, k), fx[f"split4_{k}"]) for k in KEYS}
    errs["em_split_device llk"] = mxn.rel(llk, fx["split_llk"])
    errs["A"] = mxn.rel(ubm.A, fx["final_A"])

    class Server:
        def stack_features(self, shows, start_list=None, stop_list=None):
            return numpy.concatenate([X[fx["seg_off"][int(s[4:])]:fx["seg_off"][int(s[4:]) + 1]] for s in shows])

    by_list = Mixture()
    llk2 = by_list.EM_split(Server(), [f"show{i}" for i in range(8)], 8, iterations=(1, 2, 2))
    errs.update({f"EM_split {k}": mxn.rel(getattr(by_list, k), fx[f"split4_{k}"]) for k in KEYS})
    errs["EM_split llk"] = mxn.rel(llk2, fx["split_llk"])
    four = _mixture(_state(fx, "split2"))
    ullk = four.EM_uniform(X, 4, iteration_min=3, iteration_max=3, do_init=False)
    errs.update({f"EM_uniform {k}": mxn.rel(getattr(four, k), fx[f"uniform2_{k}"]) for k in KEYS})
    errs["EM_uniform llk"] = mxn.rel(ullk, fx["uniform_llk"])
    _check(errs)
    early = _mixture(_state(fx, "split2")).EM_uniform(X, 4, iteration_min=1, iteration_max=10, llk_gain=float(fx["early_gain"]), do_init=False)
    assert len(early) == int(fx["early_iterations"]) and mxn.rel(early, fx["early_llk"]) < TOL


def test_accumulate_stat_with_a_duck_typed_server(gpu, fx, final):
    import torch
    from sidekit_amd.statserver import StatServer
    ubm, _, _ = final
    X, off = fx["X"], fx["seg_off"]
    names = numpy.array([f"show{i}" for i in range(8)], dtype="|O")

    class Server:
        features_extractor = None

        def load(self, show, channel=0):
            i = int(show[4:])
            pad = numpy.full((2, X.shape[1]), 99.0)     # two frames the VAD labels drop
            cep = numpy.concatenate((pad[:1], X[off[i]:off[i + 1]], pad[1:]))
            vad = numpy.ones(cep.shape[0], dtype=bool)
            vad[0] = vad[-1] = False
            return cep, vad

    server = StatServer()
    server.modelset, server.segset = names, names.copy()
    server.start, server.stop = numpy.empty(8, dtype="|O"), numpy.empty(8, dtype="|O")
    server.accumulate_stat(ubm, Server())
    assert server.validate() and server.stat0.shape == (8, 8) and server.stat1.shape == (8, 8 * 23)
    resident = StatServer()
    resident.modelset, resident.segset, resident.start, resident.stop = names, names.copy(), server.start, server.stop
    resident.accumulate_stat_device(ubm, torch.as_tensor(X).to(gpu), off)
    _check({"stat0": mxn.rel(server.stat0, fx["acc_stat0"]), "stat1": mxn.rel(server.stat1, fx["acc_stat1"]),
            "resident stat0": mxn.rel(resident.stat0, fx["acc_stat0"]), "resident stat1": mxn.rel(resident.stat1, fx["acc_stat1"])})
    assert numpy.array_equal(resident.stat0, server.stat0) and numpy.array_equal(resident.stat1, server.stat1)
    with pytest.raises(Exception, match="dimension of ubm and features differ: 23 / 22"):
        resident.accumulate_stat_device(ubm, torch.zeros(4, 22, device=gpu), [0] * 9)


@pytest.mark.parametrize("C,D,N", [(5, 7, 150), (70, 9, 200), (1, 6, 90), (4, 1, 130), (6, 64, 100), (3, 5, 1), (5, 128, 70), (6, 40, 100),
                                   (3, 4, 33000)],
                         ids=["C5", "C70_two_component_tiles", "C1", "D1", "D64", "N1", "D128_largest", "D40_eight_column_tiles",
                              "N33000_one_segment_at_the_64_slab_cap"])
def test_tile_edges_against_the_restatement(gpu, C, D, N):
    """The statistics kernel exists for 2, 4, 8, 12 and 17 tiles of 16 columns; 2 D + 1 columns make D = 1 / 5..9 / 40 / 64 / 128 take one
    each (the fixture's D = 23 takes 4 as well), and D = 40 is the variant the D = 60 of a real front-end runs."""
    import torch
    from sidekit_amd.mixture import frame_loglik_device, gmm_stats_device
    rs = numpy.random.RandomState(100 * C + D)
    w = rs.rand(C) + 0.2
    ref = mxn.model(w / w.sum(), rs.randn(C, D), 1.0 / (0.5 + rs.rand(C, D)))
    X = rs.randn(N, D) * 1.2
    off = [0, N] if N < 3 or N > 32768 else [0, N // 3, N // 3, N]      # above 64 x 512 frames the number of slabs is capped
    ubm = _mixture(ref)
    x = torch.as_tensor(X).to(gpu)
    s0, s1, s2, llk = gmm_stats_device(ubm, x, off, order=2)
    r0, r1, r2, rl = mxn.stats(ref, X, off)
    lp = mxn.log_posteriors(ref, X)
    _check({"lse": mxn.rel(_np(frame_loglik_device(ubm, x)), mxn.frame_lse(lp)), "lp": mxn.rel(ubm.compute_log_posterior_probabilities(X), lp),
            "stat0": mxn.rel(_np(s0), r0), "stat1": mxn.rel(_np(s1), r1), "stat2": mxn.rel(_np(s2), r2), "llk": mxn.rel(_np(llk), rl)})


def test_bits_depend_on_the_segment_alone(gpu, fx, final):
    import torch
    from sidekit_amd.mixture import gmm_stats_device
    ubm, _, _ = final
    X, off = fx["X"], fx["seg_off"]
    x = torch.as_tensor(X).to(gpu)
    first = gmm_stats_device(ubm, x, off, order=2)
    again = gmm_stats_device(ubm, x, off, order=2)
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "two runs differ"
    grouped = gmm_stats_device(ubm, x, off, order=2, max_workspace_bytes=1)      # one segment per kernel call
    assert all(torch.equal(a, b) for a, b in zip(first, grouped)), "the grouping of segments changed bits"
    a, b = int(off[6]), int(off[7])
    assert b - a == 700
    alone = gmm_stats_device(ubm, x[a:b].clone(), None, order=2)
    moved_x = torch.cat((x[:37], x[a:b], x[b:])).contiguous()                       # the same 700 frames at offset 37, behind other frames
    moved = gmm_stats_device(ubm, moved_x, [0, 37, 737, moved_x.shape[0]], order=2)
    for t_all, t_alone, t_moved in zip(first, alone, moved):
        assert torch.equal(t_all[6], t_alone[0]), "the 700-frame segment differs between the 8-segment call and a call on its slice"
        assert torch.equal(t_all[6], t_moved[1]), "the 700-frame segment differs at another offset"


def test_empty_segment_and_a_far_frame(gpu, fx, final):
    import torch
    from sidekit_amd.mixture import frame_loglik_device, gmm_stats_device
    ubm, ref, _ = final
    X, off = fx["X"], fx["seg_off"]
    assert off[2] == off[3]
    s0, s1, s2, llk = gmm_stats_device(ubm, torch.as_tensor(X).to(gpu), off, order=2)
    for t in (s0[2], s1[2], s2[2], llk[2]):
        assert torch.count_nonzero(t).item() == 0, "the empty segment must give exact zeros"
    far = X[:3].copy()
    far[1] = ubm.mu[0] + 1200.0 / numpy.sqrt(ubm.invcov.min())                  # at least 1000 standard deviations from every component in every coefficient
    assert numpy.all(numpy.abs(far[1] - ubm.mu) * numpy.sqrt(ubm.invcov) >= 1000.0)
    lse = frame_loglik_device(ubm, far)
    assert numpy.all(numpy.isfinite(lse)) and lse[1] < -1e5
    assert mxn.rel(lse, mxn.frame_lse(mxn.log_posteriors(ref, far))) < TOL
    f0, f1, _, _ = gmm_stats_device(ubm, far, None, order=1)
    assert numpy.all(numpy.isfinite(f0)) and numpy.all(numpy.isfinite(f1)) and abs(f0.sum() - 3.0) < 1e-9
