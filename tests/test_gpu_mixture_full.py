"""The full-covariance GMM on the GPU (sidekit_amd/mixture_full.py, csrc/gmm_full.hip) against the reference's own output
(tests/golden/mixture_full.npz, written by make_mixture_full_golden.py from the imported reference module, with the reference's factor) and
the float64 numpy restatement with either factor (tests/tools/mixture_full_numpy.py, held to 1e-12 against that fixture by
tests/test_mixture_full_cpu.py).

TOL = 1e-9 relative max-norm, this project's bound for float64 quantities (tests/test_gpu_mixture.py).  Every comparison prints the error
it measured.  The bitwise tests are exact: no floating-point atomics, the cut of a segment depends on its own length and C alone, and
stat2 is one triangle and its mirror image.
"""
import copy
import os
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import mixture_full_numpy as mfn  # noqa: E402
import mixture_numpy as mxn  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9
STARTS, ITERATIONS = ("split0", "split2"), 3
KEYS = ("w", "mu", "invcov", "invchol", "det", "cst")
DIAG_KEYS = ("w", "mu", "invcov", "cov_var_ctl")


@pytest.fixture(scope="module")
def base(golden_dir):
    return dict(numpy.load(os.path.join(golden_dir, "mixture.npz")))


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(numpy.load(os.path.join(golden_dir, "mixture_full.npz")))


def _full(state, reference_factor=False):
    """A FullMixture from a model dict (the restatement's, or a fixture state)"""
    from sidekit_amd.mixture_full import FullMixture
    m = FullMixture(reference_factor=reference_factor)
    for k in KEYS:
        setattr(m, k, numpy.array(state[k], dtype=numpy.float64))
    m.A = numpy.zeros(m.w.shape)
    return m


def _state(fx, tag):
    return {k: fx[f"{tag}_{k}"] for k in KEYS}


def _diag(base, tag):
    from sidekit_amd.mixture import Mixture
    m = Mixture()
    m.w, m.mu, m.invcov, m.cov_var_ctl = (numpy.array(base[f"{tag}_{k}"], dtype=numpy.float64) for k in DIAG_KEYS)
    m.cst, m.det = numpy.zeros(m.w.shape), numpy.zeros(m.w.shape)
    m._compute_all()
    return m


def _check(errs):
    print({k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < TOL, f"{k} differs by {v:.3e} (relative max-norm, bound {TOL})"


def _np(t):
    return t if isinstance(t, numpy.ndarray) else t.cpu().numpy()


def _dense_factor(C, D, seed):
    """a general matrix per component: neither triangular nor symmetric, condition at most about 10"""
    rs = numpy.random.RandomState(seed)
    return numpy.stack([numpy.eye(D) + 0.3 * rs.randn(D, D) / numpy.sqrt(D) for _ in range(C)])


@pytest.fixture(scope="module")
def eight(base, fx):
    """the 8-component model, and the restatement's statistics of the eight segments under the default factor (computed once)"""
    state = _state(fx, "eight")
    return state, mfn.stats(state, base["X"], base["seg_off"], False)


def _against(ubm, ref, X, off, gpu, reference_factor=False, M=None, want=None):
    """lp, lse and the statistics of the segments against the restatement -> the errors, and the device statistics"""
    import torch
    from sidekit_amd.mixture_full import frame_loglik_full_device, gmm_stats_full_device
    x = torch.as_tensor(X).to(gpu)
    lse = frame_loglik_full_device(ubm, x, factor=M)
    assert lse.is_cuda and lse.dtype == torch.float64
    got = gmm_stats_full_device(ubm, x, off, order=2, factor=M)
    C, D = ubm.mu.shape
    S = len(off) - 1
    assert got[0].is_cuda and got[0].shape == (S, C) and got[1].shape == (S, C, D) and got[2].shape == (S, C, D, D) and got[3].shape == (S,)
    r0, r1, r2, rl = mfn.stats(ref, X, off, reference_factor, M=M) if want is None else want
    ref_lp = mfn.log_posteriors(ref, X, reference_factor, M=M)
    errs = {"lse": mxn.rel(_np(lse), mxn.frame_lse(ref_lp)), "stat0": mxn.rel(_np(got[0]), r0), "stat1": mxn.rel(_np(got[1]), r1),
            "stat2": mxn.rel(_np(got[2]), r2), "llk": mxn.rel(_np(got[3]), rl)}
    if M is None:
        errs["lp"] = mxn.rel(ubm.compute_log_posterior_probabilities_full(X), ref_lp)
    return errs, got


# ---- fixture and restatement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", STARTS)
def test_reference_factor_against_the_fixture_and_the_restatement(gpu, base, fx, start):
    """C = 2 and 4, D = 23 (odd, no multiple of 4), a 0-frame, a 3-frame and a 700-frame segment; the model after the first recorded
    iteration, whose second E-step the fixture holds"""
    X, off = base["X"], base["seg_off"]
    state = _state(fx, f"{start}_it0")
    ubm = _full(state, reference_factor=True)
    errs, got = _against(ubm, state, X, off, gpu, True)
    errs = {f"{k} vs restatement": v for k, v in errs.items()}
    errs.update({"lp vs fixture": mxn.rel(ubm.compute_log_posterior_probabilities_full(X), fx[f"{start}_lp1"]),
                 "sum stat0 vs fixture": mxn.rel(_np(got[0]).sum(0), fx[f"{start}_it1_acc_w"]),
                 "sum stat1 vs fixture": mxn.rel(_np(got[1]).sum(0), fx[f"{start}_it1_acc_mu"]),
                 "sum stat2 vs fixture": mxn.rel(_np(got[2]).sum(0), fx[f"{start}_it1_acc_invcov"]),
                 "total llk vs fixture": mxn.rel(_np(got[3]).sum(), fx[f"{start}_it1_llk"])})
    init = _full({k: fx[f"{start}_init_{k}"] for k in KEYS}, reference_factor=True)
    errs["lp of the diagonal model vs fixture"] = mxn.rel(init.compute_log_posterior_probabilities_full(X), fx[f"{start}_lp0"])
    _check(errs)


@pytest.mark.parametrize("start", STARTS)
def test_default_factor_against_the_restatement(gpu, base, fx, start):
    X, off = base["X"], base["seg_off"]
    state = _state(fx, f"{start}_it0")
    errs, _ = _against(_full(state), state, X, off, gpu, False)
    _check(errs)


def test_eight_components_both_factors_and_a_dense_factor(gpu, base, eight):
    X, off = base["X"], base["seg_off"]
    state, want = eight
    errs = {f"default {k}": v for k, v in _against(_full(state), state, X, off, gpu, False, want=want)[0].items()}
    errs.update({f"reference {k}": v for k, v in _against(_full(state, True), state, X, off, gpu, True)[0].items()})
    M = _dense_factor(8, 23, 5)
    errs.update({f"dense {k}": v for k, v in _against(_full(state), state, X, off, gpu, M=M)[0].items()})
    _check(errs)


def test_replaced_mu(gpu, base, eight):
    from sidekit_amd.mixture_full import frame_loglik_full_device
    X = base["X"]
    state, _ = eight
    ubm = _full(state)
    new_mu = state["mu"] + 0.25 * numpy.random.RandomState(12).randn(*state["mu"].shape)
    want = mfn.log_posteriors(state, X, False, mu=new_mu)
    _check({"lp, replaced mu": mxn.rel(ubm.compute_log_posterior_probabilities_full(X, new_mu.flatten()), want),
            "lse, replaced mu": mxn.rel(frame_loglik_full_device(ubm, X, new_mu), mxn.frame_lse(want))})
    assert mxn.rel(want, mfn.log_posteriors(state, X, False)) > 1e-3


def test_f32_frames_are_the_bits_of_the_widened_frames(gpu, base, eight):
    import torch
    from sidekit_amd.mixture_full import frame_loglik_full_device, gmm_stats_full_device
    state, _ = eight
    ubm = _full(state)
    X32, off = base["X"].astype(numpy.float32), base["seg_off"]
    wide = X32.astype(numpy.float64)
    x = torch.as_tensor(X32).to(gpu)
    errs, got = _against(ubm, state, wide, off, gpu, False)
    _check(errs)
    narrow = gmm_stats_full_device(ubm, x, off, order=2)
    assert all(torch.equal(a, b) for a, b in zip(narrow, got)), "widening in the load is exact"
    assert torch.equal(frame_loglik_full_device(ubm, x), frame_loglik_full_device(ubm, torch.as_tensor(wide).to(gpu)))


def test_order_1_is_order_2_without_stat2_and_stat2_is_symmetric(gpu, base, eight):
    import torch
    from sidekit_amd.mixture_full import gmm_stats_full_device
    state, _ = eight
    x, off = torch.as_tensor(base["X"]).to(gpu), base["seg_off"]
    for ubm in (_full(state), _full(state, True)):
        s0, s1, s2, llk = gmm_stats_full_device(ubm, x, off, order=2)
        o0, o1, o2, ollk = gmm_stats_full_device(ubm, x, off, order=1)
        assert o2 is None and torch.equal(o0, s0) and torch.equal(o1, s1) and torch.equal(ollk, llk), "order 1 is order 2 without stat2"
        assert torch.equal(s2, s2.transpose(2, 3)), "stat2 must be symmetric bit for bit"
        assert torch.count_nonzero(s2[6]).item() == s2[6].numel()
    assert off[2] == off[3]
    for t in (s0[2], s1[2], s2[2], llk[2]):
        assert torch.count_nonzero(t).item() == 0, "the empty segment must give exact zeros"


# ---- EM --------------------------------------------------------------------------------------------------------------------------------------
def test_em_one_step_from_every_recorded_state(gpu, base, fx):
    """each recorded iteration from the fixture's previous state, with the reference's factor: one E and one M step"""
    X, errs = base["X"], {}
    for start in STARTS:
        for it in range(ITERATIONS):
            prev = {k: fx[f"{start}_init_{k}" if it == 0 else f"{start}_it{it - 1}_{k}"] for k in KEYS}
            m = _full(prev, reference_factor=True)
            accum = copy.deepcopy(m)
            accum._reset()
            llk = m._expectation(accum, X)
            errs.update({f"{start} it{it} acc_w": mxn.rel(accum.w, fx[f"{start}_it{it}_acc_w"]),
                         f"{start} it{it} acc_mu": mxn.rel(accum.mu, fx[f"{start}_it{it}_acc_mu"]),
                         f"{start} it{it} acc_invcov": mxn.rel(accum.invcov, fx[f"{start}_it{it}_acc_invcov"]),
                         f"{start} it{it} llk": mxn.rel(llk, fx[f"{start}_it{it}_llk"])})
            m._maximization(accum)
            errs.update({f"{start} it{it} {k}": mxn.rel(getattr(m, k), fx[f"{start}_it{it}_{k}"]) for k in KEYS})
    _check(errs)


def test_em_end_to_end(gpu, base, fx):
    import torch
    from sidekit_amd.mixture_full import FullMixture, em_diag2full_device
    X, off, errs = base["X"], base["seg_off"], {}
    x = torch.as_tensor(X).to(gpu)

    class Server:
        def stack_features(self, shows, start_list=None, stop_list=None):
            return numpy.concatenate([X[off[int(s[4:])]:off[int(s[4:]) + 1]] for s in shows])

    for start in STARTS:
        diag = _diag(base, start)
        det_before = diag.det.copy()
        seen = []
        full, llk = em_diag2full_device(diag, x, iterations=ITERATIONS, reference_factor=True, after_iteration=lambda m, v: seen.append(v))
        assert seen == llk and len(llk) == ITERATIONS and full.reference_factor
        errs.update({f"{start} reference factor {k}": mxn.rel(getattr(full, k), fx[f"{start}_it2_{k}"]) for k in KEYS})
        errs[f"{start} reference factor llk"] = mxn.rel(llk, [fx[f"{start}_it{i}_llk"] / fx[f"{start}_it{i}_acc_w"].sum() for i in range(ITERATIONS)])
        trace = mfn.em_diag2full(mxn.model(*(base[f"{start}_{k}"] for k in DIAG_KEYS)), X, ITERATIONS, False)
        full, llk = em_diag2full_device(diag, x, iterations=ITERATIONS)
        assert not full.reference_factor and numpy.all(numpy.diff(llk) >= 0), "EM with the transposed factor does not lose likelihood"
        errs.update({f"{start} default {k}": mxn.rel(getattr(full, k), trace[-1][0][k]) for k in KEYS})
        errs[f"{start} default llk"] = mxn.rel(llk, [l for _, l in trace])
        by_list = FullMixture()
        llk2 = by_list.EM_diag2full(diag, Server(), [f"show{i}" for i in range(8)], iterations=ITERATIONS)
        errs.update({f"{start} EM_diag2full {k}": mxn.rel(getattr(by_list, k), trace[-1][0][k]) for k in KEYS})
        errs[f"{start} EM_diag2full llk"] = mxn.rel(llk2, [l for _, l in trace])
        assert numpy.array_equal(diag.det, det_before), "the diagonal mixture is not changed"
    _check(errs)


# ---- bits ------------------------------------------------------------------------------------------------------------------------------------
def test_bits_depend_on_the_segment_alone(gpu, base, eight):
    import torch
    from sidekit_amd.mixture_full import gmm_stats_full_device
    state, _ = eight
    ubm = _full(state)
    X, off = base["X"], base["seg_off"]
    x = torch.as_tensor(X).to(gpu)
    first = gmm_stats_full_device(ubm, x, off, order=2)
    again = gmm_stats_full_device(ubm, x, off, order=2)
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "two runs differ"
    grouped = gmm_stats_full_device(ubm, x, off, order=2, max_workspace_bytes=1)      # one segment per kernel call
    assert all(torch.equal(a, b) for a, b in zip(first, grouped)), "the grouping of segments changed bits"
    a, b = int(off[6]), int(off[7])
    assert b - a == 700
    alone = gmm_stats_full_device(ubm, x[a:b].clone(), None, order=2)
    moved_x = torch.cat((x[:37], x[a:b], x[b:])).contiguous()                       # the same 700 frames at offset 37, behind other frames
    moved = gmm_stats_full_device(ubm, moved_x, [0, 37, 737, moved_x.shape[0]], order=2)
    for t_all, t_alone, t_moved in zip(first, alone, moved):
        assert torch.equal(t_all[6], t_alone[0]), "the 700-frame segment differs between the 8-segment call and a call on its slice"
        assert torch.equal(t_all[6], t_moved[1]), "the 700-frame segment differs at another offset"


def test_long_segment_is_cut_into_slabs_and_the_last_frame(gpu, base, eight):
    """C = 8: slabs(L, 8) = min(ceil(L / 512), 64), so 1500 frames make three slabs (of 512, 512 and 476 frames); a one-frame segment
    sits on the last frame of X"""
    import torch
    from sidekit_amd import mixture_full
    from sidekit_amd.mixture_full import gmm_stats_full_device
    state, _ = eight
    ubm = _full(state)
    assert mixture_full._slabs(1500, 8) == 3 and mixture_full._slabs(499, 8) == 1
    rs = numpy.random.RandomState(21)
    X = base["X"][rs.randint(0, 1260, 2000)] + 0.05 * rs.randn(2000, 23)
    off = [0, 1500, 1999, 2000]
    errs, got = _against(ubm, state, X, off, gpu, False)
    _check(errs)
    x = torch.as_tensor(X).to(gpu)
    o0, o1, _, _ = gmm_stats_full_device(ubm, x, off, order=1)
    assert torch.equal(o0, got[0]) and torch.equal(o1, got[1]) and torch.equal(got[2], got[2].transpose(2, 3))
    alone = gmm_stats_full_device(ubm, x[:1500].clone(), None, order=2)
    last = gmm_stats_full_device(ubm, x[1999:].clone(), None, order=2)
    for t_all, t_alone, t_last in zip(got, alone, last):
        assert torch.equal(t_all[0], t_alone[0]) and torch.equal(t_all[2], t_last[0]), "a segment's bits depend on its neighbours"


# ---- edge shapes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,D,N", [(3, 1, 200), (3, 96, 200), (65, 5, 200), (1, 16, 70), (4, 60, 130)],
                         ids=["D1", "D96_largest", "C65", "C1_D16_column_tile_edge", "D60"])
def test_edge_shapes_against_the_restatement(gpu, C, D, N):
    """D + 1 columns of [1, X] in tiles of 16: D = 1, 16 (the 17th column opens a second tile), 60 and the largest, 96; C = 1 and
    C = 65.  Designed so that the posteriors are soft (at D = 96 four in five lie within (0.01, 0.99)): random symmetric positive
    definite precision matrices, a common one with eigenvalues in [0.2, 10] scaled by up to 1.1 plus one of each component's own with
    eigenvalues in [0.004, 0.2] (condition at most 100, asserted), means within the common spread, frames drawn around them."""
    rs = numpy.random.RandomState(100 * C + D)

    def spd(lo, hi):
        q = numpy.linalg.qr(rs.randn(D, D))[0]
        a = numpy.dot(q * numpy.exp(rs.uniform(numpy.log(lo), numpy.log(hi), D)), q.T)
        return (a + a.T) / 2

    common = spd(0.2, 10.0)
    invcov = numpy.stack([(1.0 + 0.1 * rs.rand()) * common + spd(0.004, 0.2) for _ in range(C)])
    w = rs.rand(C) + 0.2
    mu = rs.randn(C, D) / numpy.sqrt(D)
    ref = mfn.model(w / w.sum(), mu, invcov)
    assert max(numpy.linalg.cond(ic) for ic in ref["invcov"]) <= 100.0
    X = mu[rs.randint(0, C, N)] + numpy.dot(rs.randn(N, D), numpy.linalg.cholesky(numpy.linalg.inv(common)).T)
    pp = mxn.sum_log_probabilities(mfn.log_posteriors(ref, X))[0]
    assert C == 1 or ((pp > 0.01) & (pp < 0.99)).mean() > 0.4, "the posteriors are meant to be soft"
    off = [0, N // 3, N // 3, N]
    errs = {f"default {k}": v for k, v in _against(_full(ref), ref, X, off, gpu, False)[0].items()}
    errs.update({f"dense {k}": v for k, v in _against(_full(ref), ref, X, off, gpu, M=_dense_factor(C, D, 7) * 0.5)[0].items()})
    _check(errs)
    from sidekit_amd import _lib
    from sidekit_amd.mixture_full import frame_loglik_full_device
    assert D <= _lib.SC_GMM_FULL_MAX_D
    if D == _lib.SC_GMM_FULL_MAX_D:
        wide = mfn.model([1.0], numpy.zeros((1, D + 1)), numpy.eye(D + 1)[None])
        with pytest.raises(ValueError, match="at most 96 dimensions"):
            frame_loglik_full_device(_full(wide), numpy.zeros((4, D + 1)))


# ---- StatServer ------------------------------------------------------------------------------------------------------------------------------
def test_accumulate_stat_full(gpu, base, eight):
    import torch
    from sidekit_amd.statserver import StatServer
    state, (r0, r1, _, _) = eight
    ubm = _full(state)
    X, off = base["X"], base["seg_off"]
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
    server.accumulate_stat_full(ubm, Server())
    assert server.validate() and server.stat0.shape == (8, 8) and server.stat1.shape == (8, 8 * 23)
    resident = StatServer()
    resident.modelset, resident.segset, resident.start, resident.stop = names, names.copy(), server.start, server.stop
    resident.accumulate_stat_full_device(ubm, torch.as_tensor(X).to(gpu), off)
    _check({"stat0": mxn.rel(server.stat0, r0), "stat1": mxn.rel(server.stat1, r1.reshape(8, -1)),
            "resident stat0": mxn.rel(resident.stat0, r0), "resident stat1": mxn.rel(resident.stat1, r1.reshape(8, -1))})
    assert numpy.array_equal(resident.stat0, server.stat0) and numpy.array_equal(resident.stat1, server.stat1)
    diag = _diag(base, "split4")
    for call in (lambda: server.accumulate_stat_full(diag, Server()), lambda: resident.accumulate_stat_full_device(diag, torch.as_tensor(X).to(gpu), off)):
        with pytest.raises(AssertionError, match="has to be a FullMixture"):
            call()
    for call in (lambda: server.accumulate_stat(ubm, Server()), lambda: resident.accumulate_stat_device(ubm, torch.as_tensor(X).to(gpu), off)):
        with pytest.raises(AssertionError, match="has to be a Mixture"):
            call()
    with pytest.raises(Exception, match="dimension of ubm and features differ: 23 / 22"):
        resident.accumulate_stat_full_device(ubm, torch.zeros(4, 22, device=gpu), [0] * 9)
