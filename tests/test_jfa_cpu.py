"""Joint factor analysis without a GPU (sidekit_amd/jfa_scoring.py, csrc/jfa.hip, the JFA methods of sidekit_amd/statserver.py): the numpy
restatement the GPU tests lean on against the reference's own output (tests/golden/jfa.npz, written by make_jfa_golden.py from the
imported reference module), the reference's parameter lists, the mirror's wiring, the entry points' own header against their binding
table and the built library, their argument checks through the C ABI, the refusals, ``subtract_weighted_stat1`` and what importing the
module loads.

The restatement is held to 1e-12 relative max-norm, the bar of the other restatements of float64 algebra (the generator measured at most
2.1e-15 on this set, whose inverted and solved matrices have condition numbers below 31).
"""
import inspect
import os
import subprocess
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ivector_numpy as ivn  # noqa: E402
import jfa_numpy as jfn  # noqa: E402

from sidekit_amd import _lib, jfa_scoring  # noqa: E402
from sidekit_amd.bosaris import Ndx  # noqa: E402
from sidekit_amd.mixture import Mixture  # noqa: E402
from sidekit_amd.statserver import StatServer  # noqa: E402

RESTATEMENT_TOL = 1e-12
C, D, RANK_F, RANK_G, SPEAKERS = 6, 5, 4, 3, 12


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(numpy.load(os.path.join(golden_dir, "jfa.npz")))


def _ubm(fx):
    m = Mixture()
    m.w, m.mu, m.invcov = (numpy.array(fx[k], dtype=numpy.float64) for k in ("w", "mu", "invcov"))
    m.cov_var_ctl = 1.0 / m.invcov
    m.cst, m.det = numpy.zeros(m.w.shape), numpy.zeros(m.w.shape)
    m._compute_all()
    return m


def _server(models, segments, stat0, stat1):
    s = StatServer()
    s.modelset, s.segset = numpy.array(models, dtype="|O"), numpy.array(segments, dtype="|O")
    s.start, s.stop = numpy.empty(len(models), dtype="|O"), numpy.empty(len(models), dtype="|O")
    s.stat0, s.stat1 = numpy.array(stat0, dtype=numpy.float64), numpy.array(stat1, dtype=numpy.float64)
    return s


def _training_server(fx):
    n = fx["stat0"].shape[0]
    return _server([f"spk{s:02d}" for s in fx["speaker_of"]], [f"sess{i:02d}" for i in range(n)], fx["stat0"], fx["stat1"])


def test_fixture_is_the_set_its_generator_describes(fx):
    n = fx["stat0"].shape[0]
    per_speaker = numpy.bincount(fx["speaker_of"])
    assert 36 <= n <= 48 and per_speaker.shape == (SPEAKERS,) and per_speaker.min() >= 2 and per_speaker.max() <= 5
    assert numpy.any(numpy.diff(fx["speaker_of"]) < 0), "the speakers' sessions are interleaved"
    assert fx["stat0"].shape == (n, C) and fx["stat1"].shape == (n, C * D) and tuple(fx["it_nb"]) == (3, 3, 3) and int(fx["batch_size"]) == 16
    for k in ("stat0", "stat1", "enroll_stat0", "enroll_stat1", "test_stat0", "test_stat1"):   # a StatServer file stores float32
        numpy.testing.assert_array_equal(fx[k], fx[k].astype(numpy.float32).astype(numpy.float64))
    assert fx["F"].shape == fx["F_init"].shape == (C * D, RANK_F) and fx["G"].shape == fx["G_init"].shape == (C * D, RANK_G)
    assert fx["H"].shape == fx["H_init"].shape == fx["A_H"].shape == fx["C_H"].shape == (C * D,)
    assert fx["A_F"].shape == (C, RANK_F, RANK_F) and fx["C_F"].shape == (RANK_F, C * D) and fx["R_F"].shape == (RANK_F, RANK_F)
    assert fx["A_G"].shape == (C, RANK_G, RANK_G) and fx["C_G"].shape == (RANK_G, C * D) and fx["R_G"].shape == (RANK_G, RANK_G)
    assert fx["hid_v_y"].shape == (n, RANK_F) and fx["hid_v_x"].shape == (n, 0) and fx["hid_u_y"].shape == (n, 0) and fx["hid_u_x"].shape == (n, RANK_G)
    assert fx["hid_vud_z"].shape == (n, C * D)
    assert list(fx["enroll_of"]) == [0, 1, 0, 2, 3, 0] and fx["test_stat0"].shape == (9, C) and fx["ndx_mask"].shape == (5, 10)
    assert fx["scores_checked"].shape == fx["scores_unchecked"].shape == (4, 9) and not fx["ndx_mask"][:4, :9].all()
    for a, r in ((fx["A_F"], fx["R_F"]), (fx["A_G"], fx["R_G"])):
        assert max(numpy.linalg.cond(m) for m in a) <= 1e4 and numpy.linalg.cond(r) <= 1e4
    sigma = 1.0 / fx["invcov"].reshape(-1)
    W = numpy.hstack((fx["F"], fx["G"])) / numpy.sqrt(sigma)[:, None]
    lam = numpy.eye(RANK_F + RANK_G)[None] + ivn.unpack(fx["stat0"].dot(ivn.gram(W, C, D)), RANK_F + RANK_G)
    assert max(numpy.linalg.cond(m) for m in lam) <= 1e3


def test_restatement_matches_the_reference_fixture(fx):
    ours = jfn.restated(fx)
    errs = {k: jfn.rel(ours[k], fx[k]) for k in jfn.RECORDED if fx[k].size}
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert len(errs) == len(jfn.RECORDED) - 2   # the two empty estimates: x without U, y without V
    for k, v in errs.items():
        assert v < RESTATEMENT_TOL, f"{k} differs by {v:.3e} (relative max-norm, bound {RESTATEMENT_TOL})"
    for k in ("hid_v_x", "hid_u_y"):
        assert ours[k].shape == fx[k].shape


def test_reference_parameter_lists():
    expect = {"subtract_weighted_stat1": "(self, sts)",
              "estimate_between_class": "(self, itNb, V, mean, sigma_obs, batch_size=100, Ux=None, Dz=None, minDiv=True, num_thread=1, "
                                        "re_estimate_residual=False, save_partial=False)",
              "estimate_within_class": "(self, it_nb, U, mean, sigma_obs, batch_size=100, Vy=None, Dz=None, min_div=True, num_thread=1, "
                                       "save_partial=False)",
              "estimate_map": "(self, itNb, D, mean, Sigma, Vy=None, Ux=None, num_thread=1, save_partial=False)",
              "estimate_hidden": "(self, mean, sigma, V=None, U=None, D=None, batch_size=100, num_thread=1)",
              "factor_analysis": "(self, rank_f, rank_g=0, rank_h=None, re_estimate_residual=False, it_nb=(10, 10, 10), min_div=True, ubm=None, "
                                 "batch_size=100, num_thread=1, save_partial=False, init_matrices=(None, None, None))"}
    for name, sig in expect.items():
        assert str(inspect.signature(getattr(StatServer, name))) == sig, name
    module = {"jfa_scoring": "(ubm, enroll, test, ndx, mean, sigma, V, U, D, batch_size=100, num_thread=1, check_missing=True)",
              "jfa_shift_device": "(stat0, stat1, W=None, H=None, rows=None, mean=None, scale=None, out=None)",
              "estimate_hidden_device": "(stat0, stat1, mean, sigma, V=None, U=None, D=None, max_workspace_bytes=1073741824)",
              "factor_analysis_device": "(stat0, stat1, model_index, ubm, rank_f, rank_g=0, rank_h=None, it_nb=(10, 10, 10), min_div=True, "
                                        "init_matrices=(None, None, None), max_workspace_bytes=1073741824)",
              "jfa_score_device": "(ubm, enroll_stat0, enroll_stat1, test_stat0, test_stat1, mean, sigma, V, U, D)"}
    for name, sig in module.items():
        assert str(inspect.signature(getattr(jfa_scoring, name))) == sig, name


def test_mirror_wiring():
    import sidekit_amd
    assert "jfa_scoring" in sidekit_amd.SUBMODULES
    code = ("import sidekit_amd; sidekit_amd.install_as_sidekit(); from sidekit.jfa_scoring import jfa_scoring; "
            "import sidekit_amd.jfa_scoring as m; assert jfa_scoring is m.jfa_scoring; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_importing_the_module_loads_neither_torch_nor_the_library():
    code = ("import sys; import sidekit_amd.jfa_scoring, sidekit_amd._lib as l; "
            "assert 'torch' not in sys.modules and l._lib is None; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_header_binding_table_and_library_agree():
    """What tests/test_abi.py checks for include/sidekit_amd.h, for the JFA header and table."""
    import ctypes
    import re
    src = open(os.path.join(ROOT, "include", "sidekit_amd", "jfa.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?(?:int|char\s*\*|void)\s*\**\s*((?:xt|sc|sk)_\w+)\s*\(", src, flags=re.M)))
    assert declared == ["sc_jfa_map_acc", "sc_jfa_shift"]
    assert sorted(_lib.JFA_SIGNATURES) == declared, "ctypes binding table and header disagree"
    others = (_lib.SIGNATURES, _lib.GAUSSIAN_SIGNATURES, _lib.MIXTURE_SIGNATURES, _lib.IVECTOR_SIGNATURES, _lib.GMM_SCORING_SIGNATURES,
              _lib.FEATURES_SIGNATURES, _lib.CEPSTRUM_SIGNATURES)
    assert not any(set(_lib.JFA_SIGNATURES) & set(t) for t in others)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(cdll, name), f"{name} declared in include/sidekit_amd/jfa.h but not exported"
    lib = _lib.lib()
    for name, (res, args) in _lib.JFA_SIGNATURES.items():
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    ctype = {"void*": _lib._P, "int32_t": _lib._I32, "int64_t": _lib._I64, "double": _lib._F64}
    flat = re.sub(r"\s+", " ", src)
    for name, (_, args) in _lib.JFA_SIGNATURES.items():
        params = re.search(r"int %s\((.*?)\);" % name, flat).group(1).split(",")
        kinds = ["void*" if "*" in q else q.replace("const", "").split()[0] for q in params]
        assert [ctype[k] for k in kinds] == args, (name, kinds)
    assert int(re.search(r"#define SC_JFA_MAP_SLAB (\d+)", src).group(1)) == 256
    assert jfa_scoring.TV_MAX_RANK == 192


def test_entry_points_check_their_arguments_before_anything_is_enqueued():
    """SK_EARG through the C ABI on a host with no GPU: nothing was enqueued, or there would have been a HIP error instead."""
    lib = _lib.lib()
    p = 4096   # any non-null address: a refused call dereferences nothing

    def shift(stat1=p, stat0=p, N=3, C=2, D=4, W=p, H=p, Nh=3, R=5, row=p, mean=p, scale=p, out=p):
        return lib.sc_jfa_shift(stat1, stat0, N, C, D, W, H, Nh, R, row, mean, scale, out, None)

    def acc(stat0=p, stat1=p, M=3, C=2, D=4, Dv=p, Sigma=p, A=p, Cacc=p):
        return lib.sc_jfa_map_acc(stat0, stat1, M, C, D, Dv, Sigma, A, Cacc, None)

    cases = {"shift stat1 null": shift(stat1=None), "shift stat0 null": shift(stat0=None), "shift out null": shift(out=None),
             "shift R = 193": shift(R=193), "shift R < 0": shift(R=-1), "shift N = 0": shift(N=0), "shift N < 0": shift(N=-2),
             "shift C = 0": shift(C=0), "shift C < 0": shift(C=-1), "shift D = 0": shift(D=0), "shift D < 0": shift(D=-1),
             "shift W null with R > 0": shift(W=None), "shift H null with R > 0": shift(H=None), "shift both null with R > 0": shift(W=None, H=None),
             "shift Nh = 0 with R > 0": shift(Nh=0), "shift W with R = 0": shift(R=0, H=None), "shift H with R = 0": shift(R=0, W=None),
             "shift W and H with R = 0": shift(R=0),
             "acc stat0 null": acc(stat0=None), "acc stat1 null": acc(stat1=None), "acc D null": acc(Dv=None), "acc Sigma null": acc(Sigma=None),
             "acc A null": acc(A=None), "acc Cacc null": acc(Cacc=None), "acc M = 0": acc(M=0), "acc M < 0": acc(M=-1), "acc C = 0": acc(C=0),
             "acc C < 0": acc(C=-4), "acc D = 0": acc(D=0), "acc D < 0": acc(D=-1)}
    assert all(rc == _lib.SK_EARG for rc in cases.values()), cases
    assert "sc_jfa_map_acc" in _lib.last_error()
    assert shift(R=-1) == _lib.SK_EARG and "sc_jfa_shift" in _lib.last_error()


def _jfa_arguments(fx):
    return fx["mu"].reshape(-1), 1.0 / fx["invcov"].reshape(-1), fx["F"], fx["G"], fx["H"]


def _scoring_set(fx):
    enroll = _server([f"m{s}" for s in fx["enroll_of"]], [f"e{i}" for i in range(6)], fx["enroll_stat0"], fx["enroll_stat1"])
    test = _server([f"t{i}" for i in range(9)], [f"t{i}" for i in range(9)], fx["test_stat0"], fx["test_stat1"])
    ndx = Ndx()
    ndx.modelset = numpy.array(["m0", "m1", "m2", "m3", "m_missing"], dtype="|O")
    ndx.segset = numpy.array([f"t{i}" for i in range(9)] + ["t_missing"], dtype="|O")
    ndx.trialmask = fx["ndx_mask"].copy()
    return enroll, test, ndx


def test_refusals(fx):
    ubm, server = _ubm(fx), _training_server(fx)
    mean, sigma, F, G, H = _jfa_arguments(fx)
    init = (fx["F_init"], fx["G_init"], fx["H_init"])
    enroll, test, ndx = _scoring_set(fx)
    refused = {
        "ubm=None": lambda: server.factor_analysis(RANK_F, RANK_G, True, it_nb=(1, 1, 1), init_matrices=init),
        "ubm=None, device": lambda: jfa_scoring.factor_analysis_device(None, None, None, None, RANK_F),
        "2-D sigma, hidden": lambda: server.estimate_hidden(mean, numpy.diag(sigma), F, G, H),
        "2-D sigma, hidden on the device": lambda: jfa_scoring.estimate_hidden_device(None, None, mean, numpy.diag(sigma), F),
        "2-D sigma, between": lambda: server.estimate_between_class(1, F, mean, numpy.diag(sigma)),
        "2-D sigma, within": lambda: server.estimate_within_class(1, G, mean, numpy.diag(sigma)),
        "2-D sigma, map": lambda: server.estimate_map(1, H, mean, numpy.diag(sigma)),
        "2-D sigma, scoring": lambda: jfa_scoring.jfa_scoring(ubm, enroll, test, ndx, mean, numpy.diag(sigma), F, G, H),
        "re_estimate_residual": lambda: server.factor_analysis(RANK_F, RANK_G, True, True, (1, 1, 1), True, ubm, init_matrices=init),
        "re_estimate_residual, between": lambda: server.estimate_between_class(1, F, mean, sigma, re_estimate_residual=True),
        "save_partial": lambda: server.factor_analysis(RANK_F, RANK_G, True, False, (1, 1, 1), True, ubm, save_partial="partial", init_matrices=init),
        "save_partial, between": lambda: server.estimate_between_class(1, F, mean, sigma, save_partial=True),
        "save_partial, within": lambda: server.estimate_within_class(1, G, mean, sigma, save_partial="partial"),
        "save_partial, map": lambda: server.estimate_map(1, H, mean, sigma, save_partial="partial"),
    }
    for name, call in refused.items():
        with pytest.raises(NotImplementedError):
            call()
    full = _ubm(fx)
    full.invcov = numpy.stack([numpy.diag(v) for v in full.invcov])
    assert full.validate()
    for call in (lambda: server.factor_analysis(RANK_F, RANK_G, True, it_nb=(1, 1, 1), ubm=full, init_matrices=init),
                 lambda: jfa_scoring.factor_analysis_device(None, None, None, full, RANK_F),
                 lambda: jfa_scoring.jfa_scoring(full, enroll, test, ndx, mean, sigma, F, G, H),
                 lambda: jfa_scoring.jfa_score_device(full, None, None, None, None, mean, sigma, F, G, H)):
        with pytest.raises(NotImplementedError, match="full-covariance"):
            call()
    wide = numpy.zeros((C * D, 193))
    for call in (lambda: server.factor_analysis(193, RANK_G, True, ubm=ubm), lambda: server.factor_analysis(RANK_F, 193, True, ubm=ubm),
                 lambda: jfa_scoring.factor_analysis_device(None, None, None, ubm, 193),
                 lambda: jfa_scoring.factor_analysis_device(None, None, None, ubm, RANK_F, 193),
                 lambda: server.estimate_hidden(mean, sigma, wide), lambda: server.estimate_hidden(mean, sigma, None, wide),
                 lambda: server.estimate_hidden(mean, sigma, wide[:, :100], wide[:, :93]),
                 lambda: jfa_scoring.estimate_hidden_device(None, None, mean, sigma, wide[:, :100], wide[:, :93]),
                 lambda: server.estimate_between_class(1, wide, mean, sigma), lambda: server.estimate_within_class(1, wide, mean, sigma),
                 lambda: jfa_scoring.jfa_scoring(ubm, enroll, test, ndx, mean, sigma, wide[:, :100], wide[:, :93], H),
                 lambda: jfa_scoring.jfa_score_device(ubm, None, None, None, None, mean, sigma, wide, G, H)):
        with pytest.raises(ValueError, match="192"):
            call()
    numpy.testing.assert_array_equal(server.stat1, fx["stat1"])
    numpy.testing.assert_array_equal(enroll.stat1, fx["enroll_stat1"])


def test_without_a_gpu_everything_raises(fx, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    ubm, server = _ubm(fx), _training_server(fx)
    mean, sigma, F, G, H = _jfa_arguments(fx)
    enroll, test, ndx = _scoring_set(fx)
    init = (fx["F_init"], fx["G_init"], fx["H_init"])
    for call in (lambda: server.factor_analysis(RANK_F, RANK_G, True, it_nb=(1, 1, 1), ubm=ubm, init_matrices=init),
                 lambda: server.estimate_hidden(mean, sigma, F, G, H), lambda: server.estimate_between_class(1, F, mean, sigma),
                 lambda: server.estimate_within_class(1, G, mean, sigma), lambda: server.estimate_map(1, H, mean, sigma),
                 lambda: jfa_scoring.jfa_scoring(ubm, enroll, test, ndx, mean, sigma, F, G, H),
                 lambda: jfa_scoring.jfa_shift_device(None, None)):
        with pytest.raises(RuntimeError, match="no GPU is visible"):
            call()
    numpy.testing.assert_array_equal(server.stat1, fx["stat1"])


def test_subtract_weighted_stat1_against_the_fixture_and_its_incompatibility(fx):
    """The fixture's z is f D / (1 + n D^2) with f the whitened statistics less n (W [y x]): the same subtraction, from the recorded
    y and x, through the method; and the alignment by sorted segset with the sessions of the second server in another order."""
    server = _training_server(fx)
    mean, sigma, F, G, H = _jfa_arguments(fx)
    n = server.stat0.shape[0]
    white = _training_server(fx)
    white.whiten_stat1(mean, sigma)
    supervectors = _training_server(fx)
    supervectors.stat1 = numpy.hstack((fx["hid_vud_y"], fx["hid_vud_x"])).dot(numpy.hstack((F, G)).T)
    order = numpy.random.RandomState(0).permutation(n)
    shuffled = _server(supervectors.modelset[order], supervectors.segset[order], supervectors.stat0[order], supervectors.stat1[order])
    keep = white.stat1.copy()
    out = white.subtract_weighted_stat1(shuffled)
    assert out is not white and numpy.array_equal(white.stat1, keep) and numpy.array_equal(out.stat0, white.stat0)
    numpy.testing.assert_array_equal(out.stat1, white.subtract_weighted_stat1(supervectors).stat1)
    numpy.testing.assert_array_equal(out.stat1, white.stat1 - numpy.repeat(white.stat0, D, axis=1) * supervectors.stat1)
    z = out.stat1 * H / (1.0 + numpy.repeat(white.stat0, D, axis=1) * H ** 2)
    err = jfn.rel(z, fx["hid_vud_z"])
    print(f"z from subtract_weighted_stat1: {err:.2e}")
    assert err < RESTATEMENT_TOL
    fewer = _server(server.modelset[:-1], server.segset[:-1], server.stat0[:-1], server.stat1[:-1])
    renamed = _training_server(fx)
    renamed.segset = renamed.segset.copy()
    renamed.segset[3] = "elsewhere"
    other_model = _training_server(fx)
    other_model.modelset = other_model.modelset.copy()
    other_model.modelset[0] = "nobody"
    narrower = _server(server.modelset, server.segset, server.stat0, server.stat1[:, :-D])
    for bad in (fewer, renamed, other_model, narrower):
        with pytest.raises(Exception, match="Statserver are not compatible"):
            server.subtract_weighted_stat1(bad)
