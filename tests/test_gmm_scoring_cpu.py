"""GMM-UBM verification without a GPU (sidekit_amd/gmm_scoring.py, StatServer.adapt_mean_map*, csrc/gmm_score.hip): MAP adaptation on the
host and the numpy restatement the GPU tests lean on against the reference's own output (tests/golden/gmm_scoring.npz, written by
make_gmm_scoring_golden.py from the imported reference modules), the reference's signatures, the refusals, the ``sidekit`` alias, the
entry point's own header against its binding table and the built library, and its argument checks through the C ABI.

The restatement and the host methods are held to 1e-12 relative max-norm, the bar make_backend_golden.py sets for float64 algebra
restated in numpy (the generator measured 0 on this set: the same operations in the same order).
"""
import inspect
import os
import subprocess
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gmm_scoring_numpy as gsn  # noqa: E402
import mixture_numpy as mxn  # noqa: E402

from sidekit_amd import _lib, gmm_scoring  # noqa: E402
from sidekit_amd.bosaris import Ndx  # noqa: E402
from sidekit_amd.mixture import Mixture  # noqa: E402
from sidekit_amd.statserver import StatServer  # noqa: E402

RESTATEMENT_TOL = 1e-12
KEYS = ("w", "mu", "invcov", "cov_var_ctl")
SETTINGS = ((16, False, "map_r16_plain"), (16, True, "map_r16_norm"), (0.5, False, "map_r0p5_plain"), (0.5, True, "map_r0p5_norm"))


@pytest.fixture(scope="module")
def fx(golden_dir):
    out = dict(numpy.load(os.path.join(golden_dir, "gmm_scoring.npz")))
    out.update({"mix_" + k: v for k, v in numpy.load(os.path.join(golden_dir, "mixture.npz")).items()})
    return out


def _ubm(fx):
    m = Mixture()
    m.w, m.mu, m.invcov, m.cov_var_ctl = (numpy.array(fx[f"mix_split4_{k}"], dtype=numpy.float64) for k in KEYS)
    m.cst, m.det = numpy.zeros(m.w.shape), numpy.zeros(m.w.shape)
    m._compute_all()
    return m


def _server(fx):
    s = StatServer()
    s.modelset, s.segset = fx["modelset"].astype("|O"), fx["segset"].astype("|O")
    s.start, s.stop = numpy.empty(8, dtype="|O"), numpy.empty(8, dtype="|O")
    s.stat0, s.stat1 = fx["stat0"].copy(), fx["stat1"].copy()
    return s


def _assert_all(errs, tol=RESTATEMENT_TOL):
    print({k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < tol, f"{k} differs by {v:.3e} (relative max-norm, bound {tol})"


def test_map_adaptation_matches_the_reference_fixture(fx):
    ubm, server = _ubm(fx), _server(fx)
    errs = {}
    for r, norm, tag in SETTINGS:
        out = server.adapt_mean_map(ubm, r, norm)
        assert out.validate() and out.stat0.shape == (8, 1) and numpy.all(out.stat0 == 1) and out.stat1.shape == (8, 8 * 23) and out.stat1.dtype == numpy.float64
        assert list(out.modelset) == list(server.modelset) and list(out.segset) == list(server.segset)
        errs[tag] = mxn.rel(out.stat1, fx[tag])
    # the session without a frame: 0 / 0 is 0, and alpha = eps / (eps + r) of the float32 eps, as the reference has it
    assert numpy.all(server.stat0[2] == 0)
    eps = float(numpy.finfo(numpy.float32).eps)
    numpy.testing.assert_array_equal(server.adapt_mean_map(ubm, 16).stat1[2], (1 - eps / (eps + 16)) * ubm.get_mean_super_vector())
    multi = server.adapt_mean_map_multisession(ubm, 16)
    assert multi.validate() and list(multi.modelset) == list(multi.segset) == list(fx["multi_modelset"]) == ["spk0", "spk1", "spk2", "spk3"]
    assert multi.stat0.shape == (4, 1) and numpy.all(multi.stat0 == 1) and multi.start.shape == multi.stop.shape == (4,)
    errs["multisession"] = mxn.rel(multi.stat1, fx["multi_stat1"])
    _assert_all(errs)
    assert mxn.rel(server.adapt_mean_map_multisession(ubm, 16, True).stat1,
                   gsn.adapt_mean_map_multisession(mxn.model(*(fx[f"mix_split4_{k}"] for k in KEYS)), fx["modelset"], fx["stat0"], fx["stat1"], 16, True)[1]) < RESTATEMENT_TOL
    assert str(inspect.signature(StatServer.adapt_mean_map)) == "(self, ubm, r=16, norm=False)"
    assert str(inspect.signature(StatServer.adapt_mean_map_multisession)) == "(self, ubm, r=16, norm=False)"


def test_restatement_matches_the_reference_fixture(fx):
    m = mxn.model(*(fx[f"mix_split4_{k}"] for k in KEYS))
    X, off = fx["mix_X"], fx["mix_seg_off"]
    errs = {tag: mxn.rel(gsn.adapt_mean_map(m, fx["stat0"], fx["stat1"], r, norm), fx[tag]) for r, norm, tag in SETTINGS}
    ids, means = gsn.adapt_mean_map_multisession(m, fx["modelset"], fx["stat0"], fx["stat1"], 16, False)
    assert list(ids) == list(fx["multi_modelset"])
    errs["multisession"] = mxn.rel(means, fx["multi_stat1"])
    seg = [int(s[4:]) for s in fx["score_segset"]]
    order = [list(fx["enroll_modelset"]).index(n) for n in fx["score_modelset"]]
    sums, lens = gsn.llk(m, fx["enroll_stat1"][order], X, off)
    scale = numpy.abs(sums[:, seg] / lens[seg]).max()
    all_llr = gsn.llr(m, fx["enroll_stat1"][order], X, off)
    assert numpy.isnan(all_llr[:, 2]).all() and lens[2] == 0, "a trial on the empty segment is the mean of nothing"
    errs["scores over the largest mean llk"] = numpy.abs(all_llr[:, seg] - fx["scoremat"]).max() / scale
    errs["masked scores"] = numpy.abs(gsn.llr(m, fx["enroll_stat1"][order], X, off, None)[:, seg] * fx["masked_scoremask"] - fx["masked_scoremat"]).max() / scale
    _assert_all(errs)
    assert numpy.all(fx["scoremat"][list(fx["score_modelset"]).index("ubm")] == 0) and numpy.all(fx["masked_scoremat"][~fx["masked_scoremask"]] == 0)
    assert not fx["masked_scoremask"][list(fx["masked_modelset"]).index("spk1")].any() and not fx["masked_scoremask"][:, list(fx["masked_segset"]).index("show4")].any()


def test_reference_signatures():
    assert str(inspect.signature(gmm_scoring.gmm_scoring)) == "(ubm, enroll, ndx, feature_server, num_thread=1)"
    assert str(inspect.signature(gmm_scoring.gmm_scoring_singleThread)) == "(ubm, enroll, ndx, feature_server, score_mat, seg_idx=None)"
    assert str(inspect.signature(gmm_scoring.gmm_llk_device)) == "(ubm, models, frames, seg_off=None, mask=None, max_workspace_bytes=1073741824)"
    assert str(inspect.signature(gmm_scoring.gmm_llr_device)) == "(ubm, models, frames, seg_off=None, mask=None, max_workspace_bytes=1073741824)"
    assert str(inspect.signature(gmm_scoring.map_adapt_device)) == "(stat0, stat1, ubm, r=16, multisession_index=None)"


def test_full_covariance_and_wrong_types_are_refused(fx):
    ubm, server = _ubm(fx), _server(fx)
    enroll = server.adapt_mean_map_multisession(ubm)
    ndx = Ndx(models=numpy.repeat(enroll.modelset, 2), testsegs=numpy.tile(numpy.array(["show1", "show3"], dtype="|O"), 4))

    class Features:
        def load(self, show, channel=0):
            raise AssertionError("nothing is loaded for a refused call")

    for args, word in (((object(), enroll, ndx), "Mixture"), ((ubm, numpy.zeros(3), ndx), "StatServer"), ((ubm, enroll, "ndx.h5"), "Ndx")):
        with pytest.raises(AssertionError, match=word):
            gmm_scoring.gmm_scoring(*args, Features())
        with pytest.raises(AssertionError, match=word):
            gmm_scoring.gmm_scoring_singleThread(*args, Features(), numpy.zeros((4, 2)))
    full = _ubm(fx)
    full.invcov = numpy.stack([numpy.diag(v) for v in full.invcov])
    for call in (lambda: gmm_scoring.gmm_scoring(full, enroll, ndx, Features()),
                 lambda: gmm_scoring.gmm_scoring_singleThread(full, enroll, ndx, Features(), numpy.zeros((4, 2))),
                 lambda: gmm_scoring.gmm_llk_device(full, enroll.stat1, fx["mix_X"]), lambda: gmm_scoring.gmm_llr_device(full, enroll.stat1, fx["mix_X"]),
                 lambda: server.adapt_mean_map(full, norm=True), lambda: server.adapt_mean_map_multisession(full, norm=True)):
        with pytest.raises(NotImplementedError, match="full-covariance"):
            call()


def test_import_loads_neither_torch_nor_the_library():
    code = ("import sys, sidekit_amd.gmm_scoring, sidekit_amd._lib as l; "
            "assert 'torch' not in sys.modules and l._lib is None, sorted(m for m in sys.modules if m.startswith('torch'))[:3]")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_install_as_sidekit_resolves_gmm_scoring():
    import sidekit_amd
    assert "gmm_scoring" in sidekit_amd.SUBMODULES
    saved = {k: v for k, v in sys.modules.items() if k == "sidekit" or k.startswith("sidekit.")}
    try:
        sidekit_amd.install_as_sidekit()
        import sidekit.gmm_scoring
        from sidekit.gmm_scoring import gmm_scoring as aliased   # the reference's own import line
        assert sys.modules["sidekit.gmm_scoring"] is gmm_scoring and aliased is gmm_scoring.gmm_scoring
    finally:
        for k in [k for k in sys.modules if k == "sidekit" or k.startswith("sidekit.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_header_binding_table_and_library_agree():
    """What tests/test_abi.py checks for include/sidekit_amd.h, for the scoring entry point's own header and table."""
    import ctypes
    import re
    src = open(os.path.join(ROOT, "include", "sidekit_amd", "gmm_scoring.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?(?:int|char\s*\*|void)\s*\**\s*((?:xt|sc|sk)_\w+)\s*\(", src, flags=re.M)))
    assert declared == ["sc_gmm_score_models"]
    assert sorted(_lib.GMM_SCORING_SIGNATURES) == declared, "ctypes binding table and header disagree"
    assert not set(_lib.GMM_SCORING_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.GAUSSIAN_SIGNATURES) | set(_lib.MIXTURE_SIGNATURES) | set(_lib.IVECTOR_SIGNATURES))
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(cdll, name), f"{name} declared in include/sidekit_amd/gmm_scoring.h but not exported"
    lib = _lib.lib()
    for name, (res, args) in _lib.GMM_SCORING_SIGNATURES.items():
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    ctype = {"void*": _lib._P, "int32_t": _lib._I32, "int64_t": _lib._I64, "double": _lib._F64}
    flat = re.sub(r"\s+", " ", src)
    for name, (_, args) in _lib.GMM_SCORING_SIGNATURES.items():
        params = re.search(r"int %s\((.*?)\);" % name, flat).group(1).split(",")
        kinds = ["void*" if "*" in q else q.replace("const", "").split()[0] for q in params]
        assert [ctype[k] for k in kinds] == args, (name, kinds)
    assert int(re.search(r"#define SC_GMM_SCORE_MAX_M (\d+)", src).group(1)) == gmm_scoring.MAX_MODELS


def test_entry_point_checks_its_arguments_before_anything_is_enqueued():
    """SK_EARG through the C ABI on a host with no GPU: nothing was enqueued, or there would have been a HIP error instead."""
    lib = _lib.lib()
    p, F64, F32 = 4096, _lib.XT_F64, _lib.XT_F32   # any non-null address: a refused call dereferences nothing

    def score(X=p, dt=F32, N=5, D=4, mus=p, M=2, ic=p, B=p, C=3, off=p, S=1, max_len=5, mask=None, llk=p):
        return lib.sc_gmm_score_models(X, dt, N, D, mus, M, ic, B, C, off, S, max_len, mask, llk, None)

    cases = {"X null": score(X=None), "mus null": score(mus=None), "invcov null": score(ic=None), "B null": score(B=None), "seg_off null": score(off=None),
             "llk null": score(llk=None), "M = 0": score(M=0), "M < 0": score(M=-1), "M > grid": score(M=65536), "C = 0": score(C=0),
             "C > grid": score(C=65535 * 64 + 1), "D = 0": score(D=0), "D = 129": score(D=129), "N = 0": score(N=0), "N = 2^31": score(N=1 << 31),
             "S = 0": score(S=0), "bf16": score(dt=_lib.XT_BF16), "i64": score(dt=_lib.XT_I64), "f64 is fine, i16 is not": score(dt=_lib.XT_I16),
             "max_len < 0": score(max_len=-1), "max_len > N": score(max_len=6)}
    assert all(rc == _lib.SK_EARG for rc in cases.values()), cases
    assert "sc_gmm_score_models" in _lib.last_error()
