"""The SVM back end without a GPU (sidekit_amd/svm_training.py, svm_scoring.py, sv_utils.py, the SVM methods of StatServer,
csrc/svm.hip): the numpy restatement the GPU tests lean on against libsvm and the reference's own modules (tests/golden/svm.npz, written
by make_svm_golden.py), the reference's signatures, the model files, the ``sidekit`` aliases, the entry point's header against its binding
table and the built library, and its argument checks through the C ABI.

A model's bar is ``max(10 d, 1e-12)`` with the ``d`` the generator measured between the restatement and libsvm on that model
(tests/tools/svm_fixture.py, make_svm_golden.py's docstring has the reasoning).
"""
import gzip
import inspect
import os
import pickle
import subprocess
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import svm_fixture as sfx  # noqa: E402
import svm_numpy as svn  # noqa: E402

from sidekit_amd import _lib, sv_utils, svm_scoring, svm_training  # noqa: E402
from sidekit_amd.statserver import StatServer  # noqa: E402


@pytest.fixture(scope="module")
def fx(golden_dir):
    return sfx.load(golden_dir)


@pytest.mark.parametrize("tag", sfx.SETS)
def test_restatement_matches_libsvm(fx, tag):
    p = sfx.problem(fx, tag)
    M = len(p["names"])
    W, b = numpy.zeros_like(p["W"]), numpy.zeros(M)
    for m in range(M):
        W[m], b[m], out = svn.train(p["bg"], p["en"][p["model_of"] == m], p["c"][m], eps=1e-12)
        assert out["status"] == svn.CONVERGED and out["iterations"] == fx[f"{tag}_iterations"][m] and out["tau_steps"] == fx[f"{tag}_tau_steps"][m]
        a = numpy.abs(out["coef"])
        assert ((a > 0) & (a < p["c"][m])).sum() == fx[f"{tag}_free"][m] and (a >= p["c"][m]).sum() == fx[f"{tag}_at_c"][m]
    sfx.assert_within_bars(tag, p, W, b)


def test_fixture_holds_the_cases_it_was_built_for(fx):
    assert fx["nofree_free"][0] == 0 and fx["nofree_at_c"][0] == 8, "no free variable: rho is the midpoint of the bounds"
    assert fx["twin_tau_steps"][0] > 0, "a pair of curvature 0 is selected: the tau branch"
    assert [fx[f"n{n}_bg"].shape[0] + 1 for n in (255, 256, 257)] == [255, 256, 257]
    assert sorted(set(numpy.bincount(fx["batch7_model_of"]))) == [1, 2, 5] and fx["batch7_bg"].shape[0] == 33
    assert fx["n2_bg"].shape[0] == 1 and fx["n2_en"].shape[0] == 1
    for tag in sfx.SETS:
        assert max(fx[f"{tag}_d_w"].max(), fx[f"{tag}_d_b"].max()) <= 1e-5, "the generator refuses a loose problem"
    for tag in ("eq1", "eq3", "batch7"):   # the default cost is the reference's
        p = sfx.problem(fx, tag)
        for m in range(len(p["names"])):
            assert p["c"][m] == svn.default_c(svn.gram(p["bg"], p["en"][p["model_of"] == m]))


def test_default_tolerance_satisfies_the_stopping_rule(fx):
    """what the GPU test asks of the device's coefficients at eps = 1e-3, asked of the restatement"""
    p = sfx.problem(fx, "batch7")
    for m in range(7):
        own = p["en"][p["model_of"] == m]
        _, b, out = svn.train(p["bg"], own, p["c"][m])
        assert out["status"] == svn.CONVERGED
        sfx.assert_solves(svn.gram(p["bg"], own), 33, out["coef"], b, p["c"][m], 1e-3, out["iterations"])


def test_max_iter_is_a_status_not_an_error(fx):
    p = sfx.problem(fx, "n257")
    _, _, out = svn.train(p["bg"], p["en"], p["c"][0], max_iter=3)
    assert out["status"] == svn.MAX_ITER and out["iterations"] == 3 and out["gap"] >= 1e-3


def test_scores_and_nap_match_the_reference_fixture(fx):
    for tag in ("eq3", "batch7"):
        p = sfx.problem(fx, tag)
        order = [p["names"].index(n) for n in fx[f"{tag}_score_modelset"]]
        assert "ghost" in fx[f"{tag}_ndx_modelset"] and "ghost" not in fx[f"{tag}_score_modelset"]
        assert "absent" in fx[f"{tag}_ndx_segset"] and "absent" not in fx[f"{tag}_score_segset"]
        assert not fx[f"{tag}_scoremask"].all() and numpy.all(fx[f"{tag}_scoremat"][~fx[f"{tag}_scoremask"]] == 0)
        want = svn.scores(p["W"][order], p["b"][order], fx[f"{tag}_test"] / sfx.SCALE, fx[f"{tag}_scoremask"])
        assert numpy.abs(want - fx[f"{tag}_scoremat"]).max() <= 1e-12 * numpy.abs(want).max()
    stat1 = fx["nap_q"] / sfx.SCALE
    assert stat1.shape == (20, 12) and fx["nap_N"].shape == (12, 3)
    N = svn.nap_matrix(stat1, 3)
    sign = numpy.sign((N * fx["nap_N"]).sum(axis=0))
    assert numpy.abs(N * sign - fx["nap_N"]).max() <= 1e-10 * numpy.abs(fx["nap_N"]).max(), "NAP columns, up to their signs"
    assert numpy.abs(N @ N.T - fx["nap_N"] @ fx["nap_N"].T).max() <= 1e-10 * numpy.abs(fx["nap_N"] @ fx["nap_N"].T).max(), "N N'"


def test_reference_signatures():
    assert str(inspect.signature(svm_training.svm_training)) == "(svmDir, background_sv, enroll_sv, num_thread=1)"
    assert str(inspect.signature(svm_training.svm_training_singleThread)) == "(K, msn, bsn, svm_dir, background_sv, models, enroll_sv)"
    assert str(inspect.signature(svm_training.svm_train_device)) == "(background, enroll, model_of, c=None, eps=0.001, max_iter=100000)"
    assert str(inspect.signature(svm_scoring.svm_scoring)) == "(svm_filename_structure, test_sv, ndx, num_thread=1)"
    assert str(inspect.signature(svm_scoring.svm_scoring_singleThread)) == "(svm_filename_structure, test_sv, ndx, score, seg_idx=None)"
    assert str(inspect.signature(svm_scoring.svm_score_device)) == "(W, b, test)"
    assert str(inspect.signature(sv_utils.save_svm)) == "(svm_file_name, w, b)"
    assert str(inspect.signature(sv_utils.read_svm)) == "(svm_file_name)"
    assert str(inspect.signature(sv_utils.check_file_list)) == "(input_file_list, file_name_structure)"
    assert str(inspect.signature(StatServer.precompute_svm_kernel_stat1)) == "(self)"
    assert str(inspect.signature(StatServer.get_nap_matrix_stat1)) == "(self, co_rank)"
    assert str(inspect.signature(StatServer.get_model_segments)) == "(self, mod_id)"


def test_model_files_round_trip_and_are_the_reference_format(fx, tmp_path):
    w, b = fx["eq3_W"][1], float(fx["eq3_b"][1])
    name = str(tmp_path / "new_dir" / "spk.svm")    # the directory is created
    sv_utils.save_svm(name, w[:, None], b)           # the reference saves a (D, 1) column
    with gzip.open(name, "rb") as f:                 # what the reference's reader does
        stored = pickle.load(f)
    assert isinstance(stored, tuple) and len(stored) == 2 and numpy.array_equal(stored[0], w[:, None]) and stored[1] == b
    w2, b2 = sv_utils.read_svm(name)
    assert w2.shape == w.shape and numpy.array_equal(w2, w) and b2 == b
    ref = str(tmp_path / "reference.svm")            # a file the reference wrote
    open(ref, "wb").write(fx["eq3_ref_svm_file"].tobytes())
    w3, b3 = sv_utils.read_svm(ref)
    assert numpy.array_equal(w3, fx["eq3_W"][0]) and b3 == fx["eq3_b"][0]


def test_check_file_list(tmp_path):
    names = numpy.array(["a", "b", "c", "d"], dtype="|O")
    for n in ("b", "d"):
        sv_utils.save_svm(str(tmp_path / f"{n}.svm"), numpy.zeros(2), 0.0)
    out, idx = sv_utils.check_file_list(names, str(tmp_path / "{}.svm"))
    assert list(out) == ["b", "d"] and list(idx) == [1, 3] and numpy.array_equal(names[idx], out)
    out, idx = sv_utils.check_file_list(names, str(tmp_path / "none" / "{}.svm"))
    assert out.shape == (0,) and idx.shape == (0,)


def test_get_model_segments(fx):
    s = StatServer()
    s.modelset = numpy.array([fx["eq3_names"][m] for m in fx["eq3_model_of"]], dtype="|O")
    s.segset = numpy.array([f"eq3_s{i}" for i in range(9)], dtype="|O")
    assert list(s.get_model_segments("eq3_m1")) == list(fx["eq3_segments_of_m1"]) and s.get_model_segments("nobody").shape == (0,)


def test_import_loads_neither_torch_nor_the_library():
    code = ("import sys, sidekit_amd.svm_training, sidekit_amd.svm_scoring, sidekit_amd.sv_utils, sidekit_amd._lib as l; "
            "assert 'torch' not in sys.modules and l._lib is None, sorted(m for m in sys.modules if m.startswith('torch'))[:3]")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_install_as_sidekit_resolves_the_svm_modules():
    import sidekit_amd
    assert {"svm_training", "svm_scoring", "sv_utils"} <= set(sidekit_amd.SUBMODULES)
    saved = {k: v for k, v in sys.modules.items() if k == "sidekit" or k.startswith("sidekit.")}
    try:
        sidekit_amd.install_as_sidekit()
        import sidekit.sv_utils
        import sidekit.svm_scoring
        import sidekit.svm_training
        from sidekit.svm_training import svm_training as aliased   # the reference's own import line
        assert sys.modules["sidekit.svm_training"] is svm_training and aliased is svm_training.svm_training
        assert sys.modules["sidekit.svm_scoring"] is svm_scoring and sys.modules["sidekit.sv_utils"] is sv_utils
    finally:
        for k in [k for k in sys.modules if k == "sidekit" or k.startswith("sidekit.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_header_binding_table_and_library_agree():
    """What tests/test_abi.py checks for include/sidekit_amd.h, for the SVM entry point's own header and table."""
    import ctypes
    import re
    src = open(os.path.join(ROOT, "include", "sidekit_amd", "svm.h")).read()
    macros = src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?(?:int|char\s*\*|void)\s*\**\s*((?:xt|sc|sk)_\w+)\s*\(", src, flags=re.M)))
    assert declared == ["sc_svm_train"]
    assert sorted(_lib.SVM_SIGNATURES) == declared, "ctypes binding table and header disagree"
    others = (_lib.SIGNATURES, _lib.GAUSSIAN_SIGNATURES, _lib.MIXTURE_SIGNATURES, _lib.IVECTOR_SIGNATURES, _lib.GMM_SCORING_SIGNATURES,
              _lib.JFA_SIGNATURES, _lib.FEATURES_SIGNATURES, _lib.CEPSTRUM_SIGNATURES)
    assert not any(set(_lib.SVM_SIGNATURES) & set(t) for t in others)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(cdll, name), f"{name} declared in include/sidekit_amd/svm.h but not exported"
    lib = _lib.lib()
    for name, (res, args) in _lib.SVM_SIGNATURES.items():
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    ctype = {"void*": _lib._P, "int32_t": _lib._I32, "int64_t": _lib._I64, "double": _lib._F64}
    flat = re.sub(r"\s+", " ", src)
    for name, (_, args) in _lib.SVM_SIGNATURES.items():
        params = re.search(r"int %s\((.*?)\);" % name, flat).group(1).split(",")
        kinds = ["void*" if "*" in q else q.replace("const", "").split()[0] for q in params]
        assert [ctype[k] for k in kinds] == args, (name, kinds)
    lds, reserved = (int(re.search(r"#define %s (\d+)" % k, macros).group(1)) for k in ("SC_SVM_LDS_BYTES", "SC_SVM_LDS_RESERVED"))
    assert lds == 160 * 1024 and "#define SC_SVM_MAX_N ((SC_SVM_LDS_BYTES - SC_SVM_LDS_RESERVED) / 24)" in macros
    assert (lds - reserved) // 24 == _lib.SC_SVM_MAX_N == svm_training.MAX_N == 6784
    for k, v in (("SC_SVM_CONVERGED", _lib.SC_SVM_CONVERGED), ("SC_SVM_MAX_ITER", _lib.SC_SVM_MAX_ITER), ("SC_SVM_BAD_OFFSETS", _lib.SC_SVM_BAD_OFFSETS)):
        assert int(re.search(r"#define %s (\d+)" % k, macros).group(1)) == v
    assert "LARGEST index" in macros and "LARGEST index" in svn.__doc__, "the header and the restatement state the same tie rule"


def test_entry_point_checks_its_arguments_before_anything_is_enqueued():
    """SK_EARG through the C ABI on a host with no GPU: nothing was enqueued, or there would have been a HIP error instead."""
    lib = _lib.lib()
    p = 4096   # any non-null address: a refused call dereferences nothing

    def train(Kbb=p, B=8, Keb=p, Ne=3, Kee=p, ee_len=3, en_off=p, ee_off=p, M=3, max_csn=1, C=p, eps=1e-3, max_iter=100, coef=p, rho=p,
              iters=p, gap=p, status=p):
        return lib.sc_svm_train(Kbb, B, Keb, Ne, Kee, ee_len, en_off, ee_off, M, max_csn, C, eps, max_iter, coef, rho, iters, gap, status, None)

    cases = {"K_bb null": train(Kbb=None), "K_eb null": train(Keb=None), "K_ee null": train(Kee=None), "en_off null": train(en_off=None),
             "ee_off null": train(ee_off=None), "C null": train(C=None), "coef null": train(coef=None), "rho null": train(rho=None),
             "iters null": train(iters=None), "gap null": train(gap=None), "status null": train(status=None),
             "B = 0": train(B=0), "B < 0": train(B=-1), "M = 0": train(M=0), "M < 0": train(M=-2), "Ne = 0": train(Ne=0),
             "max_csn = 0": train(max_csn=0), "ee_len = 0": train(ee_len=0),
             "n = MAX_N + 1": train(B=_lib.SC_SVM_MAX_N, max_csn=1), "n = MAX_N + 1 by csn": train(B=1, max_csn=_lib.SC_SVM_MAX_N),
             "n overflows int32": train(B=2 ** 31 - 1, max_csn=2 ** 31 - 1),
             "eps = 0": train(eps=0.0), "eps < 0": train(eps=-1e-3), "eps nan": train(eps=float("nan")),
             "max_iter = 0": train(max_iter=0), "max_iter < 0": train(max_iter=-5)}
    assert all(rc == _lib.SK_EARG for rc in cases.values()), cases
    assert "sc_svm_train" in _lib.last_error()


def test_compute_calls_need_a_gpu(fx):
    import torch
    assert not torch.cuda.is_available()
    p = sfx.problem(fx, "n2")
    s = StatServer()
    s.stat1 = p["bg"]
    for call, module in ((lambda: svm_training.svm_train_device(p["bg"], p["en"], p["model_of"]), "svm_training"),
                         (lambda: svm_scoring.svm_score_device(p["W"], p["b"], p["en"]), "svm_scoring"),
                         (lambda: s.precompute_svm_kernel_stat1(), "svm_training"), (lambda: s.get_nap_matrix_stat1(1), "svm_training")):
        with pytest.raises(RuntimeError, match=f"sidekit_amd.{module} computes on the GPU only"):
            call()
