"""The Gaussian back-end without a GPU (sidekit_amd/lid_utils.py, csrc/gaussian_backend.hip): the numpy restatement the GPU tests lean
on against the reference's own output (tests/golden/gaussian_backend.npz, written by make_gaussian_backend_golden.py from the imported
reference module), the reference's signatures, the refusals that must come before any device is touched, the ``sidekit`` alias, the
entry points' own header against their binding table and the built library, and their argument checks through the C ABI.

The restatement is held to 1e-12 relative max-norm, the bar make_backend_golden.py sets for a restatement of float64 algebra (the
generator measured at most 4.3e-16 on this set).
"""
import inspect
import os
import subprocess
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gaussian_backend_numpy as gbn  # noqa: E402
import plda_em_numpy as pen  # noqa: E402

from sidekit_amd import _lib, lid_utils  # noqa: E402
from sidekit_amd.statserver import StatServer  # noqa: E402

RESTATEMENT_TOL = 1e-12


@pytest.fixture(scope="module")
def fx(golden_dir):
    return numpy.load(os.path.join(golden_dir, "gaussian_backend.npz"))


def _stat_server(ids, X):
    return StatServer.from_arrays(ids, numpy.array([f"seg{i:04d}" for i in range(X.shape[0])], dtype="|O"), X)


def test_restatement_matches_the_reference_fixture(fx):
    X, ids, T, alpha = fx["X"], fx["modelset"].astype("|O"), fx["T"], float(fx["alpha"])
    means, sigma, cst = gbn.train_tied(X, ids)
    hmeans, sigmas, csts = gbn.train_hetero(X, ids, alpha)
    numpy.testing.assert_array_equal(hmeans, means)
    errs = {"means": pen.rel(means, fx["means"]), "tied sigma": pen.rel(sigma, fx["tied_sigma"]), "tied cst": pen.rel(cst, fx["tied_cst"]),
            "hetero sigma": pen.rel(sigmas, fx["hetero_sigma"]), "hetero cst": pen.rel(csts, fx["hetero_cst"]),
            "tied ll": pen.rel(gbn.loglik(T, means, sigma, cst), fx["tied_ll"]),
            "hetero ll": pen.rel(gbn.loglik(T, means, sigmas, csts), fx["hetero_ll"]),
            "tied llr": pen.rel(gbn.closed_set_llr(fx["tied_ll"]), fx["tied_llr"]),
            "hetero llr": pen.rel(gbn.closed_set_llr(fx["hetero_ll"]), fx["hetero_llr"]),
            "hand llr": pen.rel(gbn.closed_set_llr(fx["hand"], float(fx["p_tar_hand"])), fx["hand_llr"])}
    print({k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < RESTATEMENT_TOL, f"{k} differs by {v:.3e} (relative max-norm, bound {RESTATEMENT_TOL})"
    assert numpy.all(numpy.isfinite(gbn.closed_set_llr(fx["hand"], float(fx["p_tar_hand"]))))


def test_fixture_is_the_set_its_generator_describes(fx):
    counts = numpy.unique(fx["modelset"], return_counts=True)[1]
    assert sorted(counts) == sorted([3, 40, 17, 130, 5, 64, 29]) and fx["X"].shape == (288, 45) and fx["T"].shape == (301, 45)
    hand = fx["hand"]
    top2 = numpy.sort(hand, axis=0)[-2:]
    assert top2[1, 0] - top2[0, 0] == 800.0 and top2[1, 1] == top2[0, 1] and numpy.ptp(hand[:, 2]) == 0.0 and hand[:, 3].max() < -9990.0
    # the log-likelihood arg-max names the class a test row was drawn from far more often than chance: the set is a real identification task
    assert (fx["hetero_ll"].argmax(axis=0) == fx["test_classes"]).mean() > 0.5     # chance: 1 / 7


def test_reference_signatures():
    expect = {"log_sum_exp": "(x)", "compute_log_likelihood_ratio": "(M, p_tar=0.5)", "gaussian_backend_train": "(train_ss)",
              "gaussian_backend_train_hetero": "(train_ss, alpha=0.1)", "_gaussian_backend_train": "(data, label)",
              "gaussian_backend_test": "(test_ss, params, diag=False, compute_llr=True)",
              "gaussian_backend_test_hetero": "(test_ss, params, diag=False, compute_llr=True)",
              "gaussian_backend_hetero_device": "(xv, class_index, alpha=0.1)", "gaussian_backend_device": "(xv, class_index)",
              "class_scatter_device": "(xv, class_index)", "gaussian_loglik_device": "(xv, means, sigma, cst)"}
    for name, sig in expect.items():
        assert str(inspect.signature(getattr(lid_utils, name))) == sig, name
    assert list(inspect.signature(lid_utils.closed_set_llr_device).parameters)[:2] == ["M", "p_tar"]
    assert inspect.signature(lid_utils.closed_set_llr_device).parameters["p_tar"].default == 0.5
    x = numpy.array([[0.0, -1000.0, 3.0], [1.0, -1000.0, -2.0]])
    numpy.testing.assert_allclose(lid_utils.log_sum_exp(x), [numpy.log(1 + numpy.e), -1000 + numpy.log(2), 3 + numpy.log1p(numpy.exp(-5))], rtol=1e-15)


def test_refusals_come_before_any_device_call(fx):
    """Each of these raises its own error on a host with no GPU, where touching the device is a RuntimeError ("no GPU is visible")."""
    means = _stat_server(fx["classes"].astype("|O"), fx["means"])
    test = _stat_server(numpy.array(["a", "b"], dtype="|O"), fx["T"][:2])
    tied = (means, fx["tied_sigma"], float(fx["tied_cst"]))
    hetero = (means, list(fx["hetero_sigma"]), list(fx["hetero_cst"]))
    with pytest.raises(NotImplementedError, match="Mixture"):
        lid_utils.gaussian_backend_test(test, tied, diag=True)
    with pytest.raises(NotImplementedError, match="Mixture"):
        lid_utils.gaussian_backend_test_hetero(test, hetero, diag=True)
    short = _stat_server(numpy.array(["a", "b"], dtype="|O"), fx["T"][:2, :44])
    with pytest.raises(AssertionError, match="dimension mismatch"):
        lid_utils.gaussian_backend_test(short, tied)
    with pytest.raises(AssertionError, match="dimension mismatch"):
        lid_utils.gaussian_backend_test_hetero(short, hetero)
    with pytest.raises(AssertionError):                                     # the reference's own assert: a tied back-end has one 2-D covariance
        lid_utils.gaussian_backend_test(test, (means, fx["hetero_sigma"], float(fx["tied_cst"])))
    one = _stat_server(fx["classes"][:1].astype("|O"), fx["means"][:1])
    with pytest.raises(AssertionError, match="C >= 2"):
        lid_utils.gaussian_backend_test(test, (one, fx["tied_sigma"], float(fx["tied_cst"])))
    with pytest.raises(AssertionError, match="C >= 2"):
        lid_utils.compute_log_likelihood_ratio(numpy.zeros((1, 5)))
    with pytest.raises(AssertionError, match="p_tar"):
        lid_utils.compute_log_likelihood_ratio(numpy.zeros((3, 5)), p_tar=1.0)
    with pytest.raises(AssertionError, match="dimension mismatch"):         # device-level: a covariance of another size than the means
        lid_utils.gaussian_loglik_device(numpy.zeros((2, 45)), fx["means"], fx["tied_sigma"][:44, :44], 0.0)
    with pytest.raises(AssertionError, match="per class"):
        lid_utils.gaussian_loglik_device(numpy.zeros((2, 45)), fx["means"], fx["hetero_sigma"][:3], fx["hetero_cst"][:3])


def test_import_loads_neither_torch_nor_the_library():
    code = ("import sys, sidekit_amd.lid_utils, sidekit_amd._lib as l; "
            "assert 'torch' not in sys.modules and l._lib is None, sorted(m for m in sys.modules if m.startswith('torch'))[:3]")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_install_as_sidekit_resolves_lid_utils():
    import sidekit_amd
    assert "lid_utils" in sidekit_amd.SUBMODULES
    saved = {k: v for k, v in sys.modules.items() if k == "sidekit" or k.startswith("sidekit.")}
    try:
        sidekit_amd.install_as_sidekit()
        import sidekit.lid_utils
        from sidekit.lid_utils import gaussian_backend_train, gaussian_backend_test_hetero   # noqa: F401  (the reference's own import lines)
        assert sidekit.lid_utils is lid_utils and gaussian_backend_train is lid_utils.gaussian_backend_train
    finally:
        for k in [k for k in sys.modules if k == "sidekit" or k.startswith("sidekit.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_header_binding_table_and_library_agree():
    """What tests/test_abi.py checks for include/sidekit_amd.h, for the Gaussian back-end's own header and table."""
    import ctypes
    import re
    src = open(os.path.join(ROOT, "include", "sidekit_amd", "gaussian_backend.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?(?:int|char\s*\*|void)\s*\**\s*((?:xt|sc|sk)_\w+)\s*\(", src, flags=re.M)))
    assert declared == ["sc_class_scatter", "sc_closed_set_llr", "sc_gauss_loglik"]
    assert sorted(_lib.GAUSSIAN_SIGNATURES) == declared, "ctypes binding table and header disagree"
    assert not set(_lib.GAUSSIAN_SIGNATURES) & set(_lib.SIGNATURES)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(cdll, name), f"{name} declared in include/sidekit_amd/gaussian_backend.h but not exported"
    lib = _lib.lib()
    for name, (res, args) in _lib.GAUSSIAN_SIGNATURES.items():
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    # the argument lists, type by type, against the declarations
    ctype = {"void*": _lib._P, "int32_t": _lib._I32, "int64_t": _lib._I64, "double": _lib._F64}
    flat = re.sub(r"\s+", " ", src)
    for name, (_, args) in _lib.GAUSSIAN_SIGNATURES.items():
        params = re.search(r"int %s\((.*?)\);" % name, flat).group(1).split(",")
        kinds = ["void*" if "*" in q else q.replace("const", "").split()[0] for q in params]
        assert [ctype[k] for k in kinds] == args, (name, kinds)


def test_entry_points_check_their_arguments_before_anything_is_enqueued():
    """SK_EARG through the C ABI on a host with no GPU: nothing was enqueued, or there would have been a HIP error instead."""
    lib = _lib.lib()
    p = 4096   # any non-null address: a refused call dereferences nothing
    cases = {"null": lib.sc_closed_set_llr(None, 3, 5, 0.5, None, None), "C = 1": lib.sc_closed_set_llr(p, 1, 5, 0.5, p, None),
             "p_tar = 0": lib.sc_closed_set_llr(p, 3, 5, 0.0, p, None), "p_tar = 1": lib.sc_closed_set_llr(p, 3, 5, 1.0, p, None),
             "p_tar = nan": lib.sc_closed_set_llr(p, 3, 5, float("nan"), p, None), "N = 0": lib.sc_closed_set_llr(p, 3, 0, 0.5, p, None),
             "loglik null": lib.sc_gauss_loglik(p, 5, 4, p, None, p, 2, p, None), "loglik C = 0": lib.sc_gauss_loglik(p, 5, 4, p, p, p, 0, p, None),
             "loglik C > grid": lib.sc_gauss_loglik(p, 5, 4, p, p, p, 65536, p, None), "loglik N = 0": lib.sc_gauss_loglik(p, 0, 4, p, p, p, 2, p, None),
             "loglik N > int": lib.sc_gauss_loglik(p, 1 << 31, 4, p, p, p, 2, p, None),
             "scatter null": lib.sc_class_scatter(p, _lib.XT_F64, 5, 4, None, p, 2, 3, p, None),
             "scatter dtype": lib.sc_class_scatter(p, _lib.XT_BF16, 5, 4, p, p, 2, 3, p, None),
             "scatter C > N": lib.sc_class_scatter(p, _lib.XT_F64, 5, 4, p, p, 6, 3, p, None),
             "scatter max_count = 0": lib.sc_class_scatter(p, _lib.XT_F64, 5, 4, p, p, 2, 0, p, None),
             "scatter max_count > N": lib.sc_class_scatter(p, _lib.XT_F32, 5, 4, p, p, 2, 6, p, None)}
    assert all(rc == _lib.SK_EARG for rc in cases.values()), cases
    assert "sc_class_scatter" in _lib.last_error()
