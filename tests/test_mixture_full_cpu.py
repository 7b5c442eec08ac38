"""Full-covariance mixtures without a GPU (sidekit_amd/mixture_full.py, include/sidekit_amd/gmm_full.h, csrc/gmm_full.hip): the header
against its binding table and the built library, the argument checks of the entry points through the C ABI, the numpy restatement the GPU
tests lean on (tests/tools/mixture_full_numpy.py) against what the reference computed (tests/golden/mixture_full.npz), the transposed
factor against scipy's log density, the host half of ``FullMixture`` against the fixture, its HDF5 file, and the refusals that stay.

The restatement is held to 1e-12 relative max-norm, the bar of tests/test_mixture_cpu.py for float64 algebra restated in numpy; the log
density to 1e-10: two float64 evaluations of a quadratic form of 23 terms with condition numbers up to 80 (a Cholesky solve here, an
eigen-decomposition in scipy) differ by about cond x D x 2^-53 = 2e-13 of its value.
"""
import copy
import inspect
import os
import subprocess
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import mixture_full_numpy as mfn  # noqa: E402
import mixture_numpy as mxn  # noqa: E402

import sidekit_amd  # noqa: E402
from sidekit_amd import _lib, mixture_full  # noqa: E402
from sidekit_amd.mixture import Mixture  # noqa: E402
from sidekit_amd.mixture_full import FullMixture  # noqa: E402
from sidekit_amd.statserver import StatServer  # noqa: E402

RESTATEMENT_TOL, DENSITY_TOL = 1e-12, 1e-10
STARTS, ITERATIONS = ("split0", "split2"), 3
KEYS = ("w", "mu", "invcov", "invchol", "det", "cst")
DIAG_KEYS = ("w", "mu", "invcov", "cov_var_ctl")


@pytest.fixture(scope="module")
def base(golden_dir):
    return dict(numpy.load(os.path.join(golden_dir, "mixture.npz")))


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(numpy.load(os.path.join(golden_dir, "mixture_full.npz")))


def _diag(base, tag):
    m = Mixture()
    m.w, m.mu, m.invcov, m.cov_var_ctl = (numpy.array(base[f"{tag}_{k}"], dtype=numpy.float64) for k in DIAG_KEYS)
    m.cst, m.det = numpy.zeros(m.w.shape), numpy.zeros(m.w.shape)
    m._compute_all()
    return m


def _assert_all(errs, tol=RESTATEMENT_TOL):
    print({k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < tol, f"{k} differs by {v:.3e} (relative max-norm, bound {tol})"


# ---- bindings and refusals ----------------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree():
    """What tests/test_gmm_topc_em_cpu.py checks for gmm_topc_em.h, for the full-covariance header and table."""
    import ctypes
    import re
    src = open(os.path.join(ROOT, "include", "sidekit_amd", "gmm_full.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?(?:int|char\s*\*|void)\s*\**\s*((?:xt|sc|sk)_\w+)\s*\(", src, flags=re.M)))
    assert declared == ["sc_gmm_full_frame_loglik", "sc_gmm_full_stats"]
    assert sorted(_lib.GMM_FULL_SIGNATURES) == declared, "ctypes binding table and header disagree"
    others = (_lib.SIGNATURES, _lib.GAUSSIAN_SIGNATURES, _lib.MIXTURE_SIGNATURES, _lib.IVECTOR_SIGNATURES, _lib.GMM_SCORING_SIGNATURES,
              _lib.GMM_TOPC_SIGNATURES, _lib.GMM_TOPC_STATS_SIGNATURES, _lib.GMM_TOPC_EM_SIGNATURES, _lib.JFA_SIGNATURES, _lib.SVM_SIGNATURES,
              _lib.FEATURES_SIGNATURES, _lib.CEPSTRUM_SIGNATURES)
    assert not any(set(_lib.GMM_FULL_SIGNATURES) & set(t) for t in others)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(cdll, name), f"{name} declared in include/sidekit_amd/gmm_full.h but not exported"
    lib = _lib.lib()
    for name, (res, args) in _lib.GMM_FULL_SIGNATURES.items():
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    ctype = {"void*": _lib._P, "int32_t": _lib._I32, "int64_t": _lib._I64, "double": _lib._F64}
    flat = re.sub(r"\s+", " ", src)
    for name, (_, args) in _lib.GMM_FULL_SIGNATURES.items():
        params = re.search(r"int %s\((.*?)\);" % name, flat).group(1).split(",")
        kinds = ["void*" if "*" in q else q.replace("const", "").split()[0] for q in params]
        assert [ctype[k] for k in kinds] == args, (name, kinds)
    assert '#include "mixture.h"' in src
    assert re.findall(r"#define (SC_\w+) (\d+)", src) == [("SC_GMM_FULL_MAX_D", "96"), ("SC_GMM_FULL_SLAB_TARGET", "1024")]
    assert (_lib.SC_GMM_FULL_MAX_D, _lib.SC_GMM_FULL_SLAB_TARGET) == (96, 1024) == (mixture_full.MAX_D, mixture_full.SLAB_TARGET)
    assert _lib.SC_GMM_FULL_MAX_D >= 80


def test_signatures_and_lazy_names():
    assert str(inspect.signature(FullMixture.__init__)) == "(self, mixture_file_name='', name='empty', reference_factor=False)"
    assert str(inspect.signature(FullMixture.EM_diag2full)) == "(self, diagonal_mixture, features_server, featureList, iterations=2, num_thread=1)"
    assert str(inspect.signature(FullMixture._maximization)) == "(self, accum, ceil_cov=10, floor_cov=0.01)"
    assert str(inspect.signature(FullMixture.compute_log_posterior_probabilities_full)) == "(self, cep, mu=None)"
    assert str(inspect.signature(mixture_full.frame_loglik_full_device)) == "(ubm, frames, mu=None, factor=None)"
    assert str(inspect.signature(mixture_full.gmm_stats_full_device)) == \
        "(ubm, frames, seg_off=None, order=2, max_workspace_bytes=1073741824, factor=None)"
    assert str(inspect.signature(mixture_full.em_diag2full_device)) == \
        "(diagonal_mixture, frames, iterations=2, reference_factor=False, after_iteration=None)"
    assert str(inspect.signature(StatServer.accumulate_stat_full)) == \
        "(self, ubm, feature_server, seg_indices=None, channel_extension=('', '_b'), num_thread=1)"
    assert str(inspect.signature(StatServer.accumulate_stat_full_device)) == "(self, ubm, frames, seg_off)"
    for name in ("FullMixture", "frame_loglik_full_device", "gmm_stats_full_device", "em_diag2full_device"):
        assert getattr(sidekit_amd, name) is getattr(mixture_full, name)
    assert "mixture_full" in sidekit_amd.SUBMODULES and not issubclass(FullMixture, Mixture)


def test_entry_points_check_their_arguments_before_anything_is_enqueued():
    """SK_EARG through the C ABI on a host with no GPU: nothing was enqueued, or there would have been a HIP error instead."""
    lib = _lib.lib()
    p, F32 = 4096, _lib.XT_F32   # any non-null address: a refused call dereferences nothing

    def loglik(X=p, dt=F32, N=5, D=4, mu=p, M=p, g=p, C=3, lse=p, lp=p):
        return lib.sc_gmm_full_frame_loglik(X, dt, N, D, mu, M, g, C, lse, lp, None)

    def stats(X=p, dt=F32, N=5, D=4, mu=p, M=p, g=p, C=3, lse=p, off=p, S=2, max_len=5, order=2, s0=p, s1=p, s2=p, llk=p):
        return lib.sc_gmm_full_stats(X, dt, N, D, mu, M, g, C, lse, off, S, max_len, order, s0, s1, s2, llk, None)

    cases = {"X null": loglik(X=None), "mu null": loglik(mu=None), "M null": loglik(M=None), "g null": loglik(g=None), "lse null": loglik(lse=None),
             "bf16": loglik(dt=_lib.XT_BF16), "i64": loglik(dt=_lib.XT_I64), "N = 0": loglik(N=0), "N = 2^31": loglik(N=1 << 31),
             "D = 0": loglik(D=0), "D = 97": loglik(D=97), "D = 128": loglik(D=128), "C = 0": loglik(C=0), "C > max": loglik(C=65535 * 64 + 1),
             "s: X null": stats(X=None), "s: mu null": stats(mu=None), "s: M null": stats(M=None), "s: g null": stats(g=None),
             "s: lse null": stats(lse=None), "s: off null": stats(off=None), "s: stat0 null": stats(s0=None), "s: stat1 null": stats(s1=None),
             "s: order 2 without stat2": stats(s2=None), "s: order 0": stats(order=0), "s: order 3": stats(order=3), "s: S = 0": stats(S=0),
             "s: max_len < 0": stats(max_len=-1), "s: max_len > N": stats(max_len=6), "s: i16": stats(dt=_lib.XT_I16), "s: D = 97": stats(D=97),
             "s: C = 0": stats(C=0), "s: grid": stats(N=1 << 20, max_len=1 << 20, S=1 << 20, C=1 << 12)}
    assert all(rc == _lib.SK_EARG for rc in cases.values()), cases
    assert stats(D=97) == _lib.SK_EARG and "sc_gmm_full_stats" in _lib.last_error() and "D=97" in _lib.last_error()
    assert loglik(D=97) == _lib.SK_EARG and "sc_gmm_full_frame_loglik" in _lib.last_error()


def test_refusals_that_stay_and_the_new_door(base, fx):
    """``Mixture`` refuses a 3-D ``invcov`` as before (tests/test_mixture_cpu.py pins it; asserted here too), the diagonal doors of the
    StatServer refuse a ``FullMixture`` and the full ones a ``Mixture``."""
    import torch
    m = _diag(base, "split0")
    m.invcov = numpy.stack([numpy.diag(v) for v in m.invcov])
    X = base["X"][:4]
    for call in (lambda: m.compute_log_posterior_probabilities(X), lambda: m.compute_log_posterior_probabilities_full(X),
                 lambda: m._expectation(copy.deepcopy(m), X), lambda: m._compute_all(), lambda: m.init_from_diag(m),
                 lambda: m.EM_diag2full(m, None, []), lambda: m._maximization(m)):
        with pytest.raises(NotImplementedError, match="full-covariance"):
            call()
    full = FullMixture()
    full.init_from_diag(_diag(base, "split0"))
    server = StatServer()
    server.segset = numpy.array(["a"], dtype="|O")
    for call in (lambda: server.accumulate_stat(full, None), lambda: server.accumulate_stat_topc(full, None),
                 lambda: server.accumulate_stat_device(full, X, [0, 4]), lambda: server.accumulate_stat_topc_device(full, X, [0, 4])):
        with pytest.raises(AssertionError, match="has to be a Mixture"):
            call()
    diag = _diag(base, "split0")
    for call in (lambda: server.accumulate_stat_full(diag, None), lambda: server.accumulate_stat_full_device(diag, X, [0, 4])):
        with pytest.raises(AssertionError, match="has to be a FullMixture"):
            call()
    with pytest.raises(AssertionError, match="Must be diagonal"):
        full.get_invcov_super_vector()
    if not torch.cuda.is_available():
        for call in (lambda: full.compute_log_posterior_probabilities_full(X), lambda: full._expectation(copy.deepcopy(full), X),
                     lambda: mixture_full.frame_loglik_full_device(full, X), lambda: mixture_full.gmm_stats_full_device(full, X),
                     lambda: mixture_full.em_diag2full_device(diag, X), lambda: server.accumulate_stat_full_device(full, X, [0, 4])):
            with pytest.raises(RuntimeError, match="no GPU is visible"):
                call()


def test_import_loads_neither_torch_nor_the_library():
    code = ("import sys, sidekit_amd.mixture_full, sidekit_amd._lib as l; "
            "assert 'torch' not in sys.modules and l._lib is None, sorted(m for m in sys.modules if m.startswith('torch'))[:3]")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# ---- the numpy model ----------------------------------------------------------------------------------------------------------------------
def test_restatement_matches_the_reference_fixture(base, fx):
    """Everything the fixture records, with the reference's factor"""
    X, errs = base["X"], {}
    for start in STARTS:
        m = mfn.init_from_diag(mxn.model(*(base[f"{start}_{k}"] for k in DIAG_KEYS)))
        for k in KEYS + ("cov_var_ctl",):
            errs[f"{start} init {k}"] = mxn.rel(m[k], fx[f"{start}_init_{k}"])
        errs[f"{start} lp0"] = mxn.rel(mfn.log_posteriors(m, X, True), fx[f"{start}_lp0"])
        errs[f"{start} lp0, either factor of a diagonal matrix"] = mxn.rel(mfn.log_posteriors(m, X, False), fx[f"{start}_lp0"])
        for it in range(ITERATIONS):
            m, _, (s0, s1, s2, llk) = mfn.em_step(m, X, True)
            for name, got in (("acc_w", s0), ("acc_mu", s1), ("acc_invcov", s2), ("llk", llk)):
                errs[f"{start} it{it} {name}"] = mxn.rel(got, fx[f"{start}_it{it}_{name}"])
            for k in KEYS:
                errs[f"{start} it{it} {k}"] = mxn.rel(m[k], fx[f"{start}_it{it}_{k}"])
            if it == 0:
                errs[f"{start} lp1"] = mxn.rel(mfn.log_posteriors(m, X, True), fx[f"{start}_lp1"])
    _assert_all(errs)
    eight = mfn.em_step(mfn.init_from_diag(mxn.model(*(base[f"split4_{k}"] for k in DIAG_KEYS))), X, False)[0]
    _assert_all({f"eight {k}": mxn.rel(eight[k], fx[f"eight_{k}"]) for k in KEYS})
    assert max(numpy.linalg.cond(ic) for ic in fx["eight_invcov"]) <= 300


def test_transposed_factor_is_the_log_density_and_em_is_monotone(base, fx):
    """``lp = log w + log N(x; mu, invcov^-1)`` with ``M = invchol'``, not with ``M = invchol``; four EM iterations from each recorded
    state do not lose likelihood with it, and do with the reference's factor (the table of the module's docstring)"""
    from scipy.stats import multivariate_normal
    X, errs = base["X"], {}
    for tag in ("split0_it0", "split2_it0", "eight"):
        m = {k: fx[f"{tag}_{k}"] for k in KEYS}
        want = numpy.stack([numpy.log(m["w"][c]) + multivariate_normal.logpdf(X, m["mu"][c], numpy.linalg.inv(m["invcov"][c]))
                            for c in range(m["w"].shape[0])], axis=1)
        errs[f"{tag} lp"] = mxn.rel(mfn.log_posteriors(m, X, False), want)
        assert mxn.rel(mfn.log_posteriors(m, X, True), want) > 1e-3, "the reference's factor is another quadratic form"
    _assert_all(errs, DENSITY_TOL)
    table = {"split0": ((-45.41, -51.04, -52.35, -52.37), (-45.41, -36.44, -36.19, -36.01)),
             "split2": ((-39.04, -40.77, -40.47, -40.47), (-39.04, -33.82, -33.74, -33.60))}
    for start in STARTS:
        d = mxn.model(*(base[f"{start}_{k}"] for k in DIAG_KEYS))
        for reference_factor in (True, False):
            llk = numpy.array([l for _, l in mfn.em_diag2full(d, X, 4, reference_factor)])   # per unit of occupation = per frame
            per_frame = [round(float(v), 2) for v in llk]
            print(start, "reference's factor" if reference_factor else "transposed factor", per_frame)
            assert numpy.allclose(llk, table[start][0 if reference_factor else 1], atol=6e-3)
            assert numpy.all(numpy.diff(llk) >= 0) != reference_factor


# ---- the host half ------------------------------------------------------------------------------------------------------------------------
def test_host_half_against_the_fixture(base, fx):
    """``init_from_diag``, ``_compute_all`` and ``_maximization`` (from the restatement's statistics) against what the reference left"""
    X, errs = base["X"], {}
    for start in STARTS:
        diag = _diag(base, start)
        before = copy.deepcopy(diag)
        full = FullMixture(reference_factor=True)
        full.init_from_diag(diag)
        assert full.validate() and full.distrib_nb() == diag.distrib_nb() and full.dim() == 23 and full.sv_size() == diag.sv_size()
        for k in KEYS + ("cov_var_ctl",):
            errs[f"{start} init {k}"] = mxn.rel(getattr(full, k), fx[f"{start}_init_{k}"])
        assert numpy.array_equal(full.A, numpy.zeros(full.w.shape))
        m = mfn.init_from_diag(mxn.model(*(base[f"{start}_{k}"] for k in DIAG_KEYS)))
        accum = copy.deepcopy(full)
        for it in range(ITERATIONS):
            accum._reset()
            assert not accum.w.any() and not accum.mu.any() and not accum.invcov.any()
            m, _, (s0, s1, s2, _) = mfn.em_step(m, X, True)
            accum.w += s0
            accum.mu += s1
            accum.invcov += s2
            full._maximization(accum)
            for k in KEYS:
                errs[f"{start} it{it} {k}"] = mxn.rel(getattr(full, k), fx[f"{start}_it{it}_{k}"])
            assert numpy.array_equal(full.invchol, numpy.tril(full.invchol)), "invchol holds what the reference stores: the lower factor"
        for k in ("w", "mu", "invcov", "cst", "det"):   # copies, not aliases: the reference's EM_diag2full overwrites the diagonal mixture's det
            assert numpy.array_equal(getattr(diag, k), getattr(before, k)), k
    _assert_all(errs)


def test_hdf5_round_trip(fx, tmp_path):
    """A ``FullMixture`` through ``write`` and ``read`` (``hdf5_lite``): the reference's eight dataset names, two of them 3-D"""
    from sidekit_amd import hdf5_lite
    m = FullMixture(reference_factor=True)
    for k in KEYS:
        setattr(m, k, numpy.array(fx[f"split2_it1_{k}"]))
    m.cov_var_ctl, m.A = numpy.array(fx["split2_init_cov_var_ctl"]), numpy.zeros(4)
    path = str(tmp_path / "full.h5")
    m.write(path)
    with hdf5_lite.File(path) as f:
        assert sorted(f.keys()) == sorted(["w", "mu", "invcov", "invchol", "cov_var_ctl", "cst", "det", "a"])
        shapes = {k: f[k][()].shape for k in f.keys()}
        assert all(f[k][()].dtype == numpy.float64 for k in f.keys())
    assert shapes == {"w": (4,), "mu": (4, 23), "invcov": (4, 23, 23), "invchol": (4, 23, 23), "cov_var_ctl": (4,), "cst": (4,), "det": (4,),
                      "a": (4,)}
    back = FullMixture(path)
    assert back.reference_factor is False, "the choice of factor is not stored"
    for k in KEYS + ("cov_var_ctl", "A"):
        numpy.testing.assert_array_equal(getattr(back, k), getattr(m, k))
    assert back.validate() and back.distrib_nb() == back.get_distrib_nb() == 4 and back.dim() == 23 and back.sv_size() == 92
    numpy.testing.assert_array_equal(back.get_mean_super_vector(), m.mu.flatten())
    m.write(path, prefix="ubm/")
    other = FullMixture()
    other.read(path, prefix="ubm/")
    numpy.testing.assert_array_equal(other.invcov, m.invcov)


def test_slab_cut_of_the_python_layer_is_the_header_formula():
    """``slabs(L, C) = min(ceil(L / 512), max(1, min(64, 1024 / C)))``, at least 1, and the groups it gives"""
    cut = mixture_full._slabs
    assert [cut(L, 2) for L in (0, 1, 512, 513, 1025, 40000)] == [1, 1, 1, 2, 3, 64]
    assert [cut(100000, C) for C in (1, 16, 17, 512, 600, 1024, 2048)] == [64, 64, 60, 2, 1, 1, 1]
    per_segment = 4 * (1 + 23 + 23 * 23)
    assert mixture_full._segment_groups([3, 301, 0, 64, 130, 17, 700, 45], 4, per_segment, 1 << 30) == [(0, 8)]
    assert mixture_full._segment_groups([3, 301, 0, 64, 130, 17, 700, 45], 4, per_segment, 3 * per_segment * 8) == \
        [(0, 3), (3, 6), (6, 7), (7, 8)]
