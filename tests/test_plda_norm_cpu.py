"""Cohort normalisation of PLDA scores without a GPU: the four declarations and their argument checks, every check of the Python layer that
runs before a device is touched, and the driver's parser."""
import inspect
import os
import re

import numpy
import pytest
import torch

import sidekit_amd
from sidekit_amd import _lib, iv_scoring, score_normalization as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARATIONS = {
    "sc_plda_cohort_moments": "int sc_plda_cohort_moments(const double* d_X, int32_t N, const double* d_C, int32_t M, int32_t D, const double* d_Phi, "
                              "const double* d_Psi, double cst, double scaling, int32_t self_offset, double* d_mean, double* d_std, void* stream);",
    "sc_topk_stats_f64": "int sc_topk_stats_f64(const double* d_scores, int32_t n_rows, int32_t n_cols, int32_t k, double* d_mean, double* d_std, "
                         "void* stream);",
    "sc_norm_apply_f64": "int sc_norm_apply_f64(double* d_S, int32_t Ne, int32_t Nt, const double* d_mean_e, const double* d_std_e, "
                         "const double* d_mean_t, const double* d_std_t, void* stream);",
    "sc_plda_hist_norm": "int sc_plda_hist_norm(const double* d_E, int32_t Ne, const double* d_T, int32_t Nt, int32_t D, const double* d_Phi, "
                         "const double* d_Psi, double cst, double scaling, const int32_t* d_labels_e, const int32_t* d_labels_t, int32_t self_offset, "
                         "const double* d_mean_e, const double* d_std_e, const double* d_mean_t, const double* d_std_t, double lo, double hi, "
                         "int32_t nbins, uint64_t* d_hist_tar, uint64_t* d_hist_non, void* stream);",
}
P, I32, F64 = _lib._P, _lib._I32, _lib._F64
ARGTYPES = {
    "sc_plda_cohort_moments": [P, I32, P, I32, I32, P, P, F64, F64, I32, P, P, P],
    "sc_topk_stats_f64": [P, I32, I32, I32, P, P, P],
    "sc_norm_apply_f64": [P, I32, I32, P, P, P, P, P],
    "sc_plda_hist_norm": [P, I32, P, I32, I32, P, P, F64, F64, P, P, I32, P, P, P, P, F64, F64, I32, P, P, P],
}


def test_the_four_symbols_are_declared_exported_and_bound():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "sidekit_amd.h")).read())
    lib = _lib.lib()
    for name, want in DECLARATIONS.items():
        assert want in text, name
        assert _lib.SIGNATURES[name] == (_lib.ctypes.c_int, ARGTYPES[name]) and getattr(lib, name).argtypes == ARGTYPES[name]
    assert len(_lib.SIGNATURES) == 55                                                   # the 50 before them, these four and xt_debug_block
    for name in ("plda_cohort_stats_device", "plda_znorm_device", "plda_tnorm_device", "plda_snorm_device", "plda_normalised_histograms",
                 "plda_normalised_range_from_sample"):
        assert sidekit_amd._LAZY[name] == "score_normalization" and getattr(sidekit_amd, name) is getattr(sn, name)
    assert sidekit_amd.plda_norm_histograms is iv_scoring.plda_norm_histograms
    p = inspect.signature(sn.plda_cohort_stats_device).parameters
    assert list(p) == ["xv", "cohort_xv", "mu", "F", "Sigma", "G", "scaling_factor", "side", "topk", "self_offset", "max_workspace_bytes"]
    assert p["side"].default == "enrol" and p["max_workspace_bytes"].default == 1 << 30
    p = inspect.signature(sn.plda_normalised_histograms).parameters
    assert list(p) == ["enroll_xv", "test_xv", "enroll_labels", "test_labels", "cohort_xv", "mu", "F", "Sigma", "G", "scaling_factor", "kind", "topk",
                       "self_offset", "lo", "hi", "bins", "max_workspace_bytes"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("lo", "hi", "bins", "max_workspace_bytes")) and p["kind"].default == "s"
    p = inspect.signature(iv_scoring.plda_norm_histograms).parameters
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is None for k in ("enroll_norm", "test_norm", "lo", "hi", "bins", "device"))
    assert "does NOT share statistics" in sn.plda_snorm_device.__doc__


def test_argument_errors_return_before_any_device_call():
    lib, EARG = _lib.lib(), _lib.SK_EARG
    # sc_plda_cohort_moments: X N C M D Phi Psi cst scaling self_offset mean std stream (non-null stand-ins are never dereferenced)
    ok = [1, 4, 1, 5, 8, 1, 1, 0.0, 1.0, -1, 1, 1, None]
    def moments(**change):
        a = list(ok)
        for k, v in change.items():
            a[int(k[1:])] = v
        return lib.sc_plda_cohort_moments(*a)
    for pointer in (0, 2, 5, 6, 10, 11):
        assert moments(**{f"a{pointer}": None}) == EARG and "sc_plda_cohort_moments" in _lib.last_error(), pointer
    for a in ({"a3": 0}, {"a3": -2}, {"a4": 0}, {"a4": -1}, {"a1": -1}):
        assert moments(**a) == EARG, a
    assert moments(a3=1, a9=0) == EARG and "keeps no pair" in _lib.last_error()
    assert moments(a1=0, a0=None, a10=None, a11=None) == _lib.SK_OK                     # N == 0 does nothing
    for k in (1, 0, -3, 8):
        assert lib.sc_topk_stats_f64(1, 3, 7, k, 1, 1, None) == EARG and "1 < k <= n_cols" in _lib.last_error()
    assert lib.sc_topk_stats_f64(None, 3, 7, 2, 1, 1, None) == EARG
    assert lib.sc_norm_apply_f64(1, 3, 4, None, None, None, None, None) == EARG and "at least one" in _lib.last_error()
    assert lib.sc_norm_apply_f64(1, 3, 4, 1, None, None, None, None) == EARG
    assert lib.sc_norm_apply_f64(1, 3, 4, 1, 1, None, 1, None) == EARG and "come together" in _lib.last_error()
    assert lib.sc_norm_apply_f64(None, 3, 4, 1, 1, None, None, None) == EARG and lib.sc_norm_apply_f64(1, 0, 4, 1, 1, None, None, None) == EARG
    # sc_plda_hist_norm: sc_plda_hist's arguments with the four statistics pointers after self_offset
    okh = [1, 4, 1, 4, 8, 1, 1, 0.0, 1.0, 1, 1, -1, 1, 1, 1, 1, -1.0, 1.0, 8192, 1, 1, None]
    def hist(**change):
        a = list(okh)
        for k, v in change.items():
            a[int(k[1:])] = v
        return lib.sc_plda_hist_norm(*a)
    for pointer in (0, 2, 5, 6, 9, 10, 19, 20):
        assert hist(**{f"a{pointer}": None}) == EARG and "sc_plda_hist_norm" in _lib.last_error(), pointer
    for lone in (12, 13, 14, 15):
        assert hist(**{f"a{lone}": None}) == EARG and "come together" in _lib.last_error()
    assert hist(a12=None, a13=None, a14=None, a15=None) == EARG and "at least one" in _lib.last_error()
    assert hist(a18=4096) == EARG and "nbins must be 8192" in _lib.last_error()
    assert hist(a16=1.0, a17=1.0) == EARG and hist(a17=float("inf")) == EARG and hist(a16=float("nan")) == EARG
    for size in (1, 3, 4):
        assert hist(**{f"a{size}": 0}) == EARG


@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to pick a device fails the test: the checks under test come first."""
    def touched(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(iv_scoring, "_device", touched)
    monkeypatch.setattr(sn, "_device_of", touched)


def _model(D=8, rank=3, seed=0):
    rs = numpy.random.RandomState(seed)
    A = rs.randn(D, D)
    return rs.randn(D), rs.randn(D, rank), A @ A.T + D * numpy.eye(D)


def test_python_checks_fire_before_any_device_call(no_device):
    mu, F, Sigma = _model()
    x, t, c = numpy.zeros((5, 8)), numpy.zeros((6, 8)), numpy.zeros((9, 8))
    le, lt = numpy.zeros(5, dtype=numpy.int32), numpy.zeros(6, dtype=numpy.int32)
    m = (mu, F, Sigma)
    S = sn.plda_cohort_stats_device
    with pytest.raises(ValueError, match="side is 'enrol' or 'test'"):
        S(x, c, *m, side="both")
    with pytest.raises(ValueError, match="matrices of one width"):
        S(x, numpy.zeros((9, 7)), *m)
    with pytest.raises(ValueError, match="must be a matrix"):
        S(numpy.zeros(8), c, *m)
    with pytest.raises(ValueError, match="the cohort is empty"):
        S(x, numpy.zeros((0, 8)), *m)
    with pytest.raises(ValueError, match="the vectors are 8 wide"):
        S(x, c, mu[:7], F, Sigma)
    with pytest.raises(ValueError, match="Sigma is not finite"):
        S(x, c, mu, F, Sigma * numpy.nan)
    for k in (1, 0, 10):
        with pytest.raises(ValueError, match="1 < topk <= cohort size"):
            S(x, c, *m, topk=k)
    with pytest.raises(ValueError, match="self_offset applies to whole-cohort statistics"):
        S(x, c, *m, topk=3, self_offset=0)
    scores = torch.zeros(5, 6, dtype=torch.float64)
    for fn, args in ((sn.plda_znorm_device, (x, c)), (sn.plda_tnorm_device, (t, c)), (sn.plda_snorm_device, (x, t, c))):
        with pytest.raises(ValueError, match="contiguous float64 device tensor"):
            fn(scores, *args, *m)
        with pytest.raises(ValueError, match="matrices of one width"):
            fn(scores, *args[:-1], numpy.zeros((9, 7)), *m)
    with pytest.raises(ValueError, match="1 < topk <= cohort size"):
        sn.plda_snorm_device(scores, x, t, c, *m, topk=10)
    H, R = sn.plda_normalised_histograms, sn.plda_normalised_range_from_sample
    rng = dict(lo=-5.0, hi=5.0)
    for missing in ({}, {"lo": -5.0}, {"hi": 5.0}):
        with pytest.raises(ValueError, match="lo and hi are required"):
            H(x, t, le, lt, c, *m, **missing)
    with pytest.raises(ValueError, match="hi must exceed lo"):
        H(x, t, le, lt, c, *m, lo=1.0, hi=1.0)
    with pytest.raises(TypeError):
        H(x, t, le, lt, c, *m, None, 1.0, "s", None, None, -5.0, 5.0)                      # lo / hi are keywords
    for fn, head in ((H, (x, t, le, lt, c)), (R, (x, t, c))):
        kw = rng if fn is H else {}
        for kind in ("zt", "as", None):
            with pytest.raises(ValueError, match="kind is 'z', 't' or 's'"):
                fn(*head, *m, kind=kind, **kw)
        for kind in ("z", "t"):
            with pytest.raises(ValueError, match="topk .* goes with kind='s' only"):
                fn(*head, *m, kind=kind, topk=3, **kw)
        with pytest.raises(ValueError, match="1 < topk <= cohort size"):
            fn(*head, *m, kind="s", topk=10, **kw)
        with pytest.raises(ValueError, match="matrices of one width"):
            fn(*head[:-1], numpy.zeros((9, 7)), *m, **kw)
    # iv_scoring.plda_norm_histograms: the pairs are checked as cosine_histograms checks its own
    N = iv_scoring.plda_norm_histograms
    ones5, ones6 = numpy.ones(5), numpy.ones(6)
    with pytest.raises(ValueError, match="enroll_norm is a .mean, std. pair"):
        N(x, t, le, lt, *m, enroll_norm=(ones5, None), **rng)
    with pytest.raises(ValueError, match="test_norm is a .mean, std. pair"):
        N(x, t, le, lt, *m, test_norm=(ones6,), **rng)
    with pytest.raises(ValueError, match="enroll_norm: the std has shape"):
        N(x, t, le, lt, *m, enroll_norm=(ones5, ones6), **rng)
    with pytest.raises(ValueError, match="test_norm: the mean has shape"):
        N(x, t, le, lt, *m, test_norm=(ones5, ones6), **rng)
    with pytest.raises(ValueError, match="lo and hi are required"):
        N(x, t, le, lt, *m, enroll_norm=(ones5, ones5))


def test_without_a_gpu_the_error_is_the_usual_one_once_the_checks_pass():
    assert not torch.cuda.is_available()
    mu, F, Sigma = _model()
    x, c, lab = numpy.zeros((5, 8)), numpy.zeros((9, 8)), numpy.zeros(5, dtype=numpy.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sn.plda_cohort_stats_device(x, c, mu, F, Sigma)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sn.plda_normalised_histograms(x, x, lab, lab, c, mu, F, Sigma, lo=-1.0, hi=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        iv_scoring.plda_norm_histograms(x, x, lab, lab, mu, F, Sigma, enroll_norm=(numpy.ones(5), numpy.ones(5)), lo=-1.0, hi=1.0)


def test_driver_parser(capsys):
    from sidekit_amd.bin import shard_extract_score
    base = ["--utterances", "1600", "--trials", "250"]
    for argv, message in ((["--all-pairs-plda-norm", "as"], "--all-pairs-plda-norm requires --all-pairs-plda"),
                          (["--all-pairs", "--all-pairs-plda-norm", "s"], "--all-pairs-plda-norm requires --all-pairs-plda"),
                          (["--all-pairs-plda", "--all-pairs-plda-norm", "as", "--norm-cohort", "300", "--norm-topk", "1"], "need 1 < K <= --norm-cohort"),
                          (["--all-pairs-plda", "--all-pairs-plda-norm", "as", "--norm-cohort", "300", "--norm-topk", "301"], "need 1 < K <= --norm-cohort"),
                          (["--all-pairs-plda", "--all-pairs-plda-norm", "s", "--norm-cohort", "1101"], "the cohort comes out of the 1100 PLDA training rows"),
                          (["--all-pairs-plda", "--all-pairs-plda-norm", "s", "--norm-cohort", "300", "--plda-norm-hist-range", "2", "2"], "HI must exceed LO"),
                          (["--all-pairs-plda", "--all-pairs-plda-norm", "zt"], "invalid choice"),
                          (["--all-pairs-plda", "--all-pairs-plda-norm", "s", "--norm-cohort", "300", "--device", "cpu"], "runs on the GPU")):
        with pytest.raises(SystemExit):
            shard_extract_score.main(base + argv)
        assert message in capsys.readouterr().err, argv
