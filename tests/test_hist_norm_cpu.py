"""Normalised all-pairs histograms without a GPU: the argument checks that run before any device is touched, the driver's flag
checks (before extraction starts), and the declaration of sc_cosine_hist_norm in the public header."""
import os
import re

import numpy
import pytest
import torch

import sidekit_amd
from sidekit_amd import iv_scoring
from sidekit_amd import score_normalization as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to pick a device fails the test: the checks under test come first."""
    def touched(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(sn, "_device_of", touched)
    monkeypatch.setattr(iv_scoring, "_device", touched)


def test_normalised_histograms_checks_fire_before_any_device_call(no_device):
    x, c = numpy.zeros((5, 8), dtype=numpy.float32), numpy.zeros((7, 8), dtype=numpy.float32)
    lab = numpy.zeros(5, dtype=numpy.int32)
    rng = dict(lo=-8.0, hi=8.0)
    for fn, extra in ((sn.normalised_histograms, rng), (sn.normalised_range_from_sample, {})):
        args = (lambda e, t, co: (e, t, lab, lab, co)) if fn is sn.normalised_histograms else (lambda e, t, co: (e, t, co))
        with pytest.raises(ValueError, match="multiple of 4"):
            fn(*args(x, x, numpy.zeros((7, 12), dtype=numpy.float32)), **extra)                 # cohort of another dimension
        with pytest.raises(ValueError, match="multiple of 4"):
            fn(*args(x, numpy.zeros((5, 12), dtype=numpy.float32), c), **extra)                 # test side of another dimension
        with pytest.raises(ValueError, match="empty"):
            fn(*args(x, x, numpy.zeros((0, 8), dtype=numpy.float32)), **extra)
        with pytest.raises(ValueError, match="kind"):
            fn(*args(x, x, c), kind="q", **extra)
        with pytest.raises(ValueError, match="zt-norm"):
            fn(*args(x, x, c), kind="zt", **extra)
        with pytest.raises(ValueError, match="kind='s' only"):
            fn(*args(x, x, c), kind="z", topk=3, **extra)
        with pytest.raises(ValueError, match="topk"):
            fn(*args(x, x, c), kind="s", topk=8, **extra)                                       # topk > M
    for missing in ({}, {"lo": -8.0}, {"hi": 8.0}):
        with pytest.raises(ValueError, match="lo and hi are required"):
            sn.normalised_histograms(x, x, lab, lab, c, **missing)
    with pytest.raises(ValueError, match="hi must exceed lo"):
        sn.normalised_histograms(x, x, lab, lab, c, lo=1.0, hi=1.0)
    with pytest.raises(TypeError):
        sn.normalised_histograms(x, x, lab, lab, c, "s", None, False, None, -8.0, 8.0)         # lo / hi are keywords


def test_cosine_histograms_norm_pairs_are_checked_before_any_device_call(no_device):
    x, t = numpy.zeros((5, 8), dtype=numpy.float32), numpy.zeros((6, 8), dtype=numpy.float32)
    le, lt = numpy.zeros(5, dtype=numpy.int32), numpy.zeros(6, dtype=numpy.int32)
    m5, s5, m6, s6 = numpy.zeros(5, "f"), numpy.ones(5, "f"), numpy.zeros(6, "f"), numpy.ones(6, "f")
    with pytest.raises(ValueError, match="multiple of 4"):
        iv_scoring.cosine_histograms(x, numpy.zeros((6, 12), dtype=numpy.float32), le, lt, enroll_norm=(m5, s5))
    with pytest.raises(ValueError, match="5 rows"):
        iv_scoring.cosine_histograms(x, t, le, lt, enroll_norm=(m6, s6))
    with pytest.raises(ValueError, match="6 rows"):
        iv_scoring.cosine_histograms(x, t, le, lt, enroll_norm=(m5, s5), test_norm=(m6, s5))
    with pytest.raises(ValueError, match="comes with its std"):
        iv_scoring.cosine_histograms(x, t, le, lt, enroll_norm=(m5, None))
    with pytest.raises(ValueError, match="comes with its std"):
        iv_scoring.cosine_histograms(x, t, le, lt, test_norm=m6)


class _NeverExtracts:
    embedding_size = 16
    compute_dtype = "fp32"

    def __call__(self, x, is_eval=False):
        raise AssertionError("extraction started before the flags were checked")


class _NoScoring:
    pass


def test_driver_flags_are_checked_before_extraction(monkeypatch, capsys):
    from sidekit_amd.bin import shard_extract_score
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    base = ["--utterances", "192", "--batch", "16", "--seconds", "0.2", "--trials", "48", "--speakers", "12", "--backend", "gloo", "--device", "cpu"]
    run = lambda extra: shard_extract_score.main(base + extra, model=_NeverExtracts(), scoring=_NoScoring)
    with pytest.raises(SystemExit):
        run(["--all-pairs-norm", "s", "--norm-cohort", "64"])                                   # without --all-pairs
    assert "requires --all-pairs" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        run(["--all-pairs", "--all-pairs-norm", "s", "--norm-cohort", "97"])                    # 192 - 2 * 48 = 96 training rows
    assert "--norm-cohort 97" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        run(["--all-pairs", "--all-pairs-norm", "as", "--norm-cohort", "64", "--norm-topk", "65"])
    assert "--norm-topk 65" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        run(["--all-pairs", "--all-pairs-norm", "s", "--norm-cohort", "64"])                    # the normalised pass has no CPU stand-in
    assert "runs on the GPU" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        run(["--all-pairs", "--all-pairs-norm", "zt"])


def test_header_declares_sc_cosine_hist_norm():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "sidekit_amd.h")).read())
    want = ("int sc_cosine_hist_norm(const float* d_E, int32_t Ne, const float* d_T, int32_t Nt, int32_t D, const int32_t* d_labels_e, "
            "const int32_t* d_labels_t, int32_t self_offset, const float* d_mean_e, const float* d_std_e, const float* d_mean_t, "
            "const float* d_std_t, float lo, float hi, int32_t nbins, uint64_t* d_hist_tar, uint64_t* d_hist_non, void* stream);")
    assert want in text
    assert len(sidekit_amd._lib.SIGNATURES["sc_cosine_hist_norm"][1]) == 18


def test_new_names_are_exported_and_the_c_entry_checks_its_pairs():
    for name in ("normalised_histograms", "normalised_range_from_sample"):
        assert sidekit_amd._LAZY[name] == "score_normalization" and getattr(sidekit_amd, name) is getattr(sn, name)
        assert name in sn.__doc__
    import inspect
    p = inspect.signature(sn.normalised_histograms).parameters
    assert list(p)[:9] == ["enroll_xv", "test_xv", "enroll_labels", "test_labels", "cohort_xv", "kind", "topk", "normalize", "self_offset"]
    assert p["lo"].kind is p["hi"].kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(iv_scoring.cosine_histograms).parameters
    assert p["enroll_norm"].default is None and p["test_norm"].default is None
    lib, EARG = sidekit_amd._lib.lib(), sidekit_amd._lib.SK_EARG                                # argument errors return before any device call
    call = lambda me, se, mt, sd: lib.sc_cosine_hist_norm(1, 4, 1, 4, 8, 1, 1, -1, me, se, mt, sd, -1.0, 1.0, 8192, 1, 1, None)
    assert call(None, None, None, None) == EARG and "at least one" in sidekit_amd._lib.last_error()
    assert call(1, None, 1, 1) == EARG and "together" in sidekit_amd._lib.last_error()
    assert call(1, 1, None, 1) == EARG
    assert lib.sc_cosine_hist_norm(1, 4, 1, 4, 8, 1, 1, -1, 1, 1, None, None, -1.0, 1.0, 4096, 1, 1, None) == EARG     # nbins
    assert lib.sc_cosine_hist_norm(1, 4, 1, 4, 6, 1, 1, -1, 1, 1, None, None, -1.0, 1.0, 8192, 1, 1, None) == EARG     # D % 4
