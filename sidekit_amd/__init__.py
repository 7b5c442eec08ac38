"""sidekit_amd -- MI355X-native x-vector extraction and trial scoring behind SIDEKIT's Python surface.

Sub-modules mirror the reference package layout for the hot path only:
``sidekit_amd.nnet.xvector.Xtractor``, ``sidekit_amd.iv_scoring``, ``sidekit_amd.factor_analyser``, ``sidekit_amd.statserver``,
``sidekit_amd.bosaris``, ``sidekit_amd.score_normalization``, ``sidekit_amd.lid_utils``, ``sidekit_amd.mixture``, ``sidekit_amd.mixture_full``, ``sidekit_amd.gmm_scoring``, ``sidekit_amd.jfa_scoring``, ``sidekit_amd.sidekit_io``, ``sidekit_amd.frontend.vad``,
``sidekit_amd.features_server``, ``sidekit_amd.frontend.normfeat``, ``sidekit_amd.frontend.features``, ``sidekit_amd.features_extractor``, ``sidekit_amd.plp``, ``sidekit_amd.features_context``,
``sidekit_amd.svm_training``, ``sidekit_amd.svm_scoring``, ``sidekit_amd.sv_utils``.
``install_as_sidekit()`` registers them under the ``sidekit`` names so that reference-style drivers
(``extract_xvectors.py``, scoring scripts) import them unchanged.
"""
import importlib
import sys

import numpy

PARALLEL_MODULE = 'multiprocessing'  # sidekit/__init__.py:56
PARAM_TYPE = numpy.float32           # sidekit/__init__.py:57
STAT_TYPE = numpy.float64            # sidekit/__init__.py:58

__version__ = "0.2.0"

# the reference package re-exports these names at top level (sidekit/__init__.py:61-121); resolved on first use so that
# `import sidekit_amd` alone loads neither torch nor the HIP library
_LAZY = {
    "IdMap": "bosaris", "Ndx": "bosaris", "Key": "bosaris", "Scores": "bosaris", "effective_prior": "bosaris",
    "logit_effective_prior": "bosaris", "fast_minDCF": "bosaris",
    "StatServer": "statserver",
    "cosine_scoring": "iv_scoring", "PLDA_scoring": "iv_scoring", "fast_PLDA_scoring": "iv_scoring", "full_PLDA_scoring": "iv_scoring",
    "mahalanobis_scoring": "iv_scoring", "two_covariance_scoring": "iv_scoring",
    "plda_histograms": "iv_scoring", "plda_range_from_sample": "iv_scoring", "plda_norm_histograms": "iv_scoring",
    "FactorAnalyser": "factor_analyser",
    "Mixture": "mixture", "split_candidates": "mixture", "gmm_topc_refine_device": "mixture", "em_split_topc_device": "mixture",
    "FullMixture": "mixture_full", "frame_loglik_full_device": "mixture_full", "gmm_stats_full_device": "mixture_full",
    "em_diag2full_device": "mixture_full",
    "asnorm": "score_normalization", "znorm": "score_normalization", "tnorm": "score_normalization", "ztnorm": "score_normalization",
    "asnorm_trials": "score_normalization", "cohort_stats_device": "score_normalization", "znorm_device": "score_normalization",
    "tnorm_device": "score_normalization", "snorm_device": "score_normalization", "ztnorm_device": "score_normalization",
    "normalised_histograms": "score_normalization", "normalised_range_from_sample": "score_normalization",
    "plda_cohort_stats_device": "score_normalization", "plda_znorm_device": "score_normalization", "plda_tnorm_device": "score_normalization",
    "plda_snorm_device": "score_normalization", "plda_normalised_histograms": "score_normalization",
    "plda_normalised_range_from_sample": "score_normalization",
    "vad_energy": "frontend.vad",
    "FeaturesServer": "features_server",
    "FeaturesExtractor": "features_extractor",
    "PlpExtractor": "plp", "plp_device": "plp",
    "ContextFeaturesServer": "features_context",
    "write_matrix_hdf5": "sidekit_io", "read_plda_hdf5": "sidekit_io", "write_plda_hdf5": "sidekit_io",
}

# every module of the mirror, by its reference name
SUBMODULES = ("bosaris", "bosaris.idmap", "bosaris.ndx", "bosaris.key", "bosaris.scores", "bosaris.detplot", "statserver", "iv_scoring", "factor_analyser",
              "score_normalization", "lid_utils", "mixture", "mixture_full", "gmm_scoring", "jfa_scoring", "sidekit_io", "nnet", "nnet.xvector", "nnet.preprocessor", "frontend", "frontend.vad",
              "features_server", "frontend.normfeat", "frontend.features", "features_extractor", "plp", "features_context", "sv_utils", "svm_training", "svm_scoring")


def __getattr__(name):
    if name in _LAZY:
        value = getattr(importlib.import_module(f"{__name__}.{_LAZY[name]}"), name)
        globals()[name] = value
        return value
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def install_as_sidekit():
    """Alias this package as ``sidekit`` in ``sys.modules``: afterwards ``from sidekit.nnet.xvector import
    Xtractor``, ``from sidekit.iv_scoring import cosine_scoring``, ``sidekit.bosaris.detplot.rocch``,
    ``sidekit.score_normalization.asnorm`` ... resolve to the MI355X implementations.  A module that cannot be imported
    (e.g. the HIP library is not built) raises here, loudly, instead of leaving a partial alias behind."""
    pkg = sys.modules[__name__]
    if sys.modules.get("sidekit", pkg) is not pkg:
        raise ImportError("another package is already imported as `sidekit`; install_as_sidekit() must run before it")
    sys.modules["sidekit"] = pkg
    for sub in SUBMODULES:
        sys.modules["sidekit." + sub] = importlib.import_module(f"{__name__}.{sub}")
    return pkg
