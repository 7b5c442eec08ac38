"""ctypes binding of ``libsidekit_amd.so`` (the C ABI declared in ``include/sidekit_amd.h``).

There is no CPU fallback: if the HIP library is missing or cannot be loaded the import of any
compute entry point raises.  PyTorch is imported first so that the library binds to the same
``libamdhip64`` runtime instance torch uses (device pointers and streams are then interchangeable).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libsidekit_amd.so")
if os.environ.get("SIDEKIT_AMD_LIB"):   # tuning aid: another build of the SAME library (A/B runs of kernel variants); never a different backend
    LIB_PATH = os.path.abspath(os.environ["SIDEKIT_AMD_LIB"])
    import warnings
    warnings.warn(f"SIDEKIT_AMD_LIB is set: loading {LIB_PATH} instead of the shipped csrc/libsidekit_amd.so (A/B tuning aid)", RuntimeWarning)
# The library reads SIDEKIT_AMD_LANES and SIDEKIT_AMD_SMALL_GRID (csrc/xt_api.hip); the Python side SIDEKIT_AMD_LIB and SIDEKIT_AMD_PIPELINE_DEPTH.
# Say so instead of silently ignoring any other SIDEKIT_AMD_* variable.
_PRODUCT_VARS = {"SIDEKIT_AMD_LIB", "SIDEKIT_AMD_LANES", "SIDEKIT_AMD_SMALL_GRID", "SIDEKIT_AMD_PIPELINE_DEPTH"}
for _tuning in sorted(k for k in os.environ if k.startswith("SIDEKIT_AMD_") and k not in _PRODUCT_VARS):
    import warnings
    warnings.warn(f"{_tuning} is set but the library ignores it", RuntimeWarning)

SK_OK, SK_EARG, SK_ESHAPE, SK_EHIP, SK_EWORKSPACE, SK_ESTATE = 0, -1, -2, -3, -4, -5
XT_ARCH_HALFRESNET34, XT_ARCH_TDNN = 0, 1
XT_F32, XT_BF16, XT_F64, XT_I64, XT_I16 = 0, 1, 2, 3, 4
XT_LOSS_AAM, XT_LOSS_CCE = 0, 1
SC_EPI_RANK1, SC_EPI_POSTERIOR = 0, 1
XT_PROF_SLOTS = 16
PROF_NAMES = ("conv_L1", "conv_L1S", "conv_L2A", "conv_L2S", "conv_L2", "conv_L3A", "conv_L3S", "conv_L3", "conv_L4A", "conv_L4S",
              "conv_L4", "frontend", "stem", "se_residual", "pool_tail", "tdnn")


class XtConfig(ctypes.Structure):
    _fields_ = [("arch", ctypes.c_int32), ("dtype", ctypes.c_int32), ("loss", ctypes.c_int32), ("n_spk", ctypes.c_int32),
                ("emb_dim", ctypes.c_int32), ("aam_s", ctypes.c_float)]


_P = ctypes.c_void_p
_I32, _I64, _SZ, _F64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_double

# name -> (restype, argtypes); every symbol of include/sidekit_amd.h
SIGNATURES = {
    "xt_create": (ctypes.c_int, [ctypes.POINTER(XtConfig), ctypes.POINTER(_P)]),
    "xt_destroy": (ctypes.c_int, [_P]),
    "xt_set_tensor": (ctypes.c_int, [_P, ctypes.c_char_p, _P, ctypes.POINTER(_I64), _I32, _I32]),
    "xt_num_keys": (ctypes.c_int, [_P]),
    "xt_key_name": (ctypes.c_char_p, [_P, _I32]),
    "xt_finalize": (ctypes.c_int, [_P]),
    "xt_reserve": (ctypes.c_int, [_P, _I32, _I64]),
    "xt_forward": (ctypes.c_int, [_P, _P, _I64, _P, _I32, _I64, _P, _P, _P]),
    "xt_forward_pcm16": (ctypes.c_int, [_P, _P, _I64, _P, _I32, _I64, _P, _P, _P]),
    "xt_reserve_slots": (ctypes.c_int, [_P, _I32, _I32, _I64]),
    "xt_forward_begin": (ctypes.c_int, [_P, _I32, _P, _I32, _I64, _P, _I32, _I64, _P, _P, _P]),
    "xt_forward_end": (ctypes.c_int, [_P, _I32, _P]),
    "xt_forward_features": (ctypes.c_int, [_P, _P, _P, _I32, _I32, _P, _P, _P]),
    "xt_features": (ctypes.c_int, [_P, _P, _I64, _P, _I32, _I64, _P, _P]),
    "xt_set_norm_embedding": (ctypes.c_int, [_P, _I32]),
    "xt_set_lanes": (ctypes.c_int, [_P, _I32]),
    "xt_get_lanes": (ctypes.c_int, [_P]),
    "xt_set_profile": (ctypes.c_int, [_P, _I32]),
    "xt_get_profile": (ctypes.c_int, [_P, ctypes.POINTER(_F64), ctypes.POINTER(_I64), _I32]),
    "xt_set_debug": (ctypes.c_int, [_P, _I32]),
    "xt_debug_tap": (ctypes.c_int, [_P, ctypes.c_char_p, _P, _SZ, ctypes.POINTER(_SZ)]),
    "xt_last_error": (ctypes.c_char_p, []),
    "sk_resample": (ctypes.c_int, [_P, _I32, _I64, _I32, _I32, _P, _I64, ctypes.POINTER(_I64), _P]),
    "sk_frame_log_energy": (ctypes.c_int, [_P, _I32, _I64, _P, _I32, _I32, _I32, _F64, _P, _I32, _P, _P]),
    "sk_vad_energy": (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _F64, _F64, _F64, _I32, _P, _P, _P]),
    "sk_collect_labels": (ctypes.c_int, [_P, _I32, _I64, _P, _P, _I32, _P, _I32, _I32, _P, _I64, _P, _P]),
    "sk_collect_segments": (ctypes.c_int, [_P, _I32, _I64, _P, _P, _P, _P, _P, _I32, _P, _I64, _P, _P]),
    "sc_cosine": (ctypes.c_int, [_P, _I32, _P, _I32, _I32, _P, _P]),
    "sc_plda_fast": (ctypes.c_int, [_P, _I32, _P, _I32, _I32, _P, _P, _F64, _F64, _P, _P]),
    "sc_release_workspace": (ctypes.c_int, []),
    "sc_normalize_rows": (ctypes.c_int, [_P, _I32, _I32, _P, _P]),
    "sc_cosine_hist": (ctypes.c_int, [_P, _I32, _P, _I32, _I32, _P, _P, _I32, ctypes.c_float, ctypes.c_float, _I32, _P, _P, _P]),
    "sc_cosine_hist_norm": (ctypes.c_int, [_P, _I32, _P, _I32, _I32, _P, _P, _I32, _P, _P, _P, _P, ctypes.c_float, ctypes.c_float, _I32, _P, _P, _P]),
    "sc_plda_hist": (ctypes.c_int, [_P, _I32, _P, _I32, _I32, _P, _P, _F64, _F64, _P, _P, _I32, _F64, _F64, _I32, _P, _P, _P]),
    "sc_plda_hist_norm": (ctypes.c_int, [_P, _I32, _P, _I32, _I32, _P, _P, _F64, _F64, _P, _P, _I32, _P, _P, _P, _P, _F64, _F64, _I32, _P, _P, _P]),
    "sc_cosine_trials": (ctypes.c_int, [_P, _P, _I32, _P, _P, _I64, _P, _P]),
    "sc_topk_stats": (ctypes.c_int, [_P, _I32, _I32, _I32, _P, _P, _P]),
    "sc_snorm_apply": (ctypes.c_int, [_P, _I32, _I32, _P, _P, _P, _P, _P]),
    "sc_cohort_moments": (ctypes.c_int, [_P, _I32, _P, _I32, _I32, _P, _P, _I32, _P, _P, _P]),
    "sc_norm_apply": (ctypes.c_int, [_P, _I32, _I32, _P, _P, _P, _P, _P]),
    "sc_plda_cohort_moments": (ctypes.c_int, [_P, _I32, _P, _I32, _I32, _P, _P, _F64, _F64, _I32, _P, _P, _P]),
    "sc_topk_stats_f64": (ctypes.c_int, [_P, _I32, _I32, _I32, _P, _P, _P]),
    "sc_norm_apply_f64": (ctypes.c_int, [_P, _I32, _I32, _P, _P, _P, _P, _P]),
    "sc_matrix_moments": (ctypes.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _P]),
    "sc_class_sums": (ctypes.c_int, [_P, _I32, _I64, _I32, _P, _P, _I32, _P, _I32, _P, _P, _P]),
    "sc_gemm_tn": (ctypes.c_int, [_P, _P, _I32, _I64, _I32, _I32, _P, _P, _P, _P, _P]),
    "sc_dgemm_nn": (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _F64, _P, _P, _I32, _P, _P]),
    "sc_scatter_within": (ctypes.c_int, [_P, _I32, _I64, _I32, _P, _P, _P, _I32, _P, _P]),
    "sc_whiten_rows": (ctypes.c_int, [_P, _I32, _I64, _I32, _P, _P, _I32, _I32, _P, _I32, _P]),
    "sk_bench_conv": (ctypes.c_int, [_I32, _I32, _I32, _I32, _I32, _I32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(_F64)]),
    "xt_debug_block": (ctypes.c_int, [_P, _I32, _P, _P, _I32, _I32, _I32, _P, _P, _P, _P]),
    "sk_pavx": (ctypes.c_int, [_P, _I64, _P, _P, _P, ctypes.POINTER(_I64)]),
    "sk_rocch_vertices": (ctypes.c_int, [_P, _I64, _I64, _I64, _P, _I64, _P, _P]),
    "sk_wav_probe": (ctypes.c_int, [_P, _I32, _I32, _P, _P, _P, _P]),
    "sk_wav_read_pcm16": (ctypes.c_int, [_P, _P, _P, _P, _I32, _I32, _P, _I64, _I32, _P]),
}

# name -> (restype, argtypes); every symbol of include/sidekit_amd/gaussian_backend.h (sidekit_amd/lid_utils.py)
GAUSSIAN_SIGNATURES = {
    "sc_class_scatter": (ctypes.c_int, [_P, _I32, _I64, _I32, _P, _P, _I32, _I64, _P, _P]),
    "sc_gauss_loglik": (ctypes.c_int, [_P, _I64, _I32, _P, _P, _P, _I32, _P, _P]),
    "sc_closed_set_llr": (ctypes.c_int, [_P, _I32, _I64, _F64, _P, _P]),
}

# name -> (restype, argtypes); every symbol of include/sidekit_amd/mixture.h (sidekit_amd/mixture.py)
MIXTURE_SIGNATURES = {
    "sc_gmm_frame_loglik": (ctypes.c_int, [_P, _I32, _I64, _I32, _P, _P, _P, _I32, _P, _P, _P]),
    "sc_gmm_stats": (ctypes.c_int, [_P, _I32, _I64, _I32, _P, _P, _P, _I32, _P, _P, _I32, _I64, _I32, _P, _P, _P, _P, _P]),
}

# name -> (restype, argtypes); every symbol of include/sidekit_amd/gmm_scoring.h (sidekit_amd/gmm_scoring.py)
GMM_SCORING_SIGNATURES = {
    "sc_gmm_score_models": (ctypes.c_int, [_P, _I32, _I64, _I32, _P, _I32, _P, _P, _I32, _P, _I32, _I64, _P, _P, _P]),
}

# name -> (restype, argtypes); every symbol of include/sidekit_amd/gmm_topc.h (sidekit_amd/gmm_scoring.py, the top-C functions)
GMM_TOPC_SIGNATURES = {
    "sc_gmm_top_components": (ctypes.c_int, [_P, _I32, _I64, _I32, _P, _P, _P, _I32, _I32, _P, _P]),
    "sc_gmm_score_models_topc": (ctypes.c_int, [_P, _I32, _I64, _I32, _P, _I32, _P, _P, _I32, _P, _I32, _I64, _P, _P, _I32, _P, _P]),
}
SC_GMM_TOPC_MAX = 32   # include/sidekit_amd/gmm_topc.h: components per frame

# name -> (restype, argtypes); every symbol of include/sidekit_amd/gmm_topc_stats.h (sidekit_amd/mixture.py, the top-C functions)
GMM_TOPC_STATS_SIGNATURES = {
    "sc_gmm_topc_posteriors": (ctypes.c_int, [_P, _I32, _I64, _I32, _P, _P, _P, _I32, _P, _I32, _P, _P, _P]),
    "sc_gmm_topc_stats": (ctypes.c_int, [_P, _I32, _I64, _I32, _I32, _P, _P, _I32, _P, _P, _I32, _I64, _I32, _P, _P, _P, _P, _P]),
}

# name -> (restype, argtypes); every symbol of include/sidekit_amd/gmm_topc_em.h (sidekit_amd/mixture.py, top-C EM)
GMM_TOPC_EM_SIGNATURES = {
    "sc_gmm_topc_refine": (ctypes.c_int, [_P, _I32, _I64, _I32, _P, _P, _P, _I32, _P, _I32, _I32, _P, _P, _P, _P]),
}
SC_GMM_TOPC_CAND_MAX = 64   # include/sidekit_amd/gmm_topc_em.h: candidates per frame

# name -> (restype, argtypes); every symbol of include/sidekit_amd/gmm_full.h (sidekit_amd/mixture_full.py)
GMM_FULL_SIGNATURES = {
    "sc_gmm_full_frame_loglik": (ctypes.c_int, [_P, _I32, _I64, _I32, _P, _P, _P, _I32, _P, _P, _P]),
    "sc_gmm_full_stats": (ctypes.c_int, [_P, _I32, _I64, _I32, _P, _P, _P, _I32, _P, _P, _I32, _I64, _I32, _P, _P, _P, _P, _P]),
}
SC_GMM_FULL_MAX_D, SC_GMM_FULL_SLAB_TARGET = 96, 1024   # include/sidekit_amd/gmm_full.h

# name -> (restype, argtypes); every symbol of include/sidekit_amd/ivector.h (sidekit_amd/factor_analyser.py)
IVECTOR_SIGNATURES = {
    "sc_tv_gram": (ctypes.c_int, [_P, _I32, _I32, _I32, _P, _P]),
    "sc_tv_posterior": (ctypes.c_int, [_P, _P, _I32, _I32, _P, _P, _P, _P]),
}

# name -> (restype, argtypes); every symbol of include/sidekit_amd/ivector_wide.h (sidekit_amd/factor_analyser_wide.py)
IVECTOR_WIDE_SIGNATURES = {
    "sc_tvw_gram": (ctypes.c_int, [_P, _I32, _I32, _I32, _P, _P]),
    "sc_tvw_workspace": (ctypes.c_int, [_I32, _I32, _P]),
    "sc_tvw_posterior": (ctypes.c_int, [_P, _P, _I32, _I32, _F64, _P, _P, _P, _P, _I64, _P]),
}
SC_TVW_MAX_RANK = 1024   # include/sidekit_amd/ivector_wide.h

# name -> (restype, argtypes); every symbol of include/sidekit_amd/jfa.h (sidekit_amd/jfa_scoring.py)
JFA_SIGNATURES = {
    "sc_jfa_shift": (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _P, _P, _I32, _I32, _P, _P, _P, _P, _P]),
    "sc_jfa_map_acc": (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P]),
}

# name -> (restype, argtypes); every symbol of include/sidekit_amd/svm.h (sidekit_amd/svm_training.py)
SVM_SIGNATURES = {
    "sc_svm_train": (ctypes.c_int, [_P, _I32, _P, _I32, _P, _I64, _P, _P, _I32, _I32, _P, _F64, _I32, _P, _P, _P, _P, _P, _P]),
}
SC_SVM_MAX_N = (163840 - 1024) // 24   # include/sidekit_amd/svm.h: the points of one problem (three doubles each in the LDS of one workgroup)
SC_SVM_CONVERGED, SC_SVM_MAX_ITER, SC_SVM_BAD_OFFSETS = 0, 1, 2

# name -> (restype, argtypes); every symbol of include/sidekit_amd/features.h (sidekit_amd/features_server.py)
FEATURES_SIGNATURES = {
    "sc_feat_rasta": (ctypes.c_int, [_P, _I64, _P, _I32, _I32, _P, _I64, _P]),
    "sc_feat_delta": (ctypes.c_int, [_P, _I64, _P, _I32, _I32, _P, _I32, _P, _I64, _P]),
    "sc_feat_moments": (ctypes.c_int, [_P, _I64, _P, _I32, _I32, _P, _P, _P]),
    "sc_feat_norm": (ctypes.c_int, [_P, _I64, _P, _I32, _I32, _I32, _I32, _P, _P, _P, _I64, _P]),
}
SC_FEAT_CENTER, SC_FEAT_CENTER_REDUCE, SC_FEAT_SLIDING_CENTER, SC_FEAT_SLIDING_CENTER_REDUCE, SC_FEAT_WARP = 0, 1, 2, 3, 4

# name -> (restype, argtypes); every symbol of include/sidekit_amd/context.h (sidekit_amd/features_context.py)
CONTEXT_SIGNATURES = {
    "sc_ctx_gather": (ctypes.c_int, [_P, _I64, _P, _I32, _I32, _I64, _P, _P, _I32, _I32, _I32, _P, _I64, _P]),
    "sc_ctx_basis": (ctypes.c_int, [_P, _I64, _P, _I32, _I32, _I64, _P, _I32, _I32, _I32, _P, _I64, _P]),
    "sc_ctx_project": (ctypes.c_int, [_P, _I64, _P, _I32, _I32, _I64, _P, _I32, _I32, _I32, _P, _I64, _P]),
}
SC_CTX_MAX_BLOCKS, SC_CTX_MAX_SPAN, SC_CTX_MAX_W, SC_CTX_PROJ_MAX_D, SC_CTX_PROJ_MAX_Q = 256, 256, 64, 128, 512   # include/sidekit_amd/context.h

# name -> (restype, argtypes); every symbol of include/sidekit_amd/cepstrum.h (sidekit_amd/features_extractor.py)
CEPSTRUM_SIGNATURES = {
    "sc_mfcc": (ctypes.c_int, [_P, _I32, _I64, _F64, _P, _P, _I32, _I64, _I32, _I32, _I32, _F64, _P, _P, _P, _P, _I32, _P, _I32, _P, _I64, _P, _I64, _P]),
}
SC_MFCC_MAX_FILT = 128

# name -> (restype, argtypes); every symbol of include/sidekit_amd/plp.h (sidekit_amd/plp.py)
PLP_SIGNATURES = {
    "sc_plp_cepstra": (ctypes.c_int, [_P, _I64, _I64, _I32, _I32, _P, _P, _P, _P, _I64, _P, _I64, _P]),
}
SC_PLP_MIN_BANDS, SC_PLP_MAX_BANDS = 4, 32   # include/sidekit_amd/plp.h: critical bands of a frame

_lib = None


def lib():
    """Load (once) and return the HIP library.  Raises ImportError when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          f"(or `make -C sidekit_amd/csrc`). sidekit_amd has no CPU fallback.")
    import torch  # noqa: F401  (loads torch's libamdhip64.so.7; ours resolves to the same runtime instance)
    hip_rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(hip_rt):
        ctypes.CDLL(hip_rt, mode=ctypes.RTLD_GLOBAL)
    cdll = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in (list(SIGNATURES.items()) + list(GAUSSIAN_SIGNATURES.items()) + list(MIXTURE_SIGNATURES.items())
                              + list(IVECTOR_SIGNATURES.items()) + list(GMM_SCORING_SIGNATURES.items()) + list(FEATURES_SIGNATURES.items())
                              + list(CEPSTRUM_SIGNATURES.items()) + list(JFA_SIGNATURES.items()) + list(SVM_SIGNATURES.items())
                              + list(GMM_TOPC_SIGNATURES.items()) + list(GMM_TOPC_STATS_SIGNATURES.items())
                              + list(GMM_TOPC_EM_SIGNATURES.items()) + list(GMM_FULL_SIGNATURES.items()) + list(PLP_SIGNATURES.items())
                              + list(IVECTOR_WIDE_SIGNATURES.items()) + list(CONTEXT_SIGNATURES.items())):
        fn = getattr(cdll, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = cdll
    import atexit
    atexit.register(_release_at_exit)
    return _lib


def _release_at_exit():
    """Free the scoring workspace cache (scoring.hip); only if this process ever used the GPU."""
    try:
        import torch
        if _lib is not None and torch.cuda.is_initialized():
            _lib.sc_release_workspace()
    except Exception:   # interpreter teardown: nothing to report to
        pass


def last_error():
    msg = lib().xt_last_error()
    return msg.decode() if msg else ""


def check(rc, arg_exc=ValueError):
    """Turn an ABI error class into the Python exception the reference would raise."""
    if rc == SK_OK:
        return
    msg = last_error()
    if rc == SK_EARG:
        raise arg_exc(msg)
    raise RuntimeError(msg)


_torch = None   # imported at the first launch; lib() has imported it before anything can be launched


def launch(name, device, *args, exc=ValueError):
    """Call entry point ``name`` on ``device``: a tensor argument goes as its ``data_ptr()``, ``None`` as NULL, the device's current stream
    is appended (its raw handle: no ``Stream`` object is built per call), and the return code goes through ``check(rc, exc)``.  The symbol
    is looked up through ``lib()`` at call time."""
    global _torch
    if _torch is None:
        import torch as _torch
    fn, tensor = getattr(lib(), name), _torch.Tensor
    index = device.index if device.index is not None else _torch.cuda.current_device()
    with _torch.cuda.device(device):
        rc = fn(*[a.data_ptr() if isinstance(a, tensor) else a for a in args], _torch._C._cuda_getCurrentRawStream(index))
    if rc != SK_OK:
        check(rc, exc)
