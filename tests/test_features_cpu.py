"""Feature post-processing without a GPU (sidekit_amd/features_server.py, frontend/normfeat.py, frontend/features.py, csrc/featnorm.hip):
the entry points' own header against their binding table and the built library, their argument checks through the C ABI, the reference's
parameter lists, the package wiring, the refusals, the mask parser and the LDS arithmetic of the tile."""
import inspect
import os
import re
import subprocess
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import sidekit_amd  # noqa: E402
from sidekit_amd import _lib, features_server  # noqa: E402
from sidekit_amd.features_server import FeaturesServer  # noqa: E402
from sidekit_amd.frontend import features as fe_features, normfeat  # noqa: E402

ENTRIES = ["sc_feat_delta", "sc_feat_moments", "sc_feat_norm", "sc_feat_rasta"]


def _header():
    src = open(os.path.join(ROOT, "include", "sidekit_amd", "features.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_binding_table_and_library_agree():
    """What tests/test_abi.py checks for include/sidekit_amd.h, for the features header and table."""
    import ctypes
    _, src = _header()
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?(?:int|char\s*\*|void)\s*\**\s*((?:xt|sc|sk)_\w+)\s*\(", src, flags=re.M)))
    assert declared == ENTRIES
    assert sorted(_lib.FEATURES_SIGNATURES) == declared, "ctypes binding table and header disagree"
    others = (set(_lib.SIGNATURES) | set(_lib.GAUSSIAN_SIGNATURES) | set(_lib.MIXTURE_SIGNATURES) | set(_lib.IVECTOR_SIGNATURES)
              | set(_lib.GMM_SCORING_SIGNATURES))
    assert not set(_lib.FEATURES_SIGNATURES) & others, "the table is disjoint from the other tables"
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(cdll, name), f"{name} declared in include/sidekit_amd/features.h but not exported"
    lib = _lib.lib()
    for name, (res, args) in _lib.FEATURES_SIGNATURES.items():
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    ctype = {"void*": _lib._P, "int32_t": _lib._I32, "int64_t": _lib._I64, "double": _lib._F64}
    flat = re.sub(r"\s+", " ", src)
    for name, (_, args) in _lib.FEATURES_SIGNATURES.items():
        params = re.search(r"int %s\((.*?)\);" % name, flat).group(1).split(",")
        kinds = ["void*" if "*" in q else q.replace("const", "").split()[0] for q in params]
        assert [ctype[k] for k in kinds] == args, (name, kinds)
    define = lambda n: int(re.search(r"#define %s (\d+)" % n, src).group(1))   # noqa: E731
    assert (define("SC_FEAT_TILE"), define("SC_FEAT_COLS"), define("SC_FEAT_MAX_WIN"), define("SC_FEAT_MAX_TAPS")) == \
        (features_server.TILE, features_server.COLS, features_server.MAX_WIN, features_server.MAX_TAPS) == (256, 16, 1001, 15)
    modes = [define(n) for n in ("SC_FEAT_CENTER", "SC_FEAT_CENTER_REDUCE", "SC_FEAT_SLIDING_CENTER", "SC_FEAT_SLIDING_CENTER_REDUCE", "SC_FEAT_WARP")]
    assert modes == [features_server.MODES[k] for k in ("cms", "cmvn", "cms_sliding", "cmvn_sliding", "stg")] == [0, 1, 2, 3, 4]
    assert modes == [_lib.SC_FEAT_CENTER, _lib.SC_FEAT_CENTER_REDUCE, _lib.SC_FEAT_SLIDING_CENTER, _lib.SC_FEAT_SLIDING_CENTER_REDUCE, _lib.SC_FEAT_WARP]


def test_tile_fits_the_lds_a_workgroup_may_declare():
    T, C, W = features_server.TILE, features_server.COLS, features_server.MAX_WIN
    assert (T + W - 1) * C * 4 == 80384, "the staged rows of a 256 x 16 tile at the longest window"
    assert features_server.tile_lds_bytes(W) == (1258 * C + T * (C + 1)) * 4 == 97920 <= 163840
    assert features_server.tile_lds_bytes(301) == (558 * C + T * (C + 1)) * 4 == 53120 and 3 * 53120 <= 163840
    for win in range(3, W + 1, 2):
        stride = (features_server.tile_lds_bytes(win) // 4 - T * (C + 1)) // C
        assert stride % 4 == 2 and 0 <= stride - (T + win - 1) <= 2, "the column stride holds the staged rows and starts the columns on the even banks"
    text = open(os.path.join(ROOT, "sidekit_amd", "csrc", "featnorm.hip")).read()
    assert "97,920 B" in text and "53,120 B" in text, "the kernel file states the same budget"


def test_entry_points_check_their_arguments_before_anything_is_enqueued():
    """SK_EARG through the C ABI on a host with no GPU: nothing was enqueued, or there would have been a HIP error instead."""
    lib = _lib.lib()
    p, q = 4096, 8192   # any non-null addresses: a refused call dereferences nothing

    def rasta(x=p, ldx=5, off=p, S=2, D=5, y=q, ldy=5):
        return lib.sc_feat_rasta(x, ldx, off, S, D, y, ldy, None)

    def delta(x=p, ldx=5, off=p, S=2, D=5, filt=p, L=7, y=q, ldy=5):
        return lib.sc_feat_delta(x, ldx, off, S, D, filt, L, y, ldy, None)

    def moments(x=p, ldx=5, off=p, S=2, D=5, mean=p, std=p):
        return lib.sc_feat_moments(x, ldx, off, S, D, mean, std, None)

    def norm(x=p, ldx=5, off=p, S=2, D=5, mode=_lib.SC_FEAT_WARP, win=301, mean=p, std=p, y=q, ldy=5):
        return lib.sc_feat_norm(x, ldx, off, S, D, mode, win, mean, std, y, ldy, None)

    cases = {"rasta x null": rasta(x=None), "rasta offsets null": rasta(off=None), "rasta y null": rasta(y=None), "rasta S < 0": rasta(S=-1),
             "rasta D = 0": rasta(D=0), "rasta D < 0": rasta(D=-2), "rasta ldx < D": rasta(ldx=4), "rasta ldy < D": rasta(ldy=4),
             "rasta in place": rasta(y=p),
             "delta x null": delta(x=None), "delta offsets null": delta(off=None), "delta y null": delta(y=None), "delta filter null": delta(filt=None),
             "delta S < 0": delta(S=-1), "delta D = 0": delta(D=0), "delta L even": delta(L=6), "delta L = 0": delta(L=0), "delta L < 0": delta(L=-1),
             "delta L = 17": delta(L=17), "delta in place": delta(y=p), "delta ldy < D": delta(ldy=3),
             "moments x null": moments(x=None), "moments offsets null": moments(off=None), "moments mean null": moments(mean=None),
             "moments std null": moments(std=None), "moments S < 0": moments(S=-3), "moments D = 0": moments(D=0),
             "norm x null": norm(x=None), "norm offsets null": norm(off=None), "norm y null": norm(y=None), "norm S < 0": norm(S=-1),
             "norm D = 0": norm(D=0), "norm mode -1": norm(mode=-1), "norm mode 5": norm(mode=5), "norm win even": norm(win=300),
             "norm win 1": norm(win=1), "norm win 1003": norm(win=1003), "norm win < 0": norm(win=-301),
             "norm warp in place": norm(y=p), "norm sliding in place": norm(mode=_lib.SC_FEAT_SLIDING_CENTER, y=p),
             "norm sliding reduce in place": norm(mode=_lib.SC_FEAT_SLIDING_CENTER_REDUCE, y=p),
             "norm centre without mean": norm(mode=_lib.SC_FEAT_CENTER, mean=None),
             "norm reduce without std": norm(mode=_lib.SC_FEAT_CENTER_REDUCE, std=None),
             "norm sliding without mean": norm(mode=_lib.SC_FEAT_SLIDING_CENTER, mean=None),
             "norm sliding reduce without std": norm(mode=_lib.SC_FEAT_SLIDING_CENTER_REDUCE, std=None), "norm ldx < D": norm(ldx=2)}
    assert all(rc == _lib.SK_EARG for rc in cases.values()), {k: v for k, v in cases.items() if v != _lib.SK_EARG}
    assert "sc_feat_norm" in _lib.last_error()
    for call, name in ((rasta, "sc_feat_rasta"), (delta, "sc_feat_delta"), (moments, "sc_feat_moments")):
        assert call(D=0) == _lib.SK_EARG and name in _lib.last_error(), "the message names the entry"
    # an empty batch is nothing to do, not an error; and what is allowed in place passes the checks (S = 0: nothing is enqueued either)
    assert rasta(S=0) == delta(S=0) == moments(S=0) == norm(S=0) == _lib.SK_OK
    assert norm(S=0, mode=_lib.SC_FEAT_CENTER, y=p) == norm(S=0, mode=_lib.SC_FEAT_CENTER_REDUCE, y=p) == _lib.SK_OK
    assert norm(S=0, mean=None, std=None) == norm(S=0, mode=_lib.SC_FEAT_SLIDING_CENTER, std=None) == _lib.SK_OK
    assert norm(S=0, mode=_lib.SC_FEAT_CENTER, win=300) == norm(S=0, mode=_lib.SC_FEAT_CENTER_REDUCE, win=-1) == _lib.SK_OK, "the table modes do not read win"
    assert norm(S=0, win=3) == norm(S=0, win=1001) == delta(S=0, L=1) == delta(S=0, L=15) == _lib.SK_OK


def test_reference_parameter_lists():
    expect = {
        "__init__": "(self, features_extractor=None, feature_filename_structure=None, sources=None, dataset_list=None, mask=None, feat_norm=None, "
                    "global_cmvn=None, dct_pca=False, dct_pca_config=None, sdc=False, sdc_config=None, delta=None, double_delta=None, "
                    "delta_filter=None, context=None, traps_dct_nb=None, rasta=None, keep_all_features=True)",
        "post_processing": "(self, feat, label, global_mean=None, global_std=None)",
        "_mask": "(self, cep)", "_normalize": "(self, label, cep, global_mean=None, global_std=None)", "_delta_and_2delta": "(self, cep)",
        "_rasta": "(self, cep, label)",
        "load": "(self, show, channel=0, input_feature_filename=None, label=None, start=None, stop=None)",
        "get_features": "(self, show, channel=0, input_feature_filename=None, label=None, start=None, stop=None)",
        "get_features_per_speaker": "(self, show, idmap, channel=0, input_feature_filename=None, label=None)",
        "mean_std": "(self, show, channel=0, start=None, stop=None)",
        "stack_features": "(self, show_list, channel_list=None, feature_filename_list=None, label_list=None, start_list=None, stop_list=None)",
        "stack_features_device": "(self, show_list, channel_list=None, feature_filename_list=None, label_list=None, start_list=None, stop_list=None)"}
    for name, sig in expect.items():
        assert str(inspect.signature(getattr(FeaturesServer, name))) == sig, name
    functions = {normfeat.rasta_filt: "(x)", normfeat.cms: "(features, label=None, global_mean=None)",
                 normfeat.cmvn: "(features, label=None, global_mean=None, global_std=None)", normfeat.stg: "(features, label=None, win=301)",
                 normfeat.cep_sliding_norm: "(features, win=301, label=None, center=True, reduce=False)",
                 features_server.post_process_device: "(frames, seg_off, labels=None, *, rasta=False, delta=False, double_delta=False, delta_filter=None, "
                                                      "mask=None, feat_norm=None, win=301, global_mean=None, global_std=None, keep_all_features=True)"}
    for fn, sig in functions.items():
        assert str(inspect.signature(fn)) == sig, fn.__name__
    sig = inspect.signature(fe_features.compute_delta)
    assert list(sig.parameters) == ["features", "win", "method", "filt"] and sig.parameters["win"].default == 3
    assert sig.parameters["method"].default == 'filter'
    numpy.testing.assert_array_equal(sig.parameters["filt"].default, [.25, .5, .25, 0, -.25, -.5, -.25])
    server = FeaturesServer()
    numpy.testing.assert_array_equal(server.delta_filter, [.25, .5, .25, 0, -.25, -.5, -.25])
    assert (server.feature_filename_structure, server.sources, server.dct_pca_config, server.sdc_config, server.context, server.traps_dct_nb) == \
        ('{}', (), (12, 12, None), (1, 3, 7), (0, 0), 0)
    assert server.keep_all_features is True and server.rasta is False and server.delta is False and server.previous_load is None
    assert "feat_norm: None" in repr(server) and "keep_all_features: True" in repr(server) and repr(server).startswith('\t show: empty \n\n')


def test_package_wiring():
    for name in ("features_server", "frontend.normfeat", "frontend.features"):
        assert name in sidekit_amd.SUBMODULES
    assert sidekit_amd._LAZY["FeaturesServer"] == "features_server" and sidekit_amd.FeaturesServer is FeaturesServer
    import sidekit_amd.frontend as frontend
    assert frontend.stg is normfeat.stg and frontend.compute_delta is fe_features.compute_delta and callable(frontend.label_fusion)
    code = ("import sidekit_amd; sidekit_amd.install_as_sidekit(); import sidekit.features_server, sidekit.frontend.normfeat, sidekit.frontend.features; "
            "from sidekit.frontend.normfeat import stg; from sidekit.frontend.features import compute_delta; "
            "assert sidekit.features_server.FeaturesServer is sidekit_amd.features_server.FeaturesServer; "
            "assert stg is sidekit_amd.frontend.normfeat.stg and compute_delta is sidekit_amd.frontend.features.compute_delta; "
            "assert sidekit.FeaturesServer is sidekit_amd.FeaturesServer")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_import_loads_neither_torch_nor_the_library():
    code = ("import sys, sidekit_amd, sidekit_amd.features_server, sidekit_amd.frontend, sidekit_amd.frontend.normfeat, sidekit_amd.frontend.features; "
            "sidekit_amd.FeaturesServer; import sidekit_amd._lib as l; "
            "assert 'torch' not in sys.modules and l._lib is None, sorted(m for m in sys.modules if m.startswith('torch'))[:3]")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


class Source:
    def __init__(self, feat, label=None):
        self.feat, self.label = feat, label

    def extract(self, show, channel, input_audio_filename=None):
        return self.feat, self.label


def test_unbuilt_options_raise():
    feat = numpy.zeros((8, 3), dtype=numpy.float32)
    with pytest.raises(NotImplementedError, match="HDF5"):
        FeaturesServer(dataset_list='["cep"]').load("show")
    with pytest.raises(NotImplementedError, match="HDF5"):
        FeaturesServer().stack_features(["show"])
    src = Source(feat)
    for kw, word in ((dict(sources=((FeaturesServer(), False),)), "sources"), (dict(dct_pca=True), "dct_pca"), (dict(sdc=True), "sdc"),
                     (dict(context=(2, 2)), "context"), (dict(traps_dct_nb=4), "TRAP")):
        with pytest.raises(NotImplementedError, match=word):
            FeaturesServer(features_extractor=src, **kw).load("show")
    with pytest.raises(NotImplementedError, match="get_features_per_speaker"):
        FeaturesServer(features_extractor=src).get_features_per_speaker("show", None)
    with pytest.raises(NotImplementedError, match="sources"):
        FeaturesServer(features_extractor=src).get_tandem_features("show")
    with pytest.raises(NotImplementedError, match="dct_pca"):
        FeaturesServer(dct_pca=True).post_processing(feat, None)


def test_without_a_gpu_the_compute_calls_raise(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    feat = numpy.arange(40, dtype=numpy.float64).reshape(10, 4)
    keep = feat.copy()
    server = FeaturesServer(features_extractor=Source(feat), feat_norm="cmvn", delta=True)
    calls = (lambda: normfeat.rasta_filt(feat), lambda: normfeat.cms(feat), lambda: normfeat.cmvn(feat), lambda: normfeat.stg(feat),
             lambda: normfeat.cep_sliding_norm(feat), lambda: fe_features.compute_delta(feat), lambda: server.post_processing(feat, None),
             lambda: server.load("a"), lambda: server.stack_features(["a"]), lambda: server.stack_features_device(["a"]),
             lambda: server._normalize(None, feat), lambda: server._delta_and_2delta(feat),
             lambda: features_server.post_process_device(feat, None), lambda: features_server.rasta_device(feat),
             lambda: features_server.delta_device(feat), lambda: features_server.segment_moments_device(feat),
             lambda: features_server.normalise_device(feat))
    for call in calls:
        with pytest.raises(RuntimeError, match="no GPU is visible"):
            call()
    numpy.testing.assert_array_equal(feat, keep)


def test_refusals_that_need_no_gpu():
    feat = numpy.zeros((10, 4))
    with pytest.raises(Exception, match="odd length"):
        normfeat.stg(feat, win=300)
    with pytest.raises(ValueError, match="odd length"):
        normfeat.cep_sliding_norm(feat, win=300)
    with pytest.raises(ValueError, match="taps"):
        fe_features.compute_delta(feat, win=2)
    with pytest.raises(ValueError, match="taps"):
        fe_features.compute_delta(feat, win=3, filt=numpy.array([.2, .1, 0, -.1, -.2]))


def test_mask_parser():
    assert features_server.parse_mask('[1-3,10,15-20]') == [1, 2, 3, 10, 15, 16, 17, 18, 19, 20]
    assert features_server.parse_mask('[ 0 - 2 , 7 ]') == [0, 1, 2, 7] and features_server.parse_mask('[4]') == [4]
    assert FeaturesServer(mask='[0-12]').mask == list(range(13)) and FeaturesServer().mask is None
    for bad in ('[1-3;5]', '[a]', '[1-2-3]'):
        with pytest.raises(Exception, match="Wrong mask format"):
            features_server.parse_mask(bad)
    with pytest.raises(Exception, match="filter list is empty"):
        server = FeaturesServer()
        server.mask = []
        server._mask(numpy.zeros((3, 3)))
    assert FeaturesServer(mask='[0,2]')._mask(numpy.arange(12).reshape(3, 4)).tolist() == [[0, 2], [4, 6], [8, 10]]


def test_source_rows_and_the_one_entry_cache(monkeypatch):
    """start / stop cut the source rows before post-processing, the first / last row replicated beyond the stream; load() keeps its last result"""
    feat = numpy.arange(20, dtype=numpy.float32).reshape(10, 2)
    label = numpy.array([1, 1, 0, 1, 1, 1, 0, 1, 1, 1], dtype=bool)
    server = FeaturesServer(features_extractor=Source(feat, label))
    f, l, gm, gs = server._source("a", 0, None, None, -2, 12)
    assert gm is None and gs is None and f.shape == (14, 2) and l.shape == (14,)
    numpy.testing.assert_array_equal(f[:3], feat[[0, 0, 0]])
    numpy.testing.assert_array_equal(f[-3:], feat[[9, 9, 9]])
    numpy.testing.assert_array_equal(l, numpy.concatenate(([True, True], label, [True, True])))
    f, l, _, _ = server._source("a", 0, None, None, 2, 7)
    numpy.testing.assert_array_equal(f, feat[2:7])
    numpy.testing.assert_array_equal(l, label[2:7])
    f, l, _, _ = FeaturesServer(features_extractor=Source(feat))._source("a", 0, None, None, None, None)
    assert l.all() and l.shape == (10,)
    calls = []
    monkeypatch.setattr(FeaturesServer, "get_features", lambda self, show, **kw: calls.append((show, kw["start"], kw["stop"])) or (show, kw["start"]))
    assert server.load("a") == ("a", None) and server.load("a") == ("a", None) and calls == [("a", None, None)]
    assert server.load("a", start=3, stop=9) == ("a", 3) and server.load("b", start=3, stop=9) == ("b", 3) and len(calls) == 3
    assert server.load("a") == ("a", None) and len(calls) == 4, "one entry only"
