"""Context features without a GPU (sidekit_amd/features_context.py, frontend/features.py, csrc/context.hip): the entry points' own header
against their binding table and the built library, their argument checks through the C ABI, the numpy restatement
(tests/tools/context_numpy.py) against the reference's outputs (tests/golden/context.npz), the composite projection matrix, the
refusals, the reference's parameter lists and the package wiring."""
import inspect
import os
import re
import subprocess
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

import context_numpy as cn  # noqa: E402
import sidekit_amd  # noqa: E402
from sidekit_amd import _lib, features_context as fc  # noqa: E402
from sidekit_amd.features_server import FeaturesServer  # noqa: E402
from sidekit_amd.frontend import features as fe_features  # noqa: E402

ENTRIES = ["sc_ctx_basis", "sc_ctx_gather", "sc_ctx_project"]
RTOL = 1e-12


@pytest.fixture(scope="module")
def fx():
    with numpy.load(os.path.join(ROOT, "tests", "golden", "context.npz")) as z:
        return {k: z[k] for k in z.files}


def _streams(fx, D, lengths):
    by_len = dict(zip(cn.LENGTHS, cn.split(fx["x_D%d" % D], cn.LENGTHS)))
    return [by_len[n] for n in lengths]


def _close(got, ref):
    return got.shape == ref.shape and numpy.abs(got - ref).max() <= RTOL * max(numpy.abs(ref).max(), 1.0)


def test_header_binding_table_and_library_agree():
    import ctypes
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sidekit_amd", "context.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?(?:int|char\s*\*|void)\s*\**\s*((?:xt|sc|sk)_\w+)\s*\(", src, flags=re.M)))
    assert declared == ENTRIES
    assert sorted(_lib.CONTEXT_SIGNATURES) == declared, "ctypes binding table and header disagree"
    others = [getattr(_lib, name) for name in dir(_lib) if name.endswith("SIGNATURES") and name != "CONTEXT_SIGNATURES"]
    assert len(others) >= 15 and not any(set(_lib.CONTEXT_SIGNATURES) & set(t) for t in others), "the table is disjoint from the other tables"
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(cdll, name), f"{name} declared in include/sidekit_amd/context.h but not exported"
    lib = _lib.lib()
    ctype = {"void*": _lib._P, "int32_t": _lib._I32, "int64_t": _lib._I64, "double": _lib._F64}
    flat = re.sub(r"\s+", " ", src)
    for name, (res, args) in _lib.CONTEXT_SIGNATURES.items():
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
        params = re.search(r"int %s\((.*?)\);" % name, flat).group(1).split(",")
        kinds = ["void*" if "*" in q else q.replace("const", "").split()[0] for q in params]
        assert [ctype[k] for k in kinds] == args, (name, kinds)
    define = lambda n: int(re.search(r"#define %s (\d+)" % n, src).group(1))   # noqa: E731
    assert (define("SC_CTX_MAX_BLOCKS"), define("SC_CTX_MAX_SPAN"), define("SC_CTX_MAX_W"), define("SC_CTX_PROJ_MAX_D"), define("SC_CTX_PROJ_MAX_Q")) == \
        (fc.MAX_BLOCKS, fc.MAX_SPAN, fc.MAX_W, fc.PROJ_MAX_D, fc.PROJ_MAX_Q) == (256, 256, 64, 128, 512)
    assert (define("SC_CTX_TILE"), define("SC_CTX_BASIS_TILE"), define("SC_CTX_PROJ_TILE"), define("SC_CTX_COLS")) == (256, 128, 64, 16)
    assert "context.hip" in open(os.path.join(ROOT, "sidekit_amd", "csrc", "Makefile")).read()


def test_lds_budgets_are_the_stated_ones():
    """The budgets the header and the kernel file state, recomputed from the header's own constants and the kernels' layouts"""
    header = open(os.path.join(ROOT, "include", "sidekit_amd", "context.h")).read()
    kernels = open(os.path.join(ROOT, "sidekit_amd", "csrc", "context.hip")).read()
    define = lambda n: int(re.search(r"#define %s (\d+)" % n, header).group(1))   # noqa: E731
    tile, cols, span, blocks = define("SC_CTX_TILE"), define("SC_CTX_COLS"), define("SC_CTX_MAX_SPAN"), define("SC_CTX_MAX_BLOCKS")
    basis_tile, max_w, proj = define("SC_CTX_BASIS_TILE"), define("SC_CTX_MAX_W"), define("SC_CTX_PROJ_TILE")
    gather = (tile + span) * cols * 4 + 2 * blocks * 4
    basis = lambda W, J: W * J * 8 + ((basis_tile + W - 1) | 1) * cols * 4   # noqa: E731
    project = 2 * proj * 17 * 8 + proj * (proj + 1) * 8
    assert (gather, basis(max_w, max_w), project) == (34816, 44992, 50688)
    assert max(basis(W, J) for W in range(1, max_w + 1) for J in range(1, W + 1)) == 44992
    assert max(gather, 44992, project) <= 65536, "what a kernel may declare without asking for more"
    for text in (header, kernels):
        assert "34,816 B" in text and "44,992 B" in text and "50,688 B" in text, "the header and the kernel file state the same budget"


def test_entry_points_check_their_arguments_before_anything_is_enqueued():
    """SK_EARG through the C ABI on a host with no GPU: nothing was enqueued, or there would have been a HIP error instead."""
    lib = _lib.lib()
    p, q = 4096, 8192   # any non-null addresses: a refused call dereferences nothing

    def gather(x=p, ldx=5, off=p, S=2, D=5, max_rows=10, plus=p, minus=p, J=7, lo=-1, span=20, y=q, ldy=35):
        return lib.sc_ctx_gather(x, ldx, off, S, D, max_rows, plus, minus, J, lo, span, y, ldy, None)

    def basis(x=p, ldx=5, off=p, S=2, D=5, max_rows=10, b=p, W=25, J=25, left=12, y=q, ldy=125):
        return lib.sc_ctx_basis(x, ldx, off, S, D, max_rows, b, W, J, left, y, ldy, None)

    def project(x=p, ldx=5, off=p, S=2, D=5, max_rows=10, m=p, W=25, left=12, Q=60, y=q, ldy=60):
        return lib.sc_ctx_project(x, ldx, off, S, D, max_rows, m, W, left, Q, y, ldy, None)

    cases = {}
    for name, call in (("gather", gather), ("basis", basis), ("project", project)):
        cases.update({f"{name} x null": call(x=None), f"{name} offsets null": call(off=None), f"{name} y null": call(y=None),
                      f"{name} S < 0": call(S=-1), f"{name} D = 0": call(D=0), f"{name} D < 0": call(D=-3), f"{name} ldx < D": call(ldx=4),
                      f"{name} x == y": call(y=p), f"{name} max_rows = 0": call(max_rows=0)})
    cases.update({"gather plus null": gather(plus=None), "gather J = 0": gather(J=0), "gather J = 257": gather(J=257), "gather ldy < J D": gather(ldy=34),
                  "gather span < 0": gather(span=-1), "gather span 257": gather(span=257), "gather lo -257": gather(lo=-257), "gather lo 257": gather(lo=257),
                  "basis table null": basis(b=None), "basis W = 0": basis(W=0, J=0, left=0), "basis W = 65": basis(W=65), "basis J = 0": basis(J=0),
                  "basis J > W": basis(J=26), "basis left < 0": basis(left=-1), "basis left = W": basis(left=25), "basis ldy < D J": basis(ldy=124),
                  "project matrix null": project(m=None), "project W = 0": project(W=0, left=0), "project W = 65": project(W=65),
                  "project left < 0": project(left=-1), "project left = W": project(left=25), "project Q = 0": project(Q=0),
                  "project Q = 513": project(Q=513, ldy=513), "project D = 129": project(D=129, ldx=129), "project ldy < Q": project(ldy=59)})
    assert all(rc == _lib.SK_EARG for rc in cases.values()), {k: v for k, v in cases.items() if v != _lib.SK_EARG}
    for call, name in ((gather, "sc_ctx_gather"), (basis, "sc_ctx_basis"), (project, "sc_ctx_project")):
        assert call(D=0) == _lib.SK_EARG and name in _lib.last_error(), "the message names the entry"
    # an empty batch is nothing to do, not an error (S = 0: nothing is enqueued either), at the limits too
    assert gather(S=0) == basis(S=0) == project(S=0) == _lib.SK_OK
    assert gather(S=0, minus=None) == gather(S=0, J=256, ldy=1280, span=256, lo=-256) == gather(S=0, lo=0, span=0, J=1) == _lib.SK_OK
    assert basis(S=0, W=64, J=64, left=63, ldy=320) == basis(S=0, W=1, J=1, left=0) == _lib.SK_OK
    assert project(S=0, W=64, left=0, D=128, ldx=128, Q=512, ldy=512) == project(S=0, W=1, left=0, Q=1, ldy=1) == _lib.SK_OK


def test_restatement_reproduces_the_reference(fx):
    """SDC and the stacked context bit for bit; the DCT, its projection and TRAPs within 1e-12 relative in float64"""
    checked = 0
    for name, (kind, D, lengths, cfg) in cn.cases().items():
        refs = cn.split(fx[name], lengths)
        for s, ref in zip(_streams(fx, D, lengths), refs):
            if kind == "sdc":
                got = cn.sdc(s, *cfg)
                assert got.dtype == ref.dtype == numpy.float32 and numpy.array_equal(got, ref), name
            elif kind == "ctx":
                assert numpy.array_equal(cn.context(s, *cfg), ref), name
            elif kind == "dct":
                assert _close(cn.pca_dct(s, *cfg), ref), name
            elif kind == "pca":
                assert _close(cn.pca_dct(s, cfg[0], cfg[1], fx[cn.pca_name(cfg[0], cfg[1], D, cfg[2])]), ref), name
            else:
                assert _close(cn.traps(s, *cfg), ref), name
            checked += 1
    assert checked >= 100
    s = _streams(fx, 5, (40,))[0]
    for i, rows in enumerate(cn.RANGES):
        assert numpy.array_equal(cn.context(s, 3, 2, rows), fx["range_ctx_%d" % i])
        if "range_traps_%d" % i in fx:
            assert _close(cn.traps(s, 3, 2, 4, rows), fx["range_traps_%d" % i])
    assert sorted(i for i in range(len(cn.RANGES)) if "range_traps_%d" % i in fx) == [0, 2, 3], "the reference's get_traps raises when start > context[0]"


def test_host_tables(fx):
    """The tables the kernels are given: offsets, bases, and the composite of basis and PCA against the two-step product"""
    assert fc.context_offsets(3, 2).tolist() == [-3, -2, -1, 0, 1, 2] and fc.context_offsets(0, 0).tolist() == [0]
    plus, minus = fc.sdc_offsets(1, 3, 7)
    assert plus.tolist() == [-1, 2, 5, 8, 11, 14, 17] and minus.tolist() == [1, 4, 7, 10, 13, 16, 19] and plus.dtype == numpy.int32
    for left, right in cn.WINDOWS:
        assert _close(fc.dct_pca_basis(left, right), cn.dct_pca_basis(left, right))
        B = fc.dct_pca_basis(left, right)
        assert numpy.abs(B.T @ B - numpy.eye(B.shape[0])).max() < 1e-14, "the full DCT basis is orthonormal"
    assert _close(fc.traps_basis(12, 12, 16), cn.traps_basis(12, 12, 16)) and fc.traps_basis(3, 2, 4).shape == (6, 4)
    for (left, right, D, Q) in ((12, 12, 5, 7), (12, 12, 5, 40), (3, 2, 13, 7), (0, 2, 13, 40)):
        P, B = fx[cn.pca_name(left, right, D, Q)], fc.dct_pca_basis(left, right)
        M = fc.projection_matrix(B, P, D)
        assert M.shape == ((left + right + 1) * D, Q) and M.dtype == numpy.float64 and M.flags.c_contiguous
        assert _close(M, cn.composite(B, P, D))
        s = _streams(fx, D, (40,))[0]
        two_step = cn.pca_dct(s, left, right, P)
        one_step, _ = cn.project(s, M, left + right + 1, left)
        assert _close(one_step, two_step), "windows . M equals (windows . B) . P"


def test_refusals_that_need_no_gpu():
    x = numpy.zeros((10, 4), dtype=numpy.float32)
    for d, p, k in ((1, 4, 5), (1, 5, 4), (1, 4, 13), (2, 7, 2)):
        assert (k - 1) * p > 3 * k
        for call in (lambda: fc.sdc_device(x, None, d, p, k), lambda: fe_features.shifted_delta_cepstral(x, d, p, k),
                     lambda: fc.post_process_context_device(x, None, sdc=True, sdc_config=(d, p, k))):
            with pytest.raises(ValueError, match=r"\(k - 1\) p .* 3 k .*pads 3 k \+ d rows"):
                call()
    fc.sdc_offsets(1, 4, 4), fc.sdc_offsets(1, 3, 10), fc.sdc_offsets(5, 6, 2)      # on the boundary
    for bad in ((0, 3, 7), (1, 0, 7), (1, 3, 0), (1.5, 3, 7)):
        with pytest.raises(ValueError, match="integer"):
            fc.sdc_offsets(*bad)
    for call in (lambda: fc.pca_dct_device(x, None, 32, 32), lambda: fc.traps_device(x, None, 40, 24, 4), lambda: fe_features.pca_dct(x, 64, 0),
                 lambda: fc.post_process_context_device(x, None, dct_pca=True, dct_pca_config=(40, 40, None))):
        with pytest.raises(ValueError, match="beyond the 64 frames"):
            call()
    fc._window(32, 31), fc._window(0, 63)
    with pytest.raises(ValueError, match="beyond the 256 blocks"):
        fc.context_device(x, None, 128, 128)
    with pytest.raises(ValueError, match="beyond the 256 blocks"):
        fc.sdc_device(x, None, 100, 1, 60)
    with pytest.raises(ValueError, match="DCT coefficients of a window"):
        fc.traps_device(x, None, 1, 1, 4)
    with pytest.raises(ValueError, match="negative|integer"):
        fc.context_device(x, None, -1, 2)
    B = fc.dct_pca_basis(1, 1)
    with pytest.raises(ValueError, match="rows"):
        fc.projection_matrix(B, numpy.zeros((11, 3)), 4)
    with pytest.raises(ValueError, match="beyond the 128 coefficients / 512 columns"):
        fc.projection_matrix(B, numpy.zeros((12, 513)), 4)
    with pytest.raises(ValueError, match="beyond the 128 coefficients / 512 columns"):
        fc.projection_matrix(B, numpy.zeros((3 * 129, 5)), 129)
    with pytest.raises(TypeError, match="unexpected options"):
        fc.post_process_context_device(x, None, sdc=True, context=(1, 1))


class Source:
    def __init__(self, feat, label=None):
        self.feat, self.label = feat, label

    def extract(self, show, channel, input_audio_filename=None):
        return self.feat, self.label


def test_features_server_keeps_its_refusals():
    feat = numpy.zeros((8, 3), dtype=numpy.float32)
    src = Source(feat)
    for kw, word in ((dict(dct_pca=True), "dct_pca"), (dict(sdc=True), "sdc"), (dict(context=(2, 2)), "context"), (dict(traps_dct_nb=4), "TRAP")):
        with pytest.raises(NotImplementedError, match=word) as err:
            FeaturesServer(features_extractor=src, **kw).load("show")
        assert "ContextFeaturesServer" in str(err.value), "the message names the class that builds it"
    for kw, word in ((dict(dct_pca=True), "dct_pca"), (dict(sdc=True), "sdc")):
        with pytest.raises(NotImplementedError, match=word):
            FeaturesServer(**kw).post_processing(feat, None)
    assert not hasattr(FeaturesServer, "get_context") and not hasattr(FeaturesServer, "get_traps")
    # the subclass still refuses what nobody builds
    with pytest.raises(NotImplementedError, match="HDF5"):
        fc.ContextFeaturesServer(sdc=True).load("show")
    with pytest.raises(NotImplementedError, match="sources"):
        fc.ContextFeaturesServer(features_extractor=src, sources=((FeaturesServer(), False),)).load("show")


def test_without_a_gpu_the_compute_calls_raise(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    feat = numpy.arange(40, dtype=numpy.float64).reshape(10, 4)
    keep = feat.copy()
    P = numpy.ones((12, 2))
    server = fc.ContextFeaturesServer(features_extractor=Source(feat), sdc=True, context=(1, 1), traps_dct_nb=2)
    pca = fc.ContextFeaturesServer(features_extractor=Source(feat), dct_pca=True, dct_pca_config=(1, 1, P))
    calls = (lambda: fc.context_device(feat, None, 1, 1), lambda: fc.sdc_device(feat, None), lambda: fc.pca_dct_device(feat, None, 1, 1),
             lambda: fc.pca_dct_device(feat, None, 1, 1, P), lambda: fc.traps_device(feat, None, 1, 1, 2),
             lambda: fc.post_process_context_device(feat, None, sdc=True), lambda: fc.post_process_context_device(feat, None),
             lambda: fe_features.shifted_delta_cepstral(feat), lambda: fe_features.pca_dct(feat, 1, 1), lambda: server.load("a"),
             lambda: server.post_processing(feat, None), lambda: server.stack_features(["a"]), lambda: server.stack_features_device(["a"]),
             lambda: server.get_context(feat), lambda: server.get_traps(feat), lambda: pca.load("a"))
    for call in calls:
        with pytest.raises(RuntimeError, match="no GPU is visible"):
            call()
    numpy.testing.assert_array_equal(feat, keep)


def test_reference_parameter_lists_and_wiring():
    server = fc.ContextFeaturesServer
    assert str(inspect.signature(server.__init__)) == str(inspect.signature(FeaturesServer.__init__))
    assert str(inspect.signature(server.get_context)) == str(inspect.signature(server.get_traps)) == "(self, feat, start=None, stop=None, label=None)"
    for name in ("post_processing", "load", "get_features", "stack_features", "stack_features_device"):
        assert str(inspect.signature(getattr(server, name))) == str(inspect.signature(getattr(FeaturesServer, name)))
    functions = {fc.context_device: "(frames, seg_off, left, right, out=None)", fc.sdc_device: "(frames, seg_off, d=1, p=3, k=7)",
                 fc.pca_dct_device: "(frames, seg_off, left_ctx=12, right_ctx=12, p=None)",
                 fc.traps_device: "(frames, seg_off, left, right, dct_nb)",
                 fc.post_process_context_device: "(frames, seg_off, labels=None, *, dct_pca=False, dct_pca_config=None, sdc=False, "
                                                 "sdc_config=None, **options)",
                 fe_features.pca_dct: "(cep, left_ctx=12, right_ctx=12, p=None)", fe_features.shifted_delta_cepstral: "(cep, d=1, p=3, k=7)",
                 fe_features.dct_basis: "(nbasis, length)"}
    for fn, sig in functions.items():
        assert str(inspect.signature(fn)) == sig, fn.__name__
    made = server(dct_pca=True, context=(3, 2), traps_dct_nb=4)
    assert (made.dct_pca, made.dct_pca_config, made.sdc, made.sdc_config, made.context, made.traps_dct_nb) == (True, (12, 12, None), False, (1, 3, 7), (3, 2), 4)
    assert "dct_pca: True" in repr(made)
    assert "features_context" in sidekit_amd.SUBMODULES and sidekit_amd._LAZY["ContextFeaturesServer"] == "features_context"
    assert sidekit_amd.ContextFeaturesServer is server
    import sidekit_amd.frontend as frontend
    assert frontend.pca_dct is fe_features.pca_dct and frontend.shifted_delta_cepstral is fe_features.shifted_delta_cepstral
    code = ("import sys, sidekit_amd, sidekit_amd.features_context; sidekit_amd.ContextFeaturesServer; import sidekit_amd._lib as l; "
            "assert 'torch' not in sys.modules and l._lib is None; sidekit_amd.install_as_sidekit(); import sidekit.features_context; "
            "from sidekit.frontend.features import pca_dct, shifted_delta_cepstral")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
