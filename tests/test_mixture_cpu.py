"""The diagonal GMM without a GPU (sidekit_amd/mixture.py, csrc/gmm.hip): the numpy restatement the GPU tests lean on against the
reference's own output (tests/golden/mixture.npz, written by make_mixture_golden.py from the imported reference module), the reference's
signatures, the host half of EM against the restatement, the HDF5 file, the refusals, the ``sidekit`` alias, the entry points' own
header against their binding table and the built library, and their argument checks through the C ABI.

The restatement is held to 1e-12 relative max-norm, the bar make_backend_golden.py sets for a restatement of float64 algebra (the
generator measured at most 6.8e-16 on this set).
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
import mixture_numpy as mxn  # noqa: E402

from sidekit_amd import _lib, mixture  # noqa: E402
from sidekit_amd.mixture import Mixture  # noqa: E402
from sidekit_amd.statserver import StatServer  # noqa: E402

RESTATEMENT_TOL = 1e-12
KEYS = ("w", "mu", "invcov", "cov_var_ctl")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(numpy.load(os.path.join(golden_dir, "mixture.npz")))


def _state(fx, tag):
    return {k: fx[f"{tag}_{k}"] for k in KEYS}


def _mixture(state):
    m = Mixture()
    m.w, m.mu, m.invcov, m.cov_var_ctl = (numpy.array(state[k], dtype=numpy.float64) for k in KEYS)
    m.cst, m.det = numpy.zeros(m.w.shape), numpy.zeros(m.w.shape)
    m._compute_all()
    return m


def _assert_all(errs, tol=RESTATEMENT_TOL):
    print({k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < tol, f"{k} differs by {v:.3e} (relative max-norm, bound {tol})"


def test_restatement_matches_the_reference_fixture(fx):
    X, off = fx["X"], fx["seg_off"]
    errs = {}
    for i, (m, llk) in enumerate(mxn.em_split(X, 8, (1, 2, 2), off)):
        errs.update({f"split{i} {k}": mxn.rel(m[k], fx[f"split{i}_{k}"]) for k in KEYS})
        errs[f"split{i} llk"] = mxn.rel(llk, fx["split_llk"][i])
    four = mxn.model(*(fx[f"split2_{k}"] for k in KEYS))
    for i, (m, llk) in enumerate(mxn.em_uniform(four, X, 3, 3)):
        errs.update({f"uniform{i} {k}": mxn.rel(m[k], fx[f"uniform{i}_{k}"]) for k in KEYS})
        errs[f"uniform{i} llk"] = mxn.rel(llk, fx["uniform_llk"][i])
    early = mxn.em_uniform(four, X, 1, 10, float(fx["early_gain"]))
    assert len(early) == int(fx["early_iterations"]) < 10
    errs["early llk"] = mxn.rel([l for _, l in early], fx["early_llk"])
    final = mxn.model(*(fx[f"split4_{k}"] for k in KEYS))
    s0, s1, s2, llk = mxn.stats(final, X, off)
    lp = mxn.log_posteriors(final, X)
    pp, total = mxn.sum_log_probabilities(lp)
    errs.update({"A": mxn.rel(final["A"], fx["final_A"]), "cst": mxn.rel(final["cst"], fx["final_cst"]), "det": mxn.rel(final["det"], fx["final_det"]),
                 "lp": mxn.rel(lp, fx["lp"]), "lp, replaced mu": mxn.rel(mxn.log_posteriors(final, X, fx["new_mu"].flatten()), fx["lp_new_mu"]),
                 "pp": mxn.rel(pp.sum(0), fx["pp_sum"]), "total llk": mxn.rel(total, fx["total_llk"]), "llk per segment": mxn.rel(llk.sum(), fx["accum_llk"]),
                 "accum w": mxn.rel(s0.sum(0), fx["accum_w"]), "accum mu": mxn.rel(s1.sum(0), fx["accum_mu"]),
                 "accum invcov": mxn.rel(s2.sum(0), fx["accum_invcov"]), "accumulate_stat stat0": mxn.rel(s0, fx["acc_stat0"]),
                 "accumulate_stat stat1": mxn.rel(s1.reshape(8, -1), fx["acc_stat1"])})
    _assert_all(errs)


def test_fixture_is_the_set_its_generator_describes(fx):
    rs = numpy.random.RandomState(11)
    centres, scales = 2 * rs.randn(6, 23), 0.5 + rs.rand(6, 23)
    lengths = [3, 301, 0, 64, 130, 17, 700, 45]
    cls = rs.randint(0, 6, sum(lengths))
    numpy.testing.assert_array_equal(fx["X"], centres[cls] + scales[cls] * rs.randn(sum(lengths), 23) + 0.3)
    assert list(fx["lengths"]) == lengths and list(fx["seg_off"]) == list(numpy.concatenate(([0], numpy.cumsum(lengths)))) and fx["X"].shape == (1260, 23)
    assert [fx[f"split{i}_w"].shape[0] for i in range(5)] == [2, 4, 4, 8, 8] and fx["split_llk"].shape == (5,) and fx["uniform_llk"].shape == (3,)
    assert numpy.all(numpy.diff(fx["split_llk"]) > 0), "EM with splits raises the likelihood on this set"
    assert 0.002 < fx["split4_w"].min() < 0.004, "the smallest component holds about 3.5 frames"
    # no flooring decision can flip: every M-step's variance ratio is strictly inside (floor, ceil) = (0.01, 10)
    for tag in [f"split{i}" for i in range(5)] + [f"uniform{i}" for i in range(3)]:
        ratio = (1.0 / fx[f"{tag}_invcov"]) / fx[f"{tag}_cov_var_ctl"]
        assert 0.03 < ratio.min() and ratio.max() < 3.0, (tag, ratio.min(), ratio.max())
    gains = numpy.diff(fx["early_llk"])
    G = float(fx["early_gain"])
    assert numpy.all((gains >= 3 * G) | (gains <= G / 3)) and gains[-1] <= G / 3, "the early stop is at least a factor 3 from every recorded gain"
    assert fx["init5_w"].shape == (5,) and fx["acc_stat0"].shape == (8, 8) and numpy.all(fx["acc_stat0"][2] == 0) and fx["lp"].shape == (1260, 8)


def test_reference_signatures():
    expect = {"__init__": "(self, mixture_file_name='', name='empty')", "read": "(self, mixture_file_name, prefix='')",
              "write": "(self, mixture_file_name, prefix='', mode='w')", "get_distrib_nb": "(self)", "distrib_nb": "(self)", "dim": "(self)",
              "sv_size": "(self)", "_compute_all": "(self)", "validate": "(self)", "get_mean_super_vector": "(self)",
              "get_invcov_super_vector": "(self)", "compute_log_posterior_probabilities": "(self, cep, mu=None)",
              "compute_log_posterior_probabilities_full": "(self, cep, mu=None)", "variance_control": "(cov, flooring, ceiling, cov_ctl)",
              "_reset": "(self)", "_split_ditribution": "(self)", "_expectation": "(self, accum, cep)",
              "_maximization": "(self, accum, ceil_cov=10, floor_cov=0.01)", "_init_uniform": "(self, cep, distrib_nb)",
              "EM_uniform": "(self, cep, distrib_nb, iteration_min=3, iteration_max=10, llk_gain=0.01, do_init=True)",
              "EM_split": "(self, features_server, feature_list, distrib_nb, iterations=(1, 2, 2, 4, 4, 4, 4, 8, 8, 8, 8, 8, 8), num_thread=1, "
                          "llk_gain=0.01, save_partial=False, output_file_name='ubm', ceil_cov=10, floor_cov=0.01)",
              "EM_diag2full": "(self, diagonal_mixture, features_server, featureList, iterations=2, num_thread=1)",
              "init_from_diag": "(self, diag_mixture)"}
    for name, sig in expect.items():
        assert str(inspect.signature(getattr(Mixture, name))) == sig, name
    device = {"frame_loglik_device": "(ubm, frames, mu=None)",
              "gmm_stats_device": "(ubm, frames, seg_off=None, order=2, max_workspace_bytes=1073741824)",
              "em_split_device": "(frames, distrib_nb, iterations=(1, 2, 2, 4, 4, 4, 4, 8, 8, 8, 8, 8, 8), init_frames=None, ceil_cov=10, "
                                 "floor_cov=0.01, after_iteration=None)"}
    for name, sig in device.items():
        assert str(inspect.signature(getattr(mixture, name))) == sig, name
    assert str(inspect.signature(StatServer.accumulate_stat)) == "(self, ubm, feature_server, seg_indices=None, channel_extension=('', '_b'), num_thread=1)"
    assert str(inspect.signature(StatServer.accumulate_stat_device)) == "(self, ubm, frames, seg_off)"
    m = Mixture()
    assert sorted(vars(m)) == sorted(["w", "mu", "invcov", "invchol", "cov_var_ctl", "cst", "det", "A", "name"]) and m.name == "empty" and m.A == 0


def test_init_uniform_matches_the_fixture(fx):
    m = Mixture()
    m._init_uniform(fx["X"], 5)
    errs = {k: mxn.rel(getattr(m, k), fx[f"init5_{k}"]) for k in KEYS}
    errs["A"] = mxn.rel(m.A, fx["init5_A"])
    _assert_all(errs)
    # the reference's behaviour, pinned: every window runs to the end of the frames and components after the first keep the second moment
    X = fx["X"]
    numpy.testing.assert_allclose(m.mu[3], X[1260 // 5 * 3:].mean(0), rtol=1e-13)
    numpy.testing.assert_allclose(m.invcov[3], (X[1260 // 5 * 3:] ** 2).mean(0), rtol=1e-13)
    numpy.testing.assert_allclose(m.invcov[0], 1.0 / (X ** 2).mean(0), rtol=1e-13)


def test_host_half_against_the_restatement(fx):
    X, off = fx["X"], fx["seg_off"]
    errs = {}
    single = Mixture()
    single._init_single(X.mean(0), (X ** 2).mean(0))
    ref = mxn.init_single(X)
    errs.update({f"init {k}": mxn.rel(getattr(single, k), ref[k]) for k in KEYS + ("A", "cst", "det")})
    single._split_ditribution()
    ref = mxn.split(ref)
    errs.update({f"split {k}": mxn.rel(getattr(single, k), ref[k]) for k in KEYS + ("A", "cst", "det")})
    # M-step from the restatement's statistics of a recorded state
    state = _state(fx, "split2")
    ref = mxn.model(*(state[k] for k in KEYS))
    s0, s1, s2, _ = (t.sum(0) for t in mxn.stats(ref, X, off))
    m = _mixture(state)
    accum = copy.deepcopy(m)
    accum._reset()
    assert accum.A == 0.0 and not accum.w.any() and not accum.mu.any() and not accum.invcov.any()
    accum.w, accum.mu, accum.invcov = s0.copy(), s1.copy(), s2.copy()
    m._maximization(accum)
    nxt = mxn.maximization(ref, s0, s1, s2)
    errs.update({f"M-step {k}": mxn.rel(getattr(m, k), nxt[k]) for k in KEYS + ("A",)})
    _assert_all(errs)
    # variance control at a hand-made floor and ceiling: <= floor and >= ceil are replaced, the values between stay
    ctl = numpy.array([[1.0, 2.0, 4.0], [0.5, 1.0, 2.0]])
    cov = numpy.array([[0.01, 0.5, 40.0], [0.004, 11.0, 1.9]])
    want = numpy.array([[0.01, 0.5, 40.0], [0.005, 10.0, 1.9]])
    got = Mixture.variance_control(cov.copy(), 1e-2, 10, ctl)
    numpy.testing.assert_array_equal(got, want)
    numpy.testing.assert_array_equal(mxn.variance_control(cov, 1e-2, 10, ctl), want)
    # an M-step that hits both: the restatement and the class floor and ceil the same elements
    m2, a2 = _mixture(state), copy.deepcopy(m)
    a2.w, a2.mu, a2.invcov = s0.copy(), s1.copy(), s2.copy()
    m2._maximization(a2, ceil_cov=0.3, floor_cov=0.2)
    lim = mxn.maximization(ref, s0, s1, s2, ceil_cov=0.3, floor_cov=0.2)
    ratio = (1.0 / m2.invcov) / m2.cov_var_ctl
    assert numpy.isclose(ratio.min(), 0.2) and numpy.isclose(ratio.max(), 0.3) and mxn.rel(m2.invcov, lim["invcov"]) < RESTATEMENT_TOL


def test_hdf5_round_trip(fx, tmp_path):
    """A ``Mixture`` through ``write`` and ``read`` (``hdf5_lite``): the reference's eight dataset names with its shapes, float64.  A file
    written by the reference's own writer cannot be produced where the fixtures are made (there is no h5py there), so the layout is
    checked against the reference's source (``mixture.py:374-408``) and not against a file of its making."""
    from sidekit_amd import hdf5_lite
    m = _mixture(_state(fx, "split4"))
    path = str(tmp_path / "ubm.h5")
    m.write(path)
    with hdf5_lite.File(path) as f:
        assert sorted(f.keys()) == sorted(["w", "mu", "invcov", "invchol", "cov_var_ctl", "cst", "det", "a"])
        shapes = {k: f[k][()].shape for k in f.keys()}
        assert all(f[k][()].dtype == numpy.float64 for k in f.keys())
    assert shapes == {"w": (8,), "mu": (8, 23), "invcov": (8, 23), "invchol": (0,), "cov_var_ctl": (8, 23), "cst": (8,), "det": (8,), "a": (8,)}
    back = Mixture(path)
    for k in KEYS + ("cst", "det", "A", "invchol"):
        numpy.testing.assert_array_equal(getattr(back, k), getattr(m, k))
    assert back.validate() and back.distrib_nb() == back.get_distrib_nb() == 8 and back.dim() == 23 and back.sv_size() == 184
    numpy.testing.assert_array_equal(back.get_mean_super_vector(), m.mu.flatten())
    numpy.testing.assert_array_equal(back.get_invcov_super_vector(), m.invcov.flatten())
    m.write(path, prefix="ubm/")
    other = Mixture()
    other.read(path, prefix="ubm/")
    numpy.testing.assert_array_equal(other.mu, m.mu)


def test_full_covariances_are_refused(fx):
    m = _mixture(_state(fx, "split0"))
    m.invcov = numpy.stack([numpy.diag(v) for v in m.invcov])
    assert m.validate()
    X = fx["X"][:4]
    for call in (lambda: m.compute_log_posterior_probabilities(X), lambda: m.compute_log_posterior_probabilities_full(X),
                 lambda: m._expectation(copy.deepcopy(m), X), lambda: m._compute_all(), lambda: m.init_from_diag(m),
                 lambda: m.EM_diag2full(m, None, []), lambda: m._maximization(m)):
        with pytest.raises(NotImplementedError, match="full-covariance"):
            call()
    for name in ("read_alize", "read_htk", "write_alize", "merge"):
        assert not hasattr(Mixture, name)
    with pytest.raises(AssertionError, match="diagonal"):
        m.get_invcov_super_vector()


def test_import_loads_neither_torch_nor_the_library():
    code = ("import sys, sidekit_amd.mixture, sidekit_amd._lib as l; "
            "assert 'torch' not in sys.modules and l._lib is None, sorted(m for m in sys.modules if m.startswith('torch'))[:3]")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_install_as_sidekit_resolves_mixture():
    import sidekit_amd
    assert "mixture" in sidekit_amd.SUBMODULES and sidekit_amd.Mixture is Mixture
    saved = {k: v for k, v in sys.modules.items() if k == "sidekit" or k.startswith("sidekit.")}
    try:
        sidekit_amd.install_as_sidekit()
        import sidekit.mixture
        from sidekit.mixture import Mixture as aliased   # the reference's own import line
        assert sidekit.mixture is mixture and aliased is Mixture
    finally:
        for k in [k for k in sys.modules if k == "sidekit" or k.startswith("sidekit.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_header_binding_table_and_library_agree():
    """What tests/test_abi.py checks for include/sidekit_amd.h, for the mixture's own header and table."""
    import ctypes
    import re
    src = open(os.path.join(ROOT, "include", "sidekit_amd", "mixture.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?(?:int|char\s*\*|void)\s*\**\s*((?:xt|sc|sk)_\w+)\s*\(", src, flags=re.M)))
    assert declared == ["sc_gmm_frame_loglik", "sc_gmm_stats"]
    assert sorted(_lib.MIXTURE_SIGNATURES) == declared, "ctypes binding table and header disagree"
    assert not set(_lib.MIXTURE_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.GAUSSIAN_SIGNATURES))
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(cdll, name), f"{name} declared in include/sidekit_amd/mixture.h but not exported"
    lib = _lib.lib()
    for name, (res, args) in _lib.MIXTURE_SIGNATURES.items():
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    ctype = {"void*": _lib._P, "int32_t": _lib._I32, "int64_t": _lib._I64, "double": _lib._F64}
    flat = re.sub(r"\s+", " ", src)
    for name, (_, args) in _lib.MIXTURE_SIGNATURES.items():
        params = re.search(r"int %s\((.*?)\);" % name, flat).group(1).split(",")
        kinds = ["void*" if "*" in q else q.replace("const", "").split()[0] for q in params]
        assert [ctype[k] for k in kinds] == args, (name, kinds)
    # the constants the Python side restates
    assert int(re.search(r"#define SC_GMM_MAX_SLABS (\d+)", src).group(1)) == mixture.MAX_SLABS
    assert int(re.search(r"#define SC_GMM_SLAB_FRAMES (\d+)", src).group(1)) == mixture.SLAB_FRAMES
    assert int(re.search(r"#define SC_GMM_MAX_D (\d+)", src).group(1)) >= 128


def test_entry_points_check_their_arguments_before_anything_is_enqueued():
    """SK_EARG through the C ABI on a host with no GPU: nothing was enqueued, or there would have been a HIP error instead."""
    lib = _lib.lib()
    p, F64, F32 = 4096, _lib.XT_F64, _lib.XT_F32   # any non-null address: a refused call dereferences nothing

    def loglik(X=p, dt=F64, N=5, D=4, mu=p, ic=p, A=p, C=3, lse=p, lp=None):
        return lib.sc_gmm_frame_loglik(X, dt, N, D, mu, ic, A, C, lse, lp, None)

    def stats(X=p, dt=F32, N=5, D=4, mu=p, ic=p, A=p, C=3, lse=p, off=p, S=1, max_len=5, order=2, s0=p, s1=p, s2=p, llk=None):
        return lib.sc_gmm_stats(X, dt, N, D, mu, ic, A, C, lse, off, S, max_len, order, s0, s1, s2, llk, None)

    cases = {"loglik X null": loglik(X=None), "loglik mu null": loglik(mu=None), "loglik invcov null": loglik(ic=None), "loglik A null": loglik(A=None),
             "loglik lse null": loglik(lse=None), "loglik C = 0": loglik(C=0), "loglik C > grid": loglik(C=65535 * 64 + 1), "loglik D = 0": loglik(D=0),
             "loglik D > LDS": loglik(D=129), "loglik N = 2^31": loglik(N=1 << 31), "loglik N = 0": loglik(N=0), "loglik bf16": loglik(dt=_lib.XT_BF16),
             "loglik i64": loglik(dt=_lib.XT_I64),
             "stats X null": stats(X=None), "stats mu null": stats(mu=None), "stats invcov null": stats(ic=None), "stats A null": stats(A=None),
             "stats lse null": stats(lse=None), "stats seg_off null": stats(off=None), "stats stat0 null": stats(s0=None),
             "stats stat1 null": stats(s1=None), "stats stat2 null with order 2": stats(s2=None), "stats C = 0": stats(C=0),
             "stats C > grid": stats(C=65535 * 64 + 1), "stats D = 0": stats(D=0), "stats D > LDS": stats(D=129), "stats N = 2^31": stats(N=1 << 31),
             "stats S = 0": stats(S=0), "stats S < 0": stats(S=-2), "stats bf16": stats(dt=_lib.XT_BF16), "stats order 0": stats(order=0),
             "stats order 3": stats(order=3), "stats max_len < 0": stats(max_len=-1), "stats max_len > N": stats(max_len=6)}
    assert all(rc == _lib.SK_EARG for rc in cases.values()), cases
    assert "sc_gmm_stats" in _lib.last_error()
