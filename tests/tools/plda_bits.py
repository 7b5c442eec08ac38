"""SHA-256 digests of what the users of csrc/dgemm_tile.h return on fixed seeded inputs: the record a change to the tile that must not
change a bit is held against.  tests/test_gpu_backend.py recomputes both sets and asserts equality; a digest that differs is a changed
kernel, not a fixture to record again.

``digests()``: ``sc_plda_fast``, ``sc_gemm_tn`` and ``sc_dgemm_nn``, every tile form the three launch (64 and 128 tiles, one slab and
many, float32 and float64 operands, weights and centres, both epilogues).  tests/golden/plda_bits.json, recorded on the commit before
``sc_scatter_within`` joined ``dgemm_tile``'s operand forms: the added template parameter left the existing instantiations' bits alone.

``tile_digests()``: the other users -- ``sc_scatter_within``, ``sc_class_scatter``, ``sc_tv_gram``, ``sc_whiten_rows``, ``sc_gauss_loglik``,
``sc_jfa_shift``, ``sc_plda_hist`` (the 64-bit counts), ``sc_plda_hist_norm`` and ``sc_plda_cohort_moments``, one shape per instantiation
their launchers select, with odd edges (operands and shapes of tests/tools/f64_forms.py where it has them).  tests/golden/f64_tile_bits.json,
recorded with the library of the commit before the tile's operand loaders, lane map and tile store were consolidated.

Usage (on a GPU):  python tests/tools/plda_bits.py [out.json [tile]]
"""
import hashlib
import json
import os
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _sha(t):
    return hashlib.sha256(numpy.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def digests(device):
    import torch
    from sidekit_amd import _lib, iv_scoring
    from sidekit_amd import factor_analyser as fa
    rs = numpy.random.RandomState(20240)
    out = {}
    for K, M, Nn in ((1, 37, 51), (100003, 37, 51), (5000, 256, 256), (777, 129, 64)):
        for dtype in (numpy.float32, numpy.float64):
            A = torch.as_tensor((0.5 + rs.randn(K, M)).astype(dtype)).to(device)
            B = torch.as_tensor((0.25 * rs.randn(K, Nn) - 0.25).astype(dtype)).to(device)
            w, a, b = rs.uniform(0.5, 12.0, K), rs.randn(M), rs.randn(Nn)
            tag = f"gemm_tn {K}x{M}x{Nn} {numpy.dtype(dtype).name}"
            out[tag + " plain"] = _sha(fa.gemm_tn_device(A, B))
            out[tag + " weights+centres"] = _sha(fa.gemm_tn_device(A, B, w, a, b))
            out[tag + " scatter"] = _sha(fa.gemm_tn_device(A, None, None, a, a))
    A, B, r, c = rs.randn(333, 77), rs.randn(77, 45), rs.uniform(1, 9, 333), rs.uniform(0.1, 5, 45)
    Ad = torch.as_tensor(A).to(device)
    out["dgemm_nn plain"] = _sha(fa.dgemm_nn_device(Ad, B))
    out["dgemm_nn rank1"] = _sha(fa.dgemm_nn_device(Ad, B, 0.7, r, c, _lib.SC_EPI_RANK1))
    out["dgemm_nn posterior"] = _sha(fa.dgemm_nn_device(Ad, B, 1.0, r, c, _lib.SC_EPI_POSTERIOR))
    for Ne, Nt, D in ((70, 133, 50), (3000, 2900, 256)):      # 64 x 64 and 128 x 128 scoring tiles
        E, T = rs.randn(Ne, D), rs.randn(Nt, D)
        Phi, Psi = rs.randn(D, D) / D, rs.randn(D, D) / D
        out[f"plda_fast {Ne}x{Nt}x{D}"] = _sha(iv_scoring.plda_matrix_device(E, T, Phi + Phi.T, Psi, 0.37, 0.9, device))
    return out


def tile_digests(device):
    """The users of csrc/dgemm_tile.h that digests() does not reach, one shape per instantiation their launchers select."""
    import torch
    import f64_forms as ff
    from sidekit_amd import _lib
    from sidekit_amd.jfa_scoring import jfa_shift_device
    XT = {"float32": _lib.XT_F32, "float64": _lib.XT_F64}
    dev = lambda x: None if x is None else torch.as_tensor(numpy.ascontiguousarray(x)).to(device)
    empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device=device)
    out = {}
    for shape in ((17, 65), (4097, 130)):
        for dtype in ff.DTYPES:
            for weighted in (False, True):
                c = ff.gathered_case(shape, weighted, dtype)
                X, cls, Mc, w, G = dev(c["X"]), dev(c["cls"]), dev(c["Mc"]), dev(c["w"]), empty(shape[1], shape[1])
                _lib.launch("sc_scatter_within", device, X, XT[dtype], shape[0], shape[1], cls, Mc, w, c["C"], G)
                out[f"scatter_within {shape[0]}x{shape[1]} {dtype}" + (" w" if weighted else "")] = _sha(G)
    for counts, D in (((3, 1), 65), ((4096, 1), 128)):
        for dtype in ff.DTYPES:
            c = ff.class_case(counts, D, dtype)
            X, off, Mc, S = dev(c["X"]), dev(c["off"]), dev(c["Mc"]), empty(len(counts), D, D)
            _lib.launch("sc_class_scatter", device, X, XT[dtype], sum(counts), D, off, Mc, len(counts), max(counts), S)
            out[f"class_scatter {counts} {D} {dtype}"] = _sha(S)
    for C, D, R in ((3, 17, 65), (2, 5, 130)):
        F, G = dev(ff.gram_case((C, D, R))["F"]), empty(C, R * (R + 1) // 2)
        _lib.launch("sc_tv_gram", device, F, C, D, R, G)
        out[f"tv_gram {C}x{D}x{R}"] = _sha(G)
    for shape in ((65, 17, 65), (70, 37, 129), (66, 40, 256), (66, 18, 257)):
        N, D, P = shape
        for dtype in ff.DTYPES:
            for centred in (False, True):
                c = ff.whiten_case(shape, centred, dtype)
                X, mu, R = dev(c["X"]), dev(c["mu"]), dev(c["R"])
                for normalize in (0, 1):
                    for ytype in ff.DTYPES:
                        Y = torch.empty((N, P), dtype=getattr(torch, ytype), device=device)
                        _lib.launch("sc_whiten_rows", device, X, XT[dtype], N, D, mu, R, P, normalize, Y, XT[ytype])
                        out[f"whiten_rows {N}x{D}x{P} {dtype}->{ytype}" + (" mu" if centred else "") + (" normalised" if normalize else "")] = _sha(Y)
    for N, D, C in ((65, 65, 3), (129, 66, 512)):
        c = ff.loglik_case((N, D, C))
        L = empty(C, N)
        _lib.launch("sc_gauss_loglik", device, dev(c["X"]), N, D, dev(c["means"]), dev(c["W"]), dev(c["cst"]), C, L)
        out[f"gauss_loglik {N}x{D}x{C}"] = _sha(L)
    # sc_jfa_shift: one 128 x 128 instantiation; sessions and columns one past the tile edge, K = R = 17 and an even R for the pair loads
    rs = numpy.random.RandomState(20241)
    for N, C, D, R in ((129, 3, 43, 17), (129, 3, 43, 18)):
        s0, s1, W, H = dev(rs.uniform(0.5, 9.0, (N, C))), dev(rs.randn(N, C * D)), dev(rs.randn(C * D, R)), dev(rs.randn(N, R))
        out[f"jfa_shift {N}x{C}x{D}x{R}"] = _sha(jfa_shift_device(s0, s1, W, H, None, rs.randn(C * D), rs.uniform(0.5, 2.0, C * D)))
    # the persistent kernels.  sc_plda_hist walks 128 x 128 tiles, one workgroup per compute unit at most: 17 x 33 = 561 tiles give every
    # workgroup of 256 two tiles or more; sc_plda_cohort_moments walks two cohort tiles per slab from M > 128 on.
    HB = 8192
    for Ne, Nt, M, D in ((130, 200, 300, 50), (129, 129, 129, 17), (2049, 4100, 300, 17)):
        E, T, Co = dev(rs.randn(Ne, D)), dev(rs.randn(Nt, D)), dev(rs.randn(M, D))
        Phi, Psi = rs.randn(D, D) / D, rs.randn(D, D) / D
        Phi, Psi, PsiT = dev(Phi + Phi.T), dev(Psi), dev(Psi.T)
        le, lt = dev(rs.randint(0, 7, Ne).astype(numpy.int32)), dev(rs.randint(0, 7, Nt).astype(numpy.int32))
        tag = f"{Ne}x{Nt}x{M}x{D}"
        stats = []
        for side, X, P, n, off in (("enrol", E, Psi, Ne, -1), ("test", T, PsiT, Nt, 3)):
            mean, std = empty(n), empty(n)
            _lib.launch("sc_plda_cohort_moments", device, X, n, Co, M, D, Phi, P, 0.37, 0.9, off, mean, std)
            out[f"plda_cohort_moments {tag} {side} mean"], out[f"plda_cohort_moments {tag} {side} std"] = _sha(mean), _sha(std)
            stats += [mean, std]
        mat = empty(Ne, Nt)
        _lib.launch("sc_plda_fast", device, E, Ne, T, Nt, D, Phi, Psi, 0.37, 0.9, mat)
        lo, hi = float(mat.min()), float(mat.max())
        ht, hn = (torch.empty(HB, dtype=torch.int64, device=device) for _ in range(2))
        for self_offset in (-1, 1):
            _lib.launch("sc_plda_hist", device, E, Ne, T, Nt, D, Phi, Psi, 0.37, 0.9, le, lt, self_offset, lo, hi, HB, ht, hn)
            out[f"plda_hist {tag} self_offset {self_offset}"] = _sha(torch.stack([ht, hn]))
        me, se, mt, st = stats
        for kind, pairs in (("z", (me, se, None, None)), ("t", (None, None, mt, st)), ("s", (me, se, mt, st))):
            _lib.launch("sc_plda_hist_norm", device, E, Ne, T, Nt, D, Phi, Psi, 0.37, 0.9, le, lt, -1, *pairs, -8.0, 8.0, HB, ht, hn)
            out[f"plda_hist_norm {tag} {kind}"] = _sha(torch.stack([ht, hn]))
    return out


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    if len(sys.argv) > 2 and sys.argv[2] == "tile":
        digests = tile_digests
    d = digests(torch.device("cuda", 0))
    text = json.dumps(d, indent=1, sort_keys=True)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
