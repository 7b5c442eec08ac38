"""SHA-256 digests of what ``sc_plda_fast``, ``sc_gemm_tn`` and ``sc_dgemm_nn`` return on fixed seeded inputs.

tests/golden/plda_bits.json holds the digests recorded on the commit before ``sc_scatter_within`` joined ``dgemm_tile``'s operand
forms; tests/test_gpu_backend.py recomputes them: the added template parameter must leave the existing instantiations' bits alone.
The shapes take every tile form the three entry points launch (64 and 128 tiles, one slab and many, float32 and float64 operands,
weights and centres, both epilogues).

Usage (on a GPU):  python tests/tools/plda_bits.py [out.json]
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


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    d = digests(torch.device("cuda", 0))
    text = json.dumps(d, indent=1, sort_keys=True)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
