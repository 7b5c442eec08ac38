"""Every output of the diagonal-GMM entry points (sc_gmm_frame_loglik, sc_gmm_stats, sc_gmm_score_models, and on lists
sc_gmm_top_components, sc_gmm_score_models_topc, sc_gmm_topc_posteriors, sc_gmm_topc_stats, sc_gmm_topc_refine) on a fixed seeded case
list from one build of the library, written to one .npz, and the comparison of two such files bit for bit (GPU box for the dump, any box to compare):

    SIDEKIT_AMD_LIB=other/libsidekit_amd.so python scripts/gmm_dump.py a.npz
    python scripts/gmm_dump.py b.npz
    python scripts/gmm_dump.py --compare a.npz b.npz        (one JSON line; status 1 when an array differs)

A change that moves code between the csrc/gmm*.hip files, csrc/gmm_tile.h and csrc/gmm_topc_tile.h and leaves every sum's order alone
must give "identical": true.  The cases are the smallest at which a shared piece can go wrong, each well under a second:
  D  1, 16, 17, 60, 64, 65, 128: below a 16-wide k-chunk, exactly one, one and a tail, the product's shape, the last size a wave's 64
  lanes cover in one pass and the first that needs the second (the top-C kernels' lane = d and d + 64), the maximum;
  C  1, 64, 65, 130: a partial component tile, a full one, a second tile of one component, three tiles;
  segments of 3, 64, 0, 133, 65 and 700 frames in one call: an empty one, exactly one frame tile, a tile and one frame, and two slabs
  through the workspace (700 > SC_GMM_SLAB_FRAMES); seg_off ends 40 frames short of N;
  float32 and float64 frames; lse with and without lp; statistics of order 1 and 2; M = 1, 2, 3 models (3: a half-filled group at two
  models per workgroup) with no mask and with a scattered one;
  on lists of K = 1, min(C, 10) and min(C, 32): the lists themselves; scoring with M = 1, 3, 4, 5 models (a part group of the four per
  workgroup, a full one, a second group), no mask and the scattered one, on the same segments; posteriors on the device's lists and on
  a caller's with entries of -1 and C in it; statistics of order 1 and 2 on the same segments (the 700-frame one through the workspace,
  the slab reduce and the finish it shares with sc_gmm_stats); refinement from Kc = 1, min(2 K, 64) and 64 candidates per frame with
  duplicates, -1 and values >= C among them, with and without posteriors.
The file's bytes are a function of the arrays alone (fixed member order and dates), so equal files have equal SHA-256.
"""
import hashlib, io, json, os, sys, zipfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy

DIMS, COMPONENTS, LENGTHS, TAIL, MODELS = (1, 16, 17, 60, 64, 65, 128), (1, 64, 65, 130), (3, 64, 0, 133, 65, 700), 40, (1, 2, 3)
TOPC_MODELS = (1, 3, 4, 5)


def dump(path):
    import torch
    from sidekit_amd import mixture
    from sidekit_amd.gmm_scoring import gmm_llk_device, gmm_llk_topc_device, gmm_top_components_device
    dev = torch.device("cuda", 0)
    off = numpy.concatenate(([0], numpy.cumsum(LENGTHS)))
    N, S = int(off[-1]) + TAIL, len(LENGTHS)
    out = {}
    for D in DIMS:
        for C in COMPONENTS:
            rs = numpy.random.RandomState(1000 * D + C)
            ubm = mixture.Mixture()
            w = rs.rand(C) + 0.5
            ubm.w, ubm.mu, ubm.invcov = w / w.sum(), 2.0 * rs.randn(C, D), 1.0 / (0.5 + rs.rand(C, D))
            ubm.cov_var_ctl = 1.0 / ubm.invcov
            ubm._compute_all()
            X = ubm.mu[rs.randint(0, C, N)] + 1.1 * rs.randn(N, D)
            models = ubm.mu[None] + 0.3 * rs.randn(max(MODELS + TOPC_MODELS), C, D)
            for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
                x, dt, _ = mixture._frames(torch, torch.as_tensor(X).to(dev, dtype))
                key = f"D{D}_C{C}_{name}_"
                out[key + "lse"] = mixture._loglik(torch, ubm, x, dt)[0]
                out[key + "lse_beside_lp"], out[key + "lp"], _ = mixture._loglik(torch, ubm, x, dt, want_lp=True)
                for order in (1, 2):
                    stats = mixture.gmm_stats_device(ubm, x, off, order)
                    for what, t in zip(("stat0", "stat1", "stat2", "llk"), stats):
                        if t is not None:
                            out[f"{key}order{order}_{what}"] = t
                for M in MODELS:
                    mask = numpy.random.RandomState(M).rand(M, S) < 0.5
                    mask[0, -1] = True                                        # the two-slab segment is always scored
                    out[f"{key}M{M}_llk"] = gmm_llk_device(ubm, models[:M], x, off)[0]
                    out[f"{key}M{M}_masked_llk"] = gmm_llk_device(ubm, models[:M], x, off, mask)[0]
                for K in sorted({1, min(C, 10), min(C, 32)}):
                    key = f"D{D}_C{C}_{name}_K{K}_"
                    idx = out[key + "idx"] = gmm_top_components_device(ubm, x, K)
                    for M in TOPC_MODELS:
                        mask = numpy.random.RandomState(M).rand(M, S) < 0.5
                        mask[0, -1] = True
                        out[f"{key}M{M}_llk"] = gmm_llk_topc_device(ubm, models[:M], x, off, top_c=K, components=idx)[0]
                        out[f"{key}M{M}_masked_llk"] = gmm_llk_topc_device(ubm, models[:M], x, off, mask, top_c=K, components=idx)[0]
                    _, out[key + "post"], out[key + "lse"] = mixture.gmm_topc_posteriors_device(ubm, x, K, idx)
                    holed = idx.clone()                                       # a caller's list: entries below 0 and at C contribute nothing
                    holed[::3, 0], holed[1::5, K - 1] = -1, C
                    _, out[key + "holed_post"], out[key + "holed_lse"] = mixture.gmm_topc_posteriors_device(ubm, x, K, holed)
                    for order in (1, 2):
                        stats = mixture.gmm_stats_topc_device(ubm, x, off, order, K, idx)
                        for what, t in zip(("stat0", "stat1", "stat2", "llk"), stats):
                            if t is not None:
                                out[f"{key}order{order}_{what}"] = t
                    for Kc in sorted({1, min(2 * K, 64), 64}):
                        cand = numpy.random.RandomState(Kc).randint(-1, C + 2, (N, Kc)).astype(numpy.int32)   # -1, C and C + 1 among them
                        cand[::2, Kc - 1] = cand[::2, 0]                      # and a repeat in every other row
                        cand = torch.as_tensor(cand).to(dev)
                        out[f"{key}Kc{Kc}_idx"] = mixture.gmm_topc_refine_device(ubm, x, cand, K)
                        for what, t in zip(("idx", "post", "lse"), mixture.gmm_topc_refine_device(ubm, x, cand, K, posteriors=True)):
                            out[f"{key}Kc{Kc}_with_post_{what}"] = t
    torch.cuda.synchronize()
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:                 # an .npz numpy.load reads, with nothing of the clock in it
        for k in sorted(out):
            buf = io.BytesIO()
            numpy.lib.format.write_array(buf, numpy.ascontiguousarray(out[k].cpu().numpy()))
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())
    print(json.dumps({"wrote": path, "library": _library(), "arrays": len(out), "sha256": sha256(path)}))


def _library():
    from sidekit_amd import _lib
    return _lib.LIB_PATH


def sha256(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def compare(a_path, b_path):
    a, b = numpy.load(a_path), numpy.load(b_path)
    differing = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        if a[k].shape != b[k].shape or a[k].dtype != b[k].dtype or a[k].tobytes() != b[k].tobytes():   # bytes: a nan equals itself
            differing.append(k)
    finite = all(bool(numpy.isfinite(a[k]).all()) for k in a.files)
    print(json.dumps({"identical": not differing, "arrays": len(a.files), "differing": differing, "all_finite": finite,
                      "sha256": {a_path: sha256(a_path), b_path: sha256(b_path)}}))
    return 0 if not differing else 1


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    dump(sys.argv[1])
