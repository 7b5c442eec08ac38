"""Writes tests/golden/features.npz: small feature streams and what the REFERENCE's ``sidekit.frontend.normfeat``,
``sidekit.frontend.features.compute_delta`` and ``FeaturesServer.post_processing`` compute on them.

The set, from ``RandomState(2024)`` in draw order, D = 5: for every length n of LENGTHS a stream ``x_n = (1.5 randn(n, D) + [0, 1, -2, 3,
0.5]) * [1, 2, 0.5, 1, 3]`` rounded to float32, and labels ``lab_n = rand(n) < 0.7`` with ``lab_n[1] = True``; two labelled streams
``x_s301`` (430 frames of which exactly 301 are labelled) and ``x_s302`` (431 / 302): the ``<= win`` switch of the sliding norm; global
vectors ``gmean = randn(D)``, ``gstd = 0.5 + rand(D)``.  The values are continuous, so no column holds a value twice (asserted: the
streams are tie-free, but for the duplicated frame the reference itself appends in ``stg``).  The reference gets float64 copies, so its
in-place results are float64.

Recorded (``k`` is a stream's key; for the streams of more than 9 frames the first column only (COLS_BIG = 1) -- every operation works
column by column, so nothing is lost but bytes):
  rasta_k; delta_k, ddelta_k (float32, delta of delta); cms_lab_k, cmvn_lab_k, cms_glob_k, cmvn_glob_k;
  for win in (301, 5) and with / without labels: slc_{win}_{lab|all}_k, slcr_..., stg_... (cep_sliding_norm with reduce False / True, stg);
  win = 5 for the streams of at most 9 frames and for n = 303; with labels for the short streams, 650 and the two labelled streams;
  post_{norm}_{keep|drop}_k and postlab_..._k: FeaturesServer(rasta, delta, double_delta, feat_norm=norm).post_processing of column 0 of
  the streams POST, for every feat_norm, keep_all_features True and False, and the labels it returns.
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_features_golden.py
"""
import importlib
import os
import sys

import numpy

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

D, COLS_BIG = 5, 1
LENGTHS = [3, 4, 5, 6, 7, 8, 9, 299, 300, 301, 302, 303, 650, 900]
LABELLED = {"s301": (430, 301), "s302": (431, 302)}
POST = ["9", "s301", "s302"]
NORMS = ["cms", "cmvn", "cms_sliding", "cmvn_sliding", "stg"]


def streams():
    rs = numpy.random.RandomState(2024)
    shift, scale = numpy.array([0, 1, -2, 3, 0.5]), numpy.array([1, 2, 0.5, 1, 3])
    draw = lambda n: ((1.5 * rs.randn(n, D) + shift) * scale).astype(numpy.float32)   # noqa: E731
    x, lab = {}, {}
    for n in LENGTHS:
        x[str(n)] = draw(n)
        lab[str(n)] = rs.rand(n) < 0.7
        lab[str(n)][1] = True
    for k, (n, speech) in LABELLED.items():
        x[k] = draw(n)
        mark = numpy.zeros(n, dtype=bool)
        mark[rs.permutation(n)[:speech]] = True
        lab[k] = mark
    return x, lab, rs.randn(D), 0.5 + rs.rand(D)


def main():
    make_golden.import_reference()
    nf = importlib.import_module("sidekit.frontend.normfeat")
    ft = importlib.import_module("sidekit.frontend.features")
    fs = importlib.import_module("sidekit.features_server")
    x, lab, gmean, gstd = streams()
    for k, v in x.items():
        assert all(numpy.unique(v[:, c]).shape[0] == v.shape[0] for c in range(D)), f"stream {k} has ties"
    for k, (n, speech) in LABELLED.items():
        assert lab[k].sum() == speech
    out = {"gmean": gmean, "gstd": gstd, "cols_big": numpy.int64(COLS_BIG)}

    def put(name, k, value):
        value = numpy.asarray(value)
        out[f"{name}_{k}"] = value if value.shape[0] <= 9 or value.ndim == 1 else numpy.ascontiguousarray(value[:, :COLS_BIG])

    def in_place(fn, k, *args, **kw):
        a = x[k].astype(numpy.float64)
        fn(a, *args, **kw)
        return a

    for k in x:
        out[f"x_{k}"], out[f"lab_{k}"] = x[k], lab[k]
        n, small = x[k].shape[0], x[k].shape[0] <= 9
        put("rasta", k, nf.rasta_filt(x[k].astype(numpy.float64)))
        d = ft.compute_delta(x[k].astype(numpy.float64))
        assert d.dtype == numpy.float32
        put("delta", k, d)
        put("ddelta", k, ft.compute_delta(d))
        if small or k in ("299", "302"):
            put("cms_lab", k, in_place(nf.cms, k, lab[k].copy()))
            put("cmvn_lab", k, in_place(nf.cmvn, k, lab[k].copy()))
            put("cms_glob", k, in_place(nf.cms, k, lab[k].copy(), gmean))
            put("cmvn_glob", k, in_place(nf.cmvn, k, lab[k].copy(), gmean, gstd))
        for win in (301, 5):
            if win == 5 and not (small or k == "303"):
                continue
            for tag, label in (("all", None), ("lab", lab[k])):
                if tag == "lab" and not (small or k in ("650", "s301", "s302")):
                    continue
                if tag == "all" and k in LABELLED:
                    continue
                label = None if label is None else label.copy()
                put(f"slc_{win}_{tag}", k, in_place(nf.cep_sliding_norm, k, win=win, label=label, center=True, reduce=False))
                put(f"slcr_{win}_{tag}", k, in_place(nf.cep_sliding_norm, k, win=win, label=label, center=True, reduce=True))
                put(f"stg_{win}_{tag}", k, in_place(nf.stg, k, label=label, win=win))
    for k in POST:
        for norm in NORMS:
            for tag, keep in (("keep", True), ("drop", False)):
                server = fs.FeaturesServer(feat_norm=norm, delta=True, double_delta=True, rasta=True, keep_all_features=keep)
                feat, label = server.post_processing(x[k][:, :1].astype(numpy.float64), lab[k].copy())
                assert feat.dtype == numpy.float64 and feat.shape[1] == 3
                out[f"post_{norm}_{tag}_{k}"], out[f"postlab_{norm}_{tag}_{k}"] = feat, label
    path = os.path.join(HERE, "features.npz")
    numpy.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
