"""Writes tests/golden/context.npz: small float32 streams and what the REFERENCE computes on them -- ``shifted_delta_cepstral`` and
``pca_dct`` with and without a PCA matrix (sidekit/frontend/features.py:169-223) and ``FeaturesServer.get_context`` / ``get_traps``
(sidekit/features_server.py:325-394).

The reference's modules are imported with the package-shell recipe of make_vad_golden.py, its ``numpy.lib.pad`` alias included (the
reference's ``framing`` calls the alias numpy 2 removed); no reference text is copied.  The two methods are called on a reference
``FeaturesServer`` built with its own constructor.  The cases are those of tests/tools/context_numpy.py: streams of 2, 3, 7, 40, 256,
257 and 300 rows at D = 5 and 13; SDC (1, 3, 7), (2, 2, 3), (3, 1, 2) and (1, 4, 4), the last on the (k - 1) p <= 3 k boundary; windows
(3, 2), (0, 2) and (12, 12); TRAPs with 4 and 16 coefficients; PCA matrices of 7 and 40 columns; and ``start`` / ``stop`` inside and
past the ends of the 40-row stream for ``get_context`` (``get_traps`` only where the reference's padding does not raise: ``start`` at
most its left context).  The long streams go with the cheap outputs so that the file stays small.  A one-row stream is not in the
fixture: the reference's ``framing`` squeezes its single window away.

Before writing, the generator asserts that the tests' numpy restatement (tests/tools/context_numpy.py) agrees with the reference: bit
for bit for SDC and the stacked context, within 1e-12 relative for the DCT, PCA and TRAPs outputs.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_context_golden.py
"""
import importlib
import os
import sys
import warnings

import numpy

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

import make_vad_golden  # noqa: E402
import context_numpy as cn  # noqa: E402

SEED = 20240521
RTOL = 1e-12


def streams():
    """D -> the stacked float32 streams: a slow drift plus noise, so that neighbouring frames differ and no two windows agree"""
    rs = numpy.random.RandomState(SEED)
    out = {}
    for D in cn.DIMS:
        rows = []
        for n in cn.LENGTHS:
            t = numpy.arange(n)[:, None]
            rows.append((3.0 * numpy.sin(t / rs.uniform(3, 9, size=(1, D)) + rs.uniform(0, 6, size=(1, D))) + rs.randn(n, D)).astype(numpy.float32))
        out[D] = numpy.vstack(rows)
    return out


def close(a, b):
    return a.shape == b.shape and numpy.abs(a - b).max() <= RTOL * max(numpy.abs(b).max(), 1.0)


def main():
    features = make_vad_golden.import_vad_reference()[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        server = importlib.import_module("sidekit.features_server")
    x = streams()
    rs = numpy.random.RandomState(SEED + 1)
    fx = {"lengths": numpy.array(cn.LENGTHS, dtype=numpy.int32), "seed": SEED}
    by_len = {}
    for D in cn.DIMS:
        fx["x_D%d" % D] = x[D]
        by_len[D] = dict(zip(cn.LENGTHS, cn.split(x[D], cn.LENGTHS)))
    for name, (kind, D, lengths, cfg) in cn.cases().items():
        outs = []
        if kind == "pca":
            left, right, Q = cfg
            W = left + right + 1
            P = (rs.randn(D * W, Q) / numpy.sqrt(D * W)).astype(numpy.float64)
            fx[cn.pca_name(left, right, D, Q)] = P
        for n in lengths:
            s = by_len[D][n]
            if kind == "sdc":
                ref = features.shifted_delta_cepstral(s, *cfg)
                assert ref.dtype == numpy.float64 and numpy.array_equal(ref.astype(numpy.float32).astype(numpy.float64), ref), name
                assert numpy.array_equal(cn.sdc(s, *cfg).astype(numpy.float64), ref), (name, n)
                ref = ref.astype(numpy.float32)
            elif kind == "ctx":
                ref, _ = server.FeaturesServer(context=cfg).get_context(s)
                assert ref.dtype == numpy.float32 and numpy.array_equal(cn.context(s, *cfg), ref), (name, n)
            elif kind == "dct":
                ref = features.pca_dct(s, cfg[0], cfg[1])
                assert ref.dtype == numpy.float64 and close(cn.pca_dct(s, cfg[0], cfg[1]), ref), (name, n)
            elif kind == "pca":
                ref = features.pca_dct(s, cfg[0], cfg[1], P)
                assert ref.dtype == numpy.float64 and close(cn.pca_dct(s, cfg[0], cfg[1], P), ref), (name, n)
            else:
                ref, _ = server.FeaturesServer(context=cfg[:2], traps_dct_nb=cfg[2]).get_traps(s)
                assert ref.dtype == numpy.float64 and close(cn.traps(s, *cfg), ref), (name, n)
            outs.append(ref)
        fx[name] = numpy.vstack(outs)
    # start / stop on the 40-row stream
    s, label = by_len[5][40], rs.rand(40) > 0.3
    fx["range_label"] = label
    for i, (start, stop) in enumerate(cn.RANGES):
        ref, lab = server.FeaturesServer(context=(3, 2)).get_context(s, start, stop, label)
        assert numpy.array_equal(cn.context(s, 3, 2, (start, stop)), ref) and numpy.array_equal(lab, label[start:stop]), (start, stop)
        fx["range_ctx_%d" % i] = ref
        if start is None or start <= 3:
            ref, lab = server.FeaturesServer(context=(3, 2), traps_dct_nb=4).get_traps(s, start, stop, label)
            assert close(cn.traps(s, 3, 2, 4, (start, stop)), ref) and numpy.array_equal(lab, label[start:stop]), (start, stop)
            fx["range_traps_%d" % i] = ref
        else:
            try:
                server.FeaturesServer(context=(3, 2), traps_dct_nb=4).get_traps(s, start, stop, label)
                raise SystemExit("get_traps with start > context[0] was expected to raise")
            except ValueError:
                pass
    path = os.path.join(HERE, "context.npz")
    numpy.savez_compressed(path, **fx)
    print("context.npz", os.path.getsize(path), "bytes,", len(fx), "arrays")


if __name__ == "__main__":
    main()
