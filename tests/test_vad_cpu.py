"""Speech activity without a GPU: the numpy restatement against the reference's own output (tests/golden/vad.npz), the label <->
timestamp helpers, the new ABI symbols and the mirror names."""
import os
import re
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

import vad_numpy as vn  # noqa: E402
from sidekit_amd import _lib  # noqa: E402
from sidekit_amd import vad as skvad  # noqa: E402

PARAMS = ("fx", "default")


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = numpy.load(os.path.join(golden_dir, "vad.npz"))
    lengths, nframes = z["lengths"], z["nframes"]
    so, fo = numpy.concatenate([[0], numpy.cumsum(lengths)]), numpy.concatenate([[0], numpy.cumsum(nframes)])
    rows = []
    for r in range(lengths.shape[0]):
        row = {"pcm": z["pcm16"][so[r]:so[r + 1]], "le": z["le"][fo[r]:fo[r + 1]], "nf": int(nframes[r])}
        for tag in PARAMS:
            row[tag] = {"label": z[f"label_{tag}"][fo[r]:fo[r + 1]], "fused": z[f"fused_{tag}"][fo[r]:fo[r + 1]], "thr": float(z[f"thr_{tag}"][r]),
                        "params": dict(zip(("flooring", "ceiling", "alpha"), z[f"params_{tag}"].tolist()))}
        rows.append(row)
    return rows


def test_fixture_has_the_shapes_the_kernels_can_get_wrong(fx):
    assert [r["nf"] for r in fx] == [0, 1, 2, 98, 398, 1098, 48]
    assert fx[4]["pcm"].shape[0] % vn.SHIFT != 0 and fx[5]["nf"] > 1024
    assert numpy.all(fx[6]["pcm"] == fx[6]["pcm"][0])
    for tag in PARAMS:
        assert [bool(numpy.isfinite(r[tag]["thr"])) for r in fx] == [False, False, True, True, True, True, False]


def test_restatement_matches_the_reference(fx):
    for row in fx:
        assert vn.n_frames(row["pcm"].shape[0]) == row["nf"]
        le = vn.frame_log_energy(row["pcm"])
        assert le.shape == row["le"].shape
        if le.size:
            assert numpy.abs(le - row["le"]).max() <= 1e-12
        for tag in PARAMS:
            ref = row[tag]
            label, thr, z = vn.vad_energy(row["le"], **ref["params"])
            if numpy.isfinite(ref["thr"]) and ref["label"].any():
                assert numpy.abs(z - ref["thr"]).min() >= 1e-6                      # what the generator promised
                assert numpy.array_equal(label, ref["label"])
                assert abs(thr - ref["thr"]) <= 1e-9 * abs(ref["thr"])
                assert numpy.array_equal(vn.label_fusion(ref["label"], 3), ref["fused"])
            else:                                                                   # degenerate: everything kept, threshold NaN
                assert numpy.isnan(thr) and label.all() and label.shape[0] == row["nf"]


def test_first_e_step_has_no_constant_term(fx):
    """Iteration 1 is the reference's, not a textbook EM's: with the mixture's constant term in place from the start the threshold moves."""
    z = (fx[4]["le"] - fx[4]["le"].mean()) / fx[4]["le"].std()
    one = vn.em_threshold(z, n_iter=1, ceiling=1.5, alpha=0.2)
    w, mu = numpy.ones(3) / 3, numpy.array([-2.0, 0.0, 2.0])
    lp = -0.5 * ((z[:, None] - mu[None, :]) ** 2) + numpy.log(w)[None, :]
    pp = numpy.exp(lp - lp.max(axis=1, keepdims=True))
    pp /= pp.sum(axis=1, keepdims=True)
    m = (z[:, None] * pp).sum(axis=0) / pp.sum(axis=0)
    cov = numpy.clip((z[:, None] ** 2 * pp).sum(axis=0) / pp.sum(axis=0) - m * m, 0.0001, 1.5)
    textbook = m.max() - 0.2 * numpy.sqrt(cov[m.argmax()])
    assert abs(one - textbook) > 1e-3


def test_labels_and_timestamps_round_trip(fx):
    rs = numpy.random.RandomState(3)
    for n, nf in ((64077, 398), (400, 1), (560, 2), (16000, 98)):
        for _ in range(4):
            label = rs.rand(nf) < 0.5
            segs = skvad.labels_to_segments(label, n)
            assert segs == vn.labels_to_segments(label, n)
            mask = numpy.zeros(n, dtype=bool)
            for s, e in segs:
                assert 0 <= s < e <= n
                mask[s:e] = True
            assert numpy.array_equal(mask, vn.sample_mask(label, n))
            assert all(a[1] < b[0] for a, b in zip(segs, segs[1:]))                 # maximal runs: never adjacent
            x = rs.randint(-100, 100, n).astype(numpy.int16)
            assert numpy.array_equal(vn.collect_segments(x, segs), vn.collect_labels(x, label))
            ts = skvad.timestamps_from_labels(label, n)
            assert ts == ([{"start": s, "end": e} for s, e in segs] or [{"start": 0, "end": n}])
    # the last frame owns the tail; no frame keeps the whole signal; nothing labelled falls back to everything
    assert skvad.labels_to_segments([0, 1], 560) == [(160, 560)]
    assert skvad.labels_to_segments([], 300) == [(0, 300)]
    assert skvad.labels_to_segments([0, 0, 0], 720) == []
    assert skvad.timestamps_from_labels([0, 0, 0], 720) == [{"start": 0, "end": 720}]
    assert skvad.n_frames(399) == 0 and skvad.n_frames(400) == 1 and skvad.n_frames(559) == 1 and skvad.n_frames(560) == 2


def test_segments_csr():
    off, seg = skvad.segments_csr([[{"start": 1, "end": 5}, (7, 9)], [], [(0, 3)]], 3)
    assert off.tolist() == [0, 2, 2, 3] and seg.tolist() == [1, 5, 7, 9, 0, 3] and off.dtype == seg.dtype == numpy.int32
    with pytest.raises(ValueError):
        skvad.segments_csr([[]], 2)


def test_new_symbols_in_header_and_binding_table():
    header = open(os.path.join(ROOT, "include", "sidekit_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in (("sk_frame_log_energy", 12), ("sk_vad_energy", 12), ("sk_collect_labels", 13), ("sk_collect_segments", 13)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m, f"{name} is not declared in include/sidekit_amd.h"
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1])
        assert "stream" in m.group(1).split(",")[-1]
    lib = _lib.lib()
    assert lib.sk_vad_energy(None, None, 1, 1, 8, 0.0001, 1.5, 0.2, 3, None, None, None) == _lib.SK_EARG and "null" in _lib.last_error()
    assert lib.sk_collect_labels(None, 0, 1, None, None, 1, None, 1, 160, None, 1, None, None) == _lib.SK_EARG


def test_mirror_names_through_install_as_sidekit():
    import sidekit_amd
    saved = {k: v for k, v in sys.modules.items() if k == "sidekit" or k.startswith("sidekit.")}
    try:
        sidekit_amd.install_as_sidekit()
        import sidekit
        from sidekit.frontend.vad import label_fusion, vad_energy
        from sidekit.frontend import vad_energy as ve2
        assert vad_energy is ve2 is sidekit.vad_energy is sys.modules["sidekit_amd.frontend.vad"].vad_energy
        assert callable(label_fusion)
        with pytest.raises(NotImplementedError):
            vad_energy(numpy.zeros(10), distrib_nb=2)
        with pytest.raises(NotImplementedError):
            label_fusion(numpy.zeros((2, 10), dtype=bool))
    finally:
        for k in [k for k in sys.modules if k == "sidekit" or k.startswith("sidekit.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_streaming_extractor_refuses_vad_without_a_gpu():
    import torch
    from sidekit_amd.pipeline import StreamingExtractor

    class Host:
        device = torch.device("cpu")
    with pytest.raises(RuntimeError):
        StreamingExtractor(Host(), vad="energy")
    with pytest.raises(ValueError):
        StreamingExtractor(Host(), vad="silero")
    assert StreamingExtractor(Host()).stats["speech_samples"] == 0
