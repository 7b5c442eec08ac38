"""Speech activity on the GPU (csrc/vad.hip) against the reference's own output (tests/golden/vad.npz: ``power_spectrum``'s
log-energy, ``vad_energy`` labels and thresholds, scipy's closing / opening) and against numpy's concatenation for the gathers.

One batch serves every test: the fixture's seven rows (no frame, one frame, two frames, 1 s, 4 s plus a tail, 11 s, constant) in a
buffer wider than the longest row, as int16 and as the widened float32, with the padding filled with a value that must never be read."""
import json
import os
import sys

import numpy
import pytest
import scipy.io.wavfile
import scipy.ndimage
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

import second_trips as st  # noqa: E402
import vad_numpy as vn  # noqa: E402
from sidekit_amd import _lib  # noqa: E402
from sidekit_amd import vad as skvad  # noqa: E402

pytestmark = pytest.mark.gpu
PARAMS = ("fx", "default")
PAD = 37


@pytest.fixture(scope="module")
def data(gpu, golden_dir):
    z = numpy.load(os.path.join(golden_dir, "vad.npz"))
    lengths, nframes = z["lengths"], z["nframes"]
    so, fo = numpy.concatenate([[0], numpy.cumsum(lengths)]), numpy.concatenate([[0], numpy.cumsum(nframes)])
    B, ld = lengths.shape[0], int(lengths.max()) + PAD
    pcm = numpy.full((B, ld), 12345, dtype=numpy.int16)
    rows = []
    for r in range(B):
        pcm[r, :lengths[r]] = z["pcm16"][so[r]:so[r + 1]]
        row = {"n": int(lengths[r]), "nf": int(nframes[r]), "le": z["le"][fo[r]:fo[r + 1]]}
        for tag in PARAMS:
            label, thr = z[f"label_{tag}"][fo[r]:fo[r + 1]], float(z[f"thr_{tag}"][r])
            ok = numpy.isfinite(thr) and label.any()                   # otherwise: sk_vad_energy's rule, everything kept, threshold NaN
            fused = z[f"fused_{tag}"][fo[r]:fo[r + 1]]
            row[tag] = {"label": label if ok else numpy.ones(row["nf"], dtype=bool), "thr": thr if ok else numpy.nan, "ref_thr": thr,
                        "fused": fused if ok and fused.any() else numpy.ones(row["nf"], dtype=bool),
                        "kw": dict(zip(("flooring", "ceiling", "alpha"), z[f"params_{tag}"].tolist()))}
        rows.append(row)
    i16 = torch.from_numpy(pcm).to(gpu)
    f32 = torch.from_numpy(pcm.astype(numpy.float32) / 32768.0).to(gpu)
    lens = torch.from_numpy(lengths.astype(numpy.int32)).to(gpu)
    le, nf = skvad.frame_log_energy(i16, lens)
    return {"rows": rows, "pcm": pcm, "i16": i16, "f32": f32, "lens": lens, "lengths": lengths, "le": le, "nframes": nf, "B": B, "ld": ld}


def test_log_energy_matches_the_reference(data):
    """|diff| <= 1e-11: a float64 sum of 400 non-negative terms in any order is within 400 eps (9e-14 relative), one rounding for the
    pre-emphasis and one for the log on top; the log-energies are O(10)."""
    le16, nf16 = data["le"], data["nframes"]
    le32, nf32 = skvad.frame_log_energy(data["f32"], data["lens"])
    assert le16.shape == (data["B"], vn.n_frames(data["ld"])) and le16.dtype == torch.float64
    assert torch.equal(le16, le32) and torch.equal(nf16, nf32)              # int16 is widened exactly
    got, nf = le16.cpu().numpy(), nf16.cpu().numpy()
    assert nf.tolist() == [r["nf"] for r in data["rows"]]
    for r, row in enumerate(data["rows"]):
        if row["nf"]:
            err = numpy.abs(got[r, :row["nf"]] - row["le"]).max()
            print(f"row {r}: {row['nf']} frames, max |le - reference| = {err:.3e}")
            assert err <= 1e-11
        assert not got[r, row["nf"]:].any()                                  # beyond the last frame: zeros, the padding was never read
    with pytest.raises(ValueError):                                          # T_ld smaller than the frames of wav_ld
        out = torch.empty((data["B"], 4), dtype=torch.float64, device=le16.device)
        _lib.check(_lib.lib().sk_frame_log_energy(data["i16"].data_ptr(), _lib.XT_I16, data["ld"], data["lens"].data_ptr(), data["B"], 400, 160, 0.97,
                                                  out.data_ptr(), 4, nf16.data_ptr(), None))


@pytest.mark.parametrize("tag", PARAMS)
def test_labels_and_thresholds_match_the_reference(data, tag):
    kw = data["rows"][0][tag]["kw"]
    label, thr = skvad.vad_energy_device(data["le"], data["nframes"], 8, kw["flooring"], kw["ceiling"], kw["alpha"], fusion_win=0)
    label, thr = label.cpu().numpy(), thr.cpu().numpy()
    exempt = 0
    for r, row in enumerate(data["rows"]):
        want = row[tag]
        if numpy.isnan(want["thr"]):
            assert numpy.isnan(thr[r]) and label[r, :row["nf"]].all(), f"row {r}: a degenerate utterance keeps every frame, threshold NaN"
        else:
            rel = abs(thr[r] - want["thr"]) / abs(want["thr"])
            print(f"row {r} [{tag}]: threshold {thr[r]!r} reference {want['thr']!r} rel {rel:.2e}")
            assert rel <= 1e-9
            z = (row["le"] - row["le"].mean()) / row["le"].std()
            near = numpy.abs(z - want["thr"]) < 1e-9
            exempt += int(near.sum())
            assert numpy.array_equal(label[r, :row["nf"]].astype(bool)[~near], want["label"][~near]), f"row {r}"
        assert not label[r, row["nf"]:].any()
    assert exempt == 0


@pytest.mark.parametrize("tag", PARAMS)
def test_fusion_matches_scipy_on_the_reference_labels(data, tag):
    kw = data["rows"][0][tag]["kw"]
    label, thr = skvad.vad_energy_device(data["le"], data["nframes"], 8, kw["flooring"], kw["ceiling"], kw["alpha"], fusion_win=3)
    label = label.cpu().numpy()
    for r, row in enumerate(data["rows"]):
        assert numpy.array_equal(label[r, :row["nf"]].astype(bool), row[tag]["fused"]), f"row {r}"


def test_fusion_boundary_rule_on_a_hand_made_row(gpu):
    """Isolated ones and zeros at both ends and inside, runs of every short length; widths 3, 5 and one wider than the row."""
    pattern = numpy.array([1, 0, 0, 1, 1, 1, 0, 1, 0, 0, 0, 1, 1, 0, 1, 1, 1, 1, 0, 0, 1, 0, 1, 1, 0], dtype=numpy.uint8)
    rows = [pattern, pattern[::-1].copy(), 1 - pattern, numpy.array([0, 1, 1, 0, 1], dtype=numpy.uint8)]
    T = max(p.shape[0] for p in rows)
    le = numpy.zeros((len(rows), T))
    for r, p in enumerate(rows):
        le[r, :p.shape[0]] = 10.0 * p + 1e-4 * numpy.cos(numpy.arange(p.shape[0]))          # two well separated levels
    d_le = torch.from_numpy(le).to(gpu)
    nf = torch.tensor([p.shape[0] for p in rows], dtype=torch.int32, device=gpu)
    raw, _ = skvad.vad_energy_device(d_le, nf, 8, 0.0001, 1.5, 0.2, fusion_win=0)
    raw = raw.cpu().numpy()
    for r, p in enumerate(rows):
        assert numpy.array_equal(raw[r, :p.shape[0]], p), "the detector no longer separates the two levels: the test's input needs care"
    for win in (3, 5, 31):
        got, thr = skvad.vad_energy_device(d_le, nf, 8, 0.0001, 1.5, 0.2, fusion_win=win)
        got, thr = got.cpu().numpy(), thr.cpu().numpy()
        for r, p in enumerate(rows):
            want = scipy.ndimage.grey_opening(scipy.ndimage.grey_closing(p, size=win), size=win)
            if want.any():
                assert numpy.array_equal(got[r, :p.shape[0]], want), (win, r)
                assert numpy.array_equal(vn.label_fusion(p, win), want.astype(bool))
            else:
                assert got[r, :p.shape[0]].all() and numpy.isnan(thr[r])
    for bad in (2, 4, 257, -3):
        with pytest.raises(ValueError):
            skvad.vad_energy_device(d_le, nf, fusion_win=bad)


@pytest.mark.parametrize("win", st.VAD_WINDOWS)
def test_fusion_past_one_tile(gpu, win):
    """vad_energy_kernel fuses labels VAD_TILE = 2048 frames at a time with a halo of 4 r frames read across the tile's edges (r = win // 2)
    and scipy's 'reflect' rule at the row's two ends only.  Rows of 2048 (one tile), 2049, 2048 + 4 r + 1 and 4096 + 300 frames (three
    tiles), each in 24 hand-made patterns (tests/tools/second_trips.py: an isolated frame or a run of r - 1, r or r + 1 frames, of ones or
    of zeros, ending at, starting at or lying across frames 2048 and 4096, and at both ends of the row), plus a 1-frame and an ordinary
    row.  The raw labels are the designed pattern; the fused ones are scipy's closing then opening of it; a row alone has the bits it has
    in the batch.  Windows 3 (the default), 31 and 255 (halo 508).  tests/test_second_trips_cpu.py shows that fusing tile by tile without
    the halo, or with 'reflect' at a tile's edge, fails this comparison on these rows."""
    r = win // 2
    assert st.VAD_TILE == 2048 and win <= st.VAD_MAX_WIN
    patterns = st.vad_patterns(win)
    lengths = sorted({p.shape[0] for p in patterns})
    assert lengths == [1, 25, 2048, 2049, 2048 + 4 * r + 1, 4096 + 300] and lengths[3] > st.VAD_TILE and lengths[-1] > 2 * st.VAD_TILE
    le, nf = st.vad_log_energies(patterns)
    d_le, d_nf = torch.from_numpy(le).to(gpu), torch.from_numpy(nf).to(gpu)
    raw, thr = skvad.vad_energy_device(d_le, d_nf, 8, fusion_win=0, **st.VAD_KW)
    raw, thr = raw.cpu().numpy(), thr.cpu().numpy()
    for b, p in enumerate(patterns):
        if p.shape[0] > 1:
            assert numpy.array_equal(raw[b, :p.shape[0]], p), "the detector no longer separates the two levels: the test's input needs care"
        else:
            assert raw[b, 0] == 1 and numpy.isnan(thr[b])
        assert not raw[b, p.shape[0]:].any()
    got, thr = skvad.vad_energy_device(d_le, d_nf, 8, fusion_win=win, **st.VAD_KW)
    got_h, thr = got.cpu().numpy(), thr.cpu().numpy()
    changed = 0
    for b, p in enumerate(patterns):
        n = p.shape[0]
        want = scipy.ndimage.grey_opening(scipy.ndimage.grey_closing(p, size=win), size=win)
        changed += int((want != p).any())
        if n > 1 and want.any():
            assert numpy.array_equal(got_h[b, :n], want), (win, b, n, numpy.flatnonzero(got_h[b, :n] != want)[:8])
            assert numpy.array_equal(vn.label_fusion(p, win), want.astype(bool))
        else:
            assert got_h[b, :n].all() and numpy.isnan(thr[b])
        assert not got_h[b, n:].any()
    assert changed > len(patterns) // 2                                          # the fusion has work to do on most rows
    for b in (0, 24, 30, 48, 55, 72, 80, 95, 96, 97):                            # every length; alone: a batch of one, its own width
        n = patterns[b].shape[0]
        alone, _ = skvad.vad_energy_device(d_le[b:b + 1, :n].contiguous(), d_nf[b:b + 1], 8, fusion_win=win, **st.VAD_KW)
        assert torch.equal(alone[0], got[b, :n]), (win, b)


def _segments(data):
    rs = numpy.random.RandomState(9)
    cuts = numpy.sort(rs.choice(numpy.arange(1, 64077), 600, replace=False))               # 300 segments: more than one tile of runs
    return [[],                                                                             # empty list: nothing kept
            [(0, 400)],                                                                     # one segment, the whole row
            [(3, 101), (101, 333)],                                                         # adjacent, odd offsets
            [(1, 7), (13, 4001), (4001, 4002), (9999, 16000)],
            [(int(a), int(b)) for a, b in zip(cuts[::2], cuts[1::2])],
            [{"start": 77777, "end": 176033}],
            [(5, 5), (5, 6), (8000, 8000)]]                                                 # empty segments, one at the very end


@pytest.mark.parametrize("dtype", ["i16", "f32"])
def test_gathers_equal_numpy_concatenation(data, dtype):
    batch = data[dtype]
    host = batch.cpu().numpy()
    kw = data["rows"][0]["fx"]["kw"]
    for win in (0, 3):
        label, _ = skvad.vad_energy_device(data["le"], data["nframes"], 8, kw["flooring"], kw["ceiling"], kw["alpha"], fusion_win=win)
        out, out_len = skvad.collect_chunks_device(batch, data["lens"], labels=label, nframes=data["nframes"])
        out, out_len, lab = out.cpu().numpy(), out_len.cpu().numpy(), label.cpu().numpy()
        for r, row in enumerate(data["rows"]):
            want = vn.collect_labels(host[r, :row["n"]], lab[r, :row["nf"]])
            assert out_len[r] == want.shape[0], f"row {r}"
            assert numpy.array_equal(out[r, :out_len[r]], want), f"row {r}"
        assert out_len[0] == 300 and out_len[1] == 400 and out_len[6] == 8000             # the degenerate rows are kept whole
    # an unaligned destination (rows start 2 / 4 bytes off a 16-byte boundary) and a shift that is no multiple of the vector width
    wide = torch.zeros((data["B"], data["ld"] + 8), dtype=batch.dtype, device=batch.device)
    odd = torch.from_numpy((numpy.arange(vn.n_frames(data["ld"], 400, 163) * data["B"]).reshape(data["B"], -1) % 3 != 1).astype(numpy.uint8)).to(batch.device)
    nf163 = torch.tensor([vn.n_frames(n, 400, 163) for n in data["lengths"]], dtype=torch.int32, device=batch.device)
    out, out_len = skvad.collect_chunks_device(batch, data["lens"], labels=odd, nframes=nf163, shift=163, out=wide[:, 1:])
    out, out_len, lab = out.cpu().numpy(), out_len.cpu().numpy(), odd.cpu().numpy()
    for r, row in enumerate(data["rows"]):
        want = vn.collect_labels(host[r, :row["n"]], lab[r, :int(nf163[r])], 163)
        assert out_len[r] == want.shape[0] and numpy.array_equal(out[r, :out_len[r]], want), f"row {r}"
    # timestamps
    segs = _segments(data)
    out, out_len = skvad.collect_chunks_device(batch, data["lengths"], segments=segs, out=wide[:, 3:])
    out = out.cpu().numpy()
    for r, row in enumerate(data["rows"]):
        pairs = [(s["start"], s["end"]) if isinstance(s, dict) else s for s in segs[r]]
        want = vn.collect_segments(host[r, :row["n"]], pairs)
        assert out_len[r] == want.shape[0] and numpy.array_equal(out[r, :out_len[r]], want), f"row {r}"
    assert out_len[0] == 0 and out_len[1] == 400 and out_len[6] == 1


def test_bad_segments_are_refused_before_anything_is_enqueued(data):
    batch = data["i16"]
    good = _segments(data)
    for row, bad in ((3, [(10, 20), (15, 30)]),           # overlapping
                     (3, [(100, 200), (10, 20)]),         # descending
                     (2, [(0, 561)]),                     # past the utterance's end (inside the buffer)
                     (4, [(-1, 5)]),
                     (5, [(9, 3)])):                      # end before start
        segs = list(good)
        segs[row] = bad
        out = torch.full_like(batch, 7)
        with pytest.raises(ValueError):
            skvad.collect_chunks_device(batch, data["lengths"], segments=segs, out=out)
        torch.cuda.synchronize()
        assert bool((out == 7).all()), "a refused call wrote to the destination"
    with pytest.raises(ValueError):                        # dst may not overlap src
        skvad.collect_chunks_device(batch, data["lengths"], segments=good, out=batch)


@pytest.fixture(scope="module")
def model(gpu):
    from sidekit_amd.nnet import Xtractor
    m = Xtractor(16, model_archi="halfresnet34", loss="aam", seed=1234).to(gpu).eval()
    m.compute_dtype = "fp32"
    return m


def _utterances(data):
    p = data["pcm"]
    return [p[3, :16000], p[4, :30000], p[5, 20000:52345], p[4, 30000:50011]]


def test_speech_only_then_forward_equals_forward_on_host_compacted_copies(data, model, gpu):
    utts = _utterances(data)
    lens = [u.shape[0] for u in utts]
    pcm = numpy.zeros((len(utts), max(lens) + 5), dtype=numpy.int16)
    for r, u in enumerate(utts):
        pcm[r, :lens[r]] = u
    i16 = torch.from_numpy(pcm).to(gpu)
    out, new, (label, nframes, thr) = skvad.speech_only(i16, lens, return_labels=True)
    label, nframes = label.cpu().numpy(), nframes.cpu().numpy()
    assert all(0 < n < l for n, l in zip(new, lens)) and not numpy.isnan(thr.cpu().numpy()).any()
    host = numpy.zeros((len(utts), max(new)), dtype=numpy.int16)
    for r, u in enumerate(utts):
        kept = vn.collect_labels(u, label[r, :nframes[r]])
        assert kept.shape[0] == new[r]
        host[r, :new[r]] = kept
    with torch.no_grad():
        _, emb = model(out[:, :max(new)], is_eval=True, lengths=new)
        _, emb_host = model(torch.from_numpy(host).to(gpu), is_eval=True, lengths=new)
        assert torch.equal(emb, emb_host)
        out32, new32 = skvad.speech_only(torch.from_numpy(pcm.astype(numpy.float32) / 32768.0).to(gpu), lens)
        assert new32 == new
        _, emb32 = model(out32[:, :max(new32)], is_eval=True, lengths=new32)
        assert torch.equal(emb32, emb)
        # timestamps derived from the labels give the same samples through the other gather
        segs = [skvad.timestamps_from_labels(label[r, :nframes[r]], lens[r]) for r in range(len(utts))]
        out_ts, new_ts = skvad.speech_only(i16, lens, vad=segs)
        assert new_ts == new
        _, emb_ts = model(out_ts[:, :max(new)], is_eval=True, lengths=new)
        assert torch.equal(emb_ts, emb)
        _, emb_all = model(i16, is_eval=True, lengths=lens)
        assert not torch.equal(emb_all, emb)


def test_mirror_functions_match_the_reference(data):
    from sidekit_amd.frontend.vad import label_fusion, vad_energy
    row = data["rows"][4]
    label, thr = vad_energy(row["le"])                                           # the reference's defaults: ceiling 1.0, alpha 2
    assert label.dtype == bool and numpy.array_equal(label, row["default"]["label"])
    assert abs(thr - row["default"]["thr"]) <= 1e-9 * abs(row["default"]["thr"])
    label, thr = vad_energy(row["le"], flooring=0.0001, ceiling=1.5, alpha=0.2)
    assert numpy.array_equal(label, row["fx"]["label"])
    assert numpy.array_equal(label_fusion(label, 3), row["fx"]["fused"])
    assert numpy.array_equal(label_fusion(label[None, :], 5)[0], vn.label_fusion(label, 5))
    lone = numpy.array([0, 0, 1, 0, 0], dtype=bool)
    assert not label_fusion(lone, 3).any()                                       # an opening may remove everything: label_fusion has no fallback


def test_cli_round_trip(data, gpu, tmp_path):
    from sidekit_amd.bin import extract_xvectors
    from sidekit_amd.nnet.weights import seeded_state_dict
    sd = seeded_state_dict("halfresnet34", 16, seed=77)
    torch.save({"speaker_number": 16, "model_archi": {"model_type": "halfresnet34", "loss": {"type": "aam"}}, "model_state_dict": sd}, tmp_path / "model.pt")
    utts = _utterances(data) + [data["pcm"][6, :8000]]                          # the constant row: kept whole
    with open(tmp_path / "wav.scp", "w") as f:
        for i, u in enumerate(utts):
            scipy.io.wavfile.write(tmp_path / f"u{i}.wav", 16000, u)
            f.write(f"u{i} {tmp_path / f'u{i}.wav'}\n")
    base = ["--model", str(tmp_path / "model.pt"), "--wav-scp", str(tmp_path / "wav.scp"), "--device", "cuda", "--batch-size", "2"]
    extract_xvectors.cli(base + ["--out-scp", str(tmp_path / "a.scp"), "--vad-energy"])
    ts = json.load(open(tmp_path / "a_vad.json"))
    assert list(ts) == [f"u{i}" for i in range(len(utts))]
    for i, u in enumerate(utts):                                                  # the reference's cache shape: key -> [{"start", "end"}, ...]
        segs = ts[f"u{i}"]
        assert isinstance(segs, list) and segs and all(set(s) == {"start", "end"} and isinstance(s["start"], int) for s in segs)
        assert all(0 <= s["start"] < s["end"] <= u.shape[0] for s in segs) and all(a["end"] < b["start"] for a, b in zip(segs, segs[1:]))
        le = vn.frame_log_energy(u)
        label = vn.vad_energy(le, ceiling=1.5, alpha=0.2, fusion_win=3)[0]
        assert [(s["start"], s["end"]) for s in segs] == (vn.labels_to_segments(label, u.shape[0]) or [(0, u.shape[0])])
    assert ts["u4"] == [{"start": 0, "end": 8000}]
    extract_xvectors.cli(base + ["--out-scp", str(tmp_path / "b.scp"), "--speech-ts", str(tmp_path / "a_vad.json")])
    extract_xvectors.cli(base + ["--out-scp", str(tmp_path / "c.scp")])
    a, b, c = (open(tmp_path / f"{n}.ark", "rb").read() for n in "abc")
    assert a == b and len(a) == len(c) and a != c
    assert not os.path.exists(tmp_path / "c_vad.json") and not os.path.exists(tmp_path / "b_vad.json")
