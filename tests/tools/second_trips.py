"""What the tests of second trips share ("Thresholds a launch repeats at"): a persistent workgroup that takes another tile, a
launcher that starts another row block, a pass loop that runs again.

``read_sources``     the thresholds as the sources state them, by regular expression; tests/test_second_trips_cpu.py holds them to the
                     values below, which the GPU tests import, so that whoever moves a threshold is told to move the shapes too;
the data builders    the corpora the GPU cases and their CPU sensitivity checks both use (same seeds, same arrays);
the emulations       numpy restatements of each launch structure with a ``variant`` switch for the plausible wrong second pass.  They
                     restate the STRUCTURE (which tile, which block, which offset), not the arithmetic: a score is numpy's.
"""
import os
import re

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# ---- the thresholds the shapes rest on ---------------------------------------------------------------------------------------------
ROWS = 32768                   # score_norm.hip: X rows per launch of both cohort-moment launchers
COHORT_TILE = 128              # score_norm.hip: CT and PCT, cohort rows per tile
SLAB_TILES, MAX_SLABS, MIN_PER = 128, 64, 2   # per = tiles_m > 128 ? cdiv(tiles_m, 64) : 2
HT, PT = 256, 128              # scoring.hip: tile edge of cosine_hist_kernel / plda_hist_kernel
HIST_FLUSH = {"cosine": 1 << 15, "plda": 1 << 17}   # tiles per workgroup between two flushes of the LDS counters: not reached
FZ, SC_FEAT_TILE = 8, 256      # featnorm.hip / features.h: a segment's tiles are dealt to FZ workgroups
FEAT_PASS = FZ * SC_FEAT_TILE  # rows of one round of feat_delta_kernel / feat_norm_kernel: 2048
VAD_TILE, VAD_MAX_WIN = 2048, 255
CUS = 256                      # compute units of one MI355X: what the CPU checks assume, the GPU tests read the device's


def cdiv(a, b):
    return (a + b - 1) // b


def _text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _all(pattern, text, count):
    found = re.findall(pattern, text)
    assert len(found) == count, f"{pattern!r}: expected {count} matches, found {found}"
    return found


def _one(values):
    values = set(values)
    assert len(values) == 1, values
    return values.pop()


def read_sources():
    """The thresholds as the sources state them today."""
    norm, scoring = _text("sidekit_amd", "csrc", "score_norm.hip"), _text("sidekit_amd", "csrc", "scoring.hip")
    feat, vad = _text("sidekit_amd", "csrc", "featnorm.hip"), _text("sidekit_amd", "csrc", "vad.hip")
    header = _text("include", "sidekit_amd", "features.h")
    out = {"ROWS": int(_one(_all(r"constexpr int ROWS = (\d+);", norm, 2)))}
    _all(r"for \(int r0 = 0; r0 < N; r0 \+= ROWS\)", norm, 2)                          # both launchers step by it
    rule = _one(_all(r"per = tiles_m > (\d+) \? cdiv\(tiles_m, (\d+)\) : (\d+), slabs = cdiv\(tiles_m, per\)", norm, 2))
    out["SLAB_TILES"], out["MAX_SLABS"], out["MIN_PER"] = (int(v) for v in rule)
    out["COHORT_TILE"] = int(_one(_all(r"constexpr int CT = (\d+)", norm, 1) + _all(r"constexpr int PCT = (\d+)", norm, 1)))
    out["HT"] = int(_all(r"constexpr int HT = (\d+)", scoring, 1)[0])
    out["PT"] = int(_all(r"constexpr int PT = (\d+)", scoring, 1)[0])
    _all(r"for \(long tile = blockIdx\.x; tile < ntiles; tile \+= gridDim\.x\)", scoring, 2)   # the walk of both histogram kernels
    _all(r"\*grid = \(int\)\(ntiles < \(long\)cus \? ntiles : \(long\)cus\);", scoring, 1)        # one workgroup per CU, at most one per tile
    flush = _all(r"if \(\+\+since_flush == \(1 << (\d+)\)\)", scoring, 2)
    out["HIST_FLUSH"] = {"cosine": 1 << int(flush[0]), "plda": 1 << int(flush[1])}
    out["FZ"] = int(_all(r"constexpr int FT = SC_FEAT_TILE, FC = SC_FEAT_COLS, FZ = (\d+);", feat, 1)[0])
    out["SC_FEAT_TILE"] = int(_all(r"#define SC_FEAT_TILE (\d+)", header, 1)[0])
    _all(r"t0 \+= \(long\)FZ \* FT\)", feat, 3)                                           # delta, the table modes, the windowed modes
    out["VAD_TILE"] = int(_all(r"constexpr int VAD_TILE = (\d+);", vad, 1)[0])
    out["VAD_MAX_WIN"] = int(_all(r"constexpr int VAD_MAX_WIN = (\d+);", vad, 1)[0])
    _all(r"for \(int c0 = 0; c0 < n; c0 \+= VAD_TILE\)", vad, 1)
    return out


# ---- 1. histogram kernels that walk more than one tile -----------------------------------------------------------------------------
def hist_side(cus, tile):
    """(N, t): the smallest square set N = (t - 1) tile + 3 whose t x t tiles outnumber the compute units."""
    t = 1
    while t * t <= cus:
        t += 1
    return (t - 1) * tile + 3, t


def cosine_corpus(n, d=8, seed=21, n_spk=40, noise=0.6):
    """n unit float32 rows around ``n_spk`` speaker centres, and their labels."""
    rs = numpy.random.RandomState(seed)
    lab = rs.randint(0, n_spk, n).astype(numpy.int32)
    x = rs.randn(n_spk, d)[lab] + noise * rs.randn(n, d)
    return (x / numpy.linalg.norm(x, axis=1, keepdims=True)).astype(numpy.float32), lab


def plda_model(golden_dir, d):
    """(mu, F, Sigma) of tests/golden/plda_train.npz cut to its first ``d`` dimensions, as tests/test_gpu_plda_hist.py builds its ``odd`` fixture."""
    z = numpy.load(os.path.join(golden_dir, "plda_train.npz"))
    return z["mean_0"][:d].copy(), z["F_0"][:d].copy(), z["Sigma_0"][:d, :d].copy()


def plda_corpus(model, n, seed=22, n_spk=40):
    """n float64 rows drawn from the model itself (mu + F h_speaker + noise of covariance Sigma), and their labels."""
    mu, F, Sigma = model
    rs = numpy.random.RandomState(seed)
    lab = rs.randint(0, n_spk, n).astype(numpy.int32)
    h = rs.randn(n_spk, F.shape[1])
    return mu + h[lab] @ F.T + rs.randn(n, mu.shape[0]) @ numpy.linalg.cholesky(Sigma).T, lab


def device_counts(z, lo, hi, nb, lab_e, lab_t, self_offset=None):
    """The bin of every entry of a resident score matrix (float32: the cosine modules' ``_bins``; float64: the PLDA modules'), and the
    target / non-target counts without the self-trials ``j == i + self_offset``, all on the matrix's device -> (ht, hn, bins)."""
    import torch
    if z.dtype == torch.float32:
        b = torch.floor((z - float(numpy.float32(lo))) * float(numpy.float32(nb / (hi - lo))))
    else:
        b = torch.floor((z - lo) * (nb / (hi - lo)))
    b = b.clamp_(0, nb - 1).long()
    le, lt = torch.as_tensor(lab_e).to(z.device), torch.as_tensor(lab_t).to(z.device)
    tar = le[:, None] == lt[None, :]
    keep = torch.ones_like(tar)
    if self_offset is not None:
        i = torch.arange(z.shape[0], device=z.device)
        keep[i, i + self_offset] = False
    count = lambda sel: torch.bincount(b[sel], minlength=nb).cpu().numpy().astype(numpy.uint64)   # noqa: E731
    return count(tar & keep), count(~tar & keep), b


def walk_tiles(ne, nt, tile, grid, block_counts, variant=None):
    """The histograms of persistent workgroups: workgroup b of ``grid`` takes tiles b, b + grid, ...; ``block_counts(m0, n0, s0)`` gives
    the (target, non-target) counts of the tile at (m0, n0) with the per-tile terms and statistics staged for the tile at ``s0``.
    variant None: as the kernels do; "dropped": a workgroup's tiles after its first are not counted; "stale": they are binned with what
    the first tile staged."""
    tiles_n = cdiv(nt, tile)
    ntiles = cdiv(ne, tile) * tiles_n
    ht = hn = 0
    for b in range(min(grid, ntiles)):
        first = None
        for t in range(b, ntiles, grid):
            at = ((t // tiles_n) * tile, (t % tiles_n) * tile)
            if first is not None and variant == "dropped":
                break
            bt, bn = block_counts(at[0], at[1], first if (first is not None and variant == "stale") else at)
            ht, hn = ht + bt, hn + bn
            first = first or at
    return ht, hn


def staged(values, s0, count, fill):
    """``count`` entries of a per-row table as a tile at row ``s0`` stages them: rows past the end hold ``fill``."""
    out = numpy.full(count, fill, dtype=values.dtype)
    have = max(0, min(count, values.shape[0] - s0))
    out[:have] = values[s0:s0 + have]
    return out


# ---- 2. cohort moments past the row block and the slab limit -----------------------------------------------------------------------
COHORT_M, COHORT_EXTRA, COHORT_R = 33000, 130, 100      # X = C[100 : 100 + 32768 + 130] of a 33 000-row cohort
SLAB_M = (SLAB_TILES * COHORT_TILE, SLAB_TILES * COHORT_TILE + 1 + 100)   # the last shape with two tiles per slab, and the first kind beyond


def cohort_cosine(m=COHORT_M, d=4, seed=23):
    """Unit float32 rows with a common component: a row's cohort mean is of order 0.1 and differs from row to row by as much."""
    rs = numpy.random.RandomState(seed)
    x = rs.randn(m, d) + numpy.array([0.8] + [0.0] * (d - 1))
    return (x / numpy.linalg.norm(x, axis=1, keepdims=True)).astype(numpy.float32)


def first_block_samples():
    """Row ranges of the first row block that the big cases compare with calls of their own: its first rows (where a second block
    that forgets ``+ r0`` on the output would land), two inner ranges and its last rows."""
    return [(0, 130), (9973, 10103), (20011, 20075), (ROWS - 128 - 64, ROWS - 128)]


def slab_rule(m):
    tiles_m = cdiv(m, COHORT_TILE)
    per = cdiv(tiles_m, MAX_SLABS) if tiles_m > SLAB_TILES else MIN_PER
    return tiles_m, per, cdiv(tiles_m, per)


def moments_launcher(scores_of, n, m, self_offset, rows, variant=None, rows_per_launch=ROWS):
    """sc_cohort_moments / sc_plda_cohort_moments restated for the X rows ``rows`` (ascending indices): -> (mean, std) of length n, -7
    where nothing was written.  ``scores_of(x_rows, term_rows)`` gives the float64 scores (len, m) of X rows ``x_rows`` with the per-row
    terms of rows ``term_rows`` (cosine ignores them).  variant: None, or what the second row block gets wrong --
    "self_off" (no + r0 on the dropped pair), "out" (d_mean / d_std without + r0), "x" (X read from row 0), "xterm" (PLDA: w.qe
    without + r0), or for every block "slab" (a slab adds up two cohort tiles and skips the rest of its share)."""
    rows = numpy.asarray(rows)
    mean, std = numpy.full(n, -7.0), numpy.full(n, -7.0)
    tiles_m, per, slabs = slab_rule(m)
    col_tile = numpy.arange(m) // COHORT_TILE
    counted = numpy.ones(m, dtype=bool) if variant != "slab" else (col_tile % per) < MIN_PER
    for r0 in range(0, n, rows_per_launch):
        local = rows[(rows >= r0) & (rows < r0 + rows_per_launch)] - r0
        if local.size == 0:
            continue
        s = scores_of(local + (0 if variant == "x" else r0), local + (0 if variant in ("x", "xterm") else r0))
        keep = numpy.broadcast_to(counted, s.shape).copy()
        cnt = numpy.full(local.size, float(m))
        if self_offset is not None:
            drop = local + self_offset + (0 if variant == "self_off" else r0)
            inside = (drop >= 0) & (drop < m)
            keep[numpy.flatnonzero(inside), drop[inside]] = False
            cnt -= inside
        v = numpy.where(keep, s, 0.0)
        mu = v.sum(1) / cnt
        var = (v * v).sum(1) / cnt - mu * mu
        out = local + (0 if variant == "out" else r0)
        mean[out], std[out] = mu, numpy.sqrt(numpy.maximum(var, 0.0))
    return mean, std


def kept_moments(s, drop):
    """Two-pass float64 mean and population std of every row of ``s`` without column ``drop[i]`` (None: every column)."""
    keep = numpy.ones(s.shape, dtype=bool)
    if drop is not None:
        keep[numpy.arange(s.shape[0]), drop] = False
    cnt = keep.sum(1)
    mu = numpy.where(keep, s, 0.0).sum(1) / cnt
    return mu, numpy.sqrt((numpy.where(keep, s - mu[:, None], 0.0) ** 2).sum(1) / cnt)


# ---- 4. VAD label fusion past one tile ----------------------------------------------------------------------------------------------
VAD_WINDOWS = (3, 31, VAD_MAX_WIN)           # the default, one between, and the widest (halo 4 * 127 = 508)
VAD_KW = dict(flooring=0.0001, ceiling=1.5, alpha=0.2)
_FEATURES = [(value, length, place) for value in (1, 0) for length in ("one", "r-1", "r", "r+1") for place in ("left", "right", "across")]


def vad_lengths(r):
    return [VAD_TILE, VAD_TILE + 1, VAD_TILE + 4 * r + 1, 2 * VAD_TILE + 300]


def _stamp(p, anchor, value, length, place, r):
    """A run of ``value`` beside / across ``anchor`` with r + 2 frames of the other value on either side of it."""
    n = p.shape[0]
    if length < 1:
        return
    start = {"left": anchor - length, "right": anchor, "across": anchor - (length + 1) // 2}[place]
    if place == "across" and length == 1:
        start = anchor - 1 if value else anchor
    a, b = max(0, start), min(n, start + length)
    p[max(0, a - r - 2):a] = 1 - value
    p[b:min(n, b + r + 2)] = 1 - value
    p[a:b] = value


def vad_patterns(win):
    """The designed raw labels for fusion window ``win`` (r = win // 2): for each of the four lengths, 24 rows, one per kind of short
    feature -- an isolated frame or a run of r - 1, r or r + 1 frames, of ones or of zeros, ending at, starting at or lying across a
    frame -- put at frames 2048 and 4096 (where the row reaches them); the row's two ends get the next kinds in the list, ending at the
    last frame and starting at the first.  Between the features: blocks of 4 r + 9 ones and zeros, which every fusion leaves alone."""
    r = win // 2
    block = 4 * r + 9
    rows = []
    for n in vad_lengths(r):
        for k, (value, length, place) in enumerate(_FEATURES):
            p = ((numpy.arange(n) + 3 * k) // block % 2 == 0).astype(numpy.uint8)
            size = lambda name: {"one": 1, "r-1": r - 1, "r": r, "r+1": r + 1}[name]   # noqa: E731
            v1, l1, _ = _FEATURES[(k + 5) % len(_FEATURES)]
            v2, l2, _ = _FEATURES[(k + 11) % len(_FEATURES)]
            _stamp(p, n, v1, size(l1), "left", r)
            _stamp(p, 0, v2, size(l2), "right", r)
            for anchor in (2 * VAD_TILE, VAD_TILE):
                if anchor < n:
                    _stamp(p, anchor, value, size(length), place, r)
            rows.append(p)
    rows.append(numpy.array([1], dtype=numpy.uint8))                                                # one frame: degenerate, kept whole
    rows.append(numpy.array([1, 0, 0, 1, 1, 1, 0, 1, 0, 0, 0, 1, 1, 0, 1, 1, 1, 1, 0, 0, 1, 0, 1, 1, 0], dtype=numpy.uint8))   # an ordinary row
    return rows


def vad_log_energies(patterns):
    """Two well separated levels with a small jitter -> (le (B, T) float64, nframes (B,) int32)."""
    T = max(p.shape[0] for p in patterns)
    le = numpy.zeros((len(patterns), T))
    for b, p in enumerate(patterns):
        le[b, :p.shape[0]] = 10.0 * p + 1e-4 * numpy.cos(numpy.arange(p.shape[0]))
    return le, numpy.array([p.shape[0] for p in patterns], dtype=numpy.int32)


def fuse_per_tile(p, win, variant):
    """Closing then opening of raw labels one VAD_TILE at a time, wrongly: "reflect" applies the row-end rule at every tile edge (a tile
    is fused as if it were a row); "no_halo" lets a window stop at the tile's edge (the frames beyond it do not exist)."""
    from scipy.ndimage import maximum_filter1d, minimum_filter1d
    assert variant in ("reflect", "no_halo")
    if variant == "reflect":
        dilate, erode = (lambda x: maximum_filter1d(x, win, mode="reflect")), (lambda x: minimum_filter1d(x, win, mode="reflect"))
    else:
        dilate = lambda x: maximum_filter1d(x, win, mode="constant", cval=0)                          # noqa: E731
        erode = lambda x: minimum_filter1d(x, win, mode="constant", cval=1)                           # noqa: E731
    out = numpy.zeros(p.shape[0], dtype=bool)
    for c0 in range(0, p.shape[0], VAD_TILE):
        tile = numpy.ascontiguousarray(p[c0:c0 + VAD_TILE], dtype=numpy.uint8)
        out[c0:c0 + tile.shape[0]] = dilate(erode(erode(dilate(tile)))).astype(bool)
    return out
