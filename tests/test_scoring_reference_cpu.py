"""The float64 references of the trial-scoring kernels (tests/tools/scoring_f64.py) without a GPU: the thresholds the GPU shapes rest on
read out of the sources, float32 evaluations of every formula shown to pass its criterion on the very operands
tests/test_gpu_scoring_kernels.py uses, and the criteria shown to reject wrong kernels on them.  The top-k statistics: a centred float64
evaluation passes, the one-pass expression (sum v^2 - k m^2) / (k - 1) does not."""
import os
import sys

import numpy
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import scoring_f64 as sf  # noqa: E402


def _say(capsys, text):
    with capsys.disabled():
        print(text)


def _mutants(capsys, title, mutants):
    """every (name, run) must raise AssertionError"""
    lines, survivors = [], []
    for name, run in mutants:
        try:
            run()
            survivors.append(name)
        except AssertionError as e:
            lines.append(f"    rejected  {name}: {str(e)[:120]}")
    _say(capsys, f"\n  [{title}]\n" + "\n".join(lines))
    assert not survivors, f"the criteria pass these wrong kernels: {survivors}"


def test_the_sources_state_the_thresholds_the_shapes_assume():
    src = sf.read_sources()
    assert src == {k: getattr(sf, k) for k in src}, "a threshold moved: move the shapes of tests/tools/scoring_f64.py with it"
    shapes = sf.COSINE_SHAPES
    assert all(d % sf.D_MULTIPLE == 0 for _, _, d in shapes) and all(d % sf.D_MULTIPLE for d in sf.PAD_D)
    big = [(m, n) for m, n, _ in shapes if m >= sf.BIG_M and n >= sf.BIG_N]
    assert big == [(sf.BIG_M, sf.BIG_N), (sf.BIG_M + 1, sf.BIG_N + 1)]                      # the smallest 128-tile launch and a ragged one
    assert (sf.TILE, sf.TILE, sf.BK) in shapes and (sf.TILE + 1, sf.TILE - 1, sf.BK + 4) in shapes
    assert any(d < sf.BK for _, _, d in shapes) and any(d % sf.BK and d > sf.BK for _, _, d in shapes) and any(d >= 16 * sf.BK for _, _, d in shapes)
    assert all(d % sf.BK and d > sf.BK for d in sf.HIST_D) and 256 < sf.HIST_N < 512        # a k-tail after whole k-tiles, two ragged 256-tiles
    for stride, sizes in ((sf.NORM_STRIDE, sf.NORM_D), (sf.TOPK_STRIDE, sf.TOPK_NCOLS)):
        assert stride in sizes and stride + 1 in sizes and any(s > 2 * stride for s in sizes) and any(s < stride for s in sizes)
    assert 700 // sf.TOPK_STRIDE != 3 // sf.TOPK_STRIDE and max(sf.TOPK_NCOLS) > 700        # the tie across strides
    p = sf.TRIALS_PER_WG
    assert {p - 1, p, p + 1} <= set(sf.TRIAL_N) and any(n % p == 1 and n > 64 * p for n in sf.TRIAL_N)
    assert {63, 64, 65} <= set(sf.TRIAL_D) and any(d > 512 for d in sf.TRIAL_D)             # a wave's lanes stride D by 64
    assert sf.topk_cases()[0] == (2, 2) and len(sf.topk_cases()) == 17


# ---- sc_cosine ----------------------------------------------------------------------------------------------------------------------------
def test_cosine_criterion_passes_float32_and_rejects_every_mutant(capsys):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    worst = {"torch": 0.0, "fma": 0.0}
    for ne, nt, d in sf.COSINE_SHAPES:
        E, T = sf.cosine_operands(ne, nt, d)
        worst["torch"] = max(worst["torch"], sf.check_cosine(f"torch float32 {ne, nt, d}", E @ T.T, E, T)[2])
        worst["fma"] = max(worst["fma"], sf.check_cosine(f"FMA chain {ne, nt, d}", sf.fma_chain(E, T), E, T)[2])
    _say(capsys, f"\n  [sc_cosine: largest share of 2 K u S over the shapes: torch's float32 product {worst['torch']:.3f}, a sequential float32 FMA chain {worst['fma']:.3f}]")
    assert max(worst.values()) <= 0.5

    def swap_columns(E, T):
        out = (E @ T.T).clone()
        out[:, [sf.TILE + 1, sf.TILE + 2]] = out[:, [sf.TILE + 2, sf.TILE + 1]]
        return out

    def repeat_row(E, T):
        out = (E @ T.T).clone()
        out[sf.TILE] = out[sf.TILE - 1]
        return out

    every = sf.COSINE_SHAPES
    # (name, the shapes it can show on, the wrong product); "the pad columns read from the next row" is judged with the padding branch below
    mutants = [
        ("sc_cosine: last k-term dropped", every, lambda E, T: E[:, :-1] @ T[:, :-1].T),
        ("sc_cosine: two output columns swapped inside the second column tile", [s for s in every if s[1] > sf.TILE + 2], swap_columns),
        ("sc_cosine: row 64 answered with row 63", [s for s in every if s[0] > sf.TILE], repeat_row),
        ("sc_cosine: operands E and T exchanged on a non-square problem", [s for s in every if s[0] != s[1]],
         lambda E, T: (T @ E.T).reshape(E.shape[0], T.shape[0])),
    ]
    lines, survivors = [], []
    for name, shapes, wrong in mutants:
        assert len(shapes) >= 3
        for shape in shapes:
            E, T = sf.cosine_operands(*shape)
            try:
                sf.check_cosine(str(shape), wrong(E, T), E, T)
                survivors.append((name, shape))
            except AssertionError as e:
                msg = str(e)
        lines.append(f"    rejected on {len(shapes)} shapes  {name}: {msg[:100]}")
    _say(capsys, "\n".join(lines))
    assert not survivors, f"the criterion passes these wrong kernels: {survivors}"


def test_padding_branch_criterion_passes_float32_and_rejects_every_mutant(capsys):
    """cosine_matrix_device pads D to a multiple of 4 with zero columns; the result is judged against the UNPADDED operands with K = D."""
    def spill(x):
        """the pad columns of row i hold the first elements of row i + 1 (zeros after the last row): a padded view that was never zeroed"""
        n, d = x.shape
        pad = -d % sf.D_MULTIPLE
        flat = torch.cat([x.reshape(-1), torch.zeros(pad)])
        return torch.stack([flat[i * d:(i + 1) * d + pad] for i in range(n)])

    worst, rejected = 0.0, []
    for d in sf.PAD_D:
        for ne, nt in sf.PAD_SHAPES:
            E, T = sf.cosine_operands(ne, nt, d)
            Ep, Tp = sf.padded(E), sf.padded(T)
            assert Ep.shape[1] % sf.D_MULTIPLE == 0 and Ep.shape[1] - d < sf.D_MULTIPLE and bool((Ep[:, d:] == 0).all())
            worst = max(worst, sf.check_cosine(f"padded float32 {ne, nt, d}", Ep @ Tp.T, E, T)[2], sf.check_cosine("FMA chain", sf.fma_chain(Ep, Tp), E, T)[2])
            with pytest.raises(AssertionError):
                sf.check_cosine(f"pad columns read from the next row {ne, nt, d}", spill(E) @ spill(T).T, E, T)
            with pytest.raises(AssertionError):
                sf.check_cosine(f"last k-term dropped {ne, nt, d}", Ep[:, :d - 1] @ Tp[:, :d - 1].T if d > 1 else torch.zeros(ne, nt), E, T)
            rejected.append((ne, nt, d))
    _say(capsys, f"\n  [padding branch: float32 products use at most {worst:.3f} of 2 D u S; 'sc_cosine: the pad columns read from the next row instead of "
                 f"zeros' and 'last k-term dropped' rejected on all {len(rejected)} shapes]")
    assert worst <= 0.5


# ---- sc_normalize_rows --------------------------------------------------------------------------------------------------------------------
def test_normalize_criterion_passes_float32_and_rejects_the_mutant(capsys):
    worst = 0.0
    for d in list(sf.NORM_D) + [2, 7, 31, 64, 300, 777]:
        x = sf.normalize_operands(d)
        n = x.double().norm(dim=1)
        assert float(n[sf.NORM_ZERO_ROW]) == 0 and 0.9e-15 < float(n[sf.NORM_TINY_ROW]) < 1.1e-15
        worst = max(worst, sf.check_normalize(f"torch float32 D = {d}", torch.nn.functional.normalize(x, dim=1, eps=1e-12), x))
    _say(capsys, f"\n  [sc_normalize_rows: torch's float32 normalize uses at most {worst:.3f} of (D + 4) u |r|]")
    assert worst <= 0.5
    _mutants(capsys, "sc_normalize_rows", [
        (f"normalize: ||x|| + eps instead of max(||x||, eps), D = {d}",
         lambda d=d: sf.check_normalize("mutant", sf.normalize_operands(d) / (sf.normalize_operands(d).norm(dim=1, keepdim=True) + 1e-12), sf.normalize_operands(d)))
        for d in sf.NORM_D])


# ---- sc_cosine_trials ---------------------------------------------------------------------------------------------------------------------
def _trials64(E, T, ei, ti):
    """the kernel's formula in float64 numpy"""
    e, t = E.numpy().astype(numpy.float64)[ei], T.numpy().astype(numpy.float64)[ti]
    with numpy.errstate(invalid="ignore"):
        return (e * t).sum(1) / (numpy.sqrt((e * e).sum(1)) * numpy.sqrt((t * t).sum(1)))


def test_trials_criterion_passes_float64_and_rejects_every_mutant(capsys):
    worst, mutants = 0.0, []
    for d in sf.TRIAL_D:
        for n in sf.TRIAL_N:
            E, T, ei, ti = sf.trials_operands(d, n)
            assert int((ei == sf.TRIAL_ZERO_ROW).sum()) == (1 if n >= 3 else 0)
            got = _trials64(E, T, ei, ti)
            worst = max(worst, sf.check_trials(f"float64 D = {d}, n = {n}", got, E, T, ei, ti))

            def unwritten(got=got, a=(E, T, ei, ti)):
                out = got.copy()
                out[-1] = 1e30                                      # the sentinel the output buffer held
                sf.check_trials("mutant", out, *a)

            def shifted(a=(E, T, ei, ti)):
                E, T, ei, ti = a
                sf.check_trials("mutant", _trials64(E, T, ei, numpy.roll(ti, 1)), E, T, ei, ti)

            mutants.append((f"sc_cosine_trials: trial n - 1 not written, D = {d}, n = {n}", unwritten))
            if n >= 3 and d > 1:                                    # n = 1: the pair is the trial's own; D = 1: every cosine is +-1
                mutants.append((f"sc_cosine_trials: index pair (ei[k], ti[k - 1]), D = {d}, n = {n}", shifted))
    _say(capsys, f"\n  [sc_cosine_trials: numpy's float64 evaluation uses at most {worst:.3f} of 2 (D + 6) 2^-53 S / (|e| |t|)]")
    assert worst <= 0.5
    _mutants(capsys, "sc_cosine_trials", mutants)


# ---- sc_topk_stats / sc_topk_stats_f64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_topk_criteria_pass_the_centred_evaluation_and_reject_the_one_pass_one_and_every_mutant(capsys, dtype):
    """The centred float64 evaluation passes on every row of every case.  The one-pass expression of the kernel as it stood passes at
    float32 (u_T covers its cancellation) and is rejected at float64 in every case of families (b) and (c), and in most of (a).  Every
    mutant is rejected in every case it applies to.  (A float32 share close to 1 is the rounding of the result to float32 itself.)"""
    worst = {f: [0.0, 0.0] for f in sf.TOPK_FAMILIES[dtype]}
    one_pass = {f: [0, 0, 0.0] for f in sf.TOPK_FAMILIES[dtype]}                   # cases rejected, cases, largest share of the std bound
    wrong = {
        "top-k: k - 1 values taken": (dict(select="k-1"), lambda n, k, f: True),
        "top-k: every copy of a tied threshold counted": (dict(select="ties"), lambda n, k, f: k < n),
        "top-k: keys ordered by magnitude, negatives sort wrongly": (dict(select="magnitude"), lambda n, k, f: f in "ab" and k < n),
        "top-k: population std instead of unbiased std": (dict(ddof=0), lambda n, k, f: True),
        "top-k: only the first 256 columns seen": (dict(select="first256"), lambda n, k, f: n > 256 and (k >= 256 or n > 512)),   # 257 columns: a small k need not reach the last one
    }
    tally = {name: [0, 0] for name in wrong}
    for family in sf.TOPK_FAMILIES[dtype]:
        for ncols, k in sf.topk_cases():
            x, names = sf.topk_rows(ncols, k, family, dtype)
            assert x.dtype == numpy.dtype(dtype) and x.shape == (len(names), ncols) and names.count("random") == 5 and "equal" in names
            assert ("straddle" in names) == (k < ncols) and ("strides" in names) == (ncols > 700 and k < ncols)
            assert ("zeros" in names) == (family == "a" and k < ncols) and ("negative" in names) == (family == "a")
            m, s = sf.check_topk(f"centred {ncols, k, family}", *sf.topk_eval(x, k, centred=True), x, k, names)
            worst[family] = [max(worst[family][0], m), max(worst[family][1], s)]
            ms, ss = sf.topk_shares(*sf.topk_eval(x, k, centred=False), x, k)
            one_pass[family][0] += int(not ((ms <= 1).all() and (ss <= 1).all()))
            one_pass[family][1] += 1
            one_pass[family][2] = max(one_pass[family][2], float(ss[numpy.isfinite(ss)].max()))
            assert (ms <= 1).all(), "the mean's expression is not in question"
            for name, (kw, applies) in wrong.items():
                if applies(ncols, k, family):
                    tally[name][1] += 1
                    try:
                        sf.check_topk(name, *sf.topk_eval(x, k, centred=True, **kw), x, k, names)
                    except AssertionError:
                        tally[name][0] += 1
    _say(capsys, f"\n  [{dtype}: centred float64 evaluation, largest share of the (mean, std) bound: "
                 + ", ".join(f"({f}) {m:.3f}, {s:.3f}" for f, (m, s) in worst.items())
                 + "; one-pass expression rejected in " + ", ".join(f"({f}) {a} of {b} cases (std up to {w:.3g} of its bound)" for f, (a, b, w) in one_pass.items()) + "]\n"
                 + "\n".join(f"    rejected in {a} of {b} cases  {name}" for name, (a, b) in tally.items()))
    if dtype == "float32":
        assert all(a == 0 for a, _, _ in one_pass.values()), "float32 values and their squares are exact in double: the one-pass form is harmless there"
    else:
        assert one_pass["b"][0] == one_pass["b"][1] and one_pass["c"][0] == one_pass["c"][1], "the one-pass expression must not meet the std bound at float64"
    assert all(a == b and b > 0 for a, b in tally.values()), f"the criteria pass wrong kernels: {tally}"
