"""The longdouble references of the float64 back end (tests/tools/f64_forms.py) without a GPU: the thresholds the GPU shapes rest on read
out of the sources, tn_cut re-implemented and its slab counts asserted, a float64 numpy evaluation shown to pass every criterion on the very
operands tests/test_gpu_f64_forms.py uses (the largest share is printed; it must stay below 1), every wrong kernel of the list shown to
fail in every case it can show in, and what the suite's earlier criterion -- one relative max-norm against float64 numpy -- does with the
same wrong kernels on the same operands (the ones it lets through are the gap the per-element criteria close: DESIGN.md section 4h)."""
import os
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import f64_forms as ff  # noqa: E402


def _say(capsys, text):
    with capsys.disabled():
        print(text)


def test_the_sources_state_the_thresholds_the_shapes_assume():
    src = ff.read_sources()
    assert src == {k: getattr(ff, k) for k in src}, "a threshold moved: move the shape lists of tests/tools/f64_forms.py with it"
    dk, t, bt = ff.DK, ff.TILE, ff.BIG_TILE
    tn = ff.TN_SHAPES
    assert (1, 1, 1) in tn and (dk, t, t) in tn and (dk + 1, t + 1, t - 1) in tn, "TN_SHAPES: one tile and one k-tile, one past and one short"
    assert any(k < dk and m % 2 == 0 and n > 2 * t and n % 2 == 0 for k, m, n in tn), "TN_SHAPES: pair loads and three column tiles"
    assert (ff.SLAB_K + 1, 6, 5) in tn and ff.tn_cut(ff.SLAB_K, 6, 5)[2] == 1 and ff.tn_cut(ff.SLAB_K + 1, 6, 5)[2] == 2, "TN_SHAPES: the first second slab"
    big = [s for s in tn if ff.tn_cut(*s)[0]]
    assert big == [(ff.BIG_K, ff.BIG_M, ff.BIG_N), (ff.BIG_K + 1, ff.BIG_M + 1, ff.BIG_N + 2)], "TN_SHAPES: the smallest 128-tile launch and a ragged one"
    assert (ff.BIG_K - 1, ff.BIG_M, ff.BIG_N) in tn and (ff.BIG_K, ff.BIG_M, ff.BIG_N - 1) in tn, "TN_SHAPES: just below the 128-tile form on each side"
    assert ff.tn_cut(4097, 129, 130) == (True, bt, 9, 464) and ff.tn_cut(513, 6, 5) == (False, t, 2, 272), "the slab counts the shape lists claim"
    assert ff.tn_cut(4096, 128, 128)[1:3] == (bt, 8) and ff.tn_cut(4095, 128, 128)[1] == t and ff.tn_cut(4096, 128, 127)[1] == t
    ga = ff.GATHERED_SHAPES
    assert [ff.tn_cut(n, d, d)[:3] for n, d in ga] == [(False, t, 1), (False, t, 1), (False, t, 1), (False, t, 2), (True, bt, 8), (True, bt, 9)], "GATHERED_SHAPES"
    cuts = [ff.tn_cut(max(c), d, d, len(c)) for c, d in ff.CLASS_SHAPES]
    assert [c[:3] for c in cuts] == [(False, t, 2), (False, t, 1), (True, bt, 8)], "CLASS_SHAPES"
    counts, slab = ff.CLASS_SHAPES[0][0], cuts[0][3]
    assert sum(c <= slab for c in counts) == 4 and max(counts) > slab, "CLASS_SHAPES: four classes end before the second slab"
    assert {dk - 1, dk, dk + 1} <= set(counts) and any(1 in c for c, _ in ff.CLASS_SHAPES)
    nt = ff.NN_TILE
    assert (1, 1, 1) in ff.NN_SHAPES and (nt, nt, dk) in ff.NN_SHAPES and (nt + 1, nt - 1, dk + 1) in ff.NN_SHAPES, "NN_SHAPES"
    assert any(n > 2 * nt and n % 2 == 0 and k % 2 == 0 for _, n, k in ff.NN_SHAPES) and any(m > 2 * nt for m, _, _ in ff.NN_SHAPES), "NN_SHAPES"
    ps = {p for _, _, p in ff.WHITEN_SHAPES}
    assert set(ff.WHITEN_P) <= ps and {ff.WHITEN_P[0] + 1, ff.WHITEN_P[1] + 1, ff.WHITEN_P[2] + 1} <= ps, "WHITEN_SHAPES: each column regime at its edge and one past"
    assert all(n > ff.WHITEN_ROWS or n == 1 or (n, p) == (ff.WHITEN_ROWS, ff.WHITEN_P[0]) for n, _, p in ff.WHITEN_SHAPES)
    lb = [(-(-n // 128)) * c >= ff.LOGLIK_BIG for n, _, c in ff.LOGLIK_SHAPES]
    assert lb == [False, False, False, True, True] and ff.LOGLIK_SHAPES[3][0] == 1, "LOGLIK_SHAPES: the 128-row form, once with one row"
    assert any(d == t + 1 for _, d, _ in ff.LOGLIK_SHAPES) and any(d > 2 * t for _, d, _ in ff.LOGLIK_SHAPES), "LOGLIK_SHAPES: column tiles"
    g = ff.GRAM_TILE
    assert {r for _, _, r in ff.GRAM_SHAPES} >= {g, g + 1, 2 * g + 2, 3 * g} and any(d == dk + 1 for _, d, _ in ff.GRAM_SHAPES), "GRAM_SHAPES"


def test_the_operands_are_what_the_docstring_says():
    case = ff.gathered_case((513, 6), True, "float32")
    cls, C = case["cls"], case["C"]
    assert cls[1] == -1 and cls[511] == C + 5 and int((cls == C - 1).sum()) == 1 and numpy.array_equal(case["Mc"][C - 1], case["X"][256].astype(numpy.float64))
    assert case["X"].dtype == numpy.float32 and case["Mc"].dtype == numpy.float64 and 0.5 <= case["w"].min() and case["w"].max() <= 12
    for dtype in ff.DTYPES:
        for centred in (False, True):
            c = ff.whiten_case((70, 37, 129), centred, dtype)
            x = c["X"].astype(numpy.float64) - (c["mu"] if centred else 0.0)
            assert (x[ff.WHITEN_ZERO_ROW] == 0).all() and c["X"].dtype == numpy.dtype(dtype)
            assert (c["tiny"] is None) == (centred and dtype == "float32")
            if c["tiny"] is not None:
                assert 0 < numpy.linalg.norm(x[c["tiny"]] @ c["R"]) < ff.EPS_LEN / 2
    c = ff.tn_case((17, 65, 63), "w+ca+cb", "float64")
    sa = c["A"].std(0)
    assert sa.max() / sa.min() > 100 and (numpy.abs(c["ca"] - c["A"].mean(0)) < 4 * sa).all(), "a scale per column, a centre within it"
    c = ff.nn_case((64, 64, 16), "posterior")
    assert (numpy.outer(c["rowv"], c["colv"]) >= 0).all()


# ---- the cases of every entry point: (label, what the case says about itself, r, bound, eval(mutant)) ------------------------------------
def _tn_cases():
    for shape in ff.TN_SHAPES:
        for form in ff.TN_FORMS:
            for dtype in ff.DTYPES:
                case, r, b = ff.tn(shape, form, dtype)
                yield f"tn{shape} {form} {dtype}", dict(shape=shape, form=form, cut=ff.tn_cut(*shape)), r, b, lambda m, c=case: ff.tn_eval(mutant=m, **c)


def _gathered_cases():
    for shape in ff.GATHERED_SHAPES:
        for weighted in (False, True):
            for dtype in ff.DTYPES:
                case, r, b = ff.gathered(shape, weighted, dtype)
                yield (f"gathered{shape} w={weighted} {dtype}", dict(shape=shape, weighted=weighted, cut=ff.tn_cut(shape[0], shape[1], shape[1])), r, b,
                       lambda m, c=case: ff.gathered_eval(mutant=m, **c))


def _class_cases():
    for counts, D in ff.CLASS_SHAPES:
        for dtype in ff.DTYPES:
            case, r, b = ff.classes(counts, D, dtype)
            yield (f"class{counts, D} {dtype}", dict(counts=counts, D=D, cut=ff.tn_cut(max(counts), D, D, len(counts))), r, b,
                   lambda m, c=case: ff.class_eval(c["X"], c["off"], c["Mc"], c["counts"], m))


def _gram_cases():
    for shape in ff.GRAM_SHAPES:
        case, r, b = ff.gram(shape)
        yield f"gram{shape}", dict(shape=shape), r, b, lambda m, c=case: ff.gram_eval(c["F"], m)


def _nn_cases():
    for shape in ff.NN_SHAPES:
        for epi in ff.NN_EPILOGUES:
            case, r, b = ff.nn(shape, epi)
            yield f"nn{shape} {epi}", dict(shape=shape, epi=epi), r, b, lambda m, c=case: ff.nn_eval(mutant=m, **c)


def _whiten_cases():
    for shape in ff.WHITEN_SHAPES:
        for centred in (False, True):
            for dtype in ff.DTYPES:
                for normalize in (0, 1):
                    case, r, b = ff.whiten(shape, centred, dtype, normalize)
                    yield (f"whiten{shape} mu={centred} {dtype} normalize={normalize}", dict(shape=shape, normalize=normalize), r, b,
                           lambda m, c=case, nz=normalize: ff.whiten_eval(c["X"], c["mu"], c["R"], nz, m))


def _loglik_cases():
    for shape in ff.LOGLIK_SHAPES:
        case, r, b = ff.loglik(shape)
        yield f"loglik{shape}", dict(shape=shape), r, b, lambda m, c=case: ff.loglik_eval(mutant=m, **c)


# mutant -> the cases it can show in
FAMILIES = {
    "tn": (_tn_cases, {
        "drop_last_row": lambda i: True,
        "padding": lambda i: i["shape"][0] % ff.DK != 0 and i["form"] == "w+ca+cb",
        "w_from_0": lambda i: i["cut"][2] > 1 and "w" in i["form"],
        "join_early": lambda i: i["cut"][2] > 1,
        "swap_centres": lambda i: i["shape"][1] != i["shape"][2] and i["form"] == "w+ca+cb",
        "odd_row_next": lambda i: i["shape"][1] % 2 == 1,
        "transposed": lambda i: i["shape"][1:] != (1, 1)}),
    "gathered": (_gathered_cases, {
        "drop_last_row": lambda i: i["shape"][0] > 1,          # N = 1: the one row is its class's mean, the answer is 0 with or without it
        "join_early": lambda i: i["cut"][2] > 1,
        "odd_row_next": lambda i: i["shape"][1] % 2 == 1,
        "clamp_class": lambda i: i["shape"][0] > 1,
        "w_k": lambda i: i["shape"][0] > 1 and i["weighted"]}),
    "class": (_class_cases, {
        "drop_last_row": lambda i: True,
        "padding": lambda i: any(c % ff.DK for c in i["counts"]),
        "join_early": lambda i: i["cut"][2] > 1,
        "odd_row_next": lambda i: i["D"] % 2 == 1}),
    "gram": (_gram_cases, {
        "drop_last_row": lambda i: True,
        "odd_row_next": lambda i: i["shape"][2] % 2 == 1,
        "packed_shift": lambda i: True}),
    "nn": (_nn_cases, {
        "drop_last_row": lambda i: True,
        "odd_row_next": lambda i: i["shape"][2] % 2 == 1,
        "swap_rowcol": lambda i: i["epi"] != "plain" and i["shape"][:2] != (1, 1),
        "row64_is_63": lambda i: i["shape"][0] > ff.NN_TILE}),
    "whiten": (_whiten_cases, {
        "drop_last_row": lambda i: True,
        "odd_row_next": lambda i: i["shape"][1] % 2 == 1,
        "len_plus_eps": lambda i: i["normalize"] == 1,
        "len_block0": lambda i: i["normalize"] == 1 and i["shape"][2] > ff.WHITEN_P[-1],
        "row64_is_63": lambda i: i["shape"][0] > ff.WHITEN_ROWS}),
    "loglik": (_loglik_cases, {
        "drop_last_row": lambda i: True,
        "row64_is_63": lambda i: i["shape"][0] > ff.TILE,
        "V_past_64": lambda i: i["shape"][1] > ff.TILE,
        "cst_prev": lambda i: i["shape"][2] > 1}),
}

# what one relative max-norm against float64 numpy lets through: (family, mutant) -> it passed in at least one case it can show in
OLD_CRITERION_PASSES = {
    ("whiten", "len_plus_eps"),        # at (70, 37, 129) and (66, 40, 256) with mu and float32 rows, where no row is short
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_float64_numpy_passes_and_every_wrong_kernel_fails(capsys, family):
    cases, mutants = FAMILIES[family]
    worst, n_cases = 0.0, 0
    tally = {m: [0, 0, 0] for m in mutants}                     # cases it can show in, rejected by the new criterion, passed by the old one
    survivors, let_through = [], []
    for label, info, r, bound, run in cases():
        n_cases += 1
        want = run(None)
        worst = max(worst, ff.check(f"float64 numpy on {label}", want, r, bound))
        for m, applies in mutants.items():
            if not applies(info):
                continue
            got = run(m)
            tally[m][0] += 1
            if float(ff.shares(got, r, bound).max()) > 1.0:
                tally[m][1] += 1
            else:
                survivors.append((m, label))
            if ff.old_criterion(got, want, ff.OLD_TOL[family]):
                tally[m][2] += 1
                let_through.append(f"{m} on {label}")
    lines = [f"\n  [{family}: float64 numpy uses at most {worst:.3f} of its bound over {n_cases} cases]"]
    lines += [f"    {m}: rejected in {b} of {a} cases; the relative max-norm at {ff.OLD_TOL[family]:g} passes it in {c}" for m, (a, b, c) in tally.items()]
    lines += [f"    the relative max-norm passes {t}" for t in let_through]
    _say(capsys, "\n".join(lines))
    assert worst < 1.0
    assert all(a > 0 for a, _, _ in tally.values()), f"a wrong kernel has no case to show in: {tally}"
    assert not survivors, f"the criteria pass these wrong kernels: {survivors}"
    passed_old = {(family, m) for m, (_, _, c) in tally.items() if c}
    assert passed_old == {k for k in OLD_CRITERION_PASSES if k[0] == family}, f"what the relative max-norm lets through changed: {sorted(passed_old)}"


def test_a_sequential_float64_chain_passes_the_tn_criterion(capsys):
    """one accumulator per element, k ascending, no blocking: the slowest-converging order a kernel may take"""
    worst = 0.0
    for shape in ((17, 65, 63), (513, 6, 5)):
        for form in ff.TN_FORMS:
            case, r, bound = ff.tn(shape, form, "float64")
            a, b = case["A"].astype(numpy.float64), case["B"]
            a = a - case["ca"] if case["ca"] is not None else a
            b = b - case["cb"] if case["cb"] is not None else b
            a = a * case["w"][:, None] if case["w"] is not None else a
            acc = numpy.zeros(r.shape)
            for k in range(shape[0]):
                acc = acc + numpy.outer(a[k], b[k])
            worst = max(worst, ff.check(f"chain {shape} {form}", acc, r, bound))
    _say(capsys, f"\n  [a sequential float64 chain uses at most {worst:.3f} of (K + 8) u S]")
    assert worst < 1.0
