"""-m gpu: engine.Tape.sweep -- a tape swept over a box of integer points the kernel makes itself, under a context, with a
summary reduced on the device (pipamd_tape_sweep, pip_tape_sweep_kernel of csrc/pip_tape.hip), both cell widths.

Authorities: the reference's recorded answers on the golden grid (tests/golden/tape_eval/p5_grid.json) and for the
Urs_parms family of tests/golden/tape_edit; pipamd_tape_eval at the materialised box; the pivot kernels, solving the
instances of a problem solved under a context (Batch(instances=True)); tests/tape_sweep_model.py (held to the reference by
tests/test_tape_sweep_model.py).  No point is left out of any comparison."""
import ctypes as C

import numpy as np
import pytest

import tape_cases as tc
import tape_edit_model as te
import tape_model as tm
import tape_sweep_model as sm
from tape_cases import MAX64, MIN64
from test_gpu_tape_edit import family, solved
from test_gpu_tape_eval import _engine, _ints, _results, _solve_p5

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]


def results_of(t, out):
    names = t.OUTPUTS if t.ndual else t.OUTPUTS[:4]
    return _results(tuple(out[k] for k in names), t.bits, t.ndual)


def summary_of(t, summary):
    import torch
    from piplib_amd import engine as eng
    torch.cuda.synchronize()
    return eng.sweep_summary(summary, t.info["leaves"])


def hold_to_model(cells, nvar, nparm, ndual, lo, hi, ctx=(), bits=64):
    """sweep on the device, results and summary against the model: (model results, model summary)"""
    from piplib_amd import engine as eng
    t = eng.Tape(_engine(), cells, nvar, nparm, ndual, bits)
    plan = t.sweep_plan(lo, hi)
    assert plan == sm.plan(t.info, bits, nparm, lo, hi)
    summary, out = t.sweep(lo, hi, ctx=(ctx if len(ctx) else None))
    got, got_sum = results_of(t, out), summary_of(t, summary)
    t.close()
    want, want_sum = sm.sweep(cells, nvar, nparm, ndual, lo, hi, ctx, bits)
    assert len(got) == len(want) == plan["n_points"]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)
    assert got_sum == want_sum
    assert sum(got_sum["counts"].values()) == plan["n_points"]
    assert sum(got_sum["leaf_count"]) == got_sum["counts"]["solution"] + got_sum["counts"]["nil"] or not cells
    return want, want_sum


def numpy_summary(status, leaf, leaves):
    """the summary as a reduction of per-point status and leaf arrays"""
    s = {"counts": {}, "first": {}, "leaf_count": [], "leaf_first": []}
    for name, st in sm.STATUSES:
        at = np.flatnonzero(status == st)
        s["counts"][name], s["first"][name] = len(at), int(at[0]) if len(at) else -1
    for i in range(leaves):
        at = np.flatnonzero(leaf == i)
        s["leaf_count"].append(len(at))
        s["leaf_first"].append(int(at[0]) if len(at) else -1)
    return s


def identity(cols):
    """the list (theta_0 .. theta_(cols-1)): x_num shows the decoded point"""
    return tc.leaf([([int(i == j) for j in range(cols)] + [0], 1) for i in range(cols)])


def set_blocks(n):
    from piplib_amd import engine as eng
    fn = eng.lib().pipamd_debug_tape_sweep_blocks
    fn.argtypes = [C.c_int]
    assert fn(n) == 0


# ---------------------------------------------------------------- 1. the golden box
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("name,nq", [("int", 1), ("rat", 0)])
def test_golden_box(name, nq, bits):
    """p5 solved once and swept over [0,9]^2: the per-point answers are the reference's recorded ones, the summary the
    model's"""
    g = tc.golden()
    cells, _ = _solve_p5(nq, bits)
    want, want_sum = hold_to_model(cells, g["nvar"], g["nparm"], 0, [0, 0], [9, 9], (), bits)
    assert tc.answers_of(want) == g["answers"][name]
    assert sum(c > 0 for c in want_sum["leaf_count"]) >= 6


# ---------------------------------------------------------------- 2. sweep equals eval
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("dual", [False, True])
def test_sweep_equals_eval(dual, bits):
    """all six arrays equal pipamd_tape_eval at the materialised box byte for byte; the summary is a numpy reduction of
    eval's status and leaf"""
    import torch
    from piplib_amd import engine as eng
    g = tc.golden()
    cells, ndual = _solve_p5(0 if dual else 1, bits, dual=dual)
    t = eng.Tape(_engine(), cells, g["nvar"], g["nparm"], ndual, bits)
    lo, hi = [-3, -2], [12, 9]
    pts = np.array(sm.box_points(lo, hi), dtype=np.int64)
    assert len(pts) == 16 * 12
    ev = t.eval(pts)
    summary, out = t.sweep(lo, hi)
    torch.cuda.synchronize()
    names = t.OUTPUTS if ndual else t.OUTPUTS[:4]
    assert set(out) == set(names) and len(ev) == len(names)
    for k, v in zip(names, ev):
        assert out[k].dtype == v.dtype and torch.equal(out[k], v), k
    got = summary_of(t, summary)
    assert got == numpy_summary(ev[0].cpu().numpy(), ev[1].cpu().numpy(), t.info["leaves"])
    assert got["counts"]["outside"] == 0 and got["counts"]["solution"] > 100 and sum(c > 0 for c in got["leaf_count"]) >= 6
    # the summary alone, and the arrays alone, are the same figures
    alone, none = t.sweep(lo, hi, outputs=())
    assert none == {} and summary_of(t, alone) == got
    no_sum, out2 = t.sweep_into(lo, hi, t.outputs(len(pts), names))
    torch.cuda.synchronize()
    assert no_sum is None and all(torch.equal(out2[k], v) for k, v in zip(names, ev))
    t.close()


# ---------------------------------------------------------------- 3. chunk and grid edges
@pytest.mark.parametrize("bits", [64, 128])
def test_chunk_edges(bits):
    cells = tc.if_chain(5)
    for n in (1, 127, 128, 129, 257):
        hold_to_model(cells, 1, 1, 0, [-2], [-2 + n - 1], (), bits)


def test_grid_stride_loop():
    """1000 points through 1, 2 and 3 workgroups and the default grid: identical, and the model's"""
    import torch
    from piplib_amd import engine as eng
    cells = tc.if_chain(5)
    t = eng.Tape(_engine(), cells, 1, 1, 0, 64)
    want, want_sum = sm.sweep(cells, 1, 1, 0, [-3], [996])
    seen = []
    try:
        for blocks in (1, 2, 3, 0):
            set_blocks(blocks)
            summary, out = t.sweep([-3], [996])
            torch.cuda.synchronize()
            assert results_of(t, out) == want and summary_of(t, summary) == want_sum, blocks
            seen.append((summary.cpu(), {k: v.cpu() for k, v in out.items()}))
    finally:
        set_blocks(0)
    for s, o in seen[1:]:
        assert torch.equal(s, seen[0][0]) and all(torch.equal(o[k], seen[0][1][k]) for k in o)
    t.close()


# ---------------------------------------------------------------- 4. decoding
@pytest.mark.parametrize("bits", [64, 128])
def test_decoding_mixed_radix(bits):
    lo = [MIN64, -1, MAX64 - 4, 0]
    hi = [MIN64 + 2, -1, MAX64, 1]
    want, _ = hold_to_model(identity(4), 4, 4, 0, lo, hi, (), bits)
    assert len(want) == 30 and [[n for n, _ in w[2]] for w in want] == sm.box_points(lo, hi)
    assert want[0][2][0] == (MIN64, 1) and want[-1][2][2] == (MAX64, 1)


@pytest.mark.parametrize("bits", [64, 128])
def test_decoding_31_columns(bits):
    """ten columns of extent 2 among 31, lo values of both signs: 1024 points"""
    wide = (0, 3, 4, 9, 12, 17, 20, 25, 29, 30)
    lo = [(-1) ** c * ((1 << (2 * c)) + c) for c in range(31)]
    hi = [v + (c in wide) for c, v in enumerate(lo)]
    want, _ = hold_to_model(identity(31), 31, 31, 0, lo, hi, (), bits)
    assert len(want) == 1024 and [[n for n, _ in w[2]] for w in want] == sm.box_points(lo, hi)


@pytest.mark.parametrize("bits", [64, 128])
def test_no_parameters_is_one_point(bits):
    want, want_sum = hold_to_model(tc.iff([-3], tc.nil(), tc.leaf([([7], 2)])), 1, 0, 0, [], [], (), bits)
    assert want == [(tm.ST_SOLUTION, 1, [(7, 2)], [])] and want_sum["leaf_first"] == [-1, 0]
    want, want_sum = hold_to_model([], 2, 1, 0, [4], [8], (), bits)  # the empty tape: NIL, leaf -1, no leaf counted
    assert want_sum["counts"]["nil"] == 5 and want_sum["leaf_count"] == []


# ---------------------------------------------------------------- 5. both summary paths
@pytest.mark.parametrize("binned", [1, 0])
def test_both_summary_paths(binned):
    """a chain with k + 1 leaves at the planner's last binned L and the first unbinned one; the box reaches every leaf
    once and the last one 300 times"""
    import torch
    from piplib_amd import engine as eng
    k = next(k for k in range(1300, 1400)
             if sm.binned(tm.check(tc.if_chain(k), 1, 1), 64) and not sm.binned(tm.check(tc.if_chain(k + 1), 1, 1), 64))
    k += 1 - binned
    cells = tc.if_chain(k)
    t = eng.Tape(_engine(), cells, 1, 1, 0, 64)
    lo, hi = [0], [k + 299]
    assert t.sweep_plan(lo, hi) == {"n_points": k + 300, "summary_words": 8 + 2 * (k + 1), "binned": binned}
    summary, _ = t.sweep(lo, hi, outputs=())
    got = summary_of(t, summary)
    _, want = sm.sweep(cells, 1, 1, 0, lo, hi)
    assert want["leaf_count"] == [1] * k + [300] and want["leaf_first"] == list(range(k + 1))
    assert got == want
    # again into the same buffer: the call initialises it, nothing accumulates
    first = summary.clone()
    t.sweep_into(lo, hi, {}, summary=summary)
    torch.cuda.synchronize()
    assert torch.equal(summary, first)
    t.close()


# ---------------------------------------------------------------- 6. the context, hand-made rows
CONTEXTS = {
    "no rows": [],
    "one inequality": [[1, 1, -1, -1]],
    "one equality": [[0, 1, -1, 0]],
    "both": [[1, 1, 1, -4], [0, 1, -2, 0]],
    "a marker of -5": [[-5, 1, 0, -3]],
    "nothing inside": [[1, 0, 0, -1]],
    "an equality nothing meets": [[0, 2, 2, -1]],
}


@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("name", list(CONTEXTS))
def test_context_rows(name, bits):
    ctx = CONTEXTS[name]
    cells = tc.iff([1, 1, -5], identity(2), tc.nil())
    want, want_sum = hold_to_model(cells, 2, 2, 0, [-1, -2], [11, 10], ctx, bits)
    outside = [k for k, p in enumerate(sm.box_points([-1, -2], [11, 10])) if not sm.inside(p, ctx)]
    assert want_sum["counts"]["outside"] == len(outside) and want_sum["first"]["outside"] == (outside[0] if outside else -1)
    assert all(want[k] == (sm.ST_OUTSIDE, -1, [(0, 0)] * 2, []) for k in outside)
    if name in ("nothing inside", "an equality nothing meets"):
        assert len(outside) == 169 and sum(want_sum["leaf_count"]) == 0
    elif name != "no rows":
        assert 0 < len(outside) < 169


@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("case", range(len(sm.edge_rows())))
def test_context_rows_at_the_edges(case, bits):
    """the CPU test's rows: a value beyond 128 bits with the right sign, an equality met only through cancellation, a
    marker other than 0 or 1 -- at a box of the one point"""
    rows, point, inside = sm.edge_rows()[case]
    cols = len(point)
    want, want_sum = hold_to_model(tc.nil(), 1, cols, 0, point, point, rows, bits)
    assert want_sum["counts"] == {"solution": 0, "nil": int(inside), "range": 0, "outside": int(not inside)}


# ---------------------------------------------------------------- 7. the context of a solved problem
P5_CONTEXT = [[1, 1, -8], [-1, 2, 4]]  # theta_0 + theta_1 >= 8, 2 theta_1 - theta_0 + 4 >= 0: coefficients | constant


@pytest.mark.parametrize("bits", [64, 128])
def test_context_of_a_solved_problem(bits):
    """p5 solved under two context rows and swept over [0,11]^2 with the same rows in PolyLib form: every inside point
    has the answer of its instance solved by the pivot kernels; outside points are OUTSIDE"""
    import torch
    import system_model as sy
    from piplib_amd import engine as eng
    g = tc.golden()
    nvar, nparm = g["nvar"], g["nparm"]
    tab = tc.parametric_tableau(g["matrix"], nvar, nparm, g["eq_rows"])
    rows = np.array(P5_CONTEXT, dtype=np.int64)
    cells, _ = eng.solve_tableau_cells(_engine(), nvar, nparm, tab.shape[0], len(rows), -1, 1, tab, rows, bits=bits)
    ctx = [[1] + r for r in P5_CONTEXT]
    lo, hi = [0, 0], [11, 11]
    points = sm.box_points(lo, hi)
    t = eng.Tape(_engine(), cells, nvar, nparm, 0, bits)
    summary, out = t.sweep(lo, hi, ctx=ctx)
    got, got_sum = results_of(t, out), summary_of(t, summary)
    t.close()
    is_in = [sm.inside(p, ctx) for p in points]
    assert 0.3 * len(points) <= sum(is_in) <= 0.7 * len(points)
    assert got_sum["counts"]["outside"] == len(points) - sum(is_in) and sum(c > 0 for c in got_sum["leaf_count"]) >= 3
    b = eng.Batch(_engine(), (np.array(g["matrix"], dtype=np.int64), np.array(points, dtype=np.int64)), nvar, 0,
                  tflags=eng.T_INT, entier_bits=bits, instances=True, eq_rows=g["eq_rows"], simplify=1)
    b.load()
    b.solve()
    b.fetch()
    torch.cuda.synchronize()
    st = b.status.cpu().tolist()
    num, den = _ints(b.sol_num, bits), _ints(b.sol_den, bits)
    for k, p in enumerate(points):
        if not is_in[k]:
            assert got[k] == (sm.ST_OUTSIDE, -1, [(0, 0)] * nvar, []), (k, p, got[k])
            continue
        assert st[k] in (eng.ST_SOLUTION, eng.ST_NIL) and got[k][0] == st[k], (k, p, got[k][0], st[k])
        want = [sy.reduce_pair(num[k][i][0], den[k][i]) if st[k] == eng.ST_SOLUTION else (0, 0) for i in range(nvar)]
        assert got[k][2] == want, (k, p, got[k][2], want)
    assert got_sum == sm.summarise(got, tm.check(cells, nvar, nparm, 0, bits)["leaves"])


# ---------------------------------------------------------------- 8. pip_solve's edits
@pytest.mark.parametrize("bits", [64, 128])
def test_edited_tape_with_negative_parameters(bits):
    """the Urs_parms family (signed parameters) swept over the bounding box of its fixture points: the recorded answers
    at those points, the edit model's everywhere"""
    from piplib_amd import engine as eng
    g = family("urs_parms")
    cells, info = solved("urs_parms", bits)
    t = eng.Tape(_engine(), cells, info["nvar"], info["nparm"], 0, bits, edit=info)
    assert t.point_cols == g["nparm"] == 2
    pts = np.array(g["points"])
    lo, hi = pts.min(axis=0).tolist(), pts.max(axis=0).tolist()
    assert lo[0] < 0 and lo[1] < 0
    summary, out = t.sweep(lo, hi)
    got, got_sum = results_of(t, out), summary_of(t, summary)
    leaves = t.info["leaves"]
    t.close()
    box = sm.box_points(lo, hi)
    assert got == te.evaluate_cells(cells, info["nvar"], info["nparm"], 0, box, info, bits)
    at = {tuple(p): k for k, p in enumerate(box)}
    for p, a in zip(g["points"], g["answers"]):
        r = got[at[tuple(p)]]
        assert r[0] == (tm.ST_SOLUTION if a is not None else tm.ST_NIL) and te.same_answer(te.answer_of(r), a), (p, r, a)
    assert got_sum == sm.summarise(got, leaves) and sum(c > 0 for c in got_sum["leaf_count"]) >= 4


# ---------------------------------------------------------------- 9. two streams
def test_two_streams():
    import torch
    from piplib_amd import engine as eng
    g = tc.golden()
    cells = tc.cells_from_text(g["tapes"]["int"])
    t = eng.Tape(_engine(), cells, g["nvar"], g["nparm"], 0, 64)
    lo, hi, ctx = [-5, -5], [58, 58], [[1, 1, 1, -3]]
    single = t.sweep(lo, hi, ctx=ctx)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = t.sweep(lo, hi, ctx=ctx)
    with torch.cuda.stream(s2):
        b = t.sweep(lo, hi, ctx=ctx)
    torch.cuda.synchronize()
    for other in (a, b):
        assert torch.equal(other[0], single[0])
        assert all(torch.equal(other[1][k], single[1][k]) for k in single[1])
    want, want_sum = sm.sweep(cells, g["nvar"], g["nparm"], 0, lo, hi, ctx)
    assert results_of(t, single[1]) == want and summary_of(t, single[0]) == want_sum
    t.close()
