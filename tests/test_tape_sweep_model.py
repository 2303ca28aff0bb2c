"""tests/tape_sweep_model.py held to the reference: its box [0,9]^2 is the golden grid of tests/golden/tape_eval in order,
its per-point answers are the reference's recorded ones, its summary is a direct count over them; the context test at the
edges of the arithmetic.  Host only, Python ints only."""
import numpy as np
import pytest

import tape_cases as tc
import tape_model as tm
import tape_sweep_model as sm
from tape_cases import MAX64, MIN64


def test_the_box_is_the_golden_grid_in_order():
    g = tc.golden()
    assert sm.box_points([0, 0], [9, 9]) == g["points"]
    assert sm.box_points([0, 0], [9, 9]) == np.indices((10, 10)).reshape(2, -1).T.tolist()
    assert sm.box_points([], []) == [[]]
    assert sm.box_points([MIN64, -1, MAX64 - 1], [MIN64, 0, MAX64]) == [
        [MIN64, -1, MAX64 - 1], [MIN64, -1, MAX64], [MIN64, 0, MAX64 - 1], [MIN64, 0, MAX64]]


@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("name", ["int", "rat"])
def test_answers_and_summary_are_the_references(name, bits):
    g = tc.golden()
    cells = tc.cells_from_text(g["tapes"][name])
    res, summary = sm.sweep(cells, g["nvar"], g["nparm"], 0, [0, 0], [9, 9], (), bits)
    answers = g["answers"][name]
    assert tc.answers_of(res) == answers and len(res) == 100
    # a direct count over the recorded answers
    solved = [k for k, a in enumerate(answers) if a is not None]
    none = [k for k, a in enumerate(answers) if a is None]
    assert summary["counts"] == {"solution": len(solved), "nil": len(none), "range": 0, "outside": 0}
    assert summary["first"] == {"solution": solved[0] if solved else -1, "nil": none[0] if none else -1, "range": -1, "outside": -1}
    leaves = tm.check(cells, g["nvar"], g["nparm"], 0, bits)["leaves"]
    assert len(summary["leaf_count"]) == len(summary["leaf_first"]) == leaves
    assert sum(summary["leaf_count"]) == 100 and sum(c > 0 for c in summary["leaf_count"]) >= 6
    for i in range(leaves):
        at = [k for k, r in enumerate(res) if r[1] == i]
        assert summary["leaf_count"][i] == len(at) and summary["leaf_first"][i] == (at[0] if at else -1)
        # a leaf is a solution list or a NIL: its points all have, or all lack, a recorded answer
        assert len({answers[k] is None for k in at}) <= 1
    assert sm.words(summary)[:4] == [len(solved), len(none), 0, 0] and len(sm.words(summary)) == 8 + 2 * leaves


def test_context_rows_split_the_golden_box():
    g = tc.golden()
    cells = tc.cells_from_text(g["tapes"]["int"])
    ctx = [[1, 1, 0, -3], [0, 1, -1, 0]]  # theta_0 >= 3 and theta_0 == theta_1
    res, summary = sm.sweep(cells, g["nvar"], g["nparm"], 0, [0, 0], [9, 9], ctx)
    free, _ = sm.sweep(cells, g["nvar"], g["nparm"], 0, [0, 0], [9, 9])
    for k, (p, r, f) in enumerate(zip(g["points"], res, free)):
        if p[0] >= 3 and p[0] == p[1]:
            assert r == f
        else:
            assert r == (sm.ST_OUTSIDE, -1, [(0, 0)] * g["nvar"], [])
    assert summary["counts"]["outside"] == 93 and summary["first"]["outside"] == 0
    assert sum(summary["counts"].values()) == 100
    assert sum(summary["leaf_count"]) == summary["counts"]["solution"] + summary["counts"]["nil"] == 7
    # an empty tape: every inside point NIL with leaf -1, no leaf counted
    res, summary = sm.sweep([], 2, 2, 0, [0, 0], [9, 9], ctx)
    assert summary["counts"] == {"solution": 0, "nil": 7, "range": 0, "outside": 93} and summary["leaf_count"] == []
    assert all(r[1] == -1 for r in res)


@pytest.mark.parametrize("case", range(len(sm.edge_rows())))
def test_context_rows_at_the_edges(case):
    rows, point, want = sm.edge_rows()[case]
    assert sm.inside(point, rows) is want
    # beyond 128 bits with the right sign / exactly zero through cancellation, as claimed
    v = sum(a * t for a, t in zip(rows[0][1:-1], point)) + rows[0][-1]
    if case == 0:
        assert v > (1 << 128)
    if case in (3, 5):
        assert v == 0 and abs(rows[0][1] * point[0]) > MAX64


def test_plan_arithmetic():
    info = {"leaves": 7, "ifs": 6, "news": 0, "words": 40, "slots": 3, "depth": 4, "staged": 1}
    p = sm.plan(info, 64, 2, [0, 0], [9, 9])
    assert p == {"n_points": 100, "summary_words": 22, "binned": 1}
    assert sm.plan(info, 64, 0, [], [])["n_points"] == 1
    assert sm.plan(info, 64, 2, [0, 0], [(1 << 19) - 1, (1 << 19) - 2])["n_points"] == (1 << 38) - (1 << 19)
    for lo, hi, code in (([0, 0], [(1 << 19) - 1, (1 << 19) - 1], tm.E_TOOLARGE), ([MIN64], [MAX64], tm.E_TOOLARGE),
                         ([1, 0], [0, 5], tm.E_INVALID)):
        with pytest.raises(tm.TapeError) as e:
            sm.plan(info, 64, len(lo), lo, hi)
        assert e.value.code == code
    # 1 KB of slots and no staged program: 16 (L + 4) <= 64512 up to L = 4028
    big = dict(info, slots=2, staged=0, words=1 << 20)
    assert sm.binned(dict(big, leaves=4028), 64) == 1 and sm.binned(dict(big, leaves=4029), 64) == 0
    assert sm.binned(dict(big, leaves=3964), 128) == 1 and sm.binned(dict(big, leaves=3965), 128) == 0
