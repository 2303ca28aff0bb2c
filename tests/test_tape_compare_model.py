"""tests/tape_compare_model.py held to the reference: on the golden tapes of the family p5 (the integer quast against the
rational one over [0,9]^2) its classes are a direct comparison of the reference's recorded answers; a tape against
itself, and hand-made tapes of different shape that mean the same, are SAME everywhere.  Host only, Python ints only."""
import pytest

import tape_cases as tc
import tape_compare_model as cm
import tape_model as tm
import tape_sweep_model as sm
from tape_cases import MAX64


def golden_pair(bits_a=64, bits_b=64):
    g = tc.golden()
    return (cm.tape(tc.cells_from_text(g["tapes"]["int"]), g["nvar"], g["nparm"], bits=bits_a),
            cm.tape(tc.cells_from_text(g["tapes"]["rat"]), g["nvar"], g["nparm"], bits=bits_b))


def recorded_classes(g):
    """class and where per point from the recorded answers alone"""
    out = []
    for x, y in zip(g["answers"]["int"], g["answers"]["rat"]):
        if (x is None) != (y is None):
            out.append((cm.STATUS, -1))
        elif x is None or x == y:
            out.append((cm.SAME, -1))
        else:
            out.append((cm.VALUE, next(i for i, (p, q) in enumerate(zip(x, y)) if p != q)))
    return out


@pytest.mark.parametrize("bits_a,bits_b", [(64, 64), (64, 128), (128, 64), (128, 128)])
def test_integer_against_rational_is_the_recorded_answers(bits_a, bits_b):
    g = tc.golden()
    a, b = golden_pair(bits_a, bits_b)
    res, summary = cm.compare_sweep(a, b, [0, 0], [9, 9])
    want = recorded_classes(g)
    assert [(r[0], r[1]) for r in res] == want and len(res) == 100
    counts = [sum(c == k for c, _ in want) for k in range(5)]
    assert counts[cm.SAME] == sum(x == y for x, y in zip(g["answers"]["int"], g["answers"]["rat"]))
    assert summary["counts"] == dict(zip(cm.CLASSES, counts)) and sum(counts) == 100
    assert counts[cm.SAME] > 0 and counts[cm.VALUE] > 0 and counts[cm.STATUS] > 0 and counts[cm.RANGE] == 0
    for k, name in enumerate(cm.CLASSES):
        at = [i for i, (c, _) in enumerate(want) if c == k]
        assert summary["first"][name] == (at[0] if at else -1)
    assert cm.words(summary)[:5] == counts and len(cm.words(summary)) == cm.WORDS
    # the statuses are each tape's own; the list form at the materialised box is the sweep form
    for r, x, y in zip(res, g["answers"]["int"], g["answers"]["rat"]):
        assert r[2] == (tm.ST_NIL if x is None else tm.ST_SOLUTION) and r[3] == (tm.ST_NIL if y is None else tm.ST_SOLUTION)
    assert cm.compare(a, b, g["points"]) == res
    # b against a: the same classes and indices
    back, _ = cm.compare_sweep(b, a, [0, 0], [9, 9])
    assert [(r[0], r[1], r[3], r[2]) for r in back] == res


@pytest.mark.parametrize("name", ["int", "rat"])
def test_a_tape_against_itself_is_same_everywhere(name):
    g = tc.golden()
    t = cm.tape(tc.cells_from_text(g["tapes"][name]), g["nvar"], g["nparm"])
    for wa, wb, a, b in cm.widths(t, t):
        res, summary = cm.compare_sweep(a, b, [-2, -2], [11, 11])
        assert summary["counts"]["same"] == len(res) == 196 and summary["first"]["same"] == 0, (wa, wb)
        assert all(r[1] == -1 and r[2] == r[3] for r in res)


@pytest.mark.parametrize("case", range(3))
def test_equivalent_tapes_of_other_shape_are_same(case):
    name, a, b, lo, hi = cm.equivalents()[case]
    points = sm.box_points(lo, hi)
    ra, rb = cm.evaluate(a, points), cm.evaluate(b, points)
    # the shapes differ: some point reaches another ordinal, and every leaf and the NIL are reached
    assert any(x[1] != y[1] for x, y in zip(ra, rb)) or case == 1, name
    assert {x[1] for x in ra} == {0, 1, 2} and {x[0] for x in ra} == {tm.ST_SOLUTION, tm.ST_NIL}
    for wa, wb, ta, tb in cm.widths(a, b):
        res, summary = cm.compare_sweep(ta, tb, lo, hi)
        assert summary["counts"]["same"] == len(points) and all(r[1] == -1 for r in res), (name, wa, wb)


def test_class_order_where_and_the_dual_flag():
    leaf = lambda forms, duals: tc.leaf(forms, duals)
    a = cm.tape(leaf([([1, 0], 1), ([2, 1], 2)], [(1, 2), (3, 1)]), 2, 1, ndual=2)
    b = cm.tape(leaf([([1, 0], 1), ([2, 1], 2)], [(2, 4), (3, 2)]), 2, 1, ndual=2)
    pts = [[0], [1], [-3]]
    assert cm.compare(a, b, pts) == [(cm.SAME, -1, tm.ST_SOLUTION, tm.ST_SOLUTION)] * 3     # duals not looked at
    assert cm.compare(a, b, pts, cm.DUAL) == [(cm.VALUE, 3, tm.ST_SOLUTION, tm.ST_SOLUTION)] * 3  # nvar + 1: (3,1) != (3,2)
    c = cm.tape(leaf([([1, 0], 1), ([2, 3], 2)], [(5, 1), (3, 1)]), 2, 1, ndual=2)
    assert [r[:2] for r in cm.compare(a, c, pts, cm.DUAL)] == [(cm.VALUE, 1)] * 3             # an unknown comes first
    # 0 / 5 is handed out (0, 1), as theta_0 is at 0; a NIL's zeros play no part: a status difference is STATUS
    d = cm.tape(tc.iff([1, 0], leaf([([0, 0], 5), ([2, 1], 2)], [(1, 2), (3, 1)]), tc.nil()), 2, 1, ndual=2)
    assert [r[:2] for r in cm.compare(a, d, pts, cm.DUAL)] == [(cm.SAME, -1), (cm.VALUE, 0), (cm.STATUS, -1)]
    # RANGE comes first, whatever the other tape has: 2^63 leaves int64 but not 128 bits
    e = cm.tape(tc.leaf([([1, 1], 1), ([2, 1], 2)]), 2, 1)
    res = cm.compare(e, dict(e, bits=128), [[MAX64], [5]])
    assert res == [(cm.RANGE, -1, tm.ST_RANGE, tm.ST_SOLUTION), (cm.SAME, -1, tm.ST_SOLUTION, tm.ST_SOLUTION)]
    assert cm.compare(a, e, pts)[0][0] == cm.VALUE   # ndual may differ where the dual lists are not compared
    one_unknown, two_parms = cm.tape(tc.leaf([([1, 0], 1)]), 1, 1), cm.tape(tc.leaf([([1, 0, 0], 1), ([2, 0, 1], 2)]), 2, 2)
    for bad in (lambda: cm.compare(a, one_unknown, pts), lambda: cm.compare(a, two_parms, pts),
                lambda: cm.compare(a, b, pts, 2), lambda: cm.compare(a, e, pts, cm.DUAL)):
        with pytest.raises(tm.TapeError) as err:
            bad()
        assert err.value.code == tm.E_INVALID


def test_context_rows_and_the_summary():
    a, b = golden_pair()
    ctx = [[1, 1, 0, -3], [0, 1, -1, 0]]  # theta_0 >= 3 and theta_0 == theta_1
    res, summary = cm.compare_sweep(a, b, [0, 0], [9, 9], ctx)
    free, _ = cm.compare_sweep(a, b, [0, 0], [9, 9])
    for p, r, f in zip(sm.box_points([0, 0], [9, 9]), res, free):
        assert r == (f if p[0] >= 3 and p[0] == p[1] else (cm.OUTSIDE, -1, sm.ST_OUTSIDE, sm.ST_OUTSIDE))
    assert summary["counts"]["outside"] == 93 and summary["first"]["outside"] == 0 and sum(summary["counts"].values()) == 100
    # no parameters: one point; an empty tape is NIL there
    one = cm.tape(tc.leaf([([7], 2)]), 1, 0)
    assert cm.compare_sweep(one, one, [], [])[0] == [(cm.SAME, -1, tm.ST_SOLUTION, tm.ST_SOLUTION)]
    assert cm.compare_sweep(one, cm.tape([], 1, 0), [], [])[0] == [(cm.STATUS, -1, tm.ST_SOLUTION, tm.ST_NIL)]
