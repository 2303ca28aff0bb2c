"""-m gpu: pip_solve's result edits in the tape evaluator (pipamd_tape_compile_pip, the negate and unbounded marks of
csrc/pip_tape.hip), both cell widths.

Authorities: the reference's printed answers per instance for the families of tests/golden/tape_edit (Maximize,
Urs_unknowns, Urs_parms, both, Rational+Maximize); the pivot kernels, solving the same instances through
Batch(instances=True, shift=+1) and pipamd_batch_results_shifted; tests/tape_edit_model.py (held to the reference by
tests/test_tape_edit_model.py) on hand-made tapes at the edges.  No point is left out of any comparison."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import tape_cases as tc
import tape_edit_model as te
import tape_model as tm
from tape_cases import MAX64, MAX128, MIN64, MIN128
from test_gpu_tape_eval import _engine, _ints, _results

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tape_edit")
FAMILIES = ("maximize", "urs_unknowns", "urs_parms", "urs_parms_maximize", "rational_maximize")
MAXF = dict(sol_flags=7)  # SOL_MAX | SOL_REMOVE: a new big parameter under Maximize


def family(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def solved(name, bits):
    """pip_solve_many once per family and width: (cells, info)"""
    from piplib_amd import engine as eng
    g = family(name)
    prob = eng.PipInput(np.array(g["inequnk"], dtype=np.int64), np.array(g["ineqpar"], dtype=np.int64).reshape(0, g["nparm"] + 2),
                        g["bg"], g["options"])
    cells, rc, _, _, info = eng.pip_solve_many(_engine(), [prob], bits=bits)[0]
    assert rc == 0 and not info["is_void"]
    return cells, info


def device_eval(cells, nvar, nparm, points, edit, bits=64, ndual=0):
    from piplib_amd import engine as eng
    t = eng.Tape(_engine(), cells, nvar, nparm, ndual, bits, edit=edit)
    assert t.point_cols == te.point_cols(nparm, edit) and t.info == te.check(cells, nvar, nparm, ndual, edit, bits)
    pts = np.array(points, dtype=np.int64).reshape(len(points), t.point_cols)
    got = _results(t.eval(pts if t.point_cols else len(points)), bits, ndual)
    t.close()
    return got


def hold_to_model(cells, nvar, nparm, points, edit, bits=64, ndual=0):
    got = device_eval(cells, nvar, nparm, points, edit, bits, ndual)
    want = te.evaluate_cells(cells, nvar, nparm, ndual, points, edit, bits)
    assert len(got) == len(want) == len(points)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, points[k], g, w)
    return want


# ---------------------------------------------------------------- golden: pip_solve_many once, the edited tape on the grid
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("name", FAMILIES)
def test_golden_families(name, bits):
    """status and values are the reference's recorded answers at every point (of an unbounded unknown the /0 mark; its
    numerator is held to the model), and the whole result is the model's"""
    g = family(name)
    cells, info = solved(name, bits)
    assert info["nvar"] == g["nvar"] and te.point_cols(info["nparm"], info) == g["nparm"]
    got = device_eval(cells, info["nvar"], info["nparm"], g["points"], info, bits)
    assert len(got) == len(g["answers"]) >= 100
    for k, (r, a) in enumerate(zip(got, g["answers"])):
        assert r[0] == (tm.ST_SOLUTION if a is not None else tm.ST_NIL), (k, r)
        assert te.same_answer(te.answer_of(r), a), (k, g["points"][k], r, a)
    assert sum(r[0] == tm.ST_SOLUTION and any(d == 0 for _, d in r[2]) for r in got) == g["census"]["unbounded"]
    want = te.evaluate_cells(cells, info["nvar"], info["nparm"], 0, g["points"], info, bits)
    assert got == want and len(set(r[1] for r in got)) >= 4


@pytest.mark.parametrize("bits", [64, 128])
def test_two_device_paths(bits):
    """300 random points of 0..11 x 0..11 under Maximize: the edited quast evaluated there against the instance there
    solved by the pivot kernels (Batch(instances=True, shift=+1), integer with tab_simplify) and decoded by
    pipamd_batch_results_shifted: status, numerators and denominators bit for bit, unbounded unknowns included"""
    import torch
    from piplib_amd import engine as eng
    g = family("maximize")
    nvar = g["nvar"]
    points = np.random.default_rng(40 + bits).integers(0, 12, (300, g["nparm"]))
    cells, info = solved("maximize", bits)
    got = device_eval(cells, info["nvar"], info["nparm"], points.tolist(), info, bits)
    matrix = np.array(g["inequnk"], dtype=np.int64)[:, 1:]
    b = eng.Batch(_engine(), (matrix, points), nvar, 0, tflags=eng.T_INT, entier_bits=bits, shift=eng.SHIFT_MAX, instances=True,
                  eq_rows=(), simplify=1)
    b.load()
    b.solve()
    b.fetch_shifted()
    torch.cuda.synchronize()
    st = b.status.cpu().tolist()
    num, den = _ints(b.x_num, bits), _ints(b.x_den, bits)
    n_solved = unbounded = 0
    for k in range(len(points)):
        assert st[k] in (eng.ST_SOLUTION, eng.ST_NIL), (k, st[k])
        assert got[k][0] == st[k], (k, points[k], got[k][0], st[k])
        assert got[k][2] == list(zip(num[k], den[k])), (k, points[k], got[k][2], num[k], den[k])
        n_solved += st[k] == eng.ST_SOLUTION
        unbounded += st[k] == eng.ST_SOLUTION and 0 in den[k]
    assert 100 <= n_solved <= 220 and unbounded >= 50  # both kinds of points in numbers


# ---------------------------------------------------------------- hand-made edges, against the model
@pytest.mark.parametrize("bits", [64, 128])
def test_shift_to_exactly_zero_and_one(bits):
    """over D = 4: a big coefficient of 4 shifts to 0 (bounded), 5 to 1 and 3 to -1 (unbounded), 0 to -4; without
    SOL_REMOVE the shifted coefficient stays in the form and meets the point's own column"""
    cells = tc.leaf([([4, 6, 2], 4), ([5, 0, 8], 4), ([3, 1, 0], 4)])
    pts = [[0, 0], [1, 2], [-3, 5], [7, -2], [2, -1]]
    want = hold_to_model(cells, 3, 2, pts, dict(sol_bg=0, sol_flags=1), bits)
    assert [d for _, d in want[1][2]] == [2, 0, 0] and want[1][2][1][0] == 9   # (1 * 1 + 8) / gcd(9, 4), over 0
    assert all(w[2][0][1] != 0 and w[2][1][1] == 0 and w[2][2][1] == 0 for w in want)
    for flags in (5, 7, 3):
        hold_to_model(cells, 3, 2, [p[1:] for p in pts] if flags & 4 else pts, dict(sol_bg=0, sol_flags=flags), bits)
    unb0 = hold_to_model(tc.leaf([([0, 0, 0], 4), ([4, 0, 0], 4)]), 2, 2, [[3]], dict(sol_bg=0, sol_flags=5), bits)
    assert unb0[0][2] == [(0, 0), (0, 1)]  # N == 0: (0, 0) where unbounded, (0, 1) where not


def test_negate_at_the_ends_of_int64():
    cells = tc.leaf([([1, 0], 1), ([1, 0], 2)])
    pts = [[MIN64], [MIN64 + 1], [MAX64], [0], [-1], [2]]
    want = hold_to_model(cells, 2, 1, pts, dict(sol_bg=-1, sol_flags=2))
    assert [w[0] for w in want] == [tm.ST_RANGE, 1, 1, 1, 1, 1]      # -INT64_MIN is no int64, -INT64_MAX is
    assert want[1][2][0] == (MAX64, 1) and want[2][2][0] == (MIN64 + 1, 1) and want[3][2] == [(0, 1), (0, 1)]
    # the negation comes before the reduction: INT64_MIN / 2 negated is 2^62
    half = hold_to_model(tc.leaf([([1, 0], 2)]), 1, 1, [[MIN64], [MAX64]], dict(sol_bg=-1, sol_flags=2))
    assert half[0][2] == [(1 << 62, 1)] and half[1][2] == [(-MAX64, 2)]
    # a value beyond int64 that the reduction brings back
    wide = hold_to_model(tc.leaf([([4, 0], 4)]), 1, 1, [[MIN64]], dict(sol_bg=-1, sol_flags=2))
    assert wide[0][0] == tm.ST_RANGE
    hold_to_model(tc.leaf([([4, 0], 8)]), 1, 1, [[MIN64], [MAX64]], dict(sol_bg=-1, sol_flags=2))
    # INT64_MIN as a coefficient: nothing is negated at compile time
    hold_to_model(tc.leaf([([MIN64, MIN64], 1), ([MIN64, 0], 1 << 62)]), 2, 1, [[0], [1], [-1], [MAX64]], dict(sol_bg=-1, sol_flags=2))


def test_negate_at_the_ends_of_128_bits():
    c = -(1 << 64)
    # theta = 2^63 - 1: the forms are -2^127, -2^127 + 1, -2^127 over 2 (the negation comes first), 2^127 - 1
    for form, st in ((([c, c], 1), tm.ST_RANGE), (([c, c + 1], 1), 1), (([c, c], 2), tm.ST_RANGE), (([-c, -c - 1], 1), 1)):
        want = hold_to_model(tc.leaf([form]), 1, 1, [[MAX64], [0], [1]], dict(sol_bg=-1, sol_flags=2), 128)
        assert want[0][0] == st, form
    ok = hold_to_model(tc.leaf([([c, c + 1], 1)]), 1, 1, [[MAX64]], dict(sol_bg=-1, sol_flags=2), 128)
    assert ok[0][2] == [(MAX128, 1)]
    hold_to_model(tc.leaf([([MIN128, MIN128], 1), ([MIN128, 0], 1 << 100)]), 2, 1, [[0], [1], [-1]], dict(sol_bg=-1, sol_flags=2), 128)
    # without the negation -2^127 is an answer
    plain = hold_to_model(tc.leaf([([c, c], 1)]), 1, 1, [[MAX64]], None, 128)
    assert plain[0][2] == [(MIN128, 1)]


@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("bg", [0, 1, 2])
def test_big_parameter_first_middle_last(bg, bits):
    """three raw parameters, the big one at `bg`: conditions, new parameters and unknowns read the two that are kept"""
    rng = np.random.default_rng(7 + bg)
    def row(n, big):
        v = [int(x) for x in rng.integers(-5, 6, n)]
        v[bg] = big
        return v
    cells = tc.new(3, row(4, 0), 3, tc.iff(row(5, 0), tc.leaf([(row(5, 2), 2), (row(5, 5), 2)]),
                                           tc.iff(row(5, 0), tc.nil(), tc.leaf([(row(5, 1), 1), (row(5, 1), 1)]))))
    pts = rng.integers(-9, 10, (40, 2)).tolist()
    for flags in (7, 5):
        want = hold_to_model(cells, 2, 3, pts, dict(sol_bg=bg, sol_flags=flags), bits)
        assert len(set(w[1] for w in want)) == 3
    hold_to_model(cells, 2, 3, rng.integers(-9, 10, (40, 3)).tolist(), dict(sol_bg=bg, sol_flags=3), bits)  # kept: a column


@pytest.mark.parametrize("bits", [64, 128])
def test_urs_copies_dropped_around_new_parameters(bits):
    """parameters p0 p1, their negated copies at columns 2 and 3, a new parameter in front of an IF and one behind it on
    either side: NEW writes slot 2, then 3, of the kept numbering"""
    def urs(a, b, rest):
        return [a, b, -a, -b] + rest
    then = tc.new(5, urs(1, 1, [2, 0]), 2, tc.leaf([(urs(1, 0, [1, 1, 0]), 1), (urs(0, 3, [0, -1, 4]), 3)]))
    other = tc.new(5, urs(0, -1, [1, 3]), 5, tc.leaf([(urs(2, 2, [0, 7, 1]), 4), (urs(0, 0, [1, 0, 0]), 1)]))
    cells = tc.new(4, urs(1, -2, [1]), 3, tc.iff(urs(1, 1, [-2, 1]), then, other))
    pts = [[a, b] for a in range(-6, 7, 3) for b in range(-7, 8, 2)]
    edit = dict(sol_bg=-4, urs_parms=2, sol_flags=0)
    want = hold_to_model(cells, 2, 4, pts, edit, bits)
    assert {w[1] for w in want} == {0, 1} and te.check(cells, 2, 4, 0, edit, bits)["slots"] == 5
    # with a big parameter in front of the copies as well: p0 BIG p1 | -p0 -p1 (first_urs 3)
    def urs_bg(a, b, big, rest):
        return [a, big, b, -a, -b] + rest
    cells = tc.new(5, urs_bg(1, -2, 0, [1]), 3,
                   tc.iff(urs_bg(1, 1, 0, [-2, 1]), tc.leaf([(urs_bg(1, 0, 2, [1, 1]), 2), (urs_bg(0, 3, 3, [0, -1]), 2)]), tc.nil()))
    for flags in (7, 5, 1):
        edit = dict(sol_bg=1, urs_parms=2, sol_flags=flags)
        hold_to_model(cells, 2, 5, [p + [9] for p in pts] if not flags & 4 else pts, edit, bits)


def test_slot_limit_counts_kept_columns_on_the_device():
    from piplib_amd import engine as eng
    cells = tc.leaf([(list(range(1, 35)), 1)])  # 33 raw parameters and the constant
    pts = np.random.default_rng(3).integers(-50, 51, (5, 31)).tolist()
    for bits in (64, 128):
        hold_to_model(cells, 1, 33, pts, dict(sol_bg=0, urs_parms=1, sol_flags=7), bits)   # 31 kept: 32 slots
        with pytest.raises(eng.TapeError) as e:
            eng.Tape(_engine(), cells, 1, 33, 0, bits, edit=dict(sol_bg=0, sol_flags=7))   # 32 kept: 33 slots
        assert e.value.code == tm.E_TOOLARGE
        with pytest.raises(eng.TapeError) as e:
            eng.Tape(_engine(), tc.leaf([([MIN128 if bits == 128 else MIN64, 0], 1)]), 1, 1, 0, bits, edit=dict(sol_bg=0, sol_flags=1))
        assert e.value.code == tm.E_TOOLARGE


def _program(t):
    from piplib_amd import engine as eng
    fn = eng.lib().pipamd_debug_tape_program
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    words = C.c_int64()
    assert fn(t._h, None, 0, C.byref(words)) == 0 and words.value == t.info["words"]
    buf = (C.c_int64 * max(1, words.value))()
    assert fn(t._h, buf, words.value, C.byref(words)) == 0
    return list(buf)[:words.value]


@pytest.mark.parametrize("bits", [64, 128])
def test_a_tape_without_an_edit_compiles_to_the_same_words(bits):
    from piplib_amd import engine as eng
    g = tc.golden()
    for cells, nvar, nparm, ndual in ((tc.cells_from_text(g["tapes"]["int"]), g["nvar"], g["nparm"], 0),
                                      (tc.leaf([([2, 3, 1], 4)], [(1, 2), (-6, 4)]), 1, 2, 2)):
        a = eng.Tape(_engine(), cells, nvar, nparm, ndual, bits)
        b = eng.Tape(_engine(), cells, nvar, nparm, ndual, bits, edit=dict(sol_bg=0, urs_parms=0, sol_flags=0))
        c = eng.Tape(_engine(), cells, nvar, nparm, ndual, bits, edit=dict(sol_bg=-3, urs_parms=0, sol_flags=8))
        assert _program(a) == _program(b) == _program(c) and a.info == b.info == c.info and len(_program(a)) > 0
        assert a.point_cols == b.point_cols == nparm
        # and the marks are where csrc/pip_tape.h says: bit 24 of a LEAF's header, a negative D_i
        d = eng.Tape(_engine(), tc.leaf([([2, 3, 1], 4)]), 1, 2, 0, bits, edit=dict(sol_bg=0, sol_flags=3))
        ew = bits // 64
        assert _program(d)[0] == 3 | (2 << 8) | (1 << 24) and _program(d)[1] == -4 and _program(d)[1 + ew] == -2
        for t in (a, b, c, d):
            t.close()


def test_dual_lists_stay_as_they_are():
    """SOL_DUAL is accepted and ignored: the dual list behind an edited solution list is handed out as it stands"""
    cells = tc.leaf([([3, 1, 2], 2)], [(1, 2), (-6, 4), (0, 5)])
    want = hold_to_model(cells, 1, 2, [[4], [-1]], dict(sol_bg=0, sol_flags=7 | 8), 64, ndual=3)
    assert want[0][3] == [(1, 2), (-3, 2), (0, 1)]
    hold_to_model(cells, 1, 2, [[4], [-1]], dict(sol_bg=0, sol_flags=7 | 8), 128, ndual=3)
