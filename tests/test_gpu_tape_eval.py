"""-m gpu: engine.Tape -- a solution tape evaluated at many parameter points (pipamd_tape_compile / pipamd_tape_eval, the
kernel of csrc/pip_tape.hip), both cell widths.

Authorities: the reference's printed answers for every instance of the family p5 on a grid
(tests/golden/tape_eval/p5_grid.json); the pivot kernels, solving the same instances through Batch(instances=True);
tests/tape_model.py (held to the reference by tests/test_tape_model.py) on hand-made tapes at the edges of the arithmetic
and of the kernel's layout.  No point is left out of any comparison."""
import functools
import itertools

import numpy as np
import pytest

import tape_cases as tc
import tape_model as tm
from tape_cases import MAX64, MIN64

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]


@functools.lru_cache(maxsize=None)
def _engine():
    from piplib_amd import engine as eng
    return eng.Engine(0)


def _ints(t, bits):
    from piplib_amd import engine as eng
    a = t.cpu().numpy()
    return (eng.wide_to_int(a) if bits == 128 else a.astype(object)).tolist()


def _results(out, bits, ndual):
    """a Tape.eval() tuple as tape_model.evaluate() gives its results: [(status, leaf, [(n, d)], [(n, d)])]"""
    import torch
    torch.cuda.synchronize()
    st, leaf = out[0].cpu().tolist(), out[1].cpu().tolist()
    xn, xd = _ints(out[2], bits), _ints(out[3], bits)
    dn, dd = (_ints(out[4], bits), _ints(out[5], bits)) if ndual else ([[]] * len(st), [[]] * len(st))
    return [(st[k], leaf[k], list(zip(xn[k], xd[k])), list(zip(dn[k], dd[k]))) for k in range(len(st))]


def device_eval(cells, nvar, nparm, ndual, points, bits=64):
    from piplib_amd import engine as eng
    t = eng.Tape(_engine(), cells, nvar, nparm, ndual, bits)
    pts = np.array(points, dtype=np.int64).reshape(len(points), nparm)
    got = _results(t.eval(pts if nparm else len(points)), bits, ndual)
    t.close()
    return got


def hold_to_model(cells, nvar, nparm, ndual, points, bits=64):
    got = device_eval(cells, nvar, nparm, ndual, points, bits)
    want = tm.evaluate_cells(cells, nvar, nparm, ndual, points, bits)
    assert len(got) == len(want) == len(points)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, points[k], g, w)
    return want


# ---------------------------------------------------------------- golden: solve once, evaluate on the grid
def _solve_p5(nq, bits, dual=False):
    """the tape of the parametric problem p5 from the engine: (cells, ndual)"""
    from piplib_amd import engine as eng
    g = tc.golden()
    tab = tc.parametric_tableau(g["matrix"], g["nvar"], g["nparm"], g["eq_rows"])
    ctx = np.zeros((0, g["nparm"] + 1), np.int64)
    if dual:
        cells, _ = eng.traiter(_engine(), g["nvar"], g["nparm"], tab.shape[0], 0, -1, eng.T_DUAL, tab, ctx, bits=bits)
        return cells, tab.shape[0]
    cells, _ = eng.solve_tableau_cells(_engine(), g["nvar"], g["nparm"], tab.shape[0], 0, -1, nq, tab, ctx, bits=bits)
    return cells, 0


@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("name,nq", [("int", 1), ("rat", 0)])
def test_golden_grid(name, nq, bits):
    """pipamd_solve_tableau / pipamd_solve_tableau128 once, the tape at the fixture's points: status and reduced values
    are the reference's recorded answers, the leaf is the model's"""
    g = tc.golden()
    cells, _ = _solve_p5(nq, bits)
    got = device_eval(cells, g["nvar"], g["nparm"], 0, g["points"], bits)
    assert len(got) == len(g["points"]) >= 100
    assert tc.answers_of(got) == g["answers"][name]
    assert all(st == (tm.ST_SOLUTION if x is not None else tm.ST_NIL) for (st, _, _, _), x in zip(got, g["answers"][name]))
    want = tm.evaluate_cells(cells, g["nvar"], g["nparm"], 0, g["points"], bits)
    assert [r[1] for r in got] == [r[1] for r in want] and len(set(r[1] for r in got)) >= 6
    assert got == want


@pytest.mark.parametrize("bits", [64, 128])
def test_two_device_paths(bits):
    """300 random points of 0..20 x 0..20: the quast evaluated there against the instance there solved by the pivot
    kernels (Batch(instances=True), integer with tab_simplify): status, and sol_num / sol_den reduced by
    system_model.reduce_pair, bit for bit, every point"""
    import torch
    import system_model as sy
    from piplib_amd import engine as eng
    g = tc.golden()
    nvar = g["nvar"]
    points = np.random.default_rng(20 + bits).integers(0, 21, (300, g["nparm"]))
    cells, _ = _solve_p5(1, bits)
    got = device_eval(cells, nvar, g["nparm"], 0, points.tolist(), bits)
    b = eng.Batch(_engine(), (np.array(g["matrix"], dtype=np.int64), points), nvar, 0, tflags=eng.T_INT, entier_bits=bits,
                  instances=True, eq_rows=g["eq_rows"], simplify=1)
    b.load()
    b.solve()
    b.fetch()
    torch.cuda.synchronize()
    st = b.status.cpu().tolist()
    num, den = _ints(b.sol_num, bits), _ints(b.sol_den, bits)
    solved = 0
    for k in range(len(points)):
        assert st[k] in (eng.ST_SOLUTION, eng.ST_NIL), (k, st[k])
        assert got[k][0] == st[k], (k, points[k], got[k][0], st[k])
        want = [sy.reduce_pair(num[k][i][0], den[k][i]) if st[k] == eng.ST_SOLUTION else (0, 0) for i in range(nvar)]
        assert got[k][2] == want, (k, points[k], got[k][2], want)
        solved += st[k] == eng.ST_SOLUTION
    assert 100 <= solved <= 290  # both kinds of points in numbers


# ---------------------------------------------------------------- edges of the arithmetic, against the model
def test_edges_floor_and_zero_condition():
    t = tc.new(1, [1, 0], 2, tc.iff([0, 1, 2], tc.leaf([([0, 1, 0], 1)]), tc.nil()))
    pts = [[-1], [-4], [-2], [-3], [3], [0], [-5], [-6]]
    want = hold_to_model(t, 1, 1, 0, pts)
    assert [w[2][0] for w in want[:2]] == [(-1, 1), (-2, 1)]      # (-1) / 2 -> -1 and (-4) / 2 -> -2: a true floor
    assert [w[0] for w in want] == [1, 1, 1, 1, 1, 1, 2, 2]       # floor + 2 == 0 at -4 and -3: the first item
    assert hold_to_model(t, 1, 1, 0, pts, 128) == want


@pytest.mark.parametrize("bits", [64, 128])
def test_edges_exact_sums_and_the_range_of_int64(bits):
    # products that each leave int64 while the sum fits, as the instances fixture's "cancel" rows
    t = tc.leaf([([1 << 62, -(1 << 62), 1, 5], 1)])
    pts = [[4, 4, 9], [MAX64, MAX64, MAX64], [MIN64, MIN64 + 1, 0], [2, 0, -6], [2, 0, -5], [-2, 0, -5], [-2, 0, -6], [0, 0, 0]]
    want = hold_to_model(t, 1, 3, 0, pts, bits)
    assert want[0][2][0] == (14, 1)
    if bits == 64:
        assert [w[0] for w in want[3:7]] == [1, 7, 1, 7]  # 2^63 - 1 and -2^63 are answers, 2^63 and -2^63 - 1 are not
        assert want[3][2][0] == (MAX64, 1) and want[5][2][0] == (MIN64, 1)
    hold_to_model(tc.leaf([([MIN64, MIN64, MAX64, 0], 3)]), 1, 3, 0, pts + [[1, -1, 3], [3, 0, 3], [MIN64, MIN64, MIN64]], bits)
    # a numerator that fits only after the division by the gcd; N == 0
    # (the unknown that leaves the range is the second: the first one's values, already written, are taken back)
    t = tc.leaf([([6, -18], 4), ([1 << 62, 0], 4), ([0, 0], 7)])
    want = hold_to_model(t, 3, 1, 0, [[4], [7], [9], [3], [0], [-4], [-8], [-9]], bits)
    assert want[0][2] == [(3, 2), (1 << 62, 1), (0, 1)] and want[3][2][0] == (0, 1)
    assert [w[0] for w in want] == ([1, 1, 7, 1, 1, 1, 1, 7] if bits == 64 else [1] * 8)
    # a new parameter whose value leaves int64
    t = tc.new(1, [2, 1], 1, tc.leaf([([0, 1, 0], 2)]))
    want = hold_to_model(t, 1, 1, 0, [[1 << 62], [(1 << 62) - 1], [-(1 << 62)], [-(1 << 62) - 1], [5]], bits)
    assert [w[0] for w in want] == ([7, 1, 1, 7, 1] if bits == 64 else [1] * 5)


def test_edges_128_bits_checked_in_cell_order():
    t = tc.leaf([([1 << 100, 0], 1)])
    want = hold_to_model(t, 1, 1, 0, [[1 << 26], [1 << 27], [-(1 << 27)], [-(1 << 27) - 1]], 128)
    assert [w[0] for w in want] == [1, 7, 1, 7]  # 2^126, 2^127, -2^127, -2^127 - 2^100
    t = tc.iff([1 << 64, 1 << 64, -(1 << 64), 0], tc.leaf([([1 << 64, 1 << 64, -(1 << 64), 0], 1)]), tc.nil())
    pts = [[1 << 62, 1 << 62, 1 << 62], [1 << 62, -(1 << 62), 1 << 62], [1 << 62, 1, -(1 << 62)], [1 << 61, 1 << 61, -5]]
    want = hold_to_model(t, 1, 3, 0, pts, 128)
    assert [w[0] for w in want] == [7, 2, 7, 1]  # 2^126 + 2^126 leaves 128 bits before the third term brings it back
    # the widest values: coefficients and new parameters of more than 64 bits, a gcd of more than 64 bits
    t = tc.new(1, [tc.MAX128 // 3, 7], 5, tc.leaf([([0, 6, 0], 1 << 70), ([3, 5, -1], (1 << 90) + 1)]))
    hold_to_model(t, 2, 1, 0, [[3], [-3], [2], [0], [1], [-1], [4]], 128)


@pytest.mark.parametrize("bits", [64, 128])
def test_range_points_among_good_ones(bits):
    """the first, a middle and the last point of 257 leave the range; the others are not disturbed"""
    if bits == 64:  # theta = 2: 2^63 as a new parameter
        t, big = tc.new(1, [1 << 62, 0], 1, tc.leaf([([0, 1, 3], 2), ([1, 0, 0], 1)])), 2
    else:           # theta = 4: the new parameter is 2^64, and 2^63 * 2^64 leaves 128 bits in the second unknown
        t, big = tc.new(1, [1 << 62, 0], 1, tc.leaf([([1, 0, 0], 1), ([0, 1 << 63, 3], 2)])), 4
    pts = [[k % 2 - (k % 3 == 0)] for k in range(257)]
    for k in (0, 128, 256):
        pts[k] = [big]
    want = hold_to_model(t, 2, 1, 0, pts, bits)
    assert [k for k, w in enumerate(want) if w[0] == tm.ST_RANGE] == [0, 128, 256]
    assert all(w[0] == tm.ST_SOLUTION for k, w in enumerate(want) if k not in (0, 128, 256))


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("bits", [64, 128])
def test_point_counts(bits):
    g = tc.golden()
    cells = tc.cells_from_text(g["tapes"]["int"])
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 65, 257):
        hold_to_model(cells, g["nvar"], g["nparm"], 0, rng.integers(0, 12, (n, 2)).tolist(), bits)
    from piplib_amd import engine as eng
    t = eng.Tape(_engine(), cells, g["nvar"], g["nparm"], 0, bits)
    out = t.eval(np.zeros((0, 2), np.int64))
    assert [tuple(o.shape)[:1] for o in out] == [(0,)] * 4
    t.close()


@pytest.mark.parametrize("bits", [64, 128])
def test_no_parameters_nil_and_empty(bits):
    t = tc.iff([-3], tc.nil(), tc.leaf([([7], 2), ([0], 5)]))
    want = hold_to_model(t, 2, 0, 0, [[]] * 70, bits)
    assert want[0] == (tm.ST_SOLUTION, 1, [(7, 2), (0, 1)], [])
    want = hold_to_model(tc.nil(), 3, 2, 0, [[1, 2]] * 65, bits)
    assert want[64] == (tm.ST_NIL, 0, [(0, 0)] * 3, [])
    want = hold_to_model([], 3, 2, 2, [[1, 2]] * 65, bits)
    assert want[64] == (tm.ST_NIL, -1, [(0, 0)] * 3, [(0, 0)] * 2)


@pytest.mark.parametrize("bits", [64, 128])
def test_slot_limit_at_its_edge(bits):
    """30 new parameters behind one: 32 slots.  Each is the one before plus 1 and the leaf hands out the last, so a new
    parameter written to, or read from, a wrong slot shows"""
    from piplib_amd import engine as eng
    cells = tc.new_chain(1, 30)
    assert eng.tape_check(cells, 2, 1, 0, bits)["slots"] == 32
    want = hold_to_model(cells, 2, 1, 0, [[k * k - 40] for k in range(130)], bits)
    assert want[3][2] == [(9 - 40 + 30, 1), (9 - 40, 1)]
    with pytest.raises(eng.TapeError):
        eng.Tape(_engine(), tc.new_chain(1, 31), 2, 1, 0, bits)


def test_program_read_from_global_memory():
    """a chain of 2016 conditions over one parameter is a program of 8068 words: with the 1 KB of its one slot row it no
    longer fits the 64 KB of LDS (2015 conditions, 8064 words, just do), and info says the kernel reads it from global
    memory.  Point t ends in the NIL of condition t, so every jump target is exercised from some lane."""
    from piplib_amd import engine as eng
    for k, staged in ((2015, 1), (2016, 0)):
        cells = tc.if_chain(k)
        t = eng.Tape(_engine(), cells, 1, 1, 0, 64)
        assert t.info["staged"] == staged and t.info["words"] == 4 * k + 4
        t.close()
        pts = [[(37 * i) % (k + 40)] for i in range(200)] + [[k - 1], [k], [0], [-1]]
        want = hold_to_model(cells, 1, 1, 0, pts, 64)
        assert want[-4][:2] == (tm.ST_NIL, k - 1) and want[-3][:3] == (tm.ST_SOLUTION, k, [(k, 1)])
    # 128 bits: 6 k + 7 words and 2 KB of slots; 1400 conditions are 8407 words, read from global memory too
    assert eng.tape_check(tc.if_chain(1400), 1, 1, 0, 128)["staged"] == 0
    hold_to_model(tc.if_chain(1400), 1, 1, 0, [[(53 * i) % 1440] for i in range(130)], 128)


@pytest.mark.parametrize("bits", [64, 128])
def test_dual_leaves(bits):
    """the rational tape of p5 with PIPAMD_T_DUAL, from pipamd_traiter: its dual lists are held to the model"""
    g = tc.golden()
    cells, ndual = _solve_p5(0, bits, dual=True)
    assert ndual == 9 and tc.ndual_of(cells, g["nvar"]) == ndual
    want = hold_to_model(cells, g["nvar"], g["nparm"], ndual, g["points"], bits)
    assert tc.answers_of(want) == g["answers"]["rat"]
    assert sum(any(n != 0 for n, _ in w[3]) for w in want) >= 20


def test_null_outputs_in_every_combination():
    import torch
    from piplib_amd import engine as eng
    cells = tc.iff([1, -2], tc.leaf([([3, 1], 2)], duals=[(2, 4)]), tc.nil())
    t = eng.Tape(_engine(), cells, 1, 1, 1, 64)
    pts = torch.arange(0, 70, dtype=torch.int64, device="cuda").reshape(70, 1).contiguous()
    full = t.eval(pts)
    torch.cuda.synchronize()
    names = eng.Tape.OUTPUTS
    for r in range(1, 7):
        for some in itertools.combinations(names, r):
            out = {k: torch.full_like(v, -77) for k, v in zip(names, full) if k in some}
            t.eval_into(pts, out)
            torch.cuda.synchronize()
            for k, v in zip(names, full):
                if k in some:
                    assert torch.equal(out[k], v), (some, k)
    t.close()


def test_reuse_on_two_streams():
    """one tape, two evaluations on two streams: identical results, and the device program is what it was"""
    import ctypes as C
    import torch
    from piplib_amd import engine as eng
    g = tc.golden()
    cells = tc.cells_from_text(g["tapes"]["int"])
    t = eng.Tape(_engine(), cells, g["nvar"], g["nparm"], 0, 64)
    fn = eng.lib().pipamd_debug_tape_program
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    words = C.c_int64()
    assert fn(t._h, None, 0, C.byref(words)) == 0 and words.value == t.info["words"] > 0
    before, after = (C.c_int64 * words.value)(), (C.c_int64 * words.value)()
    assert fn(t._h, before, words.value, C.byref(words)) == 0
    pts = torch.as_tensor(g["points"], dtype=torch.int64, device="cuda").repeat(40, 1).contiguous()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        a = t.eval(pts)
    with torch.cuda.stream(s2):
        b = t.eval(pts)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    want = tm.evaluate_cells(cells, g["nvar"], g["nparm"], 0, g["points"], 64)
    assert _results(a, 64, 0)[:len(want)] == want and _results(b, 64, 0)[-len(want):] == want
    assert fn(t._h, after, words.value, C.byref(words)) == 0
    assert list(before) == list(after) and any(before)
    t.close()
