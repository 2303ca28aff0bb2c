"""-m gpu: engine.Tape.compare / compare_sweep -- two solution tapes, of either cell width each, compared by value at the
points of a list or of a box (pipamd_tape_compare, pipamd_tape_compare_sweep, pip_tape_compare_kernel of
csrc/pip_tape.hip), in the four width pairs.

Authorities: tests/tape_compare_model.py (held to the reference's recorded answers by tests/test_tape_compare_model.py)
for class, `where`, both statuses and the summary; pipamd_tape_eval of either tape at the same points for the statuses;
the reference's recorded answers on the golden grid for the counts.  No point is left out of any comparison."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import tape_cases as tc
import tape_compare_model as cm
import tape_edit_model as te
import tape_model as tm
import tape_sweep_model as sm
from tape_cases import MAX64, MIN64
from test_gpu_tape_edit import family, solved
from test_gpu_tape_eval import _engine, _solve_p5

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

PAIRS = [(64, 64), (64, 128), (128, 64), (128, 128)]
OUTSIDE = (cm.OUTSIDE, -1, sm.ST_OUTSIDE, sm.ST_OUTSIDE)


def device_tapes(*tapes):
    from piplib_amd import engine as eng
    return [eng.Tape(_engine(), t["cells"], t["nvar"], t["nparm"], t.get("ndual", 0), t.get("bits", 64), edit=t.get("edit"))
            for t in tapes]


def got_of(out, summary):
    """the four arrays as the model's [(class, where, sa, sb)], and the summary as its dict"""
    import torch
    from piplib_amd import engine as eng
    torch.cuda.synchronize()
    cols = [out[k].cpu().tolist() for k in eng.Tape.CMP_OUTPUTS]
    return [tuple(r) for r in zip(*cols)], eng.compare_summary(summary)


def eval_status(t, points):
    n = len(points)
    pts = np.array(points, dtype=np.int64).reshape(n, t.point_cols) if t.point_cols else n
    st = t.eval_into(pts, t.outputs(n, ("status",)))["status"]
    return st.cpu().tolist()


def hold(a, b, lo, hi, ctx=(), dual=False):
    """the sweep form on the device against the model, every point; the statuses against pipamd_tape_eval of either
    tape; without a context the list form at the materialised box gives the same arrays and summary.
    -> (model results, model summary)"""
    import torch
    ta, tb = device_tapes(a, b)
    plan = ta.compare_plan(tb, lo, hi)
    assert plan == cm.plan(ta.info, ta.bits, tb.info, tb.bits, ta.point_cols, lo, hi)
    summary, out = ta.compare_sweep(tb, lo, hi, ctx=(ctx if len(ctx) else None), dual=dual)
    got, got_sum = got_of(out, summary)
    want, want_sum = cm.compare_sweep(a, b, lo, hi, ctx, cm.DUAL if dual else 0)
    assert len(got) == len(want) == plan["n_points"]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)
    assert got_sum == want_sum and sum(got_sum["counts"].values()) == plan["n_points"]
    points = sm.box_points(lo, hi)
    ea, eb = eval_status(ta, points), eval_status(tb, points)
    for k, p in enumerate(points):
        assert (got[k][2], got[k][3]) == ((ea[k], eb[k]) if sm.inside(p, ctx) else (sm.ST_OUTSIDE, sm.ST_OUTSIDE)), (k, p)
    if not len(ctx):
        pts = np.array(points, dtype=np.int64).reshape(len(points), ta.point_cols) if ta.point_cols else len(points)
        summary2, out2 = ta.compare(tb, pts, dual=dual)
        torch.cuda.synchronize()
        assert torch.equal(summary2, summary) and all(torch.equal(out2[k], out[k]) for k in out)
    ta.close()
    tb.close()
    return want, want_sum


def set_blocks(n):
    from piplib_amd import engine as eng
    fn = eng.lib().pipamd_debug_tape_sweep_blocks
    fn.argtypes = [C.c_int]
    assert fn(n) == 0


@functools.lru_cache(maxsize=None)
def p5(nq, bits):
    g = tc.golden()
    return cm.tape(_solve_p5(nq, bits)[0], g["nvar"], g["nparm"], bits=bits)


# ---------------------------------------------------------------- 1. golden p5, the integer quast against the rational one
@pytest.mark.parametrize("bits_a,bits_b", PAIRS)
def test_golden_integer_against_rational(bits_a, bits_b):
    """the engine's own tapes over [0,9]^2: SAME where the reference's recorded answers are equal, STATUS where one of
    them is missing, VALUE elsewhere"""
    g = tc.golden()
    ai, ar = g["answers"]["int"], g["answers"]["rat"]
    want, want_sum = hold(p5(1, bits_a), p5(0, bits_b), [0, 0], [9, 9])
    for k, (r, x, y) in enumerate(zip(want, ai, ar)):
        cls = cm.STATUS if (x is None) != (y is None) else (cm.SAME if x == y else cm.VALUE)
        assert r[0] == cls, (k, r, x, y)
    same, status = sum(x == y for x, y in zip(ai, ar)), sum((x is None) != (y is None) for x, y in zip(ai, ar))
    assert want_sum["counts"] == {"same": same, "status": status, "value": 100 - same - status, "range": 0, "outside": 0}
    assert same > 0 and status > 0 and 100 - same - status > 0


# ---------------------------------------------------------------- 2. a tape against a perturbed copy
def perturbed():
    """{name: (tape a, tape b, the `where` values expected among the VALUE points -- None: a STATUS difference)}, every b
    one edit away from a; three unknowns, two parameters, two dual pairs"""
    d1, d2 = [(1, 2), (-3, 4)], [(0, 1), (5, 3)]

    def quast(l1=([2, 1, 3], 2), l2_last=([1, 0, -4], 7), cond=(1, -1, 2), second=None, duals1=d1):
        one = tc.leaf([l1, ([0, -1, 5], 3), ([1, 1, 1], 1)], duals1)
        two = tc.leaf([([1, 1, 0], 1), ([3, 0, 1], 2), l2_last], d2) if second is None else second
        return cm.tape(tc.iff(list(cond), one, tc.iff([1, 1, -7], tc.nil(), two)), 3, 2, ndual=2)

    base = quast()
    return {
        "a coefficient of unknown 0": (base, quast(l1=([3, 1, 3], 2)), {0}),
        "a coefficient of the last unknown": (base, quast(l2_last=([1, 1, -4], 7)), {2}),
        # (the points with theta_0 - theta_1 + 2 == -1 move to list one: from the NIL, or from list two, whose unknown 0
        # agrees with list one's at some of them)
        "a condition's constant": (base, quast(cond=(1, -1, 3)), {0, 1, None}),
        "a list replaced by NIL": (base, quast(second=tc.nil()), {None}),
        "a dual pair": (base, quast(duals1=[(1, 2), (-3, 5)]), {3 + 1}),
    }


@pytest.mark.parametrize("bits_a,bits_b", PAIRS)
@pytest.mark.parametrize("name", list(perturbed()))
def test_perturbed_copy(name, bits_a, bits_b):
    a, b, wheres = perturbed()[name]
    a, b = dict(a, bits=bits_a), dict(b, bits=bits_b)
    lo, hi = [-6, -5], [8, 7]
    want, want_sum = hold(a, b, lo, hi, dual=True)
    seen = {r[1] if r[0] == cm.VALUE else None for r in want if r[0] in (cm.VALUE, cm.STATUS)}
    assert seen == wheres and want_sum["counts"]["same"] > 0 and want_sum["counts"]["range"] == 0, (name, seen)
    if name == "a dual pair":  # without the flag the dual lists are not looked at
        _, plain = hold(a, b, lo, hi)
        assert plain["counts"]["same"] == len(want) and want_sum["counts"]["value"] > 0


# ---------------------------------------------------------------- 3. other shapes, the same meaning
@pytest.mark.parametrize("bits_a,bits_b", PAIRS)
@pytest.mark.parametrize("case", range(3))
def test_equivalent_tapes_are_same(case, bits_a, bits_b):
    name, a, b, lo, hi = cm.equivalents()[case]
    want, want_sum = hold(dict(a, bits=bits_a), dict(b, bits=bits_b), lo, hi)
    assert want_sum["counts"]["same"] == len(want) == 15 * 13, name


# ---------------------------------------------------------------- 4. lanes of a wave at different leaf pairs
def list_chain(k, shift=0, bump=()):
    """k conditions (i + shift) - theta_0 >= 0 ? (theta_0 + i [+ 1 for i in bump]) : ..., the last else (theta_0): every
    item a LIST of its own"""
    cells = []
    for i in range(k):
        cells += [(tm.IF, 0, 0)] + tc.form([-1, i + shift]) + tc.leaf([([1, i + (i in bump)], 1)])
    return cells + tc.leaf([([1, 0], 1)])


def nil_chain(k, shift):
    """tape_cases.if_chain with its thresholds shifted"""
    cells = []
    for i in range(k):
        cells += [(tm.IF, 0, 0)] + tc.form([-1, i + shift]) + tc.nil()
    return cells + tc.leaf([([1, 0], 1)])


@pytest.mark.parametrize("bits_a,bits_b", PAIRS)
def test_wave_divergence(bits_a, bits_b):
    """0..199 through chains of 70 conditions: every lane of the first wave at another (leaf, leaf) pair, more than 64
    pairs in the first workgroup; thresholds shifted, and single leaves bumped"""
    a = cm.tape(list_chain(70), 1, 1, bits=bits_a)
    want, want_sum = hold(a, cm.tape(list_chain(70, shift=1), 1, 1, bits=bits_b), [0], [199])
    assert want_sum["counts"]["value"] == 70 and want_sum["counts"]["same"] == 130 and want_sum["first"]["value"] == 1
    want, want_sum = hold(a, cm.tape(list_chain(70, bump=(0, 63, 64, 69)), 1, 1, bits=bits_b), [0], [199])
    assert [k for k, r in enumerate(want) if r[0] == cm.VALUE] == [0, 63, 64, 69]
    # NIL items: if_chain(70) against its thresholds shifted by 3
    want, want_sum = hold(cm.tape(tc.if_chain(70), 1, 1, bits=bits_a), cm.tape(nil_chain(70, 3), 1, 1, bits=bits_b), [0], [199])
    assert want_sum["counts"] == {"same": 197, "status": 3, "value": 0, "range": 0, "outside": 0} and want_sum["first"]["status"] == 70


@pytest.mark.parametrize("bits_a,bits_b", PAIRS)
def test_chunk_edges(bits_a, bits_b):
    a, b = cm.tape(list_chain(5), 1, 1, bits=bits_a), cm.tape(list_chain(5, bump=(1, 4)), 1, 1, bits=bits_b)
    for n in (1, 127, 128, 129):
        hold(a, b, [-2], [-2 + n - 1])


# ---------------------------------------------------------------- 5. the grid-stride loop
def test_grid_stride_loop():
    """1000 points through 2 workgroups and through the unbounded grid: identical, and the model's"""
    import torch
    a, b = cm.tape(list_chain(5), 1, 1), cm.tape(list_chain(5, shift=2, bump=(3,)), 1, 1, bits=128)
    ta, tb = device_tapes(a, b)
    want, want_sum = cm.compare_sweep(a, b, [-3], [996])
    seen = []
    try:
        for blocks in (2, 0):
            set_blocks(blocks)
            summary, out = ta.compare_sweep(tb, [-3], [996])
            assert got_of(out, summary) == (want, want_sum), blocks
            seen.append((summary.cpu(), {k: v.cpu() for k, v in out.items()}))
    finally:
        set_blocks(0)
    assert torch.equal(seen[0][0], seen[1][0]) and all(torch.equal(seen[0][1][k], seen[1][1][k]) for k in seen[0][1])
    ta.close()
    tb.close()


# ---------------------------------------------------------------- 6. RANGE
RANGE_POINTS = [[MAX64], [5], [MIN64], [-1], [MAX64 - 1], [0]]


@pytest.mark.parametrize("bits_a,bits_b", PAIRS)
def test_range(bits_a, bits_b):
    """a numerator of 65 bits, a new parameter beyond int64, and a later unknown that leaves the range after an earlier
    one differs: RANGE for a 64-bit tape exactly where pipamd_tape_eval says so, whatever the 128-bit tape beside it has"""
    wide = tc.leaf([([1, 1], 1), ([1, 0], 1)])                       # theta_0 + 1 is 2^63 at MAX64
    newp = tc.new(1, [2, 0], 1, tc.leaf([([0, 1, 0], 1), ([1, 0, 0], 1)]))  # 2 theta_0 leaves int64 at either end
    late_a = tc.leaf([([1, 0], 1), ([1, 1], 1)])
    late_b = tc.leaf([([1, -1], 1), ([1, 1], 1)])                    # unknown 0 differs everywhere, unknown 1 as in `wide`
    for ca, cb in ((wide, wide), (newp, newp), (late_a, late_b), (wide, newp)):
        a, b = cm.tape(ca, 2, 1, bits=bits_a), cm.tape(cb, 2, 1, bits=bits_b)
        ta, tb = device_tapes(a, b)
        summary, out = ta.compare(tb, np.array(RANGE_POINTS, dtype=np.int64))
        got, got_sum = got_of(out, summary)
        want = cm.compare(a, b, RANGE_POINTS)
        assert got == want and got_sum == cm.summarise(want), (got, want)
        assert [r[2] for r in got] == eval_status(ta, RANGE_POINTS) and [r[3] for r in got] == eval_status(tb, RANGE_POINTS)
        ta.close()
        tb.close()
        at_max = want[0]
        assert at_max[1] == -1 or at_max[0] == cm.VALUE
        if bits_a == 64 or bits_b == 64:
            assert at_max[0] == cm.RANGE and at_max[1] == -1
            assert at_max[2] == (tm.ST_RANGE if bits_a == 64 else tm.ST_SOLUTION)
            assert at_max[3] == (tm.ST_RANGE if bits_b == 64 else tm.ST_SOLUTION)
        else:
            assert at_max[0] == (cm.SAME if ca is cb else cm.VALUE) and at_max[2] == at_max[3] == tm.ST_SOLUTION
        assert want[1][0] == (cm.SAME if ca is cb else cm.VALUE)


# ---------------------------------------------------------------- 7. pip_solve's edits
@pytest.mark.parametrize("bits_a,bits_b", PAIRS)
def test_edited_tapes(bits_a, bits_b):
    from piplib_amd import engine as eng
    g = family("maximize")
    ca, ia = solved("maximize", bits_a)
    cb, ib = solved("maximize", bits_b)
    a = cm.tape(ca, ia["nvar"], ia["nparm"], edit=ia, bits=bits_a)
    b = cm.tape(cb, ib["nvar"], ib["nparm"], edit=ib, bits=bits_b)
    assert cm.point_cols(a) == g["nparm"] < ia["nparm"]
    pts = np.array(g["points"])
    lo, hi = pts.min(axis=0).tolist(), pts.max(axis=0).tolist()
    want, want_sum = hold(a, b, lo, hi)
    assert want_sum["counts"]["same"] == len(want) and {r[2] for r in want} >= {tm.ST_SOLUTION}
    # the same tape without its edit has another number of point columns
    ta, tb = device_tapes(a, dict(b, edit=None))
    assert ta.point_cols != tb.point_cols
    for call in (lambda: ta.compare_sweep(tb, lo, hi), lambda: ta.compare(tb, pts)):
        with pytest.raises(eng.TapeError) as err:
            call()
        assert err.value.code == tm.E_INVALID
    ta.close()
    tb.close()
    # a negate mark against the numerators negated by hand; an unbounded unknown is (n, 0), not (n, 1)
    forms = [([2, -1, 3], 2), ([0, 4, -6], 4)]
    neg = dict(sol_bg=-1, urs_parms=0, sol_flags=te.SOL_NEGATE)
    marked = cm.tape(tc.leaf(forms), 2, 2, edit=neg, bits=bits_a)
    by_hand = cm.tape(tc.leaf([([-v for v in n], d) for n, d in forms]), 2, 2, bits=bits_b)
    want, want_sum = hold(marked, by_hand, [-4, -4], [4, 4])
    assert want_sum["counts"]["same"] == 81
    _, plain = hold(cm.tape(tc.leaf(forms), 2, 2, bits=bits_a), by_hand, [-4, -4], [4, 4])
    assert plain["counts"]["value"] > 70
    shift = dict(sol_bg=0, urs_parms=0, sol_flags=te.SOL_SHIFT)
    unb = cm.tape(tc.leaf([([3, 1, 0], 1), ([1, 1, 0], 1)]), 2, 2, edit=shift, bits=bits_a)  # 3 - 1 != 0: unbounded; 1 - 1 == 0
    bounded = cm.tape(tc.leaf([([2, 1, 0], 1), ([0, 1, 0], 1)]), 2, 2, bits=bits_b)
    want, _ = hold(unb, bounded, [-2, -2], [2, 2])
    assert all(r[:2] == (cm.VALUE, 0) for r in want)


# ---------------------------------------------------------------- 8. the context
@pytest.mark.parametrize("bits_a,bits_b", PAIRS)
def test_context(bits_a, bits_b):
    from piplib_amd import engine as eng
    for rows, point, inside in sm.edge_rows():
        cols = len(point)
        a = cm.tape(tc.nil(), 1, cols, bits=bits_a)
        b = cm.tape(tc.leaf([([0] * cols + [1], 1)]), 1, cols, bits=bits_b)
        if cm.lds(cm.info(a), bits_a, cm.info(b), bits_b)[0] > tm.LDS_BYTES:
            # 31 parameters in 128 bits on either side: the two slot areas do not fit, and the entry says so
            assert cols == 31 and (bits_a, bits_b) != (64, 64)
            ta, tb = device_tapes(a, b)
            for call in (lambda: ta.compare_sweep_into(tb, point, point, {}, ctx=rows), lambda: ta.compare_into(tb, [point], {})):
                with pytest.raises(eng.TapeError) as err:
                    call()
                assert err.value.code == tm.E_TOOLARGE
            ta.close()
            tb.close()
            continue
        want, want_sum = hold(a, b, point, point, rows)
        assert want == [(cm.STATUS, -1, tm.ST_NIL, tm.ST_SOLUTION) if inside else OUTSIDE]
    # an equality and an inequality over the golden pair
    g = tc.golden()
    a = cm.tape(tc.cells_from_text(g["tapes"]["int"]), g["nvar"], g["nparm"], bits=bits_a)
    b = cm.tape(tc.cells_from_text(g["tapes"]["rat"]), g["nvar"], g["nparm"], bits=bits_b)
    want, want_sum = hold(a, b, [-1, -2], [11, 10], [[0, 1, -2, 0], [1, 1, 1, -4]])
    n_out = want_sum["counts"]["outside"]
    assert 0 < n_out < 169 and sum(want_sum["counts"].values()) == 169 and want_sum["first"]["outside"] == 0
    assert all(r == OUTSIDE for r in want if r[0] == cm.OUTSIDE) and len({r[0] for r in want}) >= 3
    # no parameters: one point; an empty tape is NIL there
    one = cm.tape(tc.iff([-3], tc.nil(), tc.leaf([([7], 2)])), 1, 0, bits=bits_a)
    want, _ = hold(one, dict(one, bits=bits_b), [], [])
    assert want == [(cm.SAME, -1, tm.ST_SOLUTION, tm.ST_SOLUTION)]
    want, _ = hold(one, cm.tape([], 1, 0, bits=bits_b), [], [])
    assert want == [(cm.STATUS, -1, tm.ST_SOLUTION, tm.ST_NIL)]
    want, want_sum = hold(cm.tape([], 2, 1, bits=bits_a), cm.tape([], 2, 1, bits=bits_b), [4], [8], [[1, 1, -5]])
    assert want_sum["counts"] == {"same": 4, "status": 0, "value": 0, "range": 0, "outside": 1}


# ---------------------------------------------------------------- 9. programs in LDS, and in global memory
@pytest.mark.parametrize("bits_a,bits_b", PAIRS)
def test_staging_switch(bits_a, bits_b):
    """the pair is staged at k conditions and read from global memory at k + 1, k from the planner: the same results"""
    other = cm.tape(list_chain(6, shift=2), 1, 1, bits=bits_b)

    ew, info_b = bits_a // 64, cm.info(other)

    def staged(k):  # (a chain of k conditions over one parameter: k IF and k NIL items, one list of one unknown)
        return cm.lds({"slots": 2, "words": k * (2 + 2 * ew) + 1 + 3 * ew}, bits_a, info_b, bits_b)[1]

    k = next(k for k in range(500, 2100) if staged(k) and not staged(k + 1))
    classes = []
    for kk, want_staged in ((k, 1), (k + 1, 0)):
        a = cm.tape(tc.if_chain(kk), 1, 1, bits=bits_a)
        lo, hi = [kk - 60], [kk + 90]
        ta, tb = device_tapes(a, other)
        assert ta.compare_plan(tb, lo, hi) == {"n_points": 151, "staged": want_staged}
        ta.close()
        tb.close()
        want, want_sum = hold(a, other, lo, hi)
        assert want_sum["counts"]["status"] == 60 and want_sum["counts"]["same"] == 91
        classes.append([r[0] for r in want])
    assert classes[0] == classes[1]


# ---------------------------------------------------------------- 10. the project's own question
def test_p5_in_64_and_in_128_bits_is_same():
    for nq in (1, 0):
        want, want_sum = hold(p5(nq, 64), p5(nq, 128), [0, 0], [9, 9])
        assert want_sum["counts"]["same"] == 100


def test_p5_with_the_device_tree_on_and_off_is_same():
    from piplib_amd import engine as eng
    g = tc.golden()
    tab = tc.parametric_tableau(g["matrix"], g["nvar"], g["nparm"], g["eq_rows"])
    prob = types.SimpleNamespace(nvar=g["nvar"], nparm=g["nparm"], ni=tab.shape[0], nc=0, bigparm=-1, nq=1, ineq=tab,
                                 ctx=np.zeros((0, g["nparm"] + 1), np.int64))
    e = eng.Engine(0)
    tapes, served = [], []
    for on in (True, False):
        e.set_device_tree(on)
        (text, rc, _, _), = eng.solve_tableaux(e, [prob], lockstep=True)
        assert rc == 0
        served.append(e.last_device_tree()[0])
        tapes.append(cm.tape(tc.cells_from_text(text), g["nvar"], g["nparm"]))
    e.set_device_tree(True)
    assert served == [1, 0]  # (the device tree finished the problem when it was on; the lock-step scheduler when off)
    want, want_sum = hold(tapes[0], tapes[1], [0, 0], [9, 9])
    assert want_sum["counts"]["same"] == 100
    assert tc.answers_of(cm.evaluate(tapes[0], g["points"])) == g["answers"]["int"]


# ---------------------------------------------------------------- 11. null outputs, two streams, no accumulation
def test_null_outputs_and_two_streams():
    import torch
    from piplib_amd import engine as eng
    a, b = p5(1, 64), p5(0, 128)
    ta, tb = device_tapes(a, b)
    lo, hi, ctx = [-5, -5], [58, 58], [[1, 1, 1, -3]]
    n = 64 * 64
    assert ta.compare_sweep_into(tb, lo, hi, {}, ctx=ctx) == (None, {})          # every output NULL: a legal call
    assert ta.compare_into(tb, np.zeros((5, 2), np.int64), {}) == (None, {})
    single = ta.compare_sweep(tb, lo, hi, ctx=ctx)
    torch.cuda.synchronize()
    want, want_sum = cm.compare_sweep(a, b, lo, hi, ctx)
    assert got_of(single[1], single[0]) == (want, want_sum)
    # each output alone is the same array; the summary alone the same figures, and a second call does not accumulate
    for name in eng.Tape.CMP_OUTPUTS:
        _, alone = ta.compare_sweep_into(tb, lo, hi, ta.compare_outputs(n, (name,)), ctx=ctx)
        torch.cuda.synchronize()
        assert list(alone) == [name] and torch.equal(alone[name], single[1][name])
    buf = torch.full((eng.CMP_WORDS,), 77, dtype=torch.int64, device=ta.dev)
    for _ in range(2):
        ta.compare_sweep_into(tb, lo, hi, {}, ctx=ctx, summary=buf)
        torch.cuda.synchronize()
        assert torch.equal(buf, single[0])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        x = ta.compare_sweep(tb, lo, hi, ctx=ctx)
    with torch.cuda.stream(s2):
        y = ta.compare_sweep(tb, lo, hi, ctx=ctx)
    torch.cuda.synchronize()
    for other in (x, y):
        assert torch.equal(other[0], single[0]) and all(torch.equal(other[1][k], single[1][k]) for k in single[1])
    # no points: the summary is still initialised
    ta.compare_into(tb, np.zeros((0, 2), np.int64), {}, summary=buf)
    torch.cuda.synchronize()
    assert buf.tolist() == [0] * 5 + [-1] * 5
    ta.close()
    tb.close()
