"""The host side of the tape sweep (pipamd_tape_sweep_plan, and the refusals of pipamd_tape_sweep that come before any HIP
call), held to tests/tape_sweep_model.py.  Host only: no engine, no GPU."""
import ctypes as C

import pytest

import tape_cases as tc
import tape_model as tm
import tape_sweep_model as sm
from piplib_amd import engine as eng
from tape_cases import MAX64, MIN64

INFO = {"leaves": 7, "ifs": 6, "news": 1, "words": 60, "slots": 4, "depth": 5, "staged": 1}


def plan_fn():
    fn = eng.lib().pipamd_tape_sweep_plan
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    return fn


def both(info, bits, cols, lo, hi):
    """(the C planner's plan or error code, the model's)"""
    out = []
    for fn in (lambda: eng.sweep_plan(info, bits, cols, lo, hi), lambda: sm.plan(info, bits, cols, lo, hi)):
        try:
            out.append(fn())
        except (eng.TapeError, tm.TapeError) as e:
            out.append(e.code)
    return tuple(out)


def test_plan_counts_the_box():
    assert both(INFO, 64, 2, [0, 0], [9, 9]) == ({"n_points": 100, "summary_words": 22, "binned": 1},) * 2
    assert both(INFO, 128, 3, [-3, MIN64, MAX64 - 4], [12, MIN64, MAX64])[0]["n_points"] == 16 * 5
    assert both(INFO, 64, 0, [], []) == ({"n_points": 1, "summary_words": 22, "binned": 1},) * 2
    g = tc.golden()
    info = eng.tape_check(tc.cells_from_text(g["tapes"]["int"]), g["nvar"], g["nparm"])
    got, want = both(info, 64, 2, [0, 0], [999, 999])
    assert got == want and got["n_points"] == 10 ** 6 and got["summary_words"] == 8 + 2 * info["leaves"] and got["binned"] == 1


def test_plan_point_limit_at_its_edge():
    # 2^38 - 1 = 524287 * 524289
    got, want = both(INFO, 64, 2, [5, -524289], [524291, -1])
    assert got == want and got["n_points"] == (1 << 38) - 1
    assert both(INFO, 64, 2, [0, 0], [(1 << 19) - 1, (1 << 19) - 1]) == (tm.E_TOOLARGE,) * 2   # 2^38
    assert both(INFO, 64, 1, [0], [(1 << 38) - 2])[0]["n_points"] == (1 << 38) - 1
    assert both(INFO, 64, 1, [0], [(1 << 38) - 1]) == (tm.E_TOOLARGE,) * 2
    # the full range of a column is a legal question: the product is formed without wrapping
    assert both(INFO, 64, 1, [MIN64], [MAX64]) == (tm.E_TOOLARGE,) * 2
    assert both(INFO, 64, 2, [MIN64, MIN64], [MAX64, MAX64]) == (tm.E_TOOLARGE,) * 2   # 2^128 wraps to 0 in 128 bits
    assert both(INFO, 64, 4, [MIN64] * 4, [MAX64] * 4) == (tm.E_TOOLARGE,) * 2
    assert both(INFO, 64, 31, [MIN64] * 31, [MAX64] * 31) == (tm.E_TOOLARGE,) * 2
    assert both(INFO, 64, 31, [MIN64] * 30 + [3], [MIN64] * 30 + [4])[0]["n_points"] == 2


def test_plan_refusals():
    fn = plan_fn()
    info, plan = eng.TapeInfo(**INFO), eng.TapeSweepPlan()
    lo, hi = (C.c_int64 * 2)(0, 0), (C.c_int64 * 2)(3, 3)
    assert fn(C.byref(info), 64, 2, lo, hi, C.byref(plan)) == 0 and plan.n_points == 16
    assert fn(None, 64, 2, lo, hi, C.byref(plan)) == tm.E_INVALID
    assert fn(C.byref(info), 64, 2, lo, hi, None) == tm.E_INVALID
    for bits in (0, 32, 65, 256, -64):
        assert fn(C.byref(info), bits, 2, lo, hi, C.byref(plan)) == tm.E_INVALID, bits
    assert fn(C.byref(info), 64, 2, None, hi, C.byref(plan)) == tm.E_INVALID
    assert fn(C.byref(info), 64, 2, lo, None, C.byref(plan)) == tm.E_INVALID
    assert fn(C.byref(info), 64, 0, None, None, C.byref(plan)) == 0 and plan.n_points == 1
    big = (C.c_int64 * 32)()
    assert fn(C.byref(info), 64, -1, big, big, C.byref(plan)) == tm.E_INVALID
    assert fn(C.byref(info), 64, tm.MAX_SLOTS, big, big, C.byref(plan)) == tm.E_INVALID
    assert fn(C.byref(info), 64, tm.MAX_SLOTS - 1, big, big, C.byref(plan)) == 0 and plan.n_points == 1
    assert both(INFO, 64, 2, [0, 4], [3, 3]) == (tm.E_INVALID,) * 2            # lo above hi
    assert both(INFO, 64, 2, [MAX64, 0], [MIN64, 3]) == (tm.E_INVALID,) * 2
    # lo above hi is refused before the size is looked at
    assert both(INFO, 64, 2, [MIN64, 1], [MAX64, 0]) == (tm.E_INVALID,) * 2


@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("staged", [1, 0])
def test_binned_at_its_edge(bits, staged):
    """16 (L + 4) bytes beside the slots, and beside the program when it is staged"""
    slots, words = 5, 1000
    room = tm.LDS_BYTES - tm.slot_bytes(slots, bits) - (8 * words if staged else 0)
    last = room // 16 - 4
    for leaves, want in ((last, 1), (last + 1, 0), (0, 1)):
        info = dict(INFO, slots=slots, words=words, staged=staged, leaves=leaves)
        got, model = both(info, bits, 1, [0], [9])
        assert got == model and got["binned"] == want and got["summary_words"] == 8 + 2 * leaves, (leaves, got)
    # real tapes: a chain of k conditions has k + 1 leaves and 4 k + 4 words (64 bits), staged up to k = 2015
    for k in (1341, 1342, 2015, 2016, 4027, 4028):
        info = eng.tape_check(tc.if_chain(k), 1, 1)
        got, model = both(info, 64, 1, [0], [k])
        assert got == model and got["n_points"] == k + 1, k
    assert [eng.sweep_plan(eng.tape_check(tc.if_chain(k), 1, 1), 64, 1, [0], [1])["binned"]
            for k in (1341, 1342, 2015, 2016, 4027, 4028)] == [1, 0, 0, 1, 1, 0]


def test_sweep_refuses_null_handles_before_any_hip_call():
    L = eng.lib()
    fn = L.pipamd_tape_sweep
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 9
    lo = (C.c_int64 * 1)(0)
    assert fn(None, None, lo, lo, 0, 0, *([None] * 9)) == tm.E_INVALID
    assert b"null engine or tape" in L.pipamd_last_error()
    assert fn(None, None, None, None, -1, 0, *([None] * 9)) == tm.E_INVALID
    knob = L.pipamd_debug_tape_sweep_blocks
    knob.argtypes = [C.c_int]
    assert knob(-1) == tm.E_INVALID and knob(3) == 0 and knob(0) == 0
    assert eng.ST_OUTSIDE == sm.ST_OUTSIDE == 11
