"""The host side of the tape comparison (pipamd_tape_compare_plan, and the refusals of pipamd_tape_compare and
pipamd_tape_compare_sweep that come before any HIP call), held to tests/tape_compare_model.py.  Host only: no engine,
no GPU."""
import ctypes as C

import pytest

import tape_cases as tc
import tape_compare_model as cm
import tape_model as tm
from piplib_amd import engine as eng
from tape_cases import MAX64, MIN64

INFO = {"leaves": 7, "ifs": 6, "news": 1, "words": 60, "slots": 4, "depth": 5, "staged": 1}
WIDE = dict(INFO, slots=tm.MAX_SLOTS, words=100000, staged=0)


def plan_fn():
    fn = eng.lib().pipamd_tape_compare_plan
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    return fn


def both(ia, ba, ib, bb, cols, lo, hi):
    """(the C planner's plan or error code, the model's)"""
    out = []
    for fn in (lambda: eng.compare_plan(ia, ba, ib, bb, cols, lo, hi), lambda: cm.plan(ia, ba, ib, bb, cols, lo, hi)):
        try:
            out.append(fn())
        except (eng.TapeError, tm.TapeError) as e:
            out.append(e.code)
    return tuple(out)


def test_plan_counts_the_box():
    assert both(INFO, 64, INFO, 128, 2, [0, 0], [9, 9]) == ({"n_points": 100, "staged": 1},) * 2
    assert both(INFO, 128, INFO, 64, 3, [-3, MIN64, MAX64 - 4], [12, MIN64, MAX64])[0]["n_points"] == 16 * 5
    assert both(INFO, 64, INFO, 64, 0, [], []) == ({"n_points": 1, "staged": 1},) * 2
    g = tc.golden()
    ia = eng.tape_check(tc.cells_from_text(g["tapes"]["int"]), g["nvar"], g["nparm"])
    ib = eng.tape_check(tc.cells_from_text(g["tapes"]["rat"]), g["nvar"], g["nparm"], bits=128)
    got, want = both(ia, 64, ib, 128, 2, [0, 0], [999, 999])
    assert got == want == {"n_points": 10 ** 6, "staged": 1}


def test_plan_point_limit_at_its_edge():
    # 2^38 - 1 = 524287 * 524289
    got, want = both(INFO, 64, INFO, 64, 2, [5, -524289], [524291, -1])
    assert got == want and got["n_points"] == (1 << 38) - 1
    assert both(INFO, 64, INFO, 64, 2, [0, 0], [(1 << 19) - 1, (1 << 19) - 1]) == (tm.E_TOOLARGE,) * 2   # 2^38
    assert both(INFO, 64, INFO, 128, 1, [0], [(1 << 38) - 2])[0]["n_points"] == (1 << 38) - 1
    assert both(INFO, 64, INFO, 128, 1, [0], [(1 << 38) - 1]) == (tm.E_TOOLARGE,) * 2
    assert both(INFO, 64, INFO, 64, 1, [MIN64], [MAX64]) == (tm.E_TOOLARGE,) * 2
    assert both(INFO, 64, INFO, 64, 31, [MIN64] * 31, [MAX64] * 31) == (tm.E_TOOLARGE,) * 2


@pytest.mark.parametrize("bits_a,bits_b", [(64, 64), (64, 128), (128, 64), (128, 128)])
def test_staged_at_its_switch(bits_a, bits_b):
    """both programs beside both slot areas: the last word count that fits, and the first that does not"""
    sa, sb = 6, 3
    room = tm.LDS_BYTES - tm.slot_bytes(sa, bits_a) - tm.slot_bytes(sb, bits_b)
    assert room > 0 and room % 8 == 0
    for words_a, words_b, want in ((room // 8 - 211, 211, 1), (room // 8 - 210, 211, 0), (room // 8, 0, 1), (0, room // 8 + 1, 0)):
        ia, ib = dict(INFO, slots=sa, words=words_a), dict(INFO, slots=sb, words=words_b)
        got, model = both(ia, bits_a, ib, bits_b, 1, [0], [9])
        assert got == model == {"n_points": 10, "staged": want}, (words_a, words_b)
    # (whether either tape is staged when evaluated alone plays no part)
    assert both(dict(INFO, staged=0), bits_a, dict(INFO, staged=0), bits_b, 1, [0], [9])[0]["staged"] == 1


def test_slot_areas_beyond_lds_are_toolarge():
    # two 128-bit tapes of 32 slots: 2 x 63,488 bytes; each alone is served
    assert tm.slot_bytes(32, 128) == 63488
    assert both(WIDE, 128, WIDE, 128, 2, [0, 0], [9, 9]) == (tm.E_TOOLARGE,) * 2
    assert both(WIDE, 128, WIDE, 64, 2, [0, 0], [9, 9]) == (tm.E_TOOLARGE,) * 2   # 63,488 + 31,744
    assert both(WIDE, 64, WIDE, 64, 2, [0, 0], [9, 9]) == ({"n_points": 100, "staged": 0},) * 2   # 2 x 31,744
    # the edge: 128 (sa - 1) 16 + 128 (sb - 1) 8 = 65536 at sa = 32, sb = 3
    assert both(WIDE, 128, dict(INFO, slots=3), 64, 1, [0], [1])[0] == {"n_points": 2, "staged": 0}
    assert both(WIDE, 128, dict(INFO, slots=4), 64, 1, [0], [1]) == (tm.E_TOOLARGE,) * 2
    # a bad box is refused before the size of the pair is looked at, as the model has it
    assert both(WIDE, 128, WIDE, 128, 2, [0, 4], [3, 3]) == (tm.E_INVALID,) * 2


def test_plan_refusals():
    fn = plan_fn()
    info, plan = eng.TapeInfo(**INFO), eng.TapeComparePlan()
    lo, hi = (C.c_int64 * 2)(0, 0), (C.c_int64 * 2)(3, 3)
    ok = lambda *a: fn(*a)
    assert ok(C.byref(info), 64, C.byref(info), 128, 2, lo, hi, C.byref(plan)) == 0 and plan.n_points == 16 and plan.staged == 1
    assert ok(None, 64, C.byref(info), 64, 2, lo, hi, C.byref(plan)) == tm.E_INVALID
    assert ok(C.byref(info), 64, None, 64, 2, lo, hi, C.byref(plan)) == tm.E_INVALID
    assert ok(C.byref(info), 64, C.byref(info), 64, 2, lo, hi, None) == tm.E_INVALID
    for bits in (0, 32, 65, 256, -64):
        assert ok(C.byref(info), bits, C.byref(info), 64, 2, lo, hi, C.byref(plan)) == tm.E_INVALID, bits
        assert ok(C.byref(info), 128, C.byref(info), bits, 2, lo, hi, C.byref(plan)) == tm.E_INVALID, bits
    assert ok(C.byref(info), 64, C.byref(info), 64, 2, None, hi, C.byref(plan)) == tm.E_INVALID
    assert ok(C.byref(info), 64, C.byref(info), 64, 2, lo, None, C.byref(plan)) == tm.E_INVALID
    assert ok(C.byref(info), 64, C.byref(info), 64, 0, None, None, C.byref(plan)) == 0 and plan.n_points == 1
    big = (C.c_int64 * 32)()
    assert ok(C.byref(info), 64, C.byref(info), 64, -1, big, big, C.byref(plan)) == tm.E_INVALID
    assert ok(C.byref(info), 64, C.byref(info), 64, tm.MAX_SLOTS, big, big, C.byref(plan)) == tm.E_INVALID
    assert ok(C.byref(info), 64, C.byref(info), 64, tm.MAX_SLOTS - 1, big, big, C.byref(plan)) == 0 and plan.n_points == 1
    assert both(INFO, 64, INFO, 64, 2, [0, 4], [3, 3]) == (tm.E_INVALID,) * 2            # lo above hi
    assert both(INFO, 64, INFO, 64, 2, [MIN64, 1], [MAX64, 0]) == (tm.E_INVALID,) * 2    # ... before the size is looked at
    assert both(INFO, 64, INFO, 32, 1, [0], [1]) == (tm.E_INVALID,) * 2


def test_entries_refuse_before_any_hip_call():
    L = eng.lib()
    cmp_, sweep = L.pipamd_tape_compare, L.pipamd_tape_compare_sweep
    cmp_.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64] + [C.c_void_p] * 7
    sweep.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7
    lo = (C.c_int64 * 1)(0)
    assert cmp_(None, None, None, 0, 0, *([None] * 7)) == tm.E_INVALID
    assert b"null engine or tape" in L.pipamd_last_error()
    assert sweep(None, None, None, 0, lo, lo, 0, 0, *([None] * 7)) == tm.E_INVALID
    assert b"null engine or tape" in L.pipamd_last_error()
    for flags in (2, 4, -1, 1 << 30):
        assert cmp_(None, None, None, flags, 0, *([None] * 7)) == tm.E_INVALID
        assert b"unknown flag bits" in L.pipamd_last_error()
        assert sweep(None, None, None, flags, lo, lo, 0, 0, *([None] * 7)) == tm.E_INVALID
        assert b"unknown flag bits" in L.pipamd_last_error()
    assert cmp_(None, None, None, eng.CMP_DUAL, -1, *([None] * 7)) == tm.E_INVALID
    assert (eng.CMP_SAME, eng.CMP_STATUS, eng.CMP_VALUE, eng.CMP_RANGE, eng.CMP_OUTSIDE) == (cm.SAME, cm.STATUS, cm.VALUE, cm.RANGE, cm.OUTSIDE)
    assert eng.CMP_WORDS == cm.WORDS == 10 and eng.CMP_DUAL == cm.DUAL == 1 and eng.CMP_CLASSES == cm.CLASSES


def test_summary_as_a_dict():
    s = eng.compare_summary([47, 2, 51, 0, 0, 0, 1, 10, -1, -1])
    assert s == {"counts": {"same": 47, "status": 2, "value": 51, "range": 0, "outside": 0},
                 "first": {"same": 0, "status": 1, "value": 10, "range": -1, "outside": -1}}
    assert cm.words(s) == [47, 2, 51, 0, 0, 0, 1, 10, -1, -1]
