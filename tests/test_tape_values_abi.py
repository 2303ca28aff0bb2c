"""The host side of pipamd_tape_sweep_values: the planner held to tests/tape_values_model.py, the struct's layout, and the
refusals of the call that come before any HIP call.  Host only: no engine, no GPU."""
import ctypes as C

import pytest

import tape_cases as tc
import tape_model as tm
import tape_values_model as vm
from piplib_amd import engine as eng
from tape_cases import MAX64, MIN64

INFO = {"leaves": 7, "ifs": 6, "news": 1, "words": 60, "slots": 4, "depth": 5, "staged": 1}


def plan_fn():
    fn = eng.lib().pipamd_tape_sweep_values_plan
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    return fn


def both(info, bits, nvar, cols, lo, hi):
    """(the C planner's plan or error code, the model's)"""
    out = []
    for fn in (lambda: eng.values_plan(info, bits, nvar, cols, lo, hi), lambda: vm.plan(info, bits, nvar, cols, lo, hi)):
        try:
            out.append(fn())
        except (eng.TapeError, tm.TapeError) as e:
            out.append(e.code)
    return tuple(out)


def test_struct_layout_and_constants():
    P = eng.TapeValuesPlan
    assert C.sizeof(P) == 32
    assert [getattr(P, n).offset for n in ("n_points", "summary_words", "work_bytes", "staged", "reserved")] == [0, 8, 16, 24, 28]
    assert (eng.VALUES_MAX_NVAR, eng.VALUES_HEAD, eng.VALUES_REC) == (vm.MAX_NVAR, vm.HEAD, vm.REC) == (64, 8, 16)
    assert eng.lib().pipamd_version() == 500
    # the C struct is filled as the ctypes one is read: reserved 0, every field written
    plan = P(-1, -1, -1, -1, -1)
    info = eng.TapeInfo(**INFO)
    lo, hi = (C.c_int64 * 2)(0, 0), (C.c_int64 * 2)(3, 3)
    assert plan_fn()(C.byref(info), 64, 5, 2, lo, hi, C.byref(plan)) == 0
    assert (plan.n_points, plan.summary_words, plan.work_bytes, plan.staged, plan.reserved) == (16, 88, 96 * 5 * 2, 1, 0)


def test_plan_counts_the_box_and_the_work():
    assert both(INFO, 64, 3, 2, [0, 0], [9, 9]) == ({"n_points": 100, "summary_words": 56, "work_bytes": 576, "staged": 1},) * 2
    assert both(INFO, 128, 2, 3, [-3, MIN64, MAX64 - 4], [12, MIN64, MAX64])[0]["n_points"] == 16 * 5
    assert both(INFO, 64, 0, 0, [], []) == ({"n_points": 1, "summary_words": 8, "work_bytes": 0, "staged": 1},) * 2
    for n in (1, 128, 129, 128 * 2047, 128 * 2047 + 1, 128 * 2048, 128 * 2048 + 1, 10 ** 6):
        got, want = both(INFO, 64, 7, 1, [0], [n - 1])
        assert got == want and got["work_bytes"] == 96 * 7 * 2 * min(-(-n // 128), 2048), n
    g = tc.golden()
    info = eng.tape_check(tc.cells_from_text(g["tapes"]["int"]), g["nvar"], g["nparm"])
    got, want = both(info, 64, g["nvar"], 2, [0, 0], [999, 999])
    assert got == want and got["n_points"] == 10 ** 6 and got["summary_words"] == 8 + 16 * g["nvar"] and got["staged"] == 1


def test_work_stays_within_32_mib():
    # 2^38 - 1 = 524287 * 524289 points and 64 unknowns: the most a legal call can ask for
    got, want = both(INFO, 64, 64, 2, [5, -524289], [524291, -1])
    assert got == want and got["n_points"] == (1 << 38) - 1 and got["summary_words"] == 8 + 16 * 64
    assert got["work_bytes"] == 24 << 20 and got["work_bytes"] <= 32 << 20
    assert both(INFO, 128, 64, 1, [0], [(1 << 38) - 2])[0]["work_bytes"] == 24 << 20


def test_plan_refusals():
    fn = plan_fn()
    info, plan = eng.TapeInfo(**INFO), eng.TapeValuesPlan()
    lo, hi = (C.c_int64 * 2)(0, 0), (C.c_int64 * 2)(3, 3)
    assert fn(C.byref(info), 64, 2, 2, lo, hi, C.byref(plan)) == 0 and plan.n_points == 16
    assert fn(None, 64, 2, 2, lo, hi, C.byref(plan)) == tm.E_INVALID
    assert fn(C.byref(info), 64, 2, 2, lo, hi, None) == tm.E_INVALID
    for bits in (0, 32, 65, 256, -64):
        assert fn(C.byref(info), bits, 2, 2, lo, hi, C.byref(plan)) == tm.E_INVALID, bits
    assert fn(C.byref(info), 64, 2, 2, None, hi, C.byref(plan)) == tm.E_INVALID
    assert fn(C.byref(info), 64, 2, 2, lo, None, C.byref(plan)) == tm.E_INVALID
    assert fn(C.byref(info), 64, 2, 0, None, None, C.byref(plan)) == 0 and plan.n_points == 1
    big = (C.c_int64 * 32)()
    assert fn(C.byref(info), 64, 2, -1, big, big, C.byref(plan)) == tm.E_INVALID
    assert fn(C.byref(info), 64, 2, tm.MAX_SLOTS, big, big, C.byref(plan)) == tm.E_INVALID
    assert fn(C.byref(info), 64, 2, tm.MAX_SLOTS - 1, big, big, C.byref(plan)) == 0 and plan.n_points == 1
    assert both(INFO, 64, 2, 2, [0, 4], [3, 3]) == (tm.E_INVALID,) * 2            # lo above hi
    assert both(INFO, 64, 2, 2, [MIN64, 1], [MAX64, 0]) == (tm.E_INVALID,) * 2    # ... before the size is looked at
    # nvar
    assert both(INFO, 64, -1, 1, [0], [9]) == (tm.E_INVALID,) * 2
    assert both(INFO, 64, 64, 1, [0], [9])[0]["summary_words"] == 8 + 16 * 64
    assert both(INFO, 64, 65, 1, [0], [9]) == (tm.E_TOOLARGE,) * 2
    assert both(INFO, 64, 1 << 20, 1, [0], [9]) == (tm.E_TOOLARGE,) * 2
    assert both(INFO, 64, 65, 1, [4], [3]) == (tm.E_INVALID,) * 2                  # the box's refusals come first
    # the sweep planner's TOOLARGE
    assert both(INFO, 64, 2, 2, [0, 0], [(1 << 19) - 1, (1 << 19) - 1]) == (tm.E_TOOLARGE,) * 2   # 2^38
    assert both(INFO, 64, 2, 1, [0], [(1 << 38) - 1]) == (tm.E_TOOLARGE,) * 2
    assert both(INFO, 64, 2, 1, [MIN64], [MAX64]) == (tm.E_TOOLARGE,) * 2
    assert both(INFO, 64, 2, 31, [MIN64] * 31, [MAX64] * 31) == (tm.E_TOOLARGE,) * 2


@pytest.mark.parametrize("bits", [64, 128])
def test_staged_at_its_switch(bits):
    """the program beside the slots and nothing else: the reduction takes no LDS"""
    slots = 5
    last = (tm.LDS_BYTES - tm.slot_bytes(slots, bits)) // 8
    for words, staged, want in ((last, 1, 1), (last + 1, 1, 0), (last, 0, 0), (0, 1, 0), (0, 0, 0), (1, 1, 1)):
        info = dict(INFO, slots=slots, words=words, staged=staged)
        got, model = both(info, bits, 3, 1, [0], [9])
        assert got == model and got["staged"] == want, (words, staged, got)
    # real tapes: a chain of k conditions has 4 k + 4 words (64 bits), staged up to k = 2015
    for k, want in ((2015, 1), (2016, 0)):
        info = eng.tape_check(tc.if_chain(k), 1, 1)
        got, model = both(info, 64, 1, 1, [0], [k])
        assert got == model and got["staged"] == want == info["staged"] and got["n_points"] == k + 1, k
    assert both(eng.tape_check([], 2, 1), 64, 2, 1, [0], [3])[0]["staged"] == 0     # the empty tape


def test_call_refuses_before_any_hip_call():
    L = eng.lib()
    fn = L.pipamd_tape_sweep_values
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.c_size_t, C.c_void_p]
    fn.restype = C.c_int
    lo = (C.c_int64 * 1)(0)
    buf = (C.c_int64 * 64)()
    assert fn(None, None, lo, lo, 0, 0, None, buf, buf, 512, None) == tm.E_INVALID
    assert b"null engine" in L.pipamd_last_error()
    assert fn(None, None, lo, lo, 0, 0, None, None, None, 0, None) == tm.E_INVALID
    assert fn(None, None, None, None, -1, 0, None, buf, buf, 512, None) == tm.E_INVALID
