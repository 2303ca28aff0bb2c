"""The host side of pip_solve's result edits and of tape sets (pipamd_tape_check_pip / _pip128, and the refusals of
pipamd_tape_compile_pip and pipamd_tape_set_* that come before any HIP call), held to tests/tape_edit_model.py.  Host
only: no engine, no GPU."""
import ctypes as C
import os
import re

import pytest

import tape_cases as tc
import tape_edit_model as te
import tape_model as tm
from piplib_amd import engine as eng

NEW_SYMBOLS = ("pipamd_tape_check_pip", "pipamd_tape_check_pip128", "pipamd_tape_compile_pip", "pipamd_tape_compile_pip128",
               "pipamd_tape_point_cols", "pipamd_tape_set_create", "pipamd_tape_set_free", "pipamd_tape_set_eval")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "piplib_amd.h")

# two unknowns over four raw parameters (a big one at column 1, one Urs copy at column 3) and one new parameter
NVAR, NPARM = 2, 4
TAPE = tc.new(4, [1, 0, 2, -2, 3], 2,
              tc.iff([1, 0, -1, 1, 0, -1], tc.leaf([([2, 4, 3, -3, 1, 5], 4), ([0, 1, 0, 0, 1, 0], 1)]), tc.nil()))


def code(fn):
    try:
        fn()
        return 0
    except (eng.TapeError, tm.TapeError) as e:
        return e.code


def both(cells, nvar, nparm, edit, ndual=0):
    """(code of the C check in 64 bits, in 128 bits, of the model)"""
    return (code(lambda: eng.tape_check(cells, nvar, nparm, ndual, 64, edit=edit)),
            code(lambda: eng.tape_check(cells, nvar, nparm, ndual, 128, edit=edit)),
            code(lambda: te.check(cells, nvar, nparm, ndual, edit, 64)))


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_exported_and_declared(name):
    assert hasattr(eng.lib(), name)
    assert re.search(r"\b" + name + r"\(", open(HEADER).read())


def test_interface_version_and_flag_numbers():
    text = open(HEADER).read()
    assert eng.lib().pipamd_version() == eng.ABI_VERSION == 500
    for word, v in (("SHIFT", 1), ("NEGATE", 2), ("REMOVE", 4), ("DUAL", 8)):
        assert re.search(rf"#define PIPAMD_SOL_{word} {v}\b", text)
        assert getattr(eng, "SOL_" + word) == v == getattr(te, "SOL_" + word)
    assert C.sizeof(eng.TapeEdit) == 16 and C.sizeof(eng.TapeSetInfo) == 32


REFUSED = {
    "reserved": dict(sol_bg=1, urs_parms=1, sol_flags=5, reserved=1),
    "reserved alone": dict(sol_bg=0, urs_parms=0, sol_flags=0, reserved=7),
    "flag bit 4": dict(sol_bg=1, urs_parms=1, sol_flags=16),
    "negative flags": dict(sol_bg=1, urs_parms=1, sol_flags=-1),
    "urs_parms < 0": dict(sol_bg=1, urs_parms=-1, sol_flags=0),
    "sol_bg == nparm": dict(sol_bg=4, urs_parms=0, sol_flags=0),
    "sol_bg > nparm": dict(sol_bg=9, urs_parms=0, sol_flags=5),
    "SHIFT without a big parameter": dict(sol_bg=-1, urs_parms=0, sol_flags=1),
    "REMOVE without a big parameter": dict(sol_bg=-1, urs_parms=1, sol_flags=4),
    "MAX and REMOVE without a big parameter": dict(sol_bg=-7, urs_parms=0, sol_flags=7),
    "Urs copies beyond nparm": dict(sol_bg=1, urs_parms=2, sol_flags=0),       # first_urs 3, 3 + 2 > 4
    "Urs copies beyond nparm, no Bg": dict(sol_bg=-1, urs_parms=3, sol_flags=0),  # first_urs 3, 3 + 3 > 4
    "REMOVE of an Urs copy": dict(sol_bg=2, urs_parms=1, sol_flags=4),   # first_urs 2: the copy IS column 2
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_edits_that_are_refused(name):
    assert both(TAPE, NVAR, NPARM, REFUSED[name]) == (tm.E_INVALID,) * 3, name
    assert both([], NVAR, NPARM, REFUSED[name]) == (tm.E_INVALID,) * 3, name


def test_what_tape_check_refuses_stays_refused():
    edit = dict(sol_bg=1, urs_parms=1, sol_flags=7)
    assert both(TAPE, NVAR, NPARM, edit) == (0, 0, 0)
    assert both(TAPE[:-1], NVAR, NPARM, edit) == (tm.E_INVALID,) * 3
    assert both(TAPE, NVAR + 1, NPARM, edit) == (tm.E_INVALID,) * 3
    assert both(TAPE, NVAR, NPARM - 1, edit) == (tm.E_INVALID,) * 3   # the raw grammar: NEW(4) with 3 in scope
    assert both(TAPE, NVAR, -1, edit) == (tm.E_INVALID,) * 3
    # pipamd_pip_info has Bg - Nn - 1 in sol_bg: any negative value is "no big parameter"
    for bg in (-1, -2, -5, -(1 << 31)):
        assert both(TAPE, NVAR, NPARM, dict(sol_bg=bg, urs_parms=2, sol_flags=0)) == (0, 0, 0), bg


@pytest.mark.parametrize("bits", [64, 128])
def test_slots_and_words_count_kept_columns(bits):
    plain = eng.tape_check(TAPE, NVAR, NPARM, 0, bits)
    assert plain["slots"] == 6
    for edit, slots in ((dict(sol_bg=1, urs_parms=1, sol_flags=7), 4), (dict(sol_bg=1, urs_parms=1, sol_flags=1), 5),
                        (dict(sol_bg=-5, urs_parms=2, sol_flags=0), 4), (dict(sol_bg=1, urs_parms=0, sol_flags=7), 5),
                        (dict(sol_bg=0, urs_parms=0, sol_flags=8), 6)):
        info = eng.tape_check(TAPE, NVAR, NPARM, 0, bits, edit=edit)
        assert info == te.check(TAPE, NVAR, NPARM, 0, edit, bits), edit
        assert info["slots"] == slots and info["slots"] == te.point_cols(NPARM, edit) + 2, edit
        assert {k: info[k] for k in ("leaves", "ifs", "news", "depth")} == {k: plain[k] for k in ("leaves", "ifs", "news", "depth")}
        drop = plain["slots"] - slots
        assert info["words"] == plain["words"] - (bits // 64) * drop * 4   # a column less in each of the four forms


@pytest.mark.parametrize("bits", [64, 128])
def test_an_edit_of_zeros_is_no_edit(bits):
    g = tc.golden()
    for cells, nvar, nparm in ((tc.cells_from_text(g["tapes"]["int"]), g["nvar"], g["nparm"]), (TAPE, NVAR, NPARM),
                               ([], 3, 0), (tc.nil(), 0, 0)):
        want = eng.tape_check(cells, nvar, nparm, 0, bits)
        assert eng.tape_check(cells, nvar, nparm, 0, bits, edit=dict(sol_bg=0, urs_parms=0, sol_flags=0)) == want
    L = eng.lib()
    fn = L.pipamd_tape_check_pip128 if bits == 128 else L.pipamd_tape_check_pip
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    info, shape = eng.TapeInfo(), eng.TapeShape(NVAR, NPARM, 0, 0)
    assert fn(eng._cell_array(TAPE, bits), len(TAPE), C.byref(shape), None, C.byref(info)) == 0      # a null edit
    assert info.as_dict() == eng.tape_check(TAPE, NVAR, NPARM, 0, bits)
    assert fn(eng._cell_array(TAPE, bits), len(TAPE), C.byref(shape), None, None) == 0               # info is optional
    assert fn(None, 3, C.byref(shape), None, C.byref(info)) == tm.E_INVALID
    assert fn(None, 0, None, None, C.byref(info)) == tm.E_INVALID


def test_slot_limit_counts_kept_columns():
    """33 raw parameters, one of them the big one: 32 kept with SOL_REMOVE (33 slots: too many), 31 kept with an Urs
    copy dropped as well (32 slots: the limit)"""
    for bits in (64, 128):
        cells = tc.leaf([([1] * 34, 1)])
        assert code(lambda: eng.tape_check(cells, 1, 33, 0, bits)) == tm.E_TOOLARGE
        assert both(cells, 1, 33, dict(sol_bg=0, urs_parms=0, sol_flags=7)) == (tm.E_TOOLARGE,) * 3
        edit = dict(sol_bg=0, urs_parms=1, sol_flags=7)
        assert both(cells, 1, 33, edit) == (0, 0, 0)
        assert eng.tape_check(cells, 1, 33, 0, bits, edit=edit)["slots"] == 32
    # new parameters count too: 31 kept parameters and one new one are 33 slots
    cells = tc.new(33, [0] * 34, 1, tc.leaf([([1] * 35, 1)]))
    assert both(cells, 1, 33, dict(sol_bg=0, urs_parms=1, sol_flags=7)) == (tm.E_TOOLARGE,) * 3
    assert both(cells, 1, 33, dict(sol_bg=0, urs_parms=2, sol_flags=7)) == (0, 0, 0)


def test_shifted_coefficient_that_leaves_the_cell_type():
    for bits, lo in ((64, tc.MIN64), (128, tc.MIN128)):
        cells = tc.leaf([([lo, 0], 1)])
        edit = dict(sol_bg=0, urs_parms=0, sol_flags=1)
        assert code(lambda: eng.tape_check(cells, 1, 1, 0, bits, edit=edit)) == tm.E_TOOLARGE
        assert code(lambda: te.check(cells, 1, 1, 0, edit, bits)) == tm.E_TOOLARGE
        ok = tc.leaf([([lo + 1, 0], 1)])
        assert code(lambda: eng.tape_check(ok, 1, 1, 0, bits, edit=edit)) == 0 == code(lambda: te.check(ok, 1, 1, 0, edit, bits))
        # conditions and new-parameter forms are not shifted
        cond = tc.iff([lo, 0], tc.nil(), tc.nil())
        assert code(lambda: eng.tape_check(cond, 1, 1, 0, bits, edit=edit)) == 0
    # int64 cells are held to int64 even though the walk computes wider
    assert code(lambda: eng.tape_check(tc.leaf([([tc.MIN64, 0], 1)]), 1, 1, 0, 128, edit=dict(sol_bg=0, sol_flags=1))) == 0


def test_null_arguments_before_any_hip_call():
    L = eng.lib()
    shape, edit, out = eng.TapeShape(1, 1, 0, 0), eng.TapeEdit(0, 0, 1, 0), C.c_void_p()
    for name, bits in (("pipamd_tape_compile_pip", 64), ("pipamd_tape_compile_pip128", 128)):
        fn = getattr(L, name)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        arr = eng._cell_array(tc.nil(), bits)
        assert fn(None, arr, 1, C.byref(shape), C.byref(edit), C.byref(out)) == tm.E_INVALID and not out.value
        assert b"null engine" in L.pipamd_last_error()
    L.pipamd_tape_point_cols.argtypes = [C.c_void_p]
    assert L.pipamd_tape_point_cols(None) == tm.E_INVALID
    L.pipamd_tape_set_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    info = eng.TapeSetInfo()
    tapes = (C.c_void_p * 1)()
    out.value = 5
    assert L.pipamd_tape_set_create(None, 1, tapes, C.byref(out), C.byref(info)) == tm.E_INVALID and not out.value
    assert L.pipamd_tape_set_create(None, 1, tapes, None, None) == tm.E_INVALID
    L.pipamd_tape_set_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 9
    assert L.pipamd_tape_set_eval(None, None, 4, *[None] * 9) == tm.E_INVALID
    L.pipamd_tape_set_free.argtypes = [C.c_void_p]
    L.pipamd_tape_set_free(None)


def test_python_binding_is_there():
    assert hasattr(eng, "TapeSet") and hasattr(eng, "TapeEdit")
    import inspect
    assert "edit" in inspect.signature(eng.Tape.__init__).parameters
    assert "edit" in inspect.signature(eng.tape_check).parameters
