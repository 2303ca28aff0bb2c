"""The host side of the tape evaluator (pipamd_tape_check / _check128, and the refusals of pipamd_tape_compile /
pipamd_tape_eval that come before any HIP call), held to tests/tape_model.py: the golden tapes are accepted in both widths
with the model's counts, every way a tape can be malformed is refused as the model refuses it, the slot limit holds at its
edge.  Host only: no engine, no GPU."""
import ctypes as C

import pytest

import tape_cases as tc
import tape_model as tm
from piplib_amd import engine as eng
from tape_model import DIV, FORM, IF, LIST, NEW, NIL, VAL

FORMS = [([2, 3, 1], 4), ([0, 1, 0], 1)]  # two unknowns over theta_0 and one new parameter
DUALS = [(1, 2), (0, 1)]
NVAR, NPARM, NDUAL = 2, 1, 2


def base(forms=FORMS, duals=DUALS, cond=([1, 0, -1], 1), new=(1, [1, 0], 2)):
    """newparm 1 = floor(theta_0 / 2); if theta_0 - 1 >= 0: the list and its dual list, else ()"""
    return tc.new(new[0], new[1], new[2], tc.iff(cond[0], tc.leaf(forms, duals), tc.nil(), cond[1]))


def swap(cells, at, cell):
    return cells[:at] + [cell] + cells[at + 1:]


def find(cells, kind, nth=0):
    return [k for k, c in enumerate(cells) if c[0] == kind][nth]


def both(cells, nvar=NVAR, nparm=NPARM, ndual=NDUAL, reserved=0):
    """(code of the C check in 64 bits, in 128 bits, of the model): 0 where the tape is accepted"""
    out = []
    for fn in (lambda: eng.tape_check(cells, nvar, nparm, ndual, 64, reserved),
               lambda: eng.tape_check(cells, nvar, nparm, ndual, 128, reserved),
               lambda: tm.check(cells, nvar, nparm, ndual, 64, reserved)):
        try:
            fn()
            out.append(0)
        except (eng.TapeError, tm.TapeError) as e:
            out.append(e.code)
    return tuple(out)


@pytest.mark.parametrize("bits", [64, 128])
def test_golden_tapes_are_accepted_with_the_models_counts(bits):
    g = tc.golden()
    for name in ("int", "rat"):
        cells = tc.cells_from_text(g["tapes"][name])
        info = eng.tape_check(cells, g["nvar"], g["nparm"], 0, bits)
        assert info == tm.check(cells, g["nvar"], g["nparm"], 0, bits)
        assert info["leaves"] >= 6 and info["ifs"] >= 5 and info["staged"] == 1
    assert eng.tape_check(tc.cells_from_text(g["tapes"]["int"]), g["nvar"], g["nparm"])["news"] >= 1
    cells = base()
    assert both(cells) == (0, 0, 0)
    assert eng.tape_check(cells, NVAR, NPARM, NDUAL, bits) == tm.check(cells, NVAR, NPARM, NDUAL, bits)


def test_empty_tape_is_accepted():
    for bits in (64, 128):
        assert eng.tape_check([], 3, 2, 1, bits) == tm.check([], 3, 2, 1, bits)
    assert eng.tape_check([], 0, 0)["slots"] == 1


B = base()
MALFORMED = {
    "unknown kind": swap(B, find(B, IF), (9, 0, 0)),
    "kind 0": swap(B, find(B, NIL), (0, 0, 0)),
    "a value where an item belongs": swap(B, find(B, NIL), (VAL, 1, 1)),
    "truncated: the last item": B[:-1],
    "truncated: inside a form": B[:find(B, LIST) + 3],
    "truncated: the divisor": B[:find(B, VAL, 2)],
    "cells behind the root item": B + tc.nil(),
    "condition of P values": base(cond=([1, -1], 1)),
    "condition of P + 2 values": base(cond=([1, 0, 0, -1], 1)),
    "unknown of P values": base(forms=[([2, 1], 4), FORMS[1]]),
    "div form of P + 2 values": base(new=(1, [1, 0, 0], 2)),
    "dual form of two values": swap(B, find(B, FORM, -1), (FORM, 2, 0)),
    "list of nvar + 1": base(forms=FORMS + [FORMS[1]]),
    "list of nvar - 1": base(forms=FORMS[:1]),
    "dual list of ndual - 1": base(duals=DUALS[:1]),
    "dual list of ndual + 1": base(duals=DUALS + [(1, 1)]),
    "no dual list": base(duals=None),
    "newparm P + 1": base(new=(2, [1, 0], 2)),
    "newparm P - 1": base(new=(0, [1, 0], 2)),
    "denominator 0 in a condition": base(cond=([1, 0, -1], 0)),
    "denominator -1 in an unknown": base(forms=[([2, 3, 1], -1), FORMS[1]]),
    "denominator 0 in the dual list": base(duals=[(1, 0), (0, 1)]),
    "unequal denominators": swap(B, find(B, VAL, 5), (VAL, 0, 3)),
    "div form over 2": swap(B, find(B, VAL, 0), (VAL, 1, 2)),
    "divisor over 2": swap(B, find(B, VAL, 2), (VAL, 2, 2)),
    "divisor 0": base(new=(1, [1, 0], 0)),
    "divisor -2": base(new=(1, [1, 0], -2)),
    "no div behind the newparm": swap(B, find(B, DIV), (IF, 0, 0)),
}


@pytest.mark.parametrize("name", list(MALFORMED))
def test_malformed_tapes_are_refused_as_the_model_refuses_them(name):
    assert both(MALFORMED[name]) == (tm.E_INVALID,) * 3, name


def test_second_list_without_duals_and_bad_shapes():
    forms = [([2, 1], 4), ([1, 0], 1)]  # the root's P is nparm
    one = tc.leaf(forms, DUALS)
    assert both(one) == (0, 0, 0)
    assert both(one, ndual=0) == (tm.E_INVALID,) * 3        # a second LIST when ndual == 0: cells behind the root item
    assert both(tc.leaf(forms), ndual=0) == (0, 0, 0)
    assert both(B, reserved=1) == (tm.E_INVALID,) * 3
    for shape in ((-1, NPARM, NDUAL), (NVAR, -1, NDUAL), (NVAR, NPARM, -1)):
        assert both(B, *shape) == (tm.E_INVALID,) * 3, shape
        assert both([], *shape) == (tm.E_INVALID,) * 3, shape


def test_null_pointers():
    L = eng.lib()
    shape, info = eng.TapeShape(1, 1, 0, 0), eng.TapeInfo()
    arr = eng._cell_array(tc.nil(), 64)
    for name in ("pipamd_tape_check", "pipamd_tape_check128"):
        fn = getattr(L, name)
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        assert fn(None, 3, C.byref(shape), C.byref(info)) == tm.E_INVALID      # null cells with n_cells > 0
        assert fn(None, 0, None, C.byref(info)) == tm.E_INVALID                # null shape
        assert fn(None, 0, C.byref(shape), None) == 0                          # info is optional
    assert L.pipamd_tape_check(arr, 1, C.byref(shape), C.byref(info)) == 0 and info.leaves == 1 and info.words == 1


def test_slot_limit_at_its_edge():
    assert tm.MAX_SLOTS == 32
    for bits in (64, 128):
        info = eng.tape_check(tc.new_chain(1, 30), 2, 1, 0, bits)
        assert info == tm.check(tc.new_chain(1, 30), 2, 1, 0, bits) and info["slots"] == 32
        # 31 rows of 128 x 16 bytes leave 2 KB of the LDS budget: the 128-bit program is read from global memory
        assert info["staged"] == (1 if bits == 64 else 0)
        with pytest.raises(eng.TapeError) as e:
            eng.tape_check(tc.new_chain(1, 31), 2, 1, 0, bits)
        assert e.value.code == tm.E_TOOLARGE
        assert eng.tape_check(tc.nil(), 0, 31, 0, bits)["slots"] == 32   # the point's own parameters count
        with pytest.raises(eng.TapeError) as e:
            eng.tape_check(tc.nil(), 0, 32, 0, bits)
        assert e.value.code == tm.E_TOOLARGE
    assert both(tc.new_chain(1, 31), 2, 1, 0) == (tm.E_TOOLARGE,) * 3
    # an invalid tape stays invalid however many slots it has
    assert both(tc.new_chain(1, 31)[:-1], 2, 1, 0) == (tm.E_INVALID,) * 3


def test_program_leaves_lds_where_the_header_says():
    """a chain of k conditions over one parameter has 4 k + 4 words; with the one slot row of 128 x 8 bytes the program
    fits PIPAMD_TAPE_LDS_BYTES up to k = 2015 (8064 words) and is read from global memory from k = 2016 on"""
    for k, staged in ((2015, 1), (2016, 0)):
        cells = tc.if_chain(k)
        info = eng.tape_check(cells, 1, 1)
        assert info == tm.check(cells, 1, 1) and info["words"] == 4 * k + 4 and info["staged"] == staged
        assert info["depth"] == k + 1 and info["leaves"] == k + 1
    assert 8 * 8064 + tm.slot_bytes(2, 64) == tm.LDS_BYTES == 65536
    assert eng.tape_check(tc.if_chain(2015), 1, 1, 0, 128)["staged"] == 0  # twice the words, twice the slot bytes


def test_compile_and_eval_refuse_null_handles_before_any_hip_call():
    L = eng.lib()
    shape = eng.TapeShape(1, 1, 0, 0)
    out = C.c_void_p()
    for name, bits in (("pipamd_tape_compile", 64), ("pipamd_tape_compile128", 128)):
        fn = getattr(L, name)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        arr = eng._cell_array(tc.nil(), bits)
        assert fn(None, arr, 1, C.byref(shape), C.byref(out)) == tm.E_INVALID and not out.value
        assert b"null engine" in L.pipamd_last_error()
    L.pipamd_tape_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 8
    assert L.pipamd_tape_eval(None, None, 4, None, None, None, None, None, None, None, None) == tm.E_INVALID
    L.pipamd_tape_free.argtypes = [C.c_void_p]
    L.pipamd_tape_free(None)
