"""tests/tape_model.py held to the reference: the tape the reference printed for the parametric problem p5, and the tape
the CPU oracle makes of it, walked in Python ints at every point of tests/golden/tape_eval/p5_grid.json, give what the
reference's pip_solve printed for that point's instance as a plain system; the oracle's tape gives the answers of
tests/golden/instances/p5.json too (points with a negative parameter among them).  The validator, the checked order of the
128-bit flavour and the text reader on hand-made tapes.  Host only."""
import functools

import numpy as np
import pytest

import instances_model as im
import pipbatch as pb
import tape_cases as tc
import tape_model as tm
from piplib_amd import engine as eng

FLAVOURS = {"int": 1, "rat": 0}  # name -> nq


@functools.lru_cache(maxsize=None)
def _oracle_cells(nq):
    g = tc.golden()
    tab = tc.parametric_tableau(g["matrix"], g["nvar"], g["nparm"], g["eq_rows"])
    prob = pb.Problem(g["nvar"], g["nparm"], tab.shape[0], 0, -1, nq, tab, np.zeros((0, g["nparm"] + 1), np.int64))
    r = pb.run_batch(pb.ORACLEPIP, [prob]).results[0]
    assert r.status == pb.ST_OK, (r.status, r.abort_code)
    return tuple(tc.cells_from_text(r.text))


def test_fixture_is_what_its_generator_promises():
    g = tc.golden()
    assert g["points"][:100] == [[n, m] for n in range(10) for m in range(10)]
    assert g["matrix"] == im.golden()["matrix"] and g["eq_rows"] == im.golden()["eq_rows"]
    for name in FLAVOURS:
        assert len(g["answers"][name]) == len(g["points"])
        assert sum(x is None for x in g["answers"][name]) >= 8
    assert sum(x is not None and any(d != 1 for _, d in x) for x in g["answers"]["rat"]) >= 20


@pytest.mark.parametrize("name", list(FLAVOURS))
@pytest.mark.parametrize("bits", [64, 128])
def test_reference_tape_walked_equals_reference_answers(name, bits):
    g = tc.golden()
    cells = tc.cells_from_text(g["tapes"][name])
    trace = {}
    got = tm.evaluate_cells(cells, g["nvar"], g["nparm"], 0, g["points"], bits, trace)
    assert tc.answers_of(got) == g["answers"][name]
    assert all(st in (tm.ST_SOLUTION, tm.ST_NIL) for st, _, _, _ in got)  # "()" is NIL, nothing leaves the range
    assert len(set(leaf for _, leaf, _, _ in got)) >= 6 and trace["zeros"] >= 1
    if name == "int":
        assert trace["news"] >= 20


@pytest.mark.parametrize("name", list(FLAVOURS))
def test_oracle_tape_walked_equals_reference_answers(name):
    g = tc.golden()
    got = tm.evaluate_cells(_oracle_cells(FLAVOURS[name]), g["nvar"], g["nparm"], 0, g["points"])
    assert tc.answers_of(got) == g["answers"][name]


@pytest.mark.parametrize("opts,nq", [("", 1), ("Rational+Dual", 0)])
def test_oracle_tape_walked_equals_instances_fixture(opts, nq):
    g = im.golden()
    got = tm.evaluate_cells(_oracle_cells(nq), g["nvar"], g["nparm"], 0, g["points"])
    assert tc.answers_of(got) == g["cases"][opts]["x"]


def test_text_reader_inverts_the_printer():
    g = tc.golden()
    for name in FLAVOURS:
        cells = tc.cells_from_text(g["tapes"][name])
        assert pb.squash(eng.tape_text(cells)) == pb.squash(g["tapes"][name])
        tm.check(cells, g["nvar"], g["nparm"])
    assert tc.cells_from_text("void\n") == []
    # every value is printed reduced on its own; the reader puts a form back over one denominator
    cells = tc.leaf([([3, 2, 1], 6)])
    assert pb.squash(eng.tape_text(cells)) == "(list#[1/21/31/6])"
    assert tc.cells_from_text(eng.tape_text(cells)) == cells


def test_hand_made_tapes():
    ev = lambda cells, nvar, nparm, point, bits=64, ndual=0: tm.evaluate_cells(cells, nvar, nparm, ndual, [point], bits)[0]
    # a true floor: (-1) / 2 -> -1, (-4) / 2 -> -2, 3 / 2 -> 1
    t = tc.new(1, [1, 0], 2, tc.leaf([([0, 1, 0], 1)]))
    assert [ev(t, 1, 1, [v])[2] for v in (-1, -4, 3)] == [[(-1, 1)], [(-2, 1)], [(1, 1)]]
    # a condition of exactly 0 takes the first item
    t = tc.iff([1, -5], tc.leaf([([0, 7], 1)]), tc.nil())
    assert [ev(t, 1, 1, [v])[:2] for v in (4, 5, 6)] == [(tm.ST_NIL, 1), (tm.ST_SOLUTION, 0), (tm.ST_SOLUTION, 0)]
    # lowest terms, N == 0, and a numerator that fits only after the division by the gcd
    t = tc.leaf([([6, 0], 4), ([0, 0], 7), ([1 << 62, 0], 4)])
    assert ev(t, 3, 1, [3])[2] == [(9, 2), (0, 1), (3 << 60, 1)]
    assert ev(t, 3, 1, [4])[2] == [(6, 1), (0, 1), (1 << 62, 1)]
    assert ev(t, 3, 1, [7])[0] == tm.ST_SOLUTION and ev(t, 3, 1, [9])[0] == tm.ST_RANGE  # 9 * 2^60 leaves int64
    assert ev(t, 3, 1, [9], 128)[2][2] == (9 << 60, 1)
    # products that each leave int64 while the sum fits (64: exact; 128: nothing leaves 128 bits either)
    t = tc.leaf([([1 << 62, -(1 << 62), 5], 1)])
    assert ev(t, 1, 2, [4, 4])[2] == [(5, 1)] and ev(t, 1, 2, [4, 4], 128)[2] == [(5, 1)]
    # the edges of int64: 2^63 - 1 and -2^63 are answers, 2^63 is not
    t = tc.leaf([([1, 1], 1)])
    assert ev(t, 1, 1, [tc.MAX64 - 1])[2] == [(tc.MAX64, 1)] and ev(t, 1, 1, [tc.MAX64])[:2] == (tm.ST_RANGE, -1)
    assert ev(tc.leaf([([1, -1], 1)]), 1, 1, [tc.MIN64 + 1])[2] == [(tc.MIN64, 1)]
    assert ev(tc.leaf([([1, -1], 1)]), 1, 1, [tc.MIN64])[0] == tm.ST_RANGE
    # a new parameter that leaves int64; in 128 bits it is a value like any other
    t = tc.new(1, [2, 0], 1, tc.leaf([([0, 1, 0], 2)]))
    assert ev(t, 1, 1, [1 << 62])[0] == tm.ST_RANGE and ev(t, 1, 1, [1 << 62], 128)[2] == [(1 << 62, 1)]
    # 128 bits, checked in cell order: a product that leaves them; a running sum that does while the total would fit
    t = tc.leaf([([1 << 100, 0], 1)])
    assert ev(t, 1, 1, [1 << 26], 128)[2] == [(1 << 126, 1)] and ev(t, 1, 1, [1 << 27], 128)[0] == tm.ST_RANGE
    t = tc.leaf([([1 << 64, 1 << 64, -(1 << 64), 0], 1)])
    assert ev(t, 1, 3, [1 << 62, 1 << 62, 1 << 62], 128)[0] == tm.ST_RANGE   # 2^126 + 2^126 leaves them first
    assert ev(t, 1, 3, [1 << 62, -(1 << 62), 1 << 62], 128)[2] == [(-(1 << 126), 1)]
    # the dual list: constants in lowest terms; the empty tape
    t = tc.leaf([([1, 0], 1)], duals=[(4, 6), (0, 5), (-3, 3)])
    assert ev(t, 1, 1, [2], ndual=3)[3] == [(2, 3), (0, 1), (-1, 1)]
    assert ev([], 2, 1, [0], ndual=1) == (tm.ST_NIL, -1, [(0, 0)] * 2, [(0, 0)])


def test_validator_counts_and_refuses():
    info = tm.check(tc.if_chain(3), 1, 1)
    assert info == {"leaves": 4, "ifs": 3, "news": 0, "words": 3 * (1 + 2 + 1) + 1 + 3, "slots": 2, "depth": 4, "staged": 1}
    info = tm.check(tc.new_chain(1, 30), 2, 1)
    assert info["slots"] == tm.MAX_SLOTS and info["news"] == 30 and info["depth"] == 31
    with pytest.raises(tm.TapeError) as e:
        tm.check(tc.new_chain(1, 31), 2, 1)
    assert e.value.code == tm.E_TOOLARGE
    assert tm.check([], 3, 2) == {"leaves": 0, "ifs": 0, "news": 0, "words": 0, "slots": 3, "depth": 0, "staged": 0}
    # the program of the 128-bit flavour has two words per value
    assert tm.check(tc.if_chain(3), 1, 1, bits=128)["words"] == 3 * (1 + 4 + 1) + 1 + 6
