"""The ragged family r5 of tests/matrices_cases.py held to the reference, as tests/test_system_model.py holds the uniform
families: the model's tableau of every system -- system_model.tableau on its kept rows and its own equalities, simplified
for the integer cases as pip_solve does -- goes through the CPU oracle, and for every system of every case of
tests/golden/matrices/r5.json (made by tests/golden/make_matrices_fixtures.py from the reference's pip_solve) the decoded
answer equals the printed list, the pivot count equals the reference's, and the model's reduction and merge of the
oracle's tableau-level dual values equal the printed dual.  No system is left out.  Host only."""
import functools
import json
import os

import pytest

import matrices_cases as mc
import pipbatch as pb
import shift_cases as sc
import shift_model as sm
import system_model as sy
from gpu_common import oracle_batch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matrices", "r5.json")


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _oracle(box, shift, nq, simp):
    """the oracle's result per system of the batch, run class by class (a class's tableaux have one shape)"""
    fam = mc.family("r5", box)
    res = [None] * len(fam.systems)
    for c, (kept, eq) in enumerate(fam.classes):
        tab = mc.tableaux(fam, c, shift, simp)
        assert tab.shape == (len(mc.members(fam, c)), len(kept) + len(eq), fam.nvar + (2 if shift else 1))
        out = oracle_batch(tab, fam.nvar, 1 if shift else 0, nq, bigparm=fam.nvar + 1 if shift else -1).results
        for b, r in zip(mc.members(fam, c), out):
            res[b] = r
    assert all(r is not None for r in res)
    return res


def _answer(r, shift):
    """the oracle's tableau-level text -> pip_solve's list of [numerator, denominator], None for "()" """
    if shift:
        f = sc.forms(r.text)
        return None if f is None else [list(sm.decode(b, c, d, shift)) for b, c, d in f]
    lists = sy.parse_lists(r.text)
    return [list(sy.reduce_pair(n, d)) for n, d in lists[0]] if lists else None


def test_fixture_is_of_this_family():
    g = _golden()
    seed, nvar, n, batch, kw, _, pseed, boxes = mc.FAMILIES["r5"]
    assert (g["seed"], g["nvar"], g["n"], g["batch"], g["kw"], g["perm_seed"]) == (seed, nvar, n, batch, kw, pseed)
    for box in boxes:
        fam = mc.family("r5", box)
        assert g["classes"][str(box)] == [[list(kept), list(eq)] for kept, eq in fam.classes]
        assert g["cls"][str(box)] == fam.cls.tolist()
        assert fam.max_rows == (13 if box else 8) and fam.ni == (14 if box else 10)
        # every word beyond a system's rows is junk, every marker is 0 or 1
        for b, (rows, eq) in enumerate(fam.systems):
            assert (fam.room[b, fam.nrows[b]:] == mc.JUNK).all()
            assert [int(m == 0) for m in fam.room[b, :fam.nrows[b], 0]] == [int(r in eq) for r in range(len(rows))]
        # the classes the family is there for
        shapes = [(len(kept), tuple(eq)) for kept, eq in fam.classes]
        assert (1, ()) in shapes and (1, (0,)) in shapes and (fam.max_rows, ()) in shapes and (fam.max_rows, (fam.max_rows - 1,)) in shapes
        assert any(len(eq) == k and 2 * k == fam.ni for k, eq in shapes)
        assert min(len(mc.members(fam, c)) for c in range(len(fam.classes))) >= 3


@pytest.mark.parametrize("box", [0, 1])
@pytest.mark.parametrize("opts", list(sy.OPTIONS))
def test_model_equals_reference(box, opts):
    fam = mc.family("r5", box)
    shift, nq, dual = sy.OPTIONS[opts]
    want = _golden()["cases"][f"box{box},{opts}"]
    assert len(want["x"]) == len(want["pivots"]) == len(want["dual"]) == len(fam.systems)
    solved = 0
    for k, r in enumerate(_oracle(box, shift, nq, nq)):  # integer cases simplified, as pip_solve does
        rows, eq = fam.systems[k]
        assert r.status == pb.ST_OK, (k, r.status, r.abort_code)
        got = _answer(r, shift)
        assert got == want["x"][k], (k, got, want["x"][k])
        assert r.pivots == want["pivots"][k], (k, r.pivots, want["pivots"][k])
        solved += got is not None
        if dual:
            t = sy.oracle_tableau_dual(rows, eq, opts)
            assert (t is None) == (got is None), k
            d = None if t is None else [list(p) for p in sy.dual(t, len(rows), eq)]
            assert d == want["dual"][k], (k, d, want["dual"][k])
        else:
            assert want["dual"][k] is None
    assert solved >= 6
