"""tests/system_model.py held to the reference: its tableau for a plain system with equalities -- expansion, shift,
tab_simplify for the integer cases, as pip_solve does it -- goes through the CPU oracle, and for every system of every
case of tests/golden/system/ (made by tests/golden/make_system_fixtures.py from the reference's pip_solve) the decoded
answer equals the printed list, the pivot count equals the reference's -- which is what pins tab_simplify and the row
order of the expansion, the answers alone do not depend on them -- and the model's reduction and merge of the oracle's
tableau-level dual values equal the printed dual.  Host only."""
import functools

import pytest

import pipbatch as pb
import shift_cases as sc
import shift_model as sm
import system_model as sy
from gpu_common import oracle_batch

FAMILIES = ["s5", "s12"]


@functools.lru_cache(maxsize=None)
def _oracle(name, box, shift, nq, simp):
    g = sy.golden(name)
    rows = sy.family_rows(g, box)
    tab = sy.tableaux(rows, sy.EQ_ROWS[name], shift, simp)
    assert tab.shape == (g["batch"], rows.shape[1] + len(sy.EQ_ROWS[name]), g["nvar"] + (2 if shift else 1))
    return oracle_batch(tab, g["nvar"], 1 if shift else 0, nq, bigparm=g["nvar"] + 1 if shift else -1).results


def _answer(r, shift):
    """the oracle's tableau-level text -> pip_solve's list of [numerator, denominator], None for "()" """
    if shift:
        f = sc.forms(r.text)
        return None if f is None else [list(sm.decode(b, c, d, shift)) for b, c, d in f]
    lists = sy.parse_lists(r.text)
    return [list(sy.reduce_pair(n, d)) for n, d in lists[0]] if lists else None


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("box", [0, 1])
@pytest.mark.parametrize("opts", list(sy.OPTIONS))
def test_model_equals_reference(name, box, opts):
    g = sy.golden(name)
    shift, nq, dual = sy.OPTIONS[opts]
    want = g["cases"][f"box{box},{opts}"]
    assert tuple(g["eq_rows"]) == sy.EQ_ROWS[name] and len(want["x"]) == len(want["pivots"]) == g["batch"]
    rows = sy.family_rows(g, box)
    nrows = rows.shape[1]
    solved = 0
    for k, r in enumerate(_oracle(name, box, shift, nq, nq)):  # integer cases simplified, as pip_solve does
        assert r.status == pb.ST_OK, (k, r.status, r.abort_code)
        got = _answer(r, shift)
        assert got == want["x"][k], (k, got, want["x"][k])
        assert r.pivots == want["pivots"][k], (k, r.pivots, want["pivots"][k])
        solved += got is not None
        if dual:
            t = sy.oracle_tableau_dual(rows[k], sy.EQ_ROWS[name], opts)
            assert (t is None) == (got is None), k
            d = None if t is None else [list(p) for p in sy.dual(t, nrows, sy.EQ_ROWS[name])]
            assert d == want["dual"][k], (k, d, want["dual"][k])
        else:
            assert want["dual"][k] is None
    assert solved >= 6


@pytest.mark.parametrize("name", FAMILIES)
def test_simplify_shows_in_the_pivot_counts(name):
    """without tab_simplify the integer cases take another number of pivots: the equality of the counts above holds
    the model's simplify to the reference's"""
    g = sy.golden(name)
    with_, without = 0, 0
    for box in (0, 1):
        for opts, (shift, nq, dual) in sy.OPTIONS.items():
            if nq:
                with_ += sum(g["cases"][f"box{box},{opts}"]["pivots"])
                without += sum(r.pivots for r in _oracle(name, box, shift, 1, 0))
    assert with_ != without, (with_, without)


def test_model_by_hand():
    rows = [[2, -4, 7], [3, 6, -5]]
    assert sy.expand(rows, (1,), 0) == [[2, -4, 7], [3, 6, -5], [-3, -6, 5]]
    assert sy.expand(rows, (0,), sm.SHIFT_MAX) == [[-2, 4, 7, -2], [2, -4, -7, 2], [-3, -6, -5, 9]]
    assert sy.expand(rows, (1,), sm.SHIFT_URS) == [[2, -4, 7, 2], [3, 6, -5, -9], [-3, -6, 5, 9]]
    # the gcd leaves the constant out and takes the big column in; the constant is divided with the floor
    assert sy.simplify([[2, -4, 7], [3, 6, -5], [-3, -6, 5], [0, 0, 3], [4, 6, 1, 3]], 2) == \
        [[1, -2, 3], [1, 2, -2], [-1, -2, 1], [0, 0, 3], [4, 6, 1, 3]]
    assert sy.simplify([[-2, 4, 7, -2], [2, -4, -7, 2]], 2) == [[-1, 2, 3, -1], [1, -2, -4, 1]]
    assert sy.reduce_pair(6, 4) == (3, 2) and sy.reduce_pair(0, 5) == (0, 1) and sy.reduce_pair(-6, 3) == (-2, 1)
    # rows 0 and 2 are equalities: u where it is not zero, else -v
    assert sy.dual([(2, 4), (0, 1), (5, 1), (0, 1), (3, 6)], 3, (0, 2)) == [(1, 2), (5, 1), (-1, 2)]
