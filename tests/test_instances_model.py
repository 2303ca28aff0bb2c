"""tests/instances_model.py held to the reference: its expansion of the golden family p5 -- one parametric system at 8
parameter points --, through tests/system_model.py's tableau (equalities expanded, shift, tab_simplify for the integer
cases, as pip_solve does it) and the CPU oracle, reproduces for every point and every option string what the reference's
pip_solve printed for that instance (tests/golden/instances/p5.json, made by tests/golden/make_instances_fixtures.py):
the answer, the dual and the pivot count.  The edge systems' constants are what their names say.  Host only."""
import functools

import numpy as np
import pytest

import instances_model as im
import pipbatch as pb
import shift_cases as sc
import shift_model as sm
import system_model as sy
from gpu_common import oracle_batch


@functools.lru_cache(maxsize=None)
def _rows():
    g = im.golden()
    rows = np.array(im.expand(g["matrix"], g["points"]), dtype=np.int64)
    assert rows.shape == (8, 7, g["nvar"] + 1) and g["nvar"] == 5 and g["nparm"] == 2 and len(g["eq_rows"]) == 2
    return rows


def _answer(r, shift):
    if shift:
        f = sc.forms(r.text)
        return None if f is None else [list(sm.decode(b, c, d, shift)) for b, c, d in f]
    lists = sy.parse_lists(r.text)
    return [list(sy.reduce_pair(n, d)) for n, d in lists[0]] if lists else None


@pytest.mark.parametrize("opts", list(sy.OPTIONS))
def test_model_equals_reference(opts):
    g = im.golden()
    shift, nq, dual = sy.OPTIONS[opts]
    want = g["cases"][opts]
    rows, nvar, eq = _rows(), g["nvar"], tuple(g["eq_rows"])
    assert len(want["x"]) == len(want["pivots"]) == len(want["dual"]) == len(rows)
    tab = sy.tableaux(rows, eq, shift, nq)  # integer cases simplified, as pip_solve does
    res = oracle_batch(tab, nvar, 1 if shift else 0, nq, bigparm=nvar + 1 if shift else -1).results
    solved = 0
    for k, r in enumerate(res):
        assert r.status == pb.ST_OK, (k, r.status, r.abort_code)
        got = _answer(r, shift)
        assert got == want["x"][k], (k, got, want["x"][k])
        assert r.pivots == want["pivots"][k], (k, r.pivots, want["pivots"][k])
        solved += got is not None
        if dual:
            t = sy.oracle_tableau_dual(rows[k], eq, opts)
            assert (t is None) == (got is None), k
            d = None if t is None else [list(p) for p in sy.dual(t, rows.shape[1], eq)]
            assert d == want["dual"][k], (k, d, want["dual"][k])
        else:
            assert want["dual"][k] is None
    assert solved >= 3 and (shift or solved <= len(rows) - 2)  # some points make the system infeasible


def test_expand_by_hand():
    m = [[2, -4, 3, -1, 7], [0, 5, 0, 0, -6]]
    assert im.expand(m, [[0, 0], [10, 4], [-1, 1 << 63]]) == \
        [[[2, -4, 7], [0, 5, -6]], [[2, -4, 33], [0, 5, -6]], [[2, -4, 4 - (1 << 63)], [0, 5, -6]]]
    assert im.expand([[1, 2, 3], [4, 5, 6]], [[], []]) == [[[1, 2, 3], [4, 5, 6]]] * 2  # no parameters
    assert im.fits([[[1, (1 << 63) - 1]], [[1, 1 << 63]], [[5, 0], [1, -(1 << 63) - 1]]], 64) == [True, False, False]
    assert im.fits([[[1, 1 << 63]], [[1, (1 << 127) - 1], [0, -(1 << 127)]], [[1, 1 << 127]]], 128) == [True, True, False]


@pytest.mark.parametrize("bits", [64, 128])
def test_edge_cases_are_what_they_say(bits):
    """every kind of edge row as the first and as the last row; good and bad systems in both widths, a bad system before
    and after a good one"""
    matrix, points, nvar, names = im.edge_cases(bits)
    rows = im.expand(matrix, points)
    ok = dict(zip(names, im.fits(rows, bits)))
    assert len(names) == len(points) == 23 and ok["benign"]
    good64 = {"max64", "min64", "cancel"}
    good128 = good64 | {"max64+1", "min64-1", "2^64+3", "max128", "min128"}
    for name, fit in ok.items():
        if name != "benign":
            assert fit == (name.split(",")[0] in (good64 if bits == 64 else good128)), name
    assert set(n.split(",")[0] for n in names) - {"benign"} == set(im.EDGE_ROWS)
    fit = im.fits(rows, bits)
    assert fit[0] and fit[-1] and any(a and not b for a, b in zip(fit, fit[1:])) and any(b and not a for a, b in zip(fit, fit[1:]))
