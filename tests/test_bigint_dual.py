"""tests/bigint_dual.py (the Python-int authority of tests/test_gpu_batch_dual.py) held to figures computed once on the
CPU: a test that quietly compared nothing against it could not pass there.  Host only, no GPU."""
import pytest

import bigint_dual as bd
import bigint_pip as bp

# family: (solutions, tableaux with a non-zero dual value, max_bits over the compared tableaux)
FIGURES = {"lexmin12": (64, 27, 25), "lexmin64": (32, 28, 43), "lexmin65": (32, 29, 40), "lexmin130": (32, 28, 37),
           "dense20": (32, 27, 90), "bulk16": (128, 13, 21)}


@pytest.mark.parametrize("name", sorted(FIGURES))
def test_family_figures(name):
    rows, idx, res = bd.family(name)
    nsol, nonzero, max_bits = FIGURES[name]
    assert len(idx) == len(res) == nsol
    assert sum(r[0] == bp.ST_SOLUTION for r in res.values()) == nsol
    ni, nvar = rows.shape[1], rows.shape[2] - 1
    for r in res.values():
        assert len(r[2]) == ni and all(d > 0 for _, d in r[2])
    assert sum(1 for r in res.values() if any(n for n, _ in r[2])) == nonzero
    assert max(r[3].max_bits for r in res.values()) == max_bits
    # the sort moves rows in every tableau: an identity `pos` would hide a wrong sort
    identity = list(range(nvar, nvar + ni))
    for b in idx:
        pos = bd.positions(rows[b])
        assert sorted(pos) == identity and pos != identity, b


def test_widths_the_families_are_comparable_in():
    """the share left out is 0 in 64 bits for the lexmin families and 0 in 128 bits for all"""
    for name, (_, _, max_bits) in FIGURES.items():
        assert max_bits < 128
        assert (max_bits < 64) == (name != "dense20")


def test_crafted_sort_keys():
    assert bd.positions(bd.CRAFTED) == [3, 8, 9, 6, 7, 10, 4, 5]
    status, pivots, dual, st = bd.solve_dual(bd.CRAFTED, 64)
    assert status == bp.ST_SOLUTION and pivots > 0
    assert dual == [(1, 1)] + [(0, 1)] * 7
    assert st.max_bits == 34 and st.exact


def test_no_solution_has_no_dual():
    rows = [[1, 0, -1], [-1, 0, 0], [0, 1, -2]]  # x0 >= 1 and -x0 >= 0
    status, _, dual, _ = bd.solve_dual(rows, 64)
    assert status == bp.ST_NIL and dual is None
