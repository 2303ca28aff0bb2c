"""The decoding rule of the shifted batch entries, held to the reference: tests/shift_model.py applied to the CPU
oracle's tableau-level results (plain systems pushed through shift_rows, solved with nparm = 1, bigparm = nvar + 1)
equals what the reference's pip_solve prints for the same plain systems under Maximize / Urs_unknowns
(tests/golden/shift/, made by tests/golden/make_shift_fixtures.py) -- every problem, both shifts, integer and rational,
bounded and unbounded.  Host only."""
import numpy as np
import pytest

import pipbatch as pb
import shift_cases as sc
import shift_model as sm
from gpu_common import oracle_batch


@pytest.mark.parametrize("name", ["v5", "v12"])
@pytest.mark.parametrize("box", [0, 1])
@pytest.mark.parametrize("shift", [sm.SHIFT_MAX, sm.SHIFT_URS])
@pytest.mark.parametrize("nq", [1, 0])
def test_decode_equals_reference(name, box, shift, nq):
    g = sc.golden(name)
    nvar = g["nvar"]
    rows = sc.plain_rows(g["seed"], nvar, g["ni"], g["batch"], g["kw"], box)
    want = g["cases"][f"box{box},shift{shift},nq{nq}"]
    assert len(want) == g["batch"]
    srows = np.array([sm.shift_rows(r, shift) for r in rows.tolist()], dtype=np.int64)
    assert (srows == sc.shifted(rows, shift)).all()
    res = oracle_batch(srows, nvar, 1, nq, bigparm=nvar + 1).results
    unbounded = 0
    for k, r in enumerate(res):
        assert r.status == pb.ST_OK, (k, r.status, r.abort_code)
        f = sc.forms(r.text)
        got = None if f is None else [list(sm.decode(b, c, d, shift)) for b, c, d in f]
        assert got == want[k], (k, got, want[k])
        unbounded += got is not None and any(d == 0 for _, d in got)
    # the families give both kinds of answer without screening
    if box and shift == sm.SHIFT_MAX:
        assert unbounded == 0
    else:
        assert unbounded > 0


def test_model_by_hand():
    assert sm.shift_rows([[2, -3, 7]], sm.SHIFT_MAX) == [[-2, 3, 7, -1]]
    assert sm.shift_rows([[2, -3, 7]], sm.SHIFT_URS) == [[2, -3, 7, 1]]
    assert sm.decode(3, 6, 3, sm.SHIFT_MAX) == (-2, 1)     # 6/3 under Maximize
    assert sm.decode(3, -34, 3, sm.SHIFT_URS) == (-34, 3)
    assert sm.decode(0, 4, 2, sm.SHIFT_URS) == (2, 0)      # the big coefficient is not the denominator: unbounded
    assert sm.decode(5, 0, 5, sm.SHIFT_MAX) == (0, 1)      # gcd(0, D) = D
