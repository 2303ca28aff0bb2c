"""Batch(shift=+-1): lexicographic maxima and unknowns of either sign from PLAIN rows (pipamd_batch_load_shifted,
pipamd_batch_results_shifted).  fetch_shifted() equals tests/shift_model.py's decode of the CPU oracle's tableau-level
result on every tableau; the load kernel's tableau equals, bit for bit in what the solve leaves, one loaded with
pipamd_batch_load from shift_model.shift_rows; two half loads equal one; 128-bit entries; tableaux without a solution
give (0, 0)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BATCH = 160
FAMILIES = {(5, 8): (31, dict(nnz=3, cmax=3, x0max=5)), (62, 32): (7094, {}), (131, 8): (44, dict(nnz=3, cmax=4, x0max=6))}


@functools.lru_cache(maxsize=None)
def _plain(nvar, ni, box, nil):
    import shift_cases as sc
    seed, kw = FAMILIES[nvar, ni]
    rows = sc.plain_rows(seed, nvar, ni, BATCH, kw, box)
    if nil:  # every fifth tableau gets x_0 >= 1 and x_0 <= 0 in place of its first two rows: no solution
        rows[::5, 0, :] = 0
        rows[::5, 0, 0], rows[::5, 0, -1] = 1, -1
        rows[::5, 1, :] = 0
        rows[::5, 1, 0] = -1
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def _expected(nvar, ni, box, nil, shift, nq):
    """(status, pivots, x_num, x_den) per tableau: shift_model.decode of the oracle's result; computed once per family"""
    import pipbatch as pb
    import shift_cases as sc
    import shift_model as sm
    from gpu_common import oracle_batch
    rows = _plain(nvar, ni, box, nil)
    srows = np.array([sm.shift_rows(r, shift) for r in rows.tolist()], dtype=np.int64)
    out = []
    for k, r in enumerate(oracle_batch(srows, nvar, 1, nq, bigparm=nvar + 1).results):
        assert r.status == pb.ST_OK, (k, r.status, r.abort_code)
        f = sc.forms(r.text)
        xs = [(0, 0)] * nvar if f is None else [sm.decode(b, c, d, shift) for b, c, d in f]
        out.append((f is not None, r.pivots, [x[0] for x in xs], [x[1] for x in xs]))
    return srows, out


def _solve(rows, nvar, nq, shift, bits=64, halves=False, nparm=0, bigparm=-1):
    import torch
    from piplib_amd import engine as eng
    e = eng.Engine(0)
    e.set_bulk_min(64)
    e.set_lean_big(bool(shift))   # the shifted batch through the lean kernel's big-parameter flavour, the model's through the general kernel
    b = eng.Batch(e, None if halves else rows, nvar, nparm, bigparm=bigparm, tflags=(eng.T_INT if nq else 0) | eng.T_ROWS_STAY,
                  entier_bits=bits, shift=shift, shape=rows.shape)
    if halves:
        h = rows.shape[0] // 2 + 3
        dev = torch.as_tensor(rows, dtype=torch.int64).to(b.dev)
        b.load_parts([dev[:h].contiguous(), dev[h:].contiguous()])
    else:
        b.load()
    b.solve()
    b.fetch()
    if shift:
        b.fetch_shifted()
    torch.cuda.synchronize()
    return b


def _ints(t, bits):
    from piplib_amd import engine as eng
    a = t.cpu().numpy()
    return eng.wide_to_int(a) if bits == 128 else a.astype(object)


@pytest.mark.parametrize("nq", [1, 0], ids=["integer", "rational"])
@pytest.mark.parametrize("shift", [1, -1], ids=["maximize", "urs"])
@pytest.mark.parametrize("nvar,ni,box,nil,bits", [
    (5, 8, 0, 0, 64), (5, 8, 1, 0, 64), (62, 32, 0, 0, 64), (62, 32, 1, 0, 64),
    (5, 8, 1, 1, 64),    # tableaux without a solution among them: (0, 0)
    (5, 8, 1, 0, 128),   # (low, high) pairs
    # 133 tableau columns: the load kernel's eight-columns-a-lane instantiation, in both entry widths
    (131, 8, 0, 0, 64), (131, 8, 1, 0, 64), (131, 8, 0, 0, 128),
])
def test_batch_shift(nvar, ni, box, nil, bits, shift, nq):
    from piplib_amd import engine as eng
    rows = _plain(nvar, ni, box, nil)
    srows, want = _expected(nvar, ni, box, nil, shift, nq)
    b = _solve(rows, nvar, nq, shift, bits)
    assert b.desc.nparm == 1 and b.desc.bigparm == nvar + 1
    st, pv = b.status.cpu().numpy(), b.pivots.cpu().numpy()
    xn, xd = _ints(b.x_num, bits), _ints(b.x_den, bits)
    unbounded = nils = 0
    for k, (has, piv, wn, wd) in enumerate(want):
        assert st[k] == (eng.ST_SOLUTION if has else eng.ST_NIL), (k, st[k])
        assert pv[k] == piv, (k, pv[k], piv)
        assert list(xn[k]) == wn and list(xd[k]) == wd, (k, list(xn[k]), wn, list(xd[k]), wd)
        unbounded += has and 0 in wd
        nils += not has
    print(nvar, ni, "box", box, "shift", shift, "nq", nq, "bits", bits, "unbounded", unbounded, "nil", nils)
    if nil:
        assert nils >= BATCH // 5
    if box and shift > 0:
        assert unbounded == 0   # the box bounds every maximum
    else:
        assert unbounded > 0
    # the load kernel, bit for bit: the same batch loaded with pipamd_batch_load from the model's shifted rows
    c = _solve(srows, nvar, nq, 0, bits, nparm=1, bigparm=nvar + 1)
    for name in ("status", "pivots", "cuts", "sol_num", "sol_den"):
        assert (getattr(b, name) == getattr(c, name)).all().item(), name
    # two part loads equal one
    h = _solve(rows, nvar, nq, shift, bits, halves=True)
    for name in ("status", "pivots", "cuts", "sol_num", "sol_den", "x_num", "x_den"):
        assert (getattr(b, name) == getattr(h, name)).all().item(), name
