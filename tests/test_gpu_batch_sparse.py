"""-m gpu: Batch(sparse=True) -- the plain system as sparse rows (pipamd_batch_load_sparse, pipamd_batch_dual_sparse;
the PipCsrRows source policy of pip_batch_load_system_kernel and pip_batch_dual_kernel, csrc/pip_kernels.hip).

Authorities: the dense entry on the dense expansion, byte for byte in the workspace (pipamd_batch_load_system, itself held
to tests/system_model.py by tests/test_gpu_batch_system.py); the CPU oracle on the model's tableau; the reference's
printed answers, duals and pivot counts of tests/golden/system/.  The helpers that hold a solved batch to those are the
dense test's own (tests/test_gpu_batch_system.py).  No system is left out of any comparison."""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

SHIFTS = [0, 1, -1]


def _tbs():
    import test_gpu_batch_system as tbs
    return tbs


def _sparse_batch(e, csr, shape, nvar, eq, shift, tflags, simp, bits=64):
    from piplib_amd import engine as eng
    b = eng.Batch(e, csr, nvar, 0, tflags=tflags, entier_bits=bits, shift=shift, shape=shape, sparse=True, eq_rows=eq, simplify=simp)
    assert b.desc.ni == shape[1] + len(eq)
    return b


def _solve_sparse(rows, nvar, eq, shift, nq, simp, dual, bits=64, e=None, csr=None):
    import sparse_cases as sp
    from piplib_amd import engine as eng
    tbs = _tbs()
    tflags = (eng.T_INT if nq else 0) | (eng.T_DUAL if dual else 0) | eng.T_ROWS_STAY  # (ROWS_STAY is ignored)
    b = _sparse_batch(e or tbs._engine(), csr if csr is not None else sp.to_csr(rows), rows.shape, nvar, eq, shift, tflags, simp, bits)
    b.load_sparse()
    return tbs._finish(b, (lambda b: b.dual_sparse()) if dual else None)


# ---------------------------------------------------------------- the workspace, byte for byte

def _eq_variants(nrows):
    return [(), (0,), (nrows - 1,), tuple(range(nrows))]


@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("nvar", [3, 63, 64, 65, 127, 128, 129])
def test_workspace_equals_the_dense_load(nvar, bits):
    """every column of every row, row tables, spare slots and headers: the zeroed workspace after load_sparse() against
    the zeroed workspace after load_system() on the dense expansion -- same engine, same descriptor.  3 tableaux of 2 .. 6
    rows; rows that are empty, the constant alone, one unknown alone, full, sparse with a stored zero
    (sparse_cases.edge_systems); no equality, the first row, the last row, every row; the three shifts; tab_simplify on and
    off.  nvar is at the edges of a lane's columns: the constant is column nvar, lane 63 or lane 0 of the next block."""
    import torch
    import sparse_cases as sp
    from piplib_amd import engine as eng
    e = eng.Engine(0)
    combo = 0
    for shift in SHIFTS:
        for simp in (0, 1):
            for v in range(4):
                nrows = 6 - combo % 5  # 6, 5, 4, 3, 2, 6, ...
                eq = _eq_variants(nrows)[v]
                a, stored = sp.edge_systems(nvar, nrows, 1000 * nvar + combo)
                csr = sp.to_csr(a, stored)
                assert (csr[2] == 0).sum() == stored.sum()
                kw = dict(tflags=eng.T_INT, entier_bits=bits, shift=shift, shape=a.shape, eq_rows=eq, simplify=simp)
                s = eng.Batch(e, csr, nvar, 0, sparse=True, **kw)
                d = eng.Batch(e, a, nvar, 0, system=True, **kw)
                assert bytes(s.desc) == bytes(d.desc) and s.ws.shape == d.ws.shape
                s.ws.zero_()
                d.ws.zero_()
                s.load_sparse()
                d.load_system()
                torch.cuda.synchronize()
                assert torch.equal(s.ws, d.ws), (shift, simp, eq, nrows)
                assert d.ws.any()
                combo += 1
    assert combo == 24


# ---------------------------------------------------------------- solved batches against the reference's answers

def _check_case(name, box, shift, mode, bits=64, golden=True):
    """tests/test_gpu_batch_system.py::_check_case with the batch loaded from sparse rows"""
    import system_model as sy
    tbs = _tbs()
    nq, simp, dual = tbs.MODES[mode]
    rows, nvar, eq = tbs._family(name, box)
    tab, res = tbs._expected(name, box, shift, nq, simp)
    b = _solve_sparse(rows, nvar, eq, shift, nq, simp, dual, bits)
    solved = tbs._against_oracle(b, res, nvar, bits)
    tbs._same(b, tbs._solve_tableau(tab, nvar, shift, nq, bits))  # cuts and the solution arrays, bit for bit
    got_x = tbs._answers(b, bits)
    opts = tbs.OPTS[shift] + ("+" if shift and dual else "") + ("Rational+Dual" if dual else "")
    if golden:
        want = sy.golden(name)["cases"][f"box{box},{opts}"]
        assert got_x == want["x"]
        if simp or not nq:  # (the reference's pivot counts are those of the simplified tableau)
            assert b.pivots.cpu().tolist() == want["pivots"]
    if dual:
        got_d = tbs._duals(b, bits)
        nrows = rows.shape[1]
        for k in range(len(rows)):
            if golden:
                w = want["dual"][k]
            else:
                t = sy.oracle_tableau_dual(rows[k], eq, opts)
                w = None if t is None else [list(p) for p in sy.dual(t, nrows, eq)]
            assert (w is None) == (got_x[k] is None), k
            assert got_d[k] == (w if w is not None else [[0, 0]] * nrows), (k, got_d[k], w)
    return solved


@pytest.mark.parametrize("mode", ["int-simplify", "int-plain", "rational-dual"])
@pytest.mark.parametrize("shift", SHIFTS, ids=["plain", "maximize", "urs"])
@pytest.mark.parametrize("box", [0, 1])
@pytest.mark.parametrize("name", ["s5", "s12"])
def test_golden_families(name, box, shift, mode):
    assert _check_case(name, box, shift, mode) >= 6


@pytest.mark.parametrize("mode", ["int-simplify", "int-plain", "rational-dual"])
@pytest.mark.parametrize("shift", SHIFTS, ids=["plain", "maximize", "urs"])
@pytest.mark.parametrize("name,bits", [("w70", 64), ("w131", 64), ("w131", 128), ("s5", 128)])
def test_wide_rows_and_128_bit_entries(name, bits, shift, mode):
    """w70: a row spans more than 64 lanes; w131: the eight-columns-a-lane instantiation; their answers and duals from
    the CPU oracle, s5's from the reference's"""
    assert _check_case(name, 1, shift, mode, bits=bits, golden=name == "s5") >= 4


# ---------------------------------------------------------------- parts

@pytest.mark.parametrize("shift", [0, -1], ids=["plain", "urs"])
def test_parts_equal_one_call(shift):
    """9 systems loaded as parts of 1, 5 and 3 (a non-zero `first`, arrays of the part's own): the workspace after the
    loads and, after the solve, results and duals equal the one-call load's"""
    import torch
    import sparse_cases as sp
    from piplib_amd import engine as eng
    tbs = _tbs()
    rows, nvar, eq = tbs._family("s5", 1)
    rows = rows[:9]
    e = tbs._engine()
    tflags = eng.T_DUAL
    one = _sparse_batch(e, sp.to_csr(rows), rows.shape, nvar, eq, shift, tflags, 0)
    one.ws.zero_()
    one.load_sparse()
    parts = _sparse_batch(e, None, rows.shape, nvar, eq, shift, tflags, 0)
    parts.ws.zero_()
    dev, at = [], 0
    for n in (1, 5, 3):
        arrays = sp.to_csr(rows[at:at + n])
        arrays = [torch.as_tensor(x).to(parts.dev) for x in arrays]
        assert arrays[0][0].item() == 0 and arrays[0].numel() == n * rows.shape[1] + 1
        parts.load_sparse_part(*arrays, at)
        dev.append((arrays, at))
        at += n
    torch.cuda.synchronize()
    assert torch.equal(one.ws, parts.ws)
    tbs._finish(one, lambda b: b.dual_sparse())

    def by_parts(b):
        out = None
        for arrays, first in dev:
            out = b.dual_sparse_part(*arrays, first, out=out)
        return out
    tbs._finish(parts, by_parts)
    tbs._same(one, parts)
    assert torch.equal(one.dual_pair[0], parts.dual_pair[0]) and torch.equal(one.dual_pair[1], parts.dual_pair[1])
    assert (one.status == eng.ST_SOLUTION).sum().item() >= 3 and one.dual_pair[1].any()


# ---------------------------------------------------------------- bad systems among good ones

def _row_lists(rows):
    """[[(cols, vals) per row] per system] of the dense systems"""
    return [[(np.flatnonzero(r).tolist(), r[np.flatnonzero(r)].tolist()) for r in system] for system in rows]


def _flatten(systems):
    ptr, cols, vals = [0], [], []
    for system in systems:
        for c, v in system:
            cols += c
            vals += v
            ptr.append(len(cols))
    return np.array(ptr, np.int64), np.array(cols, np.int32), np.array(vals, np.int64)


def _long_row(systems, k):
    """a row of system k with at least two entries"""
    return max(range(len(systems[k])), key=lambda r: len(systems[k][r][0]))


def _bad_arrays(kind, rows, nvar):
    """(CSR arrays with one bad system, its index): d_cols / d_vals have exactly nnz entries, so a pointer that were
    followed beyond nnz would leave them"""
    systems = _row_lists(rows)
    k, nrows = 3, rows.shape[1]
    r = _long_row(systems, k)
    c, v = systems[k][r]
    assert len(c) >= 2
    if kind == "column-nvar+1":
        systems[k][r] = (c[:-1] + [nvar + 1], v)
    elif kind == "negative-column":
        systems[k][r] = ([-1] + c[1:], v)
    elif kind == "equal-columns":
        systems[k][r] = ([c[0], c[0]] + c[2:], v)
    elif kind == "decreasing-columns":
        systems[k][r] = ([c[1], c[0]] + c[2:], v)
    elif kind == "row-of-nvar+2":
        systems[k][r] = (list(range(nvar + 1)) + [nvar], [1] * (nvar + 2))
    ptr, cols, vals = _flatten(systems)
    if kind == "pointer-beyond-nnz":  # the batch's last pointer: nothing else is wrong with the system
        k = len(systems) - 1
        ptr[-1] = len(cols) + 1000
    elif kind == "decreasing-pointer":  # an inner pointer of the system, within [0, nnz]
        at = k * nrows + r + 1
        assert ptr[at - 1] >= 1 and r + 1 < nrows
        ptr[at] = ptr[at - 1] - 1
    return (ptr, cols, vals), k


BAD = ["column-nvar+1", "negative-column", "equal-columns", "decreasing-columns", "pointer-beyond-nnz", "decreasing-pointer",
       "row-of-nvar+2"]


@pytest.fixture(scope="module")
def good_s12():
    """the batch without a bad system, rational with dual: (rows, nvar, eq, the solved batch)"""
    tbs = _tbs()
    rows, nvar, eq = tbs._family("s12", 1)
    rows = rows[:8]
    return rows, nvar, eq, _solve_sparse(rows, nvar, eq, 0, 0, 0, 1)


@pytest.mark.parametrize("kind", BAD)
def test_bad_system_among_good_ones(kind, good_s12):
    """input validation: the system ends ST_BADINPUT with zero results and duals, its neighbours as without it"""
    import torch
    from piplib_amd import engine as eng
    rows, nvar, eq, good = good_s12
    csr, k = _bad_arrays(kind, rows, nvar)
    assert len(csr[1]) == len(csr[2])
    b = _solve_sparse(rows, nvar, eq, 0, 0, 0, 1, csr=csr)
    assert b.csr[1].numel() == len(csr[1])  # (exactly nnz entries on the device)
    others = [i for i in range(len(rows)) if i != k]
    assert b.status[k].item() == eng.ST_BADINPUT
    assert b.pivots[k].item() == 0 and b.cuts[k].item() == 0
    assert not b.sol_num[k].any() and not b.sol_den[k].any()
    assert not b.dual_pair[0][k].any() and not b.dual_pair[1][k].any()
    for name in ("status", "pivots", "cuts", "sol_num", "sol_den"):
        assert torch.equal(getattr(b, name)[others], getattr(good, name)[others]), name
    for x, y in zip(b.dual_pair, good.dual_pair):
        assert torch.equal(x[others], y[others])
    assert (good.status == eng.ST_SOLUTION).sum().item() >= 3 and good.status[k].item() != eng.ST_BADINPUT


def test_bad_system_leaves_an_empty_tableau():
    """integer batch with tab_simplify under Maximize: the bad system's header says ni = 0, its neighbours' answers are
    the dense entry's"""
    import torch
    from piplib_amd import engine as eng
    tbs = _tbs()
    rows, nvar, eq = tbs._family("s12", 1)
    rows = rows[:8]
    csr, k = _bad_arrays("decreasing-columns", rows, nvar)
    b = _solve_sparse(rows, nvar, eq, 1, 1, 1, 0, csr=csr)
    d = tbs._solve_system(rows, nvar, eq, 1, 1, 1, 0)
    others = [i for i in range(len(rows)) if i != k]
    assert b.status[k].item() == eng.ST_BADINPUT and not b.x_num[k].any() and not b.x_den[k].any()
    for name in ("status", "pivots", "cuts", "sol_num", "sol_den", "x_num", "x_den"):
        assert torch.equal(getattr(b, name)[others], getattr(d, name)[others]), name
    job = b.ws[:25 * len(rows)].cpu().numpy().view(np.int32).reshape(len(rows), 50)  # PipJob: 200 bytes, ni is int32 12
    assert job[k, 12] == 0 and (job[others, 12] >= b.desc.ni).all()  # (the solve's cuts have become rows of the others)


# ---------------------------------------------------------------- the bulk path

@pytest.mark.parametrize("shift,lean_big", [(0, False), (1, True)], ids=["plain", "maximize-lean"])
def test_bulk_through_the_lean_launches(shift, lean_big):
    """2,048 systems of s12's shape, integer with tab_simplify: everything the dense entry gives"""
    tbs = _tbs()
    rows, nvar, eq = tbs._family("bulk12", 1)
    b = _solve_sparse(rows, nvar, eq, shift, 1, 1, 0, e=tbs._engine(lean_big))
    assert b.e.last_solve_launches() >= 2
    d = tbs._solve_system(rows, nvar, eq, shift, 1, 1, 0, e=tbs._engine(lean_big))
    tbs._same(b, d, ("status", "pivots", "cuts", "sol_num", "sol_den") + (("x_num", "x_den") if shift else ()))
    assert 100 <= (b.status == 1).sum().item() < len(rows)
