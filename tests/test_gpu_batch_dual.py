"""-m gpu: pipamd_batch_dual -- Compute_dual for rational batches of layer 1 (pip_batch_dual_kernel, csrc/pip_kernels.hip).

Authorities: tests/bigint_dual.py (Python ints; tests/test_bigint_dual.py holds it to figures computed on the CPU), a
tableau compared only where Stats.exact holds for the flavour -- which is every tableau of every family here, and the
tests assert that --, and the per-problem host tree (pipamd_traiter with T_DUAL on an engine with the device tree off,
which test_gpu_golden.py::test_compute_dual_on_gpu[host-tree] pins to the reference's fixtures; the second list of its
cells is the dual).  Pairs are compared as they are, not reduced."""
import functools

import numpy as np
import pytest

import bigint_dual as bd
import bigint_pip as bp

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

E_INVALID = -1
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def engines():
    from piplib_amd import engine as eng
    on, off = eng.Engine(0), eng.Engine(0)
    off.set_device_tree(False)
    return on, off


def _solve(e, rows, tflags, bits=64):
    from piplib_amd import engine as eng
    b = eng.Batch(e, rows, rows.shape[2] - 1, 0, tflags=tflags, entier_bits=bits)
    b.load()
    b.solve()
    b.fetch()
    return b


def _np(b, t):
    from piplib_amd import engine as eng
    a = t.cpu().numpy()
    return eng.wide_to_int(a) if b.entier_bits == 128 else a


def _pairs(b, dual):
    """[(num, den)] per tableau, Python ints"""
    n, d = _np(b, dual[0]), _np(b, dual[1])
    return [[(int(x), int(y)) for x, y in zip(nr, dr)] for nr, dr in zip(n, d)]


def _same_solve(a, b):
    """statuses, pivots and solutions of two batches"""
    import torch
    for name in ("status", "pivots", "sol_num", "sol_den"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def _host_dual(off, rows_b, bits):
    """(dual pairs | None, pivots) of one tableau from the per-problem host tree"""
    from piplib_amd import engine as eng
    ni, nvar = rows_b.shape[0], rows_b.shape[1] - 1
    cells, piv = eng.traiter(off, nvar, 0, ni, 0, -1, eng.T_DUAL, rows_b, np.zeros((0, 1), dtype=np.int64), bits=bits)
    lists = [k for k, c in enumerate(cells) if c[0] == eng.SOL_LIST]
    if len(lists) < 2:
        return None, piv
    k = lists[1]
    assert cells[k][1] == ni
    vals = [(c[1], c[2]) for c in cells[k + 1:] if c[0] == eng.SOL_VAL]
    assert len(vals) == ni
    return vals, piv


def _against_bigint(b, pairs, res, idx):
    """every tableau of idx: status, pivots and dual as bigint_dual has them; none left out"""
    st, pv = b.status.cpu().numpy(), b.pivots.cpu().numpy()
    for k in idx:
        status, pivots, dual, stats = res[k]
        assert stats.exact, (k, stats.max_bits)  # the share left out is 0
        assert st[k] == status and pv[k] == pivots, (k, st[k], status, pv[k], pivots)
        if status == bp.ST_SOLUTION:
            assert pairs[k] == dual, (k, pairs[k], dual)
        else:
            assert pairs[k] == [(0, 0)] * len(pairs[k]), k


def _against_host(off, b, pairs, rows, idx, bits):
    pv = b.pivots.cpu().numpy()
    for k in idx:
        dual, piv = _host_dual(off, rows[k], bits)
        assert dual is not None and pairs[k] == dual, (k, pairs[k], dual)
        assert pv[k] == piv, (k, pv[k], piv)


@pytest.mark.parametrize("bits", [64, 128])
def test_smallest_shape(engines, bits):
    from piplib_amd import engine as eng
    on, off = engines
    rows, idx, res = bd.family("lexmin12", bits)
    b = _solve(on, rows, eng.T_DUAL, bits)
    pairs = _pairs(b, b.dual())
    assert len(idx) == 64
    _against_bigint(b, pairs, res, idx)
    _against_host(off, b, pairs, rows, range(16), bits)
    _same_solve(b, _solve(on, rows, 0, bits))


@pytest.mark.parametrize("name", ["lexmin64", "lexmin65"])
def test_both_forms_of_the_sort(engines, name):
    """64 inequalities: the last shape with a row per lane; 65: the first with the strided scan -- and the first whose
    values take a second 64-row word of the kernel's last step"""
    from piplib_amd import engine as eng
    on, off = engines
    rows, idx, res = bd.family(name, 64)
    b = _solve(on, rows, eng.T_DUAL)
    pairs = _pairs(b, b.dual())
    assert len(idx) == 32
    _against_bigint(b, pairs, res, idx)
    _against_host(off, b, pairs, rows, range(8), 64)


def test_a_third_word_of_rows(engines):
    """130 inequalities: the kernel's last step, 64 input rows a turn, takes a third turn (65, the second, is lexmin65
    above); still the LDS form of the sort"""
    from piplib_amd import engine as eng
    on, off = engines
    rows, idx, res = bd.family("lexmin130", 64)
    assert rows.shape[1:] == (130, 11) and len(idx) == 32
    b = _solve(on, rows, eng.T_DUAL)
    pairs = _pairs(b, b.dual())
    _against_bigint(b, pairs, res, idx)
    _against_host(off, b, pairs, rows, range(4), 64)


def test_pairs_are_not_reduced(engines):
    """pipamd_batch_dual hands out solution_dual's pairs as they are (pipamd_batch_dual_system reduces them): the
    tableaux of lexmin12 whose dual, by bigint_dual alone, has a pair with a non-zero numerator and gcd above 1"""
    import math
    from piplib_amd import engine as eng
    on, _ = engines
    rows, idx, res = bd.family("lexmin12", 64)
    pick = [k for k in idx if res[k][0] == bp.ST_SOLUTION and any(n and math.gcd(n, d) > 1 for n, d in res[k][2])]
    assert 3 in pick and (68, 328) in res[3][2]  # (chosen on the CPU: 17 / 82 unreduced)
    sub = np.ascontiguousarray(rows[pick])
    b = _solve(on, sub, eng.T_DUAL)
    pairs = _pairs(b, b.dual())
    for k, got in zip(pick, pairs):
        assert res[k][3].exact
        assert got == res[k][2], (k, got, res[k][2])
        assert got != [(n // math.gcd(n, d), d // math.gcd(n, d)) for n, d in res[k][2]], k


@pytest.mark.parametrize("bits", [64, 128])
def test_sort_keys(engines, bits):
    """float rounding of keys, entries beyond int and INT_MIN, a row at smax: four copies of the crafted tableau"""
    from piplib_amd import engine as eng
    on, off = engines
    rows = np.array([bd.CRAFTED] * 4, dtype=np.int64)
    want = bd.solve_dual(bd.CRAFTED, bits)
    assert want[2] == [(1, 1)] + [(0, 1)] * 7
    b = _solve(on, rows, eng.T_DUAL, bits)
    pairs = _pairs(b, b.dual())
    _against_bigint(b, pairs, {k: want for k in range(4)}, range(4))
    _against_host(off, b, pairs, rows, range(1), bits)


@functools.lru_cache(maxsize=None)
def _nil_family():
    """lexmin12 with two rows appended: every fourth tableau x0 >= 1 and -x0 >= 0 (no solution), the others the same
    two rows made harmless (x0 >= 0, -x0 + 1000 >= 0)"""
    base = bd.family("lexmin12", 64)[0]
    B, ni, ncol = base.shape
    rows = np.zeros((B, ni + 2, ncol), dtype=np.int64)
    rows[:, :ni] = base
    rows[:, ni, 0] = 1
    rows[:, ni + 1, 0] = -1
    rows[:, ni + 1, ncol - 1] = 1000
    rows[::4, ni, ncol - 1] = -1
    rows[::4, ni + 1, ncol - 1] = 0
    return rows, {k: bd.solve_dual(rows[k], 64) for k in range(B)}


def test_no_solution(engines):
    from piplib_amd import engine as eng
    on, _ = engines
    rows, res = _nil_family()
    assert all((res[k][0] == bp.ST_NIL) == (k % 4 == 0) for k in res)
    assert all(res[k][0] == bp.ST_SOLUTION for k in res if k % 4)
    b = _solve(on, rows, eng.T_DUAL)
    pairs = _pairs(b, b.dual())
    st = b.status.cpu().numpy()
    assert all(st[k] == eng.ST_NIL and pairs[k] == [(0, 0)] * rows.shape[1] for k in range(0, len(rows), 4))
    _against_bigint(b, pairs, res, range(len(rows)))


def test_bulk_sequence(engines):
    """2,048 tableaux: the plain batch starts with the lean launches, the dual batch skips them -- same statuses, pivots
    and solutions; the duals equal those of the same tableaux in batches of 64 (the four-wave path) and bigint_dual's"""
    import torch
    from piplib_amd import engine as eng
    on, _ = engines
    rows, idx, res = bd.family("bulk16", 64)
    assert len(rows) == 2048 and len(idx) == 128
    plain = _solve(on, rows, 0)
    assert on.last_solve_launches() >= 3, on.last_solve_launches()  # lean, lean again, tail
    b = _solve(on, rows, eng.T_DUAL)
    print("launches: plain >= 3, with T_DUAL", on.last_solve_launches())
    _same_solve(b, plain)
    num, den = b.dual()
    pairs = _pairs(b, (num, den))
    _against_bigint(b, pairs, res, idx)
    for lo in (0, 1984):
        small = _solve(on, rows[lo:lo + 64], eng.T_DUAL)
        assert _pairs(small, small.dual()) == pairs[lo:lo + 64], lo
    stay = _solve(on, rows, eng.T_DUAL | eng.T_ROWS_STAY)
    _same_solve(stay, plain)
    num2, den2 = stay.dual()
    assert torch.equal(num2, num) and torch.equal(den2, den)


def test_wide_values(engines):
    """entries leave 64 bits (max_bits 90): the (low, high) output path"""
    from piplib_amd import engine as eng
    on, _ = engines
    rows, idx, res = bd.family("dense20", 128)
    assert max(r[3].max_bits for r in res.values()) > 64
    b = _solve(on, rows, eng.T_DUAL, 128)
    num, den = b.dual()
    assert tuple(num.shape) == (32, 20, 2) and tuple(den.shape) == (32, 20, 2)
    _against_bigint(b, _pairs(b, (num, den)), res, idx)


def test_parts(engines):
    import torch
    from piplib_amd import engine as eng
    on, _ = engines
    rows = bd.family("lexmin12", 64)[0]
    whole = _solve(on, rows, eng.T_DUAL)
    num, den = whole.dual()
    dev = whole.dev
    a, c = (torch.as_tensor(rows[:40]).to(dev).contiguous(), torch.as_tensor(rows[40:]).to(dev).contiguous())
    b = eng.Batch(on, None, rows.shape[2] - 1, 0, tflags=eng.T_DUAL, shape=rows.shape)
    b.load_parts([a, c])
    b.solve()
    out = (torch.full_like(num, SENTINEL), torch.full_like(den, SENTINEL))
    b.dual_part(a, 0, out=out)
    torch.cuda.synchronize(dev)
    assert torch.equal(out[0][:40], num[:40]) and bool((out[0][40:] == SENTINEL).all())
    b.dual_part(c, 40, out=out)
    torch.cuda.synchronize(dev)
    assert torch.equal(out[0], num) and torch.equal(out[1], den)
    keep = (out[0].clone(), out[1].clone())
    for first in (41, -1, 64):
        with pytest.raises(RuntimeError, match=r"error %d\b" % E_INVALID):
            b.dual_part(c, first, out=out)
    torch.cuda.synchronize(dev)
    assert torch.equal(out[0], keep[0]) and torch.equal(out[1], keep[1])


@pytest.mark.parametrize("what", ["int_and_dual", "no_dual", "nparm", "bigparm"])
def test_refusals_on_a_live_engine(engines, what):
    import torch
    from piplib_amd import engine as eng
    on, _ = engines
    rows = bd.family("lexmin12", 64)[0]
    b = _solve(on, rows, eng.T_DUAL)
    num, den = b.dual()
    out = (torch.full_like(num, SENTINEL), torch.full_like(den, SENTINEL))
    if what == "int_and_dual":
        b.desc.tflags = eng.T_INT | eng.T_DUAL
    elif what == "no_dual":
        b.desc.tflags = 0
    elif what == "nparm":
        b.desc.nparm = 1
    else:
        b.desc.bigparm = rows.shape[2]
    with pytest.raises(RuntimeError, match=r"error %d\b" % E_INVALID):
        b.dual_part(b.rows, 0, out=out)
    torch.cuda.synchronize(b.dev)
    assert bool((out[0] == SENTINEL).all()) and bool((out[1] == SENTINEL).all())
