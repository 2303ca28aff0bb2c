"""-m gpu: the deepest cut of pip_advance_kernel (PIPAMD_T_DEEPEST; csrc/pip_advance.h phase G, integrer.c:417-438)
against Python ints, case by case.

Every leg solves the case list of tests/deepest_cases.py through Batch(..., tflags=T_INT | T_DEEPEST, cap_cuts=<the
model's cut count of the batch's worst case>) and holds status, pivot count, cut count and every reduced numerator /
denominator pair to tests/bigint_pip.py's Result (deepest=True) for the same embedded tableau.  No case is left out:
anything but ST_SOLUTION / ST_NIL as the model has it -- ST_CAPACITY, ST_RUN, ST_OVERFLOW among them -- fails.  All
cases have three inequalities, so a batch needs no padding rows.

The legs:
  column blocks   every nvar of deepest_cases.NVAR: the constant column -- which the kernel picks out of wave 0's
                  registers by (nvar / CW, nvar % CPL, (nvar % CW) / CPL) -- last in a block, first and second in the
                  next, in every block up to the widest row integrer() takes
  waves           the one-wave kernel of a bulk launch (a T_DEEPEST batch takes no lean launch, pip_plan.h), the
                  four-wave tail, eight waves, and the sixteen-wave tail of a 128-bit batch of at most 256 tableaux
  pause           one pivot per launch: the cut is stored and published by one launch and loaded as the pivot row by
                  the next
  rows            T_ROWS_STAY on and off, at an even and an odd column count

Width edges are the case tags (denominators of 30 ... 33 and 61 ... 63 bits, lambda * coefficient below and beyond 63
bits, delta > 1, the lambda += D / delta loop run 0, 1 and more times).  The 64-bit engine gets the cases whose every
intermediate fits 64 bits; it is not asked about the others, since the reference's own 64-bit build wraps on them.  The
128-bit legs (entier_bits=128) run ALL cases and are what holds the arithmetic beyond 63 bits: there the kernel must be
bit-exact on every lambda * coefficient of up to 126 bits.
"""
import math

import numpy as np
import pytest

import bigint_pip as bp
import deepest_cases as dc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

T_DEEPEST = 512  # include/piplib_amd.h PIPAMD_T_DEEPEST


def _ids(bits):
    cs = dc.cases()
    return [k for k in range(len(cs)) if bits == 128 or cs[k].exact64]


def _solve(e, nvar, bits, size=64, extra=0):
    """the cases of `bits` as a batch of at least `size` tableaux of nvar unknowns on engine `e`: (ids, status, pivots,
    cuts, numerators, denominators), the values as Python ints"""
    import torch
    from piplib_amd import engine as eng
    rows, ids = dc.batch_of(_ids(bits), nvar, bits, size)
    cap = max(dc.model(k, nvar, bits).cuts for k in set(ids))
    b = eng.Batch(e, rows, nvar, 0, tflags=eng.T_INT | T_DEEPEST | extra, cap_cuts=cap, entier_bits=bits)
    b.load()
    b.solve()
    b.fetch()
    torch.cuda.synchronize()
    num, den = b.sol_num.cpu().numpy(), b.sol_den.cpu().numpy()
    if bits == 128:
        num, den = eng.wide_to_int(num), eng.wide_to_int(den)
    return ids, b.status.cpu().numpy(), b.pivots.cpu().numpy(), b.cuts.cpu().numpy(), num[:, :, 0].astype(object), den.astype(object)


def _reduced(num, den):
    out = []
    for n, d in zip(num, den):
        n, d = int(n), int(d)
        g = math.gcd(n, d)
        out.append((n // g, d // g) if g else (n, d))
    return out


def _check(got, nvar, bits):
    ids, st, pv, ct, num, den = got
    assert len(ids) >= 64 and set(ids) == set(_ids(bits))
    for b, k in enumerate(ids):
        m = dc.model(k, nvar, bits)
        assert m.stats.exact and m.status in (bp.ST_SOLUTION, bp.ST_NIL)
        assert st[b] == m.status, (b, k, st[b], m.status)
        assert pv[b] == m.pivots, (b, k, pv[b], m.pivots)
        assert ct[b] == m.cuts, (b, k, ct[b], m.cuts)
        if m.status == bp.ST_SOLUTION:
            assert _reduced(num[b], den[b]) == _reduced(m.sol_num, m.sol_den), (b, k)


@pytest.mark.parametrize("bits,nvar", [(bits, nvar) for bits in (64, 128) for nvar in dc.NVAR[bits]])
def test_column_blocks(bits, nvar):
    """the constant column in every position of the list, through the default launches of a small batch"""
    from piplib_amd import engine as eng
    e = eng.Engine(0)
    _check(_solve(e, nvar, bits), nvar, bits)
    assert e.last_solve_launches() == 1   # one tail launch finished them all


WAVES = [(64, nvar, mode) for nvar in (5, 127, 129, 257) for mode in ("bulk", "four", "eight")] + \
        [(128, nvar, mode) for nvar in (63, 65, 191, 510) for mode in ("bulk", "four", "eight", "default")]


@pytest.mark.parametrize("bits,nvar,mode", WAVES)
def test_waves_per_tableau(bits, nvar, mode):
    """bulk: 64 tableaux and more with set_bulk_min(64) go through the one-wave general kernel first (a compile-time row
    capacity, FULL at 127 unknowns, where the row is one block of 64-bit entries; the run-time one elsewhere) and finish
    there -- the tail launch behind it finds an empty list.  four / eight: set_waves_per_job; eight waves exist for one
    block of 64-bit entries, every other shape takes the four-wave kernel for it.  default (128 bits): the tail of a batch
    of at most 256 tableaux is sixteen waves up to 256 columns, four beyond."""
    from piplib_amd import engine as eng
    e = eng.Engine(0)
    if mode == "bulk":
        e.set_bulk_min(64)
    elif mode != "default":
        e.set_waves_per_job(4 if mode == "four" else 8)
    _check(_solve(e, nvar, bits), nvar, bits)
    if mode == "bulk":
        assert e.last_solve_launches() >= 2, e.last_solve_launches()   # the bulk launch went out, then the tail
    else:
        assert e.last_solve_launches() == 1, e.last_solve_launches()


@pytest.mark.parametrize("bits,nvar", [(64, 5), (64, 129), (128, 65), (128, 192)])
def test_pause_across_the_cut(bits, nvar):
    """pipamd_engine_set_iter_limit(1): every launch pauses every tableau after one pivot, so each cut is built, stored
    and published by one launch (the one-wave kernel first, then the tail's) and staged and pivoted on by the next.  The
    results are those of the solve without a limit, and the model's."""
    from piplib_amd import engine as eng
    outs = []
    for lim in (1, 0):
        e = eng.Engine(0)
        e.set_bulk_min(64)
        if lim:
            e.set_iter_limit(lim)
        outs.append(_solve(e, nvar, bits))
        if lim:
            assert e.last_solve_launches() > 4, e.last_solve_launches()
        _check(outs[-1], nvar, bits)
    for x, y in zip(outs[0][1:], outs[1][1:]):
        assert (x == y).all()


@pytest.mark.parametrize("bits,nvar", [(64, 127), (64, 128), (128, 63), (128, 64)])
@pytest.mark.parametrize("stay", (0, 1))
def test_rows_fetched_or_copied(bits, nvar, stay):
    """T_ROWS_STAY on (the kernel fetches the caller's rows) and off (the load copies them), at an even and an odd
    column count (nvar + 1)"""
    from piplib_amd import engine as eng
    e = eng.Engine(0)
    _check(_solve(e, nvar, bits, extra=eng.T_ROWS_STAY if stay else 0), nvar, bits)
