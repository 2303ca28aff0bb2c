"""Exact-arithmetic (Python int) restatement of the rational solve with Compute_dual, for problems without parameters.

TEST INFRASTRUCTURE ONLY, like bigint_pip.py, from whose pieces it is assembled (_Row, sort_rows, pivot_step, _cell,
_sgn): the loop is solve()'s rational branch, `pos` is tab_sort_rows' table (traiter.c:616-619: where each input
inequality sits after the sort) and the dual is solution_dual (traiter.c:283-291): for inequality i, if logical row
pos[i] is a unit row, (valeur(tp, 0, its unit column), Denom(tp, 0)), else (0, 1) -- the pairs sol_val receives, unreduced.

A result is comparable with a fixed-width run only where `Stats.exact` holds for that width.
"""
import numpy as np

import bigint_pip as bp


def positions(ineq):
    """tab_sort_rows' `pos` for a freshly loaded tableau: pos[i] = logical row of input inequality i after the sort."""
    ineq = np.asarray(ineq, dtype=object)
    ni, ncol = ineq.shape
    nvar = ncol - 1
    rows, orig = _load(ineq, nvar, ni)
    bp.sort_rows(rows, nvar, nvar + ni)
    return _pos(rows, orig, nvar)


def _load(ineq, nvar, ni):
    rows = [bp._Row(bp.UNIT, 1, None, i) for i in range(nvar)]
    rows += [bp._Row(bp.UNKNOWN, 1, np.array([int(x) for x in ineq[i]], dtype=object)) for i in range(ni)]
    return rows, list(rows[nvar:])


def _pos(rows, orig, nvar):
    where = {id(r): k for k, r in enumerate(rows) if k >= nvar}
    return [where[id(r)] for r in orig]


def solve_dual(ineq, bits=64):
    """ineq: (ni, nvar+1) integers (unknowns | constant).  Returns (status, pivots, dual, Stats): dual is the list of
    ni (numerator, denominator) pairs behind a solution, None otherwise."""
    ineq = np.asarray(ineq, dtype=object)
    ni, ncol = ineq.shape
    nvar = ncol - 1
    st = bp.Stats(bits)
    rows, orig = _load(ineq, nvar, ni)
    for r in orig:
        bp._note_arr(st, r.v)
    det = [1]
    bp.sort_rows(rows, nvar, nvar + ni)
    pos = _pos(rows, orig, nvar)
    nligne = nvar + ni
    try:
        while True:
            pivi = next((i for i in range(nligne) if rows[i].flag & bp.MINUS), nligne)
            if pivi >= nligne:
                for i in range(nligne):
                    r = rows[i]
                    if r.flag != bp.UNKNOWN:
                        continue
                    r.flag = bp._sgn(int(r.v[nvar]))
                    if r.flag == bp.MINUS:
                        pivi = i
                        break
            if pivi >= nligne:
                status = bp.ST_SOLUTION
                break
            if bp.pivot_step(rows, det, pivi, nvar, ni, st) < 0:
                status = bp.ST_NIL
                break
    except bp.Overflow:
        return bp.ST_OVERFLOW, st.pivots, None, st
    if status != bp.ST_SOLUTION:
        return status, st.pivots, None, st
    den0 = int(rows[0].den)
    dual = []
    for i in range(ni):
        r = rows[pos[i]]
        dual.append((int(bp._cell(rows, 0, r.unit)), den0) if (r.flag & bp.UNIT) else (0, 1))
    return status, st.pivots, dual, st


A24 = 1 << 24
# float rounding of keys (A+1 ties with A), entries beyond int and INT_MIN (ignored), a row at smax (never picked)
CRAFTED = [[1, 0, 0, -1], [A24 + 1, 1, 0, -2], [A24, 0, 1, -3], [1 << 31, 2, 1, -1], [-(1 << 31), 1, 3, -1],
           [A24 + 2, 0, 1, -1], [0, 1, 1, -4], [1, 1, 0, -2]]

# name: (generator, arguments, tableaux compared (None: all), width the figures are for)
FAMILIES = {"lexmin12": ("lexmin_batch", (11, 64, 7, 12), None, 64),
            "lexmin64": ("lexmin_batch", (13, 32, 10, 64), None, 64),
            "lexmin65": ("lexmin_batch", (14, 32, 10, 65), None, 64),
            "lexmin130": ("lexmin_batch", (16, 32, 10, 130), None, 64),
            "dense20": ("dense_batch", (15, 32, 8, 20), None, 128),
            "bulk16": ("lexmin_batch", (17, 2048, 15, 16), tuple(range(64)) + tuple(range(1984, 2048)), 64)}
_cache = {}


def family(name, bits=None):
    """(rows of the whole batch, indices compared, {index: solve_dual(rows[index], bits)}); bits defaults to the
    family's own width.  Computed once per process and width."""
    gen, args, sel, fam_bits = FAMILIES[name]
    bits = bits or fam_bits
    if (name, bits) not in _cache:
        from piplib_amd import synth
        rows = getattr(synth, gen)(*args)
        idx = list(range(len(rows))) if sel is None else list(sel)
        _cache[(name, bits)] = (rows, idx, {b: solve_dual(rows[b], bits) for b in idx})
    return _cache[(name, bits)]
