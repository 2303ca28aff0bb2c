"""The case list of tests/test_gpu_deepest_cut.py: tiny tableaux whose integer solve builds deepest cuts
(PIPAMD_T_DEEPEST, integrer.c:417-438) at the magnitudes and in the columns where pip_advance_kernel's cut code changes
path.  TEST INFRASTRUCTURE ONLY; tests/test_deepest_cases.py proves on the CPU that the list is what it claims.

The generator is a seeded, deterministic search: DRAWS tableaux of 4 unknowns and 3 inequalities, coefficients in
-3..3, constants in -9..3, one entry replaced by a number of a chosen bit length (BIT_LENGTHS in turn).  A draw is kept
where tests/bigint_pip.py, the authority, solves it with the deepest cut on

  * to ST_SOLUTION or ST_NIL with at least one cut,
  * exactly at 128 bits (Stats.exact: no intermediate the fixed-width code forms leaves the width),
  * with a first cut that is not the plain cut of the same state (lambda % D != 1): up to that cut the solve is the same
    with and without the option, so a kernel that ignored the option builds another row there.

PINNED holds draws of the same search under other seeds, for what 6,000 draws do not meet: a denominator of 61, 62
or 63 bits whose cut is still exact at 64 bits (one draw in twenty thousand).

TAGS names what a case's cuts are made of; cases() keeps, per tag, the first PER_TAG kept draws that are exact at 64
bits too and the first PER_TAG that are not, so the list stays a few dozen tableaux.

The tag "nil" is a solve that ends ST_NIL behind its deepest cuts: a pivot row without a positive coefficient
(traiter.c:374, 782).  integrer()'s own nil exit -- a fractional constant over coefficients that are all divisible by the
denominator, integrer.c:482-485 case (b) -- has no case because a tableau without parameters cannot reach it: the
columns are unknowns, slacks of integer rows and slacks of cuts, each an integer affine function n = A x + b of the
unknowns (a cut's slack is -lambda * x_i plus an integer combination of the columns it was cut from, deepest or
plain), and the unknowns' rows are x = A^-1 (n - b).  Where every coefficient of row i is divisible by its denominator,
row i of A^-1 is an integer vector, and with the integer b so is its constant term.  Three million draws of this search
and of wider ones (more rows, equality pairs, larger coefficients) met it not once; Stats.nil_cut would say so, and
tests/test_deepest_cases.py asserts that it stays off over every draw of the search.

embed() places a small tableau in `nvar` unknowns: its four columns at column 0, the last column of a column block,
the first column of the next block and nvar - 1, every other column zero, the constant at nvar.  A column block is
what one pass of a wave over a row covers: CW = 128 columns of 64-bit entries, 64 of 128-bit ones
(piplib_amd/csrc/pip_advance.h, ET<T>::CPL).  The kernel picks the cut's constant out of wave 0's registers by (nvar /
CW, nvar % CPL, (nvar % CW) / CPL); the NVAR lists put that column last in a block, first in the next, and second, in
every block either width has, and end on the widest tableau integrer() takes: it answers PIPAMD_ST_MAXCOL from nvar + 1
>= PIPAMD_MAXCOL = 512 on (pip_advance.h phase G, csrc/pip_job.h), and both widths have column blocks for 512 columns
(csrc/pip_adv_inst.h: four of 128, eight of 64), so 510 unknowns each.
"""
import functools
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

import bigint_pip as bp

SEED, DRAWS = 5, 6000
BIT_LENGTHS = (4, 30, 31, 32, 33, 40, 61, 62, 63)
NV, NI = 4, 3
PER_TAG = 2
CW = {64: 128, 128: 64}
MAXCOL = 512  # piplib_amd/csrc/pip_job.h PIPAMD_MAXCOL
NVAR_MAX = MAXCOL - 2
NVAR = {64: (5, 127, 128, 129, 255, 256, 257, 383, 384, NVAR_MAX),
        128: (5, 63, 64, 65, 127, 128, 191, 192, NVAR_MAX)}
D_BITS = (30, 31, 32, 33, 61, 62, 63)
TAGS = tuple("D%d" % b for b in D_BITS) + ("prod<=63", "prod>63", "delta=1", "delta>1", "rounds=0", "rounds=1", "rounds>=2",
                                           "nil", "cuts>=2")
# a product beyond 63 bits wraps in the 64-bit build: no case of that tag is exact there
TAGS_64 = tuple(t for t in TAGS if t != "prod>63")

# draws of the search under other seeds (see above)
PINNED = (
    [[-2, -2, 0, 1303761885582623922, 0], [3, -3, 0, 0, -2], [1, -1, -2, 2, 0]],
    [[0, 0, -1, 0, 0], [-1, 3, 1, 0, -2], [1, 0, 3, 1804454369934924660, -3]],
    [[3, 0, -3, 0, -2], [-3, 2216162485550425720, 0, 0, -2], [0, 0, -1, -2, 1]],
    [[1, 0, 2, 3, 0], [3, 0, 0, 0, -2], [-3, 1503663421420893106, -3, -1, 1]],
    [[3, 3, 0, -2, -3], [-3, 0, 0, 2, -5], [-2, 0, 3788536597134294867, -1, 2]],
    [[-1, -1, 2, 0, -8], [-3, -3, 0, 4167071541068511900, 3], [-1, 3, 0, 0, -5]],
)


@dataclass
class Small:
    """a kept draw: the tableau (3 rows of 4 unknowns | constant, Python ints), its tags, whether the 64-bit model is
    exact on it, and the 128-bit model's Result"""
    ineq: List[List[int]]
    tags: Tuple[str, ...]
    exact64: bool
    res: bp.Result


def in_search_space(m):
    """the tableau is one the search can draw: the ranges, and at most one entry outside them"""
    if len(m) != NI or any(len(r) != NV + 1 for r in m):
        return False
    out = [(i, j) for i in range(NI) for j in range(NV + 1)
           if not (-3 <= m[i][j] <= 3 if j < NV else -9 <= m[i][j] <= 3)]
    return len(out) <= 1 and all(abs(m[i][j]).bit_length() in BIT_LENGTHS for i, j in out)


def draws(seed=SEED, count=DRAWS):
    rng = np.random.default_rng(seed)
    for k in range(count):
        bl = BIT_LENGTHS[k % len(BIT_LENGTHS)]
        m = [[int(x) for x in rng.integers(-3, 4, size=NV)] + [int(rng.integers(-9, 4))] for _ in range(NI)]
        r, c = int(rng.integers(0, NI)), int(rng.integers(0, NV + 1))
        mag = (1 << (bl - 1)) | int(rng.integers(0, 1 << (bl - 1)))
        m[r][c] = mag if rng.integers(0, 2) else -mag
        yield m


def tags_of(res):
    tags = set()
    for D, delta, lam, rounds, big in res.stats.cut_log:
        if D.bit_length() in D_BITS:
            tags.add("D%d" % D.bit_length())
        tags.add("prod<=63" if big <= 63 else "prod>63")
        tags.add("delta=1" if delta == 1 else "delta>1")
        tags.add("rounds=%d" % rounds if rounds < 2 else "rounds>=2")
    if res.status == bp.ST_NIL:
        tags.add("nil")
    if res.cuts >= 2:
        tags.add("cuts>=2")
    return tuple(t for t in TAGS if t in tags)


def keep(m):
    """the Small of a draw the list can use, else None"""
    res = bp.solve(m, bits=128, deepest=True)
    if res.status not in (bp.ST_SOLUTION, bp.ST_NIL) or res.cuts < 1 or not res.stats.exact:
        return None
    D, _, lam, _, _ = res.stats.cut_log[0]
    if lam % D == 1:
        return None
    r64 = bp.solve(m, bits=64, deepest=True, stop_inexact=True)
    return Small(m, tags_of(res), r64.status is not None and r64.stats.exact, res)


@functools.lru_cache(maxsize=None)
def cases():
    """the list: PINNED, then the search's draws in order, each where a tag of its still wants a case of its kind"""
    out, have = [], {}
    for m in list(PINNED) + list(draws()):
        s = keep(m)
        if s is None:
            continue
        want = [t for t in s.tags if have.get((t, s.exact64), 0) < PER_TAG]
        if not want:
            continue
        for t in s.tags:
            have[t, s.exact64] = have.get((t, s.exact64), 0) + 1
        out.append(s)
    return tuple(out)


def columns(nvar, cw):
    """where embed() puts the four active columns: 0, the last column of a block, the first of the next, nvar - 1 -- the
    block boundary nearest the constant column that leaves the four apart; without one (a single block, or nvar - 1 on
    the only boundary) the middle of the row stands in"""
    b = cw * ((nvar - 2) // cw)
    if b < 2:
        b = nvar // 2
    cols = (0, b - 1, b, nvar - 1)
    assert 0 < b - 1 and b < nvar - 1, (nvar, cw)
    return cols


def embed(m, nvar, cw):
    """the small tableau `m` in nvar unknowns: (NI, nvar + 1) int64"""
    cols = columns(nvar, cw)
    rows = np.zeros((NI, nvar + 1), np.int64)
    for i in range(NI):
        for j in range(NV):
            rows[i, cols[j]] = m[i][j]
        rows[i, nvar] = m[i][NV]
    return rows


def project(res, nvar, cw):
    """(status, pivots, cuts, cut log, the active unknowns' solution) of a Result over an embedded tableau; the other
    unknowns must be 0 / 1"""
    cols = columns(nvar, cw)
    if res.sol_num is None:
        sol = None
    else:
        assert all(res.sol_num[j] == 0 and res.sol_den[j] == 1 for j in range(nvar) if j not in cols)
        sol = ([res.sol_num[j] for j in cols], [res.sol_den[j] for j in cols])
    return res.status, res.pivots, res.cuts, list(res.stats.cut_log), sol


@functools.lru_cache(maxsize=None)
def model(k, nvar, bits):
    """bigint_pip's Result for case k embedded in nvar unknowns, at `bits`"""
    return bp.solve(embed(cases()[k].ineq, nvar, CW[bits]), bits=bits, deepest=True)


def batch_of(ids, nvar, bits, size):
    """(rows, ids) of a batch of at least `size` tableaux: the cases `ids`, embedded, repeated in order"""
    reps = -(-size // len(ids))
    ids = list(ids) * reps
    return np.stack([embed(cases()[k].ineq, nvar, CW[bits]) for k in ids]), ids
