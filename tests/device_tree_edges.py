"""Deterministic problem families that put the device-resident traiter() (piplib_amd/csrc/pip_quast.hip) exactly at a
capacity reserve of its box (quast_caps, piplib_amd/csrc/pip_tree.cpp) and one past it.  numpy only; TEST INFRASTRUCTURE.

Tableau columns: unknowns | constant | parameters.  Context rows: parameters | constant (the layout of every problem of
this suite: synth.random_problems, oracle/batchfmt.h).

The reserves (quast_caps):   24 fork frames;  min(10, 64 * blocks - ncol) spare columns for new parameters;  S - ni cut
rows, S = min(64, ni + 24) up to 56 inequalities and min(128, ni + 24) beyond;  CR = nc + 2 * newp + depth + 2 context
rows;  SS = min(64, CR + 17) slots of a compa_test sub-problem;  4096 tape cells (SOL_SIZE);  PIPAMD_MAXPARM = 50."""
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# pip_quast.h
Q_DONE, Q_VOID, Q_FALLBACK = 0, 1, 2
Q_WHY_OVERFLOW, Q_WHY_ROWS, Q_WHY_TAPE, Q_WHY_STACK, Q_WHY_OTHER = 1, 2, 4, 8, 16
Q_WHY_MASK = 31  # (the bits above say which check fired: diagnostics)
NOT_GIVEN = -1   # every word of the record of a problem the device tree was not given

DEPTH, NEWP, CUTS, SOL_SIZE, MAXPARM = 24, 10, 24, 4096, 50


@dataclass
class Problem:
    nvar: int
    nparm: int
    ni: int
    nc: int
    bigparm: int
    nq: int
    ineq: np.ndarray  # (ni, nvar+nparm+1) int64
    ctx: np.ndarray   # (nc, nparm+1) int64


def chain(d, pad=0, nnew=0, nc=0, idle=0, nq=1, bound=1000, v=1):
    """x0 - v >= 0;  d rows p_k - 1 >= 0 without unknowns: each forks, its else branch is void -- a nest d deep with d + 1
    leaves;  nnew unknowns with 2 y_j - q_j >= 0, each on a parameter of its own: one new parameter, one cut row and two
    context rows each;  pad unknowns in no row (nparm + 2 cells per leaf, a wider tableau);  idle parameters in no row;
    nc context rows with `bound` in column 0 and -1 in column 1 + k: as the solvers read a context row (parameters, then
    the constant) that is bound p_0 - p_(k+1) >= 0, whose compa_test sub-problems are fractional and cut.
    unknowns x0 | y | pad, parameters p | q | idle"""
    nvar, nparm = 1 + nnew + pad, d + nnew + idle
    ncol = nvar + nparm + 1
    T = np.zeros((1 + d + nnew, ncol), np.int64)
    T[0, 0], T[0, nvar] = 1, -v
    for k in range(d):
        T[1 + k, nvar + 1 + k], T[1 + k, nvar] = 1, -1
    for j in range(nnew):
        T[1 + d + j, 1 + j], T[1 + d + j, nvar + 1 + d + j] = 2, -1
    ctx = np.zeros((nc, nparm + 1), np.int64)
    for k in range(nc):  # (needs nparm > nc)
        ctx[k, 0], ctx[k, 1 + k] = bound, -1
    return Problem(nvar, nparm, T.shape[0], nc, -1, nq, T, ctx)


def wide(nparm, d, nnew):
    """chain(d, nnew=nnew) with idle parameters up to nparm"""
    return chain(d, nnew=nnew, idle=nparm - d - nnew)


def cuts(m, pad=0, v=0):
    """no parameters; m pairs x_k + 2 y_k - 1 >= 0 (lexmin x_k = 0, y_k = 1/2: one cut each, two pivots), pad rows
    x_k + y_k >= 0 that only raise ni.  v: the first pair is x_0 + 2 y_0 - (2 v + 1) >= 0, y_0 = v + 1 after its cut.
    (Not 2 x >= 1: tab_simplify removes that cut.)"""
    nvar = 2 * m
    T = np.zeros((m + pad, nvar + 1), np.int64)
    for k in range(m):
        T[k, 2 * k], T[k, 2 * k + 1], T[k, nvar] = 1, 2, -1 - (2 * v if k == 0 else 0)
    for r in range(pad):
        k = r % m
        T[m + r, 2 * k] = T[m + r, 2 * k + 1] = 1
    return Problem(nvar, 0, m + pad, 0, -1, 1, T, np.zeros((0, 1), np.int64))


def tree(k, pad=0, extra=0, v=1):
    """rows x_j + 1 - p_j >= 0, j < k (x_0 + v - p_0 >= 0 the first): both branches of every fork live, 2^k leaves;  pad
    unknowns in no row, extra parameters in no row.  cells = (2^k - 1)(nparm + 3) + 2^k (1 + nvar (nparm + 2))."""
    nvar, nparm = k + pad, k + extra
    T = np.zeros((k, nvar + nparm + 1), np.int64)
    for j in range(k):
        T[j, j], T[j, nvar], T[j, nvar + 1 + j] = 1, v if j == 0 else 1, -1
    return Problem(nvar, nparm, k, 0, -1, 1, T, np.zeros((0, nparm + 1), np.int64))


def tree_cells(k, pad=0, extra=0):
    nvar, nparm = k + pad, k + extra
    return (2 ** k - 1) * (nparm + 3) + 2 ** k * (1 + nvar * (nparm + 2))


def widen(p, ncol):
    """p with unknowns in no row added until the tableau has ncol columns"""
    add = ncol - (p.nvar + p.nparm + 1)
    assert add >= 0
    T = np.concatenate([p.ineq[:, :p.nvar], np.zeros((p.ni, add), np.int64), p.ineq[:, p.nvar:]], axis=1)
    return Problem(p.nvar + add, p.nparm, p.ni, p.nc, -1, p.nq, T, p.ctx)


def pip_matrices(p):
    """p as the PolyLib matrices of pip_solve: (inequnk, ineqpar), rows marker 1 | unknowns | parameters | constant and
    marker 1 | parameters | constant; tab_Matrix2Tableau builds p's own rows from them"""
    one = np.ones((p.ni, 1), np.int64)
    dom = np.concatenate([one, p.ineq[:, :p.nvar], p.ineq[:, p.nvar + 1:], p.ineq[:, p.nvar:p.nvar + 1]], axis=1)
    ctx = np.concatenate([np.ones((p.nc, 1), np.int64), p.ctx], axis=1)
    return dom, ctx


def if_depth(text):
    """deepest nest of (if ...) in a printed quast"""
    depth, best, stack = 0, 0, []
    i = 0
    while i < len(text):
        ch = text[i]
        if ch == "(":
            is_if = text.startswith("(if", i)
            stack.append(is_if)
            depth += is_if
            best = max(best, depth)
        elif ch == ")" and stack:
            depth -= stack.pop()
        i += 1
    return best


def newparms(text):
    return text.count("(newparm")


# ---- the CPU oracle as a library: cuts and cells straight from the authority
class _Oracle:
    def __init__(self, bits):
        self.L = L = C.CDLL(os.path.join(ROOT, "oracle", f"liboracle{bits}.so"))
        L.ora_new.restype = C.c_void_p
        L.ora_free.argtypes = [C.c_void_p]
        L.ora_solve_tableau.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p, C.c_int]
        for f in (L.ora_pivots, L.ora_cuts):
            f.argtypes, f.restype = [C.c_void_p], C.c_longlong
        L.ora_ncells.argtypes = [C.c_void_p]


_ORACLES = {}


def oracle_figures(p, bits=64, simplify=True):
    """dict(status, pivots, cuts, cells) of ora_solve_tableau on p (status: ORA_* of oracle/pip_oracle.h: 0 answered, 1 void,
    3 "Too much parameters", 5 "The solution is too complex")"""
    o = _ORACLES.get(bits) or _ORACLES.setdefault(bits, _Oracle(bits))
    L = o.L
    a = np.ascontiguousarray(p.ineq, np.int64)
    c = np.ascontiguousarray(p.ctx, np.int64)
    h = L.ora_new()
    try:
        st = L.ora_solve_tableau(h, p.nvar, p.nparm, p.ni, p.nc, p.bigparm, p.nq, a.ctypes.data, c.ctypes.data, int(simplify))
        return dict(status=st, pivots=L.ora_pivots(h), cuts=L.ora_cuts(h), cells=L.ora_ncells(h))
    finally:
        L.ora_free(h)


ORA_OK, ORA_VOID, ORA_ERR_PARMS, ORA_ERR_SOLSIZE = 0, 1, 3, 5


# ---- the members the tests run: name -> constructor.  Every one is used on the GPU
# (tests/test_gpu_device_tree_edges.py) and has its structural figures asserted on the CPU
# (tests/test_device_tree_edges_model.py).
def _w(ncol, nnew):
    return widen(chain(0, nnew=nnew), ncol)


MEMBERS = {
    # fork depth: 24 frames
    "chain23": lambda: chain(23), "chain24": lambda: chain(24), "chain25": lambda: chain(25),
    # new parameters, one block: 10 spare columns
    "new9": lambda: chain(0, nnew=9), "new10": lambda: chain(0, nnew=10), "new11": lambda: chain(0, nnew=11),
    # spare columns below 10: 60 columns leave 4; two blocks: 120 leave 8, 127 leave 1
    "cols60_new4": lambda: _w(60, 4), "cols60_new5": lambda: _w(60, 5),
    "cols120_new8": lambda: _w(120, 8), "cols120_new9": lambda: _w(120, 9),
    "cols127_new1": lambda: _w(127, 1), "cols127_new2": lambda: _w(127, 2),
    # cut rows: S = ni + 24;  S capped at 64 (ni = 56: 8);  the tall classes (ni = 57, 104: 24)
    "cuts24_ni24": lambda: cuts(24, 0), "cuts25_ni25": lambda: cuts(25, 0),
    "cuts24_ni40": lambda: cuts(24, 16), "cuts25_ni40": lambda: cuts(25, 15),
    "cuts8_ni56": lambda: cuts(8, 48), "cuts9_ni56": lambda: cuts(9, 47),
    "cuts24_ni57": lambda: cuts(24, 33), "cuts25_ni57": lambda: cuts(25, 32),
    "cuts24_ni104": lambda: cuts(24, 80), "cuts25_ni104": lambda: cuts(25, 79),
    # all reserves at once: forks and new parameters fill CR together
    "chain24_new10": lambda: chain(24, nnew=10), "chain25_new10": lambda: chain(25, nnew=10),
    "chain24_new11": lambda: chain(24, nnew=11),
    # full context: nc = 17 leaves the compa_test sub-problems no spare slot
    "chain24_new10_nc17": lambda: chain(24, nnew=10, nc=17),
    # parameter count: PIPAMD_MAXPARM = 50
    "wide49_2_0": lambda: wide(49, 2, 0), "wide48_1_1": lambda: wide(48, 1, 1), "wide47_1_2": lambda: wide(47, 1, 2),
    "wide49_0_1": lambda: wide(49, 0, 1), "wide48_0_2": lambda: wide(48, 0, 2), "wide50_0_0": lambda: wide(50, 0, 0),
    "wide50_1_0": lambda: wide(50, 1, 0),
    # tape: well clear, near the end, at and over SOL_SIZE
    "tree5_8_0": lambda: tree(5, 8, 0), "tree5_9_0": lambda: tree(5, 9, 0),
    "tree5_12_0": lambda: tree(5, 12, 0), "tree4_3_26": lambda: tree(4, 3, 26),
    "tree4_12_9": lambda: tree(4, 12, 9), "tree5_13_0": lambda: tree(5, 13, 0),
}
# tape members: name -> cells of the whole answer, by tree_cells (a tape of SOL_SIZE cells and more is refused: sol.c:97)
TAPE = {"tree5_8_0": 3192, "tree5_9_0": 3416, "tree5_12_0": 4088, "tree4_3_26": 4095, "tree4_12_9": 4096, "tree5_13_0": 4312}


def member(name):
    return MEMBERS[name]()


def neighbours(rounds=11):
    """[(problem, at its reserve?)]: at-reserve and one-past members taking turns, 6 per round -- fork depth, cut rows and
    tape; every round has values of its own (v), so no two tapes of the list are the same"""
    out = []
    for i in range(rounds):
        out += [(chain(24, v=1 + i), True), (chain(25, v=1 + i), False),
                (cuts(24, 16, v=i), True), (cuts(25, 15, v=i), False),
                (tree(5, 12, 0, v=1 + i), True), (tree(5, 13, 0, v=1 + i), False)]
    return out


# ---- the figures every edge rests on: name -> (oracle status, nested ifs, new parameters, ora_cuts, ora_ncells, pivots);
# None: not looked at (the reference abandons the problem).  The reference's own build gives the same (tests/golden/
# device_tree_edges/*.json hold its text, status and pivots).
def _cuts_fig(m):
    return (ORA_OK, 0, 0, m, 4 * m + 1, 2 * m)


FIGURES = {
    "chain23": (ORA_OK, 23, 0, 0, 647, 4348), "chain24": (ORA_OK, 24, 0, 0, 699, 4925), "chain25": (ORA_OK, 25, 0, 0, 753, 5551),
    "new9": (ORA_OK, 0, 9, 9, 363, 37), "new10": (ORA_OK, 0, 10, 10, 438, 41), "new11": (ORA_OK, 0, 11, 11, 520, 45),
    "cols60_new4": (ORA_OK, 0, 4, 4, 593, 17), "cols60_new5": (ORA_OK, 0, 5, 5, 709, 21),
    "cols120_new8": (ORA_OK, 0, 8, 8, 2131, 33), "cols120_new9": (ORA_OK, 0, 9, 9, 2363, 37),
    "cols127_new1": (ORA_OK, 0, 1, 1, 507, 5), "cols127_new2": (ORA_OK, 0, 2, 2, 760, 9),
    "cuts24_ni24": _cuts_fig(24), "cuts25_ni25": _cuts_fig(25), "cuts24_ni40": _cuts_fig(24), "cuts25_ni40": _cuts_fig(25),
    "cuts8_ni56": _cuts_fig(8), "cuts9_ni56": _cuts_fig(9), "cuts24_ni57": _cuts_fig(24), "cuts25_ni57": _cuts_fig(25),
    "cuts24_ni104": _cuts_fig(24), "cuts25_ni104": _cuts_fig(25),
    "chain24_new10": (ORA_OK, 24, 10, 10, 1854, 5205), "chain25_new10": (ORA_OK, 25, 10, 10, 1938, 5841),
    "chain24_new11": (ORA_OK, 24, 11, 11, 2008, 5233),
    "chain24_new10_nc17": (ORA_OK, 24, 10, 197, 1854, 5579),
    "wide49_2_0": (ORA_OK, 2, 0, 0, 158, 8), "wide48_1_1": (ORA_OK, 1, 1, 1, 208, 8), "wide47_1_2": (ORA_OK, 1, 2, 2, 310, 13),
    "wide49_0_1": (ORA_ERR_PARMS, None, None, None, None, None), "wide48_0_2": (ORA_ERR_PARMS, None, None, None, None, None),
    "wide50_0_0": (ORA_ERR_PARMS, None, None, None, None, None), "wide50_1_0": (ORA_ERR_PARMS, None, None, None, None, None),
    "tree5_8_0": (ORA_OK, 5, 0, 0, 3192, 232), "tree5_9_0": (ORA_OK, 5, 0, 0, 3416, 232),
    "tree5_12_0": (ORA_OK, 5, 0, 0, 4088, 232), "tree4_3_26": (ORA_OK, 4, 0, 0, 4095, 87),
    "tree4_12_9": (ORA_ERR_SOLSIZE, None, None, None, SOL_SIZE, None), "tree5_13_0": (ORA_ERR_SOLSIZE, None, None, None, SOL_SIZE, None),
}
# the reference's exit code where it abandons a problem: sol.c:97 exit(26), traiter.c:174 exit(1)
REF_EXIT = {ORA_ERR_SOLSIZE: 26, ORA_ERR_PARMS: 1}

# ---- what the device tree must do with a member alone in its call: name -> Q_WHY_* bits of the hand-back, 0: served.
# The flip points are quast_caps' documented reserves (the module's first lines), not the kernel's checks.
DEVICE = {
    "chain23": 0, "chain24": 0, "chain25": Q_WHY_STACK,
    "new9": 0, "new10": 0, "new11": Q_WHY_ROWS,
    "cols60_new4": 0, "cols60_new5": Q_WHY_ROWS, "cols120_new8": 0, "cols120_new9": Q_WHY_ROWS,
    "cols127_new1": 0, "cols127_new2": Q_WHY_ROWS,
    "cuts24_ni24": 0, "cuts25_ni25": Q_WHY_ROWS, "cuts24_ni40": 0, "cuts25_ni40": Q_WHY_ROWS,
    "cuts8_ni56": 0, "cuts9_ni56": Q_WHY_ROWS, "cuts24_ni57": 0, "cuts25_ni57": Q_WHY_ROWS,
    "cuts24_ni104": 0, "cuts25_ni104": Q_WHY_ROWS,
    "chain24_new10": 0, "chain25_new10": Q_WHY_STACK, "chain24_new11": Q_WHY_ROWS,
    "wide49_2_0": 0, "wide48_1_1": 0, "wide47_1_2": 0,
    "wide49_0_1": Q_WHY_OTHER, "wide48_0_2": Q_WHY_OTHER, "wide50_0_0": Q_WHY_OTHER, "wide50_1_0": Q_WHY_OTHER,
    # tape: well clear: served;  what the reference abandons (SOL_SIZE cells and more): handed back;  in between, as measured
    # on an MI355X: the device hands back from SOL_SIZE cells on, the reference's own limit, and serves 4095
    "tree5_8_0": 0, "tree5_9_0": 0, "tree5_12_0": 0, "tree4_3_26": 0, "tree4_12_9": Q_WHY_TAPE, "tree5_13_0": Q_WHY_TAPE,
}
