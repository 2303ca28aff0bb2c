"""The cases of tests/test_gpu_quast_step_probe.py: small tableaux aimed at the edges of the device tree's wave-level
steps (tests/quast_step_model.py has the steps; tests/test_quast_step_cases.py, no GPU, checks the lists).

`cases(fn, Wb, nb)`: the deterministic list of one function for entries of Wb bits and nb column blocks.  A list is the
width-free part (everything fits 64 bits; the same Case objects serve both widths, so a 64-bit case and its 128-bit twin
cannot drift apart) followed by the cases built around B = 2^(Wb-1), the width's edge.  `edges` on a case names the edges it
stands on; EDGES lists, per function, the names the CPU test asks for.
"""
import functools
import math

import quast_step_model as qm
from quast_step_model import (CRITIC, MINUS, PLUS, UNIT, UNKNOWN, ZERO, Case, QS_BUILD_SUB, QS_CLASSIFY, QS_CUT_CHAIN, QS_DEEPEN,
                              QS_FIND_QUOTIENT, QS_MAKE_CUT, QS_PIVOT, QS_SOLVE_PLAIN, QS_SORT)

JUNK = 0x5EED5EED   # what stands in the columns beyond ncol: never read, never written


class Lcg:
    def __init__(self, seed):
        self.x = seed & qm.M64

    def next(self, lo, hi):
        """an int in lo .. hi"""
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & qm.M64
        return lo + (self.x >> 33) % (hi - lo + 1)


def tableau(tag, fn, nvar, ncol, real, layout=None, W=None, spare_rows=0, spare_slots=0, **kw):
    """real: the real rows, each (entries[ncol], denominator, flag) or just the entries; layout: the logical rows, ("u",
    column) or ("r", slot), by default the unit rows of every unknown and then the real rows"""
    W = ncol if W is None else W
    rows = []
    for r in real:
        v, d, f = r if isinstance(r, tuple) else (r, 1, UNKNOWN)
        assert len(v) == ncol, tag
        rows.append((list(v) + [JUNK + j for j in range(W - ncol)], d, f))
    if layout is None:
        layout = [("u", j) for j in range(nvar)] + [("r", s) for s in range(len(rows))]
    flag, ref, den = [], [], []
    for kind, x in layout:
        if kind == "u":
            flag.append(UNIT), ref.append(x), den.append(1)
        else:
            flag.append(rows[x][2]), ref.append(x), den.append(rows[x][1])
    nligne = len(layout)
    flag += [ZERO] * spare_rows
    ref += [0] * spare_rows
    den += [1] * spare_rows
    val = [r[0] for r in rows] + [[JUNK] * W for _ in range(spare_slots)]
    return Case(tag, fn, nvar, ncol, flag, ref, den, val, nligne=nligne, **kw)


def small_rows(g, n, ncol, lo=-3, hi=3):
    return [[g.next(lo, hi) for _ in range(ncol)] for _ in range(n)]


# the geometries every function that walks columns or rows is run on: (nb, nvar, ncol, W)
GEOM = [(1, 2, 3, 4), (1, 2, 4, 4), (1, 3, 5, 8), (1, 60, 63, 64), (1, 61, 64, 64),
        (2, 62, 65, 66), (2, 63, 66, 68), (2, 64, 66, 70), (2, 65, 67, 72), (2, 63, 127, 128), (2, 120, 128, 128), (2, 65, 128, 128)]
TALL = [64, 65, 128, 129]   # nligne where the lane-per-row loops take a second and a third pass


def geom_tag(nb, nvar, ncol, W):
    return "nb%d nvar%d ncol%d W%d" % (nb, nvar, ncol, W)


# ------------------------------------------------------------------------------------------------ pivot_step
def _pivot_geometry():
    out = []
    g = Lcg(11)
    for nb, nvar, ncol, W in GEOM:
        for block in range(nb):
            rows = small_rows(g, 4, ncol)
            lo = 0 if block == 0 else 64
            hi = min(nvar, 64) - 1 if block == 0 else nvar - 1
            p = [0 if j < nvar else g.next(-3, 3) for j in range(ncol)]
            for j in (lo, (lo + hi) // 2, hi):
                p[j] = g.next(1, 3)
            p[nvar] = -1
            dpiv = g.next(1, 2)
            rows[1] = (p, dpiv, MINUS)
            rows[3] = (rows[3], 3, PLUS)
            # the real rows first: the tournament runs on them before the unit rows settle what is left
            layout = [("r", 0), ("r", 1)] + [("u", j) for j in range(nvar)] + [("r", 2), ("r", 3)]
            out.append(tableau("geometry %s pivot in block %d" % (geom_tag(nb, nvar, ncol, W), block), QS_PIVOT, nvar, ncol, rows,
                               layout, W, pivi=1, nb=nb, det=[5 * dpiv],   # (a pivot row's denominator divides the determinant)
                               edges=("ncol%d" % ncol, "ncol%%4=%d" % (ncol % 4), "pivot block %d" % block, "W>ncol" if W > ncol else "W=ncol")
                               + (("nvar%d" % nvar,) if nb == 2 and nvar in (63, 64, 65) else ())))
    for nligne in TALL:
        nvar, ncol, W = 4, 6, 8
        rows = small_rows(g, nligne - nvar, ncol)
        rows[0] = ([1, 2, 0, 1, -2, 0], 1, MINUS)
        for k in (nligne - nvar - 1, 57, 58):   # rows in the last pass and around the first boundary with work to do
            rows[k] = ([2, 3, -1, 4, 5, -6], 2, PLUS)
        layout = [("r", s) for s in range(58)] + [("u", j) for j in range(nvar)] + [("r", s) for s in range(58, nligne - nvar)]
        out.append(tableau("geometry nligne %d" % nligne, QS_PIVOT, nvar, ncol, rows, layout, W, pivi=0, edges=("nligne%d" % nligne,)))
    return out


def _pivot_choice():
    """the tournament: which column, on tableaux whose elimination stays small"""
    out = []

    def t(tag, p, above, below=(), edges=(), nb=1, units=True, **kw):
        ncol = len(p)
        nvar = ncol - 1
        rows = [list(r) for r in above] + [list(p)] + [list(r) for r in below]
        layout = [("r", s) for s in range(len(above) + 1)] + ([("u", j) for j in range(nvar)] if units else []) + \
                 [("r", len(above) + 1 + s) for s in range(len(below))]
        out.append(tableau(tag, QS_PIVOT, nvar, ncol, rows, layout, ncol + (ncol & 1), pivi=len(above), nb=nb, edges=edges, **kw))
    t("no positive entry", [0, -1, -2, -5], [[1, 2, 3, 4]], edges=("no positive",))
    t("single candidate", [0, 3, -2, -5], [[1, 2, 3, 4]], [[2, 5, 1, 1]], edges=("single candidate",))
    t("tie resolved at the first row", [2, 2, 2, -1], [[1, 3, 2, 0], [5, 5, 5, 5], [1, 1, 1, 1]], edges=("tie first",))
    t("tie resolved at the middle row", [2, 2, 2, -1], [[1, 1, 1, 0], [5, 4, 6, 5], [1, 1, 1, 1]], edges=("tie middle",))
    t("tie resolved at the last row", [2, 4, 2, -1], [[1, 2, 1, 0], [5, 10, 5, 5], [3, 6, 2, 1]], edges=("tie last",))
    t("tie carried through the pivot row to the unit rows", [2, 4, 2, -1], [[1, 2, 1, 0], [5, 10, 5, 5]], [[7, 1, 1, 1]], edges=("tie last",))
    t("tie never resolved ends on the lowest column; no unit row for it", [2, 4, 2, -1], [[1, 2, 1, 0], [5, 10, 5, 5]],
      [[3, 6, 3, 1]], edges=("tie never", "no unit row"), units=False)
    t("the unit rows settle it: each drops its own column", [1, 1, 1, -1], [], [[1, 2, 3, 4]], edges=("unit shortcut",))
    p = [0] * 101
    p[3], p[5], p[70], p[100] = 1, 1, 1, -1
    a = [0] * 101
    a[3], a[5], a[70] = 5, 2, 2
    b = [0] * 101
    b[3], b[5], b[70] = 0, 4, 3
    t("the tournament moves within block 0, then on to block 1", p, [a, b], edges=("blocks 0-1",), nb=2)
    a = [0] * 101
    a[3], a[5], a[70] = 5, 6, 2
    t("the tournament moves from block 0 to block 1 in one row", p, [a, b], edges=("blocks 0-1",), nb=2)
    p = [0] * 101
    p[3], p[70], p[90], p[100] = 1, 1, 1, -1
    a = [0] * 101
    a[3], a[70], a[90] = 2, 2, 2
    b = [0] * 101
    b[3], b[70], b[90] = 4, 5, 5
    t("the tournament stays tied through block 1 and ends back in block 0", p, [a, b], edges=("blocks 1-0",), nb=2)
    return out


def _pivot_elimination():
    """the row update on small values: multipliers (1, 0), the gcd fold four at a time, the exact division, the hints"""
    out = []

    def t(tag, rows, ncol, edges, nvar=None, W=None):
        nvar = ncol - 1 if nvar is None else nvar
        p = [1] + [0] * (ncol - 1)
        p[nvar] = -1
        allrows = [(p, 1, MINUS)] + rows
        layout = [("r", s) for s in range(len(allrows))] + [("u", j) for j in range(nvar)]
        out.append(tableau(tag, QS_PIVOT, nvar, ncol, allrows, layout, W or ncol + 2, pivi=0, edges=edges))
    t("foo == 0 over a denominator of 1: the row keeps its bits", [([0, 5, -7, 9, 2], 1, PLUS)], 5, ("foo0 oden1",))
    t("foo == 0 over a denominator that divides the row", [([0, 6, -12, 18, 24], 6, PLUS)], 5, ("foo0 oden",))
    t("foo == 0 over a denominator partly in the row", [([0, 8, -12, 20, 4], 12, PLUS)], 5, ("foo0 oden",))
    for tz, G in ((0, 3), (0, 15), (1, 6), (1, 2), (3, 40), (62, 1 << 62), (61, 3 << 61)):
        m = [0, 5, -7, -1, 3, 1, -2] if G < 1 << 60 else [0, 1, -1, -1, 1, 1, -1]
        t("exact division by G = 2^%d * %d, negative entries" % (tz, G >> tz), [([x * G for x in m], G, PLUS)], 7, ("G tz%d" % min(tz, 2),))
    for ncol in (5, 6, 7, 8):   # ncol % 4 = 1, 2, 3, 0
        first = [0, 12, 18, 7] + [6] * (ncol - 4)
        last = [0] + [6] * (ncol - 2) + [7]
        t("G drops to 1 in the first group of four, ncol %d" % ncol, [(first, 6, PLUS)], ncol, ("G first group",))
        t("G drops to 1 in the last group, ncol %d" % ncol, [(last, 6, PLUS)], ncol, ("G last group", "ncol%%4=%d" % (ncol % 4)))
        allg = [0] + [6 * (j - 3) for j in range(1, ncol)]
        t("G divides the whole row, ncol %d" % ncol, [(allg, 6, PLUS)], ncol, ("G tz1",))
    hints = [([s * 2, 1, 1, 1, 1], 1, f) for f in (PLUS, MINUS, ZERO, UNKNOWN, CRITIC) for s in (-1, 0, 1)]
    t("the sign hint of every (old flag, sign of foo)", hints, 5, ("sign hints",))
    t("rows over the denominators 1, 2 and 3",
      [([3, 5, -7, 9, 2], 1, PLUS), ([4, 6, 2, -8, 10], 2, PLUS), ([-6, 3, 9, 0, -3], 3, ZERO)], 5, ("role swap",))
    return out


def _pivot_fits32():
    """operands of the elimination at the line of the 32-bit path: each of lpiv, fo, dpiv, v, pj at 2^31 - 1, -2^31 and
    2^31 with the others small.  Everything fits 64 bits: exact results on either side of the line."""
    out = []
    for name, x in (("2^31-1", 2**31 - 1), ("-2^31", -2**31), ("2^31", 2**31), ("-2^31-1", -2**31 - 1)):
        for where in ("lpiv", "fo", "dpiv", "v", "pj"):
            if where == "lpiv" and x <= 0:
                continue   # a pivot is positive
            if where == "dpiv" and x <= 0:
                continue
            pivot = x if where == "lpiv" else 3
            foo = x if where == "fo" else 5
            dpiv = x if where == "dpiv" else 1
            v = x if where == "v" else 7
            pj = x if where == "pj" else -2
            p = [pivot, pj, 1, -1]   # one unknown: the column is settled, the constant and two parameters follow
            r = [foo, v, -4, 6]
            layout = [("r", 0), ("r", 1), ("u", 0)]
            out.append(tableau("fits32 line: %s = %s" % (where, name), QS_PIVOT, 1, 4, [(p, dpiv, MINUS), (r, 1, PLUS)], layout, 4, pivi=0, det=[dpiv],
                               edges=("fits32 " + name,)))
    return out


def _pivot_width(Wb):
    """around B = 2^(Wb-1)"""
    B = 1 << (Wb - 1)
    out = []
    layout = [("r", 0), ("r", 1), ("u", 0), ("u", 1)]
    pre = "[B = 2^%d] " % (Wb - 1)

    def cross(tag, p0, v1, edges, col2=0, p2=0):
        # row 0 above the pivot row: column 1's entry times p0 is the tournament's cross product; column 0 wins (0 / p0)
        rows = [([0, v1, col2], 1, PLUS), ([p0, 1, p2], 1, MINUS)]
        out.append(tableau(pre + tag, QS_PIVOT, 2, 3, rows, layout, 4, pivi=1, edges=edges))
    if Wb == 64:
        cross("cross product 7 * 1317624576693539401 = 2^63 - 1", 7, 1317624576693539401, ("cross B-1",))
    else:
        cross("cross product 1 * (2^127 - 1)", 1, B - 1, ("cross B-1",))
        cross("cross product 3 * ((2^127 - 2) / 3)", 3, (B - 2) // 3, ("cross B-1",))
    cross("cross product 2 * (B/2 - 1) = B - 2", 2, B // 2 - 1, ("cross B-1",))
    cross("cross product 2 * B/2 = B", 2, B // 2, ("cross B",))
    cross("an untied column's cross product leaves the width", 2, 1, ("cross untied",), col2=B // 2)
    # the tournament's order: columns 1, 2 and 3 are all smaller than column 0 in row 0, and from column 1 -- the LOWEST of them --
    # nothing is smaller.  Going on from column 3 instead would form P * V2 = B on the way to the same column.
    h = Wb // 2
    rows = [([9, 0, 1 << (h - 1), 3 << (h - 2), 0], 1, PLUS), ([1, 1, 1 << h, 1 << h, -1], 1, MINUS)]
    out.append(tableau(pre + "the tournament goes on from the lowest smaller column: no product of the others is formed", QS_PIVOT, 4, 5,
                       rows, [("r", 0), ("r", 1)] + [("u", j) for j in range(4)], 6, pivi=1, edges=("lowest smaller",)))
    # the negated pivot row
    out.append(tableau(pre + "the pivot row holds -B: its negation leaves the width", QS_PIVOT, 2, 3, [([1, 0, -B], 1, MINUS)],
                       [("r", 0), ("u", 0), ("u", 1)], 4, pivi=0, edges=("cneg B",)))
    out.append(tableau(pre + "the pivot row holds -(B - 1)", QS_PIVOT, 2, 3, [([1, 0, -(B - 1)], 1, MINUS)],
                       [("r", 0), ("u", 0), ("u", 1)], 4, pivi=0, edges=("cneg B-1",)))
    # elimination products at the width's edge: v * lpiv - pj * fo with pivot 2, foo 1
    for v, tag, e in ((B // 2 - 1, "v * lpiv = B - 2", "elim B-1"), (B // 2, "v * lpiv = B", "elim B"),
                      (-(B // 2), "v * lpiv = -B", "elim B-1"), (-(B // 2) - 1, "v * lpiv = -B - 2", "elim B")):
        rows = [([2, 0, -1], 1, MINUS), ([1, v, 0], 1, PLUS)]
        out.append(tableau(pre + "elimination: " + tag, QS_PIVOT, 2, 3, rows, layout, 4, pivi=0, edges=(e,)))
    for d, tag, e in ((B - 2, "difference B - 2 - (-1) = B - 1", "elim B-1"), (B - 1, "difference B - 1 - (-1) = B", "elim B")):
        rows = [([1, -1, -1], 1, MINUS), ([1, d, 0], 1, PLUS)]
        out.append(tableau(pre + "elimination: " + tag, QS_PIVOT, 2, 3, rows, layout, 4, pivi=0, edges=(e,)))
    for od, tag, e in ((B // 2 - 1, "lpiv * oden = B - 2", "elim B-1"), (B // 2, "lpiv * oden = B", "elim B")):
        rows = [([2, 0, -1], 1, MINUS), ([1, 0, 0], od, PLUS)]
        out.append(tableau(pre + "elimination: " + tag, QS_PIVOT, 2, 3, rows, layout, 4, pivi=0, edges=(e,)))
    # the determinant's limbs (traiter.c:412-446): EBW = Wb
    def det(tag, det, ldet, pivot, dpiv, edges):
        rows = [([pivot, 0, -1], dpiv, MINUS)]
        out.append(tableau(pre + tag, QS_PIVOT, 2, 3, rows, [("r", 0), ("u", 0), ("u", 1)], 4, pivi=0, det=det, ldet=ldet, edges=edges, ebw=True))
    det("pivot 1 over 1: the limb is left alone", [12345], 1, 1, 1, ("det skip",))
    det("pivot 1 over 1 with det[0] of EBW - 1 bits: a new limb", [1 << (Wb - 2)], 1, 1, 1, ("det skip EBW-1",))
    det("blen(det) + blen(ppivot) = EBW - 1: limb 0 takes it", [(1 << (Wb - 4)) + 5], 1, 3, 1, ("det EBW-1",))
    det("blen(det) + blen(ppivot) = EBW: a new limb", [(1 << (Wb - 3)) + 5], 1, 3, 1, ("det EBW",))
    det("limb 0 full, limb 1 takes it", [(1 << (Wb - 3)) + 5, 7], 2, 3, 1, ("det EBW",))
    det("a new limb with ldet + 1 == MAXDET - 1", [B - 1, B - 1], 2, 3, 1, ("det MAXDET-1",))
    det("a new limb with ldet + 1 == MAXDET", [B - 1, B - 1, B - 1], 3, 3, 1, ("det MAXDET",))
    det("dppiv cancelled across two limbs", [6, 35], 2, 4, 15, ("det cancel",))
    det("dppiv not cancelled by the limbs", [6, 35], 2, 4, 11, ("det dppiv",))
    return out


def _pivot_wide_G(Wb):
    """128-bit only: G with its trailing zeros across the words"""
    out = []
    if Wb == 128:
        for tz in (63, 64, 65, 125):
            G = 3 << tz if tz < 125 else 1 << tz
            m = [0, 1, -1, 1, -1]
            rows = [([1, 0, 0, 0, -1], 1, MINUS), ([x * G for x in m], G, PLUS)]
            out.append(tableau("exact division by G = 2^%d * %d" % (tz, G >> tz), QS_PIVOT, 4, 5, rows,
                               [("r", 0), ("r", 1)] + [("u", j) for j in range(4)], 6, pivi=0, edges=("G tz%d" % tz,)))
    return out


# ------------------------------------------------------------------------------------------------ classify_rows
def _classify():
    out = []
    g = Lcg(23)
    nvar, nparm = 2, 3
    ncol = nvar + 1 + nparm
    signs = {"+": [2, 0, 5], "-": [-1, -4, 0], "0": [0, 0, 0], "+-": [3, -2, 0], "-+": [0, -2, 7]}
    for ps, parms in signs.items():
        for cs, cst in (("-", -3), ("0", 0), ("+", 4)):
            rows = [([1, -1, cst] + parms, 1, UNKNOWN), ([0, 1, 1, 1, 1, 1], 1, UNKNOWN), ([0, 1, -1, -1, -1, -1], 1, UNKNOWN),
                    ([0, 1, 5, 0, 0, 0], 1, UNKNOWN)]
            out.append(tableau("parameters %s, constant %s" % (ps, cs), QS_CLASSIFY, nvar, ncol, rows, None, 8, edges=("signs",)))
    rows = [([1, 1, -1, 0, 0, 0], 1, CRITIC), ([1, 1, -1, 0, 0, 0], 1, PLUS), ([1, 1, -1, 0, 0, 0], 1, ZERO), ([1, 1, 1, 0, 0, 0], 1, UNKNOWN),
            ([1, 1, -1, -1, 0, 0], 1, UNKNOWN | CRITIC)]
    out.append(tableau("only Unknown rows are looked at", QS_CLASSIFY, nvar, ncol, rows, None, 8, edges=("critic",)))
    out.append(tableau("nparm = 0: the sign of the constant", QS_CLASSIFY, 2, 3, [[1, 1, 2], [1, 1, 0], [1, 1, -1], [1, 1, -2]], None, 4,
                       edges=("nparm0",)))
    # the big parameter's pass
    big = nvar + 1
    rows = [([1, 1, -5, 2, -1, -1], 1, UNKNOWN), ([1, 1, 5, 0, -1, 0], 1, UNKNOWN), ([1, 1, -5, 0, 1, 0], 1, UNKNOWN),
            ([1, 1, 5, -1, 9, 9], 1, UNKNOWN), ([1, 1, 5, 1, 0, 0], 1, UNKNOWN), ([1, 1, 5, -2, 0, 0], 1, UNKNOWN)]
    out.append(tableau("big parameter: positives marked, the first negative stops the pass, zeros wait", QS_CLASSIFY, nvar, ncol, rows,
                       None, 8, bigparm=big, edges=("bigparm stop",)))
    rows = [([1, 1, -5, 1, -1, -1], 1, UNKNOWN), ([1, 1, -5, 0, -1, 0], 1, UNKNOWN), ([1, 1, 5, 0, 1, 0], 1, UNKNOWN),
            ([1, 1, 5, 1, -9, 9], 1, UNKNOWN)]
    out.append(tableau("big parameter: no negative; a zero coefficient falls to the second pass", QS_CLASSIFY, nvar, ncol, rows, None, 8,
                       bigparm=big, edges=("bigparm zero",)))
    for nb, gv, gc, W in GEOM:
        if gc - gv - 1 < 1:
            continue
        rows = small_rows(g, 5, gc, -2, 2)
        out.append(tableau("geometry %s" % geom_tag(nb, gv, gc, W), QS_CLASSIFY, gv, gc, rows, None, W, nb=nb, bigparm=gc - 1,
                           edges=("ncol%d" % gc,) + (("nvar%d" % gv,) if nb == 2 and gv in (63, 64, 65) else ())))
        out.append(tableau("geometry %s, no big parameter" % geom_tag(nb, gv, gc, W), QS_CLASSIFY, gv, gc, rows, None, W, nb=nb,
                           edges=("ncol%d" % gc,)))
    for nligne in TALL:
        for first in sorted(x for x in {0, 63, 64, nligne - 1} if x < nligne):
            for bigp in (-1, big):
                rows = [[1, 1, 3, 1, 0, 2] for _ in range(nligne)]   # (real rows only: logical row = slot)
                rows[first] = [1, 1, -3, -1, 0, -2]
                if first + 1 < len(rows):
                    rows[first + 1] = [1, 1, -3, -1, 0, -2]   # behind the first Minus: stays Unknown
                out.append(tableau("nligne %d, first Minus at real row %d, bigparm %d" % (nligne, first, bigp), QS_CLASSIFY, nvar, ncol, rows,
                                   [("r", s) for s in range(len(rows))], 6, bigparm=bigp,
                                   edges=("nligne%d" % nligne, "first minus %s" % ("last" if first == nligne - 1 else first))))
    return out


# ------------------------------------------------------------------------------------------------ sort_rows
def _sort():
    out = []
    g = Lcg(37)
    nvar = 3

    def t(tag, rows, edges, layout=None, opts=0, nb=1, W=4, pos=None):
        out.append(tableau(tag, QS_SORT, nvar, 4, rows, layout, W, opts=opts, nb=nb, edges=edges, pos=pos))
    for n in (1, 2, 63, 64, 65, 127, 128):
        for opts in (0, qm.OPT_POS):
            rows = [[g.next(-9, 9), g.next(-9, 9), g.next(-9, 9), g.next(-99, 99)] for _ in range(n)]
            t("n = %d, keys 0..9 with equals%s" % (n, ", pos" if opts else ""), rows, ("n%d" % n,) + (("pos",) if opts else ()),
              opts=opts | (qm.OPT_SKEY if n > 64 else 0))
    t("n = 65 without skey", [[1, 2, 3, 4]] * 65, ("n65 no skey",))
    t("n = 129", [[1, 2, 3, 4]] * 129, ("n129",), opts=qm.OPT_SKEY)
    t("every key equals the maximum", [[5, -5, 1, 0], [-5, 2, 2, 1], [0, 0, 5, 2]], ("none below",))
    t("every key but the first is below the maximum", [[9, 0, 0, 0], [1, 0, 0, 1], [3, 0, 0, 2], [2, 0, 0, 3], [1, 0, 0, 4]], ("all below",))
    t("equal keys: the first of equals is taken", [[7, 0, 0, 0], [2, 0, 0, 1], [-2, 0, 0, 2], [0, 2, 0, 3], [1, 0, 0, 4], [0, 0, -1, 5]],
      ("first of equals",))
    units = [("u", 0), ("u", 1), ("u", 2), ("r", 0), ("u", 1), ("r", 1), ("r", 2), ("u", 2), ("r", 3)]
    for opts in (0, qm.OPT_POS):
        t("unit rows among the rows to sort%s" % (", pos[0] goes to the last of them" if opts else ""),
          [[7, 0, 0, 0], [2, 0, 0, 1], [5, 0, 0, 2], [1, 0, 0, 3]], ("units in range",) + (("pos0 unit",) if opts else ()), units, opts)
    t("entries no int holds over a denominator of 1", [[2**31, 0, 0, 0], [-2**31, 1, 0, 1], [2**31 - 1, 0, 0, 2], [5, -(2**31) - 1, 0, 3],
                                                        [3, 0, 0, 4], [2**40, 2, 0, 5]], ("int overflow den1",))
    t("quotients at +-2^31 and beyond", [([2**32, 0, 0, 0], 2, UNKNOWN), ([-2**32, 1, 0, 1], 2, UNKNOWN), ([2**32 - 2, 0, 0, 2], 2, UNKNOWN),
                                         ([-2**32 - 2, 3, 0, 3], 2, UNKNOWN), ([2**32 + 1, 0, 0, 4], 2, UNKNOWN), ([9, 0, 0, 5], 2, UNKNOWN),
                                         ([3 * 2**33, 7, 0, 6], 3, UNKNOWN)], ("trunc 2^31",))
    t("keys at 2^24 +- 1: the float key rounds, the bound does not", [[2**24 + 1, 0, 0, 0], [2**24, 0, 0, 1], [2**24 - 1, 0, 0, 2], [5, 0, 0, 3]],
      ("float 2^24",))
    t("keys at 2^24 +- 1 over a denominator", [([3 * (2**24 + 1), 0, 0, 0], 3, UNKNOWN), ([2**25, 0, 0, 1], 2, UNKNOWN),
                                               ([2**24 - 1, 0, 0, 2], 1, UNKNOWN), ([2**25 + 3, 0, 0, 3], 2, UNKNOWN)], ("float 2^24",))
    tall = [[(s * 7) % 23 + 1, 0, 0, s] for s in range(100)]
    tall[70] = [0, 0, 0, 70]   # the smallest key sits beyond row 64 and trades places with row 0
    for opts in (0, qm.OPT_POS):
        t("a swap across the 64 boundary%s" % (", pos" if opts else ""), tall, ("swap across 64",) + (("pos",) if opts else ()),
          opts=opts | qm.OPT_SKEY)
    tall24 = [[2**24 + 1 - (s & 1), 0, 0, s] for s in range(66)] + [[2**24 - 1, 0, 0, 66], [2**24 + 9, 0, 0, 67]]
    t("a tall sort of keys 2^24 + 1 and 2^24 in turn: equal as floats, apart as ints", tall24, ("float 2^24", "first of equals"), opts=qm.OPT_SKEY)
    tallu = [("u", 0), ("u", 1), ("u", 2)] + [("r", s) for s in range(70)] + [("u", 1)] + [("r", s) for s in range(70, 100)] + [("u", 2)]
    t("a tall sort with unit rows in both halves, pos", tall, ("units in range", "pos0 unit"), tallu, qm.OPT_POS | qm.OPT_SKEY)
    return out


def _sort_wide():
    """128-bit only"""
    D = (1 << 70) + 12345
    rows = [([5 * D + 1, 0, 0, 0], D, UNKNOWN), ([-3 * D, 1 << 80, 0, 1], D, UNKNOWN), ([(1 << 100) + 1, 0, 0, 2], 1 << 99, UNKNOWN),
            ([D - 1, 0, 0, 3], D, UNKNOWN), ([(1 << 126), 0, 0, 4], 1 << 97, UNKNOWN), ([1 << 126, 0, 0, 5], 1 << 95, UNKNOWN)]
    return [tableau("128-bit entries above 2^64 over a 128-bit denominator", QS_SORT, 3, 4, rows, None, 4, edges=("wide entries",))]


# ------------------------------------------------------------------------------------------------ the cuts
def _cuts():
    out = []
    g = Lcg(41)
    D = 7

    def t(tag, fn, nvar, ncol, row, D, edges, bigparm=-1, W=None, nb=1):
        rows = [([1] * ncol, 1, PLUS), (row, D, PLUS)]
        layout = [("u", j) for j in range(1, nvar)] + [("r", 0), ("r", 1)]
        out.append(tableau("%s: %s" % (qm.FN_NAMES[fn], tag), fn, nvar, ncol, rows, layout, W or ncol + 2, pivi=len(layout) - 1,
                           bigparm=bigparm, nb=nb, edges=edges))
    # ok_var | ok_const | ok_parm
    for ok in range(8):
        row = [14, (D - 1 if ok & 1 else -7), 0, (-3 if ok & 2 else 21), (5 if ok & 4 else 0), -14]
        for fn in (QS_MAKE_CUT, QS_CUT_CHAIN):
            t("ok_var %d, ok_const %d, ok_parm %d" % (ok & 1, (ok >> 1) & 1, (ok >> 2) & 1), fn, 3, 6, row, D, ("ok%d" % ok,))
    t("entries negative, zero, multiples of D and D - 1", QS_MAKE_CUT, 4, 8, [-1, 0, 14, 6, -6, -8, 7, 13], D, ("residues",))
    t("the big parameter's column is forced to 0", QS_MAKE_CUT, 3, 7, [3, 4, 5, -3, 5, 5, 5], D, ("bigparm",), bigparm=5)
    t("the big parameter's column is the only parametric residue", QS_MAKE_CUT, 3, 7, [3, 4, 5, -3, 14, 5, 7], D, ("bigparm",), bigparm=5)
    for nb, nvar, ncol, W in GEOM:
        row = [g.next(-20, 20) for _ in range(ncol)]
        for fn in (QS_MAKE_CUT, QS_CUT_CHAIN):
            t("geometry %s" % geom_tag(nb, nvar, ncol, W), fn, nvar, ncol, row, 11, ("ncol%d" % ncol, "ncol%%4=%d" % (ncol % 4),
                                                                                   "W>ncol" if W > ncol else "W=ncol")
              + (("nvar%d" % nvar,) if nb == 2 and nvar in (63, 64, 65) else ()), W=W, nb=nb, bigparm=ncol - 1 if ncol > nvar + 1 else -1)
    # deepen: gcd(cst, D) > 1, lambda needing 0, 1 and several + dd steps, Bezout's 0
    seen = {}
    for DD in range(2, 40):
        for cst in range(0, -DD, -1):
            c = tableau("", QS_DEEPEN, 3, 4, [([1, 1, 1, 1], 1, PLUS), ([1, DD - 1, 2, cst], DD, PLUS)], [("r", 0), ("r", 1)], 4, pivi=1)
            o = qm.run(c, 64)
            key = (min(o.lambda_steps, 2), math.gcd(cst, DD) > 1, cst == 0)
            if seen.get(key, 0) < 2:
                seen[key] = seen.get(key, 0) + 1
                c.tag = "deepen D = %d, constant %d: %d steps of + dd" % (DD, cst, o.lambda_steps)
                c.edges = ("lambda steps %d" % min(o.lambda_steps, 2),) + (("gcd>1",) if key[1] and cst else ()) + (("bezout 0",) if cst == 0 else ())
                out.append(c)
    out.append(tableau("deepen: a constant that D divides, D = 1", QS_DEEPEN, 3, 4, [([1, 1, 1, 1], 1, PLUS), ([0, 0, 0, 0], 1, PLUS)],
                       [("r", 0), ("r", 1)], 4, pivi=1, edges=("bezout 0",)))
    return out


def _deepen_width(Wb):
    """lambda * c around B = 2^(Wb-1): D just above 2^(Wb/2), c = D - 1, the constant searched for a multiplier near D"""
    B = 1 << (Wb - 1)
    out = []
    below = above = None
    D0 = (1 << (Wb // 2)) - 60
    for DD in range(D0, D0 + 4000):
        if below is not None and above is not None:
            break
        for cst in (-1, -2, -3, -5, -7):
            c = tableau("", QS_DEEPEN, 2, 3, [([1, 1, 1], 1, PLUS), ([DD - 1, DD - 2, cst], DD, PLUS)], [("r", 0), ("r", 1)], 4, pivi=1)
            o = qm.run(c, Wb)
            if o.cls == "must" and above is None:
                c.tag, c.edges = "[B = 2^%d] deepen: lambda * c leaves the width, D = %d, constant %d" % (Wb - 1, DD, cst), ("lambda*c B",)
                above = c
            elif o.cls == "fits" and below is None and o.max_need >= B // 2:
                c.tag, c.edges = "[B = 2^%d] deepen: lambda * c in the width's last bit, D = %d, constant %d" % (Wb - 1, DD, cst), ("lambda*c B-1",)
                below = c
    assert below is not None and above is not None
    return [below, above]


# ------------------------------------------------------------------------------------------------ find_quotient
def _quotient(Wb):
    B = 1 << (Wb - 1)
    out = []
    nparm, CW = 4, 6

    def t(tag, cutv, ctx, edges, nc=None, nparm=nparm):
        ctx = [list(r) + [JUNK] * (CW - len(r)) for r in ctx]
        out.append(Case("[B = 2^%d] %s" % (Wb - 1, tag) if "c0 + D =" in tag else tag, QS_FIND_QUOTIENT, 1, 2, [UNIT], [0], [1], [[0, 0]], ctx=ctx, CW=CW, nc=len(ctx) if nc is None else nc,
                        nparm=nparm, cutv=list(cutv) + [0] * (CW + 2 - len(cutv)), edges=edges))
    # the cut  c0 = -3 | 2 5 0 0 | D = 7; parameter 2 is its quotient: + (2 5 7 0 | c0 + D - 1), - (-2 -5 -7 0 | -c0)
    cut = [-3, 2, 5, 0, 0, 7]
    plus, minus = [2, 5, 7, 0, 3], [-2, -5, -7, 0, 3]
    other = [[1, 0, 0, 0, 0], [0, 1, 0, -1, 5]]
    t("both defining rows", cut, other + [plus, minus], ("both rows",))
    t("both defining rows, the other way round", cut, [minus] + other + [plus], ("both rows",))
    t("only the + row", cut, other + [plus], ("one row",))
    t("only the - row", cut, other + [minus], ("one row",))
    for k, name in ((0, "a coefficient"), (3, "the tail"), (2, "D"), (4, "the constant")):
        for which in (0, 1):
            r = list(plus if which == 0 else minus)
            r[k] += 1
            t("near miss: %s of the %s row off by one" % (name, "+-"[which]), cut, other + ([r, minus] if which == 0 else [plus, r]),
              ("near miss " + name,))
    p3p, p3m = [2, 5, 0, 7, 3], [-2, -5, 0, -7, 3]
    t("two candidates: the highest parameter", cut, [plus, minus, p3p, p3m], ("two candidates",))
    t("the rows of a lower parameter only", [-3, 2, 0, 0, 0, 7], [[2, 7, 0, 0, 3], [-2, -7, 0, 0, 3]], ("both rows",))
    t("the last parameter takes part in the cut", [-3, 2, 5, 0, 1, 7], other + [plus, minus], ("cutv[nparm]",))
    t("a nonzero coefficient ends the search before the rows' parameter", [-3, 2, 0, 5, 0, 7], [[2, 7, 0, 0, 3], [-2, -7, 0, 0, 3]],
      ("search ends",))
    t("no context row", cut, [], ("nc0",))
    t("nparm = 0", [0, 7], [[5] + [0] * 4], ("nparm0",), nparm=0)
    for nc in (2, 64, 65):
        fill = [[1, 1, 1, 1, 1]] * (nc - 2)
        t("nc = %d, the rows last" % nc, cut, fill + [plus, minus], ("nc%d" % nc,))
        if nc > 2:
            t("nc = %d, the rows first and last" % nc, cut, [minus] + fill + [plus], ("nc%d" % nc,))
            t("nc = %d, the - row beyond nc" % nc, cut, fill + [plus, [0] * 5, minus], ("nc%d" % nc,), nc=nc)
    # c0 + D - 1 at the width's edge
    D = 7
    for c0, e in ((B - 1 - D, "c0+D B-1"), (B - D, "c0+D B"), (B - 1, "c0+D B")):
        t("c0 + D = %s" % ("B - 1" if c0 == B - 1 - D else ("B" if c0 == B - D else "B + D - 1")), [c0, 2, 5, 0, 0, D],
          [[2, 5, 7, 0, c0 + D - 1 if c0 + D - 1 < B else 0], [-2, -5, -7, 0, -c0]], (e,))
    return out


# ------------------------------------------------------------------------------------------------ build_sub
def _build_sub():
    out = []
    CW = 8

    def t(tag, nparm, nc, R, S, W, extra, edges):
        ctx = [[10 * r + j for j in range(CW)] for r in range(max(nc, 1))]
        out.append(Case(tag, QS_BUILD_SUB, 1, 2, [ZERO] * R, [0] * R, [5] * R, [[JUNK + j for j in range(W)] for _ in range(S)], ctx=ctx, CW=CW,
                        nc=nc, nparm=nparm, cutv=[100 + j for j in range(CW + 2)], opts=qm.OPT_EXTRA if extra else 0, det=[77, 78, 79, 80],
                        ldet=3, edges=edges))
    for extra in (0, 1):
        t("it fits exactly, extra %d" % extra, 3, 4, 7 + extra, 4 + extra, 8, extra, ("fits", "lanes beyond nparm"))
        t("a row short, extra %d" % extra, 3, 4, 6 + extra, 4 + extra, 8, extra, ("refusal",))
        t("a slot short, extra %d" % extra, 3, 4, 7 + extra, 3 + extra, 8, extra, ("refusal",))
        t("W = nparm + 1, extra %d" % extra, 3, 2, 8, 4, 4, extra, ("fits",))
        t("no parameters, extra %d" % extra, 0, 3, 8, 4, 2, extra, ("fits", "lanes beyond nparm"))
    t("no context row, the extra row alone", 7, 0, 10, 2, 8, 1, ("fits",))
    t("70 context rows: the rows' flags take a second pass", 2, 70, 80, 72, 4, 1, ("fits",))
    return out


# ------------------------------------------------------------------------------------------------ solve_plain
def _solve_plain():
    """small integer problems without parameters, picked from a deterministic stream by what the model says happens"""
    out = []
    g = Lcg(53)
    want = {}

    def problem(tag, nvar, ineq, deepest, budget=1000, spare=(8, 8), edges=()):
        return tableau(tag, QS_SOLVE_PLAIN, nvar, nvar + 1, ineq, None, nvar + 1 + (nvar & 1), spare_rows=spare[0], spare_slots=spare[1],
                       ni=len(ineq), deepest=deepest, budget=budget, edges=edges)
    for trial in range(400):
        nvar = 2 + trial % 2
        ni = 2 + trial % 3
        ineq = [[g.next(-4, 5) for _ in range(nvar)] + [g.next(-9, 9)] for _ in range(ni)]
        for deepest in (0, 1):
            c = problem("", nvar, ineq, deepest)
            o = qm.run(c, 64)
            found, bad, pivots = o.ret & 1, (o.ret >> 1) & 0x7FFF, o.ret >> 16
            if bad or o.cls != "fits":
                continue
            key = ("found" if found else "nil", min(o.cuts, 3), deepest)
            if want.get(key, 0) >= 3:
                continue
            want[key] = want.get(key, 0) + 1
            c.tag = "problem %d: %s after %d pivots and %d cuts, deepest %d" % (trial, key[0], pivots, o.cuts, deepest)
            c.edges = (key[0], "cuts %d" % key[1], "deepest %d" % deepest)
            out.append(c)
            if o.cuts >= 1 and want.get(("cap", deepest), 0) < 1:
                want[("cap", deepest)] = 1
                out.append(problem("problem %d, deepest %d, with no room for its %s cut" % (trial, deepest, "first" if o.cuts == 1 else "last"), nvar, ineq, deepest,
                                   spare=(o.cuts - 1, 8), edges=("rows cap",)))
                out.append(problem("problem %d, deepest %d, with no slot for its last cut" % (trial, deepest), nvar, ineq, deepest, spare=(8, o.cuts - 1),
                                   edges=("rows cap",)))
            if pivots >= 2 and want.get(("budget", deepest), 0) < 1:
                want[("budget", deepest)] = 1
                out.append(problem("problem %d, deepest %d, budget 0" % (trial, deepest), nvar, ineq, deepest, budget=0, edges=("budget 0",)))
                out.append(problem("problem %d, deepest %d, budget exactly met" % (trial, deepest), nvar, ineq, deepest, budget=pivots, edges=("budget met",)))
                out.append(problem("problem %d, deepest %d, budget one short" % (trial, deepest), nvar, ineq, deepest, budget=pivots - 1, edges=("budget short",)))
    out.append(problem("a row without a positive entry", 2, [[-1, -1, -1]], 0, edges=("nil no positive",)))
    # (a tableau in mid-solve: the first unknown is (2 s + 1) / 2 over a slack s, every sign settled)
    out.append(tableau("a fractional constant with nothing to cut with", QS_SOLVE_PLAIN, 2, 3, [([2, 0, 1], 2, PLUS), ([1, 0, 0], 1, PLUS)],
                       [("r", 0), ("u", 1), ("r", 1)], 4, spare_rows=2, spare_slots=2, ni=1, budget=10, edges=("nil fractional",)))
    out.append(problem("an integral answer at once", 2, [[1, 0, -3], [0, 1, -4]], 0, edges=("found",)))
    out.append(problem("65 rows to sort: beyond solve_plain's sort", 2, [[1, 1, -1]] * 65, 0, spare=(0, 0), edges=("rows sort",)))
    return out


# ------------------------------------------------------------------------------------------------ the lists
FUNCTIONS = {
    "classify_rows": (QS_CLASSIFY,), "sort_rows": (QS_SORT,), "pivot_step": (QS_PIVOT,), "cuts": (QS_MAKE_CUT, QS_DEEPEN, QS_CUT_CHAIN),
    "find_quotient": (QS_FIND_QUOTIENT,), "build_sub": (QS_BUILD_SUB,), "solve_plain": (QS_SOLVE_PLAIN,),
}
ONE_BLOCK = ("find_quotient", "build_sub", "solve_plain")   # as shipped: QK<QI, 1> only


@functools.lru_cache(maxsize=None)
def _free(name):
    """the width-free cases of a function group: all fit 64 bits"""
    if name == "classify_rows":
        return _classify()
    if name == "pivot_step":
        return _pivot_geometry() + _pivot_choice() + _pivot_elimination() + _pivot_fits32()
    if name == "cuts":
        return _cuts()
    if name == "build_sub":
        return _build_sub()
    if name == "solve_plain":
        return _solve_plain()
    if name == "sort_rows":
        return _sort()
    return []


@functools.lru_cache(maxsize=None)
def _edge(name, Wb):
    """the cases built around 2^(Wb-1)"""
    if name == "pivot_step":
        return _pivot_width(Wb) + _pivot_wide_G(Wb)
    if name == "sort_rows":
        return _sort_wide() if Wb == 128 else []
    if name == "cuts":
        return _deepen_width(Wb)
    if name == "find_quotient":
        return _quotient(Wb)
    return []


@functools.lru_cache(maxsize=None)
def all_cases(name, Wb):
    """every case of a function group at width Wb, whatever its column blocks: the 64-bit list is part of the 128-bit one,
    but for the cases whose determinant walk depends on the width (Case.ebw)"""
    out = list(_free(name)) + list(_edge(name, Wb))
    if Wb == 128:
        out += [c for c in _edge(name, 64) if not c.ebw and c.tag.startswith("[B = 2^63]")]
    return out


def cases(name, Wb, nb):
    """the list of one launch: function group, entry width, column blocks.  A case made for one block runs on two as well
    (the second block's lanes hold nothing); one made for two blocks needs them."""
    if nb == 2 and name in ONE_BLOCK:
        return []
    return [c for c in all_cases(name, Wb) if c.nb <= nb]


# per function group, the edges that must have a `fits` case, and those (a magnitude one step beyond) that must have a `must`
EDGES_FITS = {
    "pivot_step": ["ncol3", "ncol4", "ncol5", "ncol63", "ncol64", "ncol65", "ncol66", "ncol127", "ncol128", "nvar63", "nvar64", "nvar65",
                   "pivot block 0", "pivot block 1", "nligne64", "nligne65", "nligne128", "nligne129", "ncol%4=0", "ncol%4=1", "ncol%4=2",
                   "ncol%4=3", "W>ncol", "no positive", "single candidate", "tie first", "tie middle", "tie last", "tie never", "no unit row",
                   "unit shortcut", "blocks 0-1", "blocks 1-0", "lowest smaller", "cross B-1", "det skip", "det skip EBW-1", "det EBW-1", "det EBW",
                   "det MAXDET-1", "det cancel", "foo0 oden1", "foo0 oden", "fits32 2^31-1", "fits32 -2^31", "fits32 2^31", "G tz0", "G tz1",
                   "G tz2", "G first group", "G last group", "sign hints", "role swap", "cneg B-1", "elim B-1"],
    "classify_rows": ["signs", "critic", "nparm0", "bigparm stop", "bigparm zero", "ncol5", "ncol63", "ncol64", "ncol65", "ncol66", "ncol127",
                      "ncol128", "nvar63", "nvar64", "nvar65", "nligne64", "nligne65", "nligne128", "nligne129", "first minus 0",
                      "first minus 63", "first minus 64", "first minus last"],
    "sort_rows": ["n1", "n2", "n63", "n64", "n65", "n127", "n128", "n65 no skey", "n129", "none below", "all below", "first of equals",
                  "units in range", "int overflow den1", "trunc 2^31", "float 2^24", "pos", "pos0 unit", "swap across 64"],
    "cuts": ["ok%d" % k for k in range(8)] + ["residues", "bigparm", "ncol3", "ncol64", "ncol65", "ncol128", "nvar63", "nvar64", "nvar65",
                                             "W>ncol", "ncol%4=0", "ncol%4=1", "ncol%4=2", "ncol%4=3", "gcd>1", "lambda steps 0", "lambda steps 1", "lambda steps 2", "bezout 0", "lambda*c B-1"],
    "find_quotient": ["both rows", "one row", "near miss a coefficient", "near miss the tail", "near miss D", "near miss the constant",
                      "two candidates", "cutv[nparm]", "search ends", "nc2", "nc64", "nc65", "c0+D B-1"],
    "build_sub": ["fits", "refusal", "lanes beyond nparm"],
    "solve_plain": ["found", "nil", "nil no positive", "nil fractional", "cuts 0", "cuts 1", "cuts 2", "cuts 3", "deepest 0", "deepest 1", "rows cap",
                    "budget 0", "budget met", "budget short", "rows sort"],
}
EDGES_MUST = {
    "pivot_step": ["cross B", "det MAXDET", "det dppiv", "cneg B", "elim B"],
    "cuts": ["lambda*c B"],
    "find_quotient": ["c0+D B"],
}
EDGES_128 = {"pivot_step": ["G tz63", "G tz64", "G tz65", "G tz125"], "sort_rows": ["wide entries"]}
