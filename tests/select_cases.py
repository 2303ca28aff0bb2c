"""Case lists of tests/test_gpu_select_probe.py: small tableaux, built by plain functions from fixed seeds, aimed at the
edges of the device functions that decide which pivot is taken (pip_advance.h: choose_column, choose_column_slow,
sort_rows, exam_rows; pip_lean.h: lean_choose_column).  Every case carries a tag, `family: detail`; a magnitude band is
appended as ` @aNeM` (candidates of the pivot row below 2^N, entries of the other rows below 2^M).
tests/test_select_cases.py (no GPU) checks the lists themselves.

Column choice: a case runs on EVERY flavour that admits it (admits(): the flavour's shape and its exactness rule,
recomputed from the true magnitudes) -- flavour_cases() is that filter and nothing else.
"""
import random

import numpy as np

import select_model as sm
from select_model import MINUS, PLUS, UNKNOWN, ZERO, CRITIC, UNITBIT, Geometry, Tab

# ------------------------------------------------------------------------------------------------ the flavours
# fn: pipamd_debug_select's code.  PB: width of the arithmetic the cross products are formed in; EB: every entry of every
# real row, the pivot row included, is below 2^EB in magnitude (what the flavour holds a row in).  The exactness rule of a
# tournament flavour (choose_column's comment "Exact while (max a_j) * (max |entry|) < 2^62" and its SMALL note;
# F::cross<SMALL> of the lean flavours): bitlen(max candidate a_j) + bitlen(max |entry| of the other rows) <= PB - 2.
FLAVOURS = {
    "C64S_1": dict(fn=0, geom=Geometry(64, 2, 1), PB=32, EB=15), "C64S_2": dict(fn=1, geom=Geometry(64, 2, 2), PB=32, EB=15),
    "C64S_4": dict(fn=2, geom=Geometry(64, 2, 4), PB=32, EB=15),
    "C64_1": dict(fn=3, geom=Geometry(64, 2, 1), PB=64, EB=63), "C64_2": dict(fn=4, geom=Geometry(64, 2, 2), PB=64, EB=63),
    "C64_4": dict(fn=5, geom=Geometry(64, 2, 4), PB=64, EB=63),
    "C128_1": dict(fn=6, geom=Geometry(128, 1, 1), PB=128, EB=127), "C128_4": dict(fn=7, geom=Geometry(128, 1, 4), PB=128, EB=127),
    "C128_8": dict(fn=8, geom=Geometry(128, 1, 8), PB=128, EB=127),
    "SLOW64": dict(fn=9, geom=Geometry(64, 2, 4), slow=True), "SLOW128": dict(fn=10, geom=Geometry(128, 1, 8), slow=True),
    "LI_S": dict(fn=11, geom=Geometry(64, 2, 1, lean=32), PB=32, EB=15), "LI_M": dict(fn=12, geom=Geometry(64, 2, 1, lean=32), PB=64, EB=31),
    "LL_S": dict(fn=13, geom=Geometry(128, 1, 4, lean=64), PB=64, EB=31), "LL_M": dict(fn=14, geom=Geometry(128, 1, 4, lean=64), PB=128, EB=63),
}
TOURNAMENT = [f for f, d in FLAVOURS.items() if not d.get("slow")]
FN_SORT, FN_EXAM1, FN_EXAM4 = 15, 16, 17
SLOTS, ROWS = 192, 256            # what the probe's tables hold ...
SLOTS_NW4, ROWS_NW4 = 320, 384    # ... and for exam_rows<i64, 4>
BANDS = ((15, 15), (31, 31), (47, 15), (15, 47), (63, 63), (95, 31), (31, 95))
WRAP_BANDS = ((40, 40), (63, 63), (62, 2), (100, 100), (127, 127))   # choose_column_slow only
COLS = (0, 1, 126, 127, 128, 255, 256, 448, 449, 510, 511)
DECIDERS = (0, 63, 64, 65, 127, 128)


def max_candidate_column(flavour):
    """the last column a candidate of this flavour can sit in (the lean kernels keep the constant term inside the row)"""
    g = FLAVOURS[flavour]["geom"]
    return g.WP - 2 if g.lean else g.WP - 1


def shape_fits(t, flavour):
    g = FLAVOURS[flavour]["geom"]
    if t.W > g.WP or t.W % 2 or t.nvar > g.WP or t.ni > SLOTS or t.nligne > ROWS or t.pivi < 0:
        return False
    if g.lean and (t.nvar >= min(g.WP, t.W) or t.ncol != t.nvar + 1):
        return False
    lim = 1 << (g.BITS - 1)
    return all(-lim <= x < lim for r in t.rows for x in r)


def admits(t, flavour):
    """the function's stated domain, from the case's true magnitudes"""
    f = FLAVOURS[flavour]
    if not shape_fits(t, flavour):
        return False
    if f.get("slow"):
        return True
    urow = t.urow()
    if any(urow[j] == sm.NOROW for j in sm.candidates(t)):
        return False
    if max([abs(x) for r in t.rows for x in r] + [0]).bit_length() > f["EB"]:
        return False
    ab, eb = sm.magnitudes(t)
    return ab + eb <= f["PB"] - 2


def flavour_cases(flavour, cases=None):
    return [t for t in (column_cases() if cases is None else cases) if admits(t, flavour)]


# ------------------------------------------------------------------------------------------------ building a tableau
class Build:
    """logical rows appended top to bottom; slots handed out in a shuffled order, so that slot order is not row order"""

    def __init__(self, tag, nvar, W=None, seed=0, ncol=None):
        self.tag, self.nvar = tag, nvar
        self.W = W if W is not None else (nvar + 2) & ~1
        self.ncol = ncol if ncol is not None else min(nvar + 1, self.W)
        self.rng = random.Random("%s/%d" % (tag, seed))
        self.items, self.pivi = [], -1

    def unit(self, j):
        assert 0 <= j < self.nvar
        self.items.append(UNITBIT | j)

    def real(self, d, piv=False):
        row = [0] * self.W
        for j, v in d.items():
            row[j] = v
        if piv:
            self.pivi = len(self.items)
        self.items.append(row)

    def fill(self, n, cands):
        """n logical rows that cannot separate the candidates: unit rows of other columns while there are any, and real
        rows that are zero in every candidate column and non-zero elsewhere"""
        used = {x & 0x3FF for x in self.items if isinstance(x, int)} | set(cands)
        free = [j for j in range(self.nvar) if j not in used]
        other = [j for j in range(self.W) if j not in cands]
        for i in range(n):
            if free and (i % 3 != 1 or not other):
                self.unit(free.pop(self.rng.randrange(len(free))))
            else:
                self.real({self.rng.choice(other): self.rng.choice((-3, -1, 1, 2)) for _ in range(2)})

    def tab(self, **kw):
        slots = [i for i, x in enumerate(self.items) if not isinstance(x, int)]
        perm = list(range(len(slots)))
        self.rng.shuffle(perm)
        rows, ref = [None] * len(slots), []
        where = dict(zip(slots, perm))
        for i, x in enumerate(self.items):
            if isinstance(x, int):
                ref.append(x)
            else:
                rows[where[i]] = x
                ref.append(where[i])
        return Tab(self.tag, self.nvar, self.ncol, self.W, ref, rows, pivi=self.pivi, **kw)


def _shape(cols):
    """(nvar, W) just wide enough for the candidate columns; a candidate in the last column of a 64-column chunk leaves no
    constant column (nvar == W): the only way to have a candidate in a flavour's last column, and choose_column never
    reads the constant term (the lean flavours, which keep it inside the row, do not get these)"""
    top = max(cols)
    if (top + 1) % 64 == 0:
        return top + 1, top + 1
    nvar = top + 1
    return nvar, (nvar + 2) & ~1


def scenario(tag, cols, a, layout, seed=0, extra=None):
    """candidates in columns `cols` (ascending: candidate c is the c-th remaining one) with pivot-row entries `a`;
    layout: ('p',) the pivot row; ('u', c) candidate c's unit row; ('r', [v_c ...]) a real row with entry v_c in candidate
    c's column; ('f', n) n rows that cannot separate the candidates; extra: entries of the pivot row elsewhere"""
    nvar, W = _shape(cols)
    b = Build(tag, nvar, W, seed)
    for it in layout:
        if it[0] == "p":
            d = dict(zip(cols, a))
            for j, v in (extra or {}).items():
                if j < W and j not in d:
                    d[j] = v
            b.real(d, piv=True)
        elif it[0] == "u":
            b.unit(cols[it[1]])
        elif it[0] == "r":
            d = dict(zip(cols, it[1]))
            if nvar < W:
                d[nvar] = b.rng.choice((-2, 0, 1))
            b.real(d)
        else:
            b.fill(it[1], cols)
    return b.tab()


def scaled(t, ab, eb, suffix=None):
    """the same tableau with the pivot row stretched to candidates just below 2^ab and the other real rows to entries just
    below 2^eb (positive factors: no ratio changes order)"""
    p = t.ref[t.pivi]
    amax = max([abs(x) for x in t.rows[p]] + [1])   # (the whole pivot row: its other entries stay within the band too)
    emax = max([abs(x) for s, r in enumerate(t.rows) if s != p for x in r] + [1])
    sa, se = ((1 << ab) - 1) // amax, ((1 << eb) - 1) // emax
    rows = [[x * (sa if s == p else se) for x in r] for s, r in enumerate(t.rows)]
    return Tab(t.tag + (suffix or " @a%de%d" % (ab, eb)), t.nvar, t.ncol, t.W, list(t.ref), rows, pivi=t.pivi)


# ------------------------------------------------------------------------------------------------ choisir_piv
def _structural():
    out = []
    small = (0, 1, 2, 3, 4, 5)
    # no candidate; one candidate
    for cols in ((0, 1, 2), (1, 62, 63)):
        out.append(scenario("none: negative and zero pivot row", cols, (-3, 0, -1), [("r", (1, 2, 3)), ("p",), ("u", 0), ("u", 1), ("u", 2)]))
    for c in COLS + (62, 63):
        out.append(scenario("one: col %d" % c, (c,), (3,), [("r", (2,)), ("p",), ("u", 0)], extra={0: -2}))
    # candidate columns at the register and chunk edges: the column wins on a real row, loses on it, and wins by its unit row
    sets = [(0, 1), (1, 62, 63), (0, 1, 126), (1, 126, 127), (63, 64, 65), (127, 128, 129), (1, 128, 255), (126, 255, 256), (255, 256, 257),
            (0, 64, 128, 192), (63, 127, 191, 255), (1, 448), (128, 449, 510), (447, 448, 449, 511), (0, 256, 510, 511), (2, 254), (0, 126)]
    for cols in sets:
        m = len(cols)
        for w in range(m):
            v = [2 * (c + 1) + 1 for c in range(m)]
            v[w] = -1
            units = [("u", c) for c in range(m)]
            out.append(scenario("col: %s, column %d wins on a real row" % (cols, cols[w]), cols, [c + 1 for c in range(m)],
                                [("p",), ("r", [1 * (c + 1) for c in range(m)]), ("r", v)] + units))
            out.append(scenario("col: %s, unit row of column %d last" % (cols, cols[w]), cols, [2] * m,
                                [("r", [4] * m), ("p",)] + [u for u in units if u[1] != w] + [("u", w)]))
        out.append(scenario("regs: tied columns %s in different registers" % (cols,), cols, [3] * m,
                            [("p",), ("r", [6] * m), ("r", [0] * (m - 1) + [-1])] + [("u", c) for c in range(m)]))
    # full ties over all real rows: the column whose unit row is last wins
    for m, lo in ((2, 0), (3, 0), (64, 0), (64, 1), (65, 0), (130, 0)):
        cols = tuple(range(lo, lo + m))
        a = [1 + c % 3 for c in range(m)]
        real = [("r", [k * x for x in a]) for k in (2, -1, 0, 3)]
        for order in ("up", "down", "mixed"):
            idx = list(range(m))
            if order == "down":
                idx.reverse()
            elif order == "mixed":
                random.Random(m).shuffle(idx)
            units = [("u", c) for c in idx]
            out.append(scenario("tie%d: units %s below the real rows" % (m, order), cols, a, real[:2] + [("p",)] + real[2:] + units))
            out.append(scenario("tie%d: nel == count, units %s above the next real row" % (m, order), cols, a,
                                real[:1] + [("p",)] + units + [("r", [-(c + 1) for c in range(m)])] + real[1:]))
            h = m // 2
            out.append(scenario("tie%d: units %s around a real row" % (m, order), cols, a,
                                real[:1] + units[:h] + real[1:3] + [("p",)] + units[h:] + real[3:]))
    # the deciding real row at the edges of the 64-row block loop, the pivot row on either side
    for R in DECIDERS:
        for w in range(3):
            for side in ("lo", "hi"):
                if side == "lo" and R == 0:
                    continue
                v = [5, 5, 5]
                v[w] = 2
                pre = [("f", R - 1), ("p",)] if side == "lo" else [("f", R)]
                if side == "lo" and R > 2:
                    pre = [("f", R // 2), ("p",), ("f", R - 1 - R // 2)]
                post = [] if side == "lo" else [("f", 1), ("p",)]
                for cols in ((0, 1, 2), (1, 3, 70)):
                    out.append(scenario("decide%d: pivi %s, candidate %d of %s" % (R, side, w, cols), cols, (1, 1, 1),
                                        pre + [("r", v)] + post + [("u", 0), ("u", 1), ("u", 2)]))
    # a unit row of a tied column just above / just below the deciding real row (row kk - 1 and kk + 1: the knock-out test
    # `u < kk` cannot meet u == kk, a unit row and a real row never share a logical row)
    for pre in (0, 62, 63, 64):
        for cols in ((0, 1, 2), (2, 5, 9)):
            base = [("f", pre), ("p",), ("r", (2, 4, 6))]
            out.append(scenario("unit-above: row %d" % (pre + 2), cols, (1, 2, 3), base + [("u", 0), ("r", (-5, 1, 9)), ("u", 1), ("u", 2)]))
            out.append(scenario("unit-below: row %d" % (pre + 3), cols, (1, 2, 3), base + [("r", (-5, 1, 9)), ("u", 0), ("u", 1), ("u", 2)]))
            out.append(scenario("nel: every unit row above the next real row %d" % (pre + 5), cols, (1, 2, 3),
                                base + [("u", 2), ("u", 0), ("u", 1), ("r", (9, 1, -5))]))
            out.append(scenario("knock1: unit knock-outs leave one column, row %d" % (pre + 4), cols, (1, 2, 3),
                                base + [("u", 2), ("u", 0), ("r", (-9, 7, -5)), ("u", 1)]))
            out.append(scenario("zero-in-tied: a real row zero in the tied columns, row %d" % (pre + 2), cols + (cols[-1] + 1,), (1, 2, 3, 1),
                                base[:2] + [("r", (2, 4, 6, 9)), ("r", (0, 0, 0, 7)), ("r", (3, 1, 1, 0)), ("u", 0), ("u", 1), ("u", 2), ("u", 3)]))
            out.append(scenario("knocked-only: a real row non-zero only in knocked-out columns, row %d" % (pre + 4), cols + (cols[-1] + 1,),
                                (1, 2, 3, 1), base[:2] + [("r", (2, 4, 6, 2)), ("u", 0), ("u", 1), ("r", (-7, 5, 0, 0)), ("r", (1, 1, 9, 2)),
                                                          ("u", 2), ("u", 3)]))
    # tournament rounds
    for cols in (small, (1, 63, 64, 66, 100, 101)):
        units = [("u", c) for c in range(6)]
        out.append(scenario("first-not-min: descending ratios", cols, (1, 1, 1, 1, 1, 1), [("p",), ("r", (9, 7, 5, 3, 2, 1))] + units))
        out.append(scenario("first-not-min: minimum in the middle", cols, (2, 3, 1, 4, 1, 2), [("p",), ("r", (9, 7, -5, 3, 2, 1))] + units))
        out.append(scenario("several-then-tie: smaller set ties", cols, (1, 1, 1, 1, 1, 1), [("p",), ("r", (5, 2, 3, 2, 4, 2)), ("r", (0, 3, 0, 1, 0, 2))] + units))
        out.append(scenario("several-then-tie: smaller set ties, units decide", cols, (1, 2, 1, 2, 1, 3),
                            [("r", (5, 4, 3, 4, 4, 6)), ("p",), ("u", 3), ("u", 1), ("u", 5)] + [("u", c) for c in (0, 2, 4)]))
        out.append(scenario("several-then-tie: three rounds", cols, (1, 1, 1, 1, 1, 1), [("p",), ("r", (9, 5, 7, 3, 3, 4)), ("r", (1, 1, 1, 2, 1, 0))] + units))
        out.append(scenario("equal-ratio: 1/2 and 2/4", cols[:3], (2, 4, 6), [("p",), ("r", (1, 2, 3)), ("r", (4, 8, 11)), ("u", 0), ("u", 1), ("u", 2)]))
        out.append(scenario("equal-ratio: -1/2 and -2/4, then zero rows", cols[:3], (2, 4, 1), [("r", (-1, -2, 0)), ("r", (0, 0, 0)), ("p",), ("r", (3, 6, 5)),
                                                                                                 ("u", 1), ("u", 0), ("u", 2)]))
    # negative and zero entries, random layouts (many ties: small values)
    rng = random.Random(20240611)
    for i in range(60):
        m = rng.choice((2, 3, 4, 6, 9))
        cols = tuple(sorted(rng.sample(range(rng.choice((10, 64, 130))), m)))
        a = [rng.randint(1, 3) for _ in range(m)]
        layout = [("p",)] + [("u", c) for c in range(m)] + [("r", [rng.randint(-3, 3) * rng.choice((0, 1, 1)) for _ in range(m)])
                                                              for _ in range(rng.randint(1, 6))] + [("f", rng.randint(0, 3))]
        rng.shuffle(layout)
        out.append(scenario("negzero: random %d" % i, cols, a, layout, extra={j: rng.randint(-3, 0) for j in range(0, cols[-1], 3)}))
    return out


def _maxima():
    """entries AT each band's maximum, and cross products that differ by 1 just below 2^(ab+eb)"""
    out = []
    units = [("u", 0), ("u", 1), ("u", 2)]
    for ab, eb in BANDS:
        A, E = (1 << ab) - 1, (1 << eb) - 1
        sfx = " @a%de%d" % (ab, eb)
        for i, signs in enumerate(((1, 1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, -1))):
            out.append(scenario("max: all entries at the maximum, signs %d%s" % (i, sfx), (0, 1, 2), (A, A, A),
                                [("p",), ("r", [s * E for s in signs]), ("r", [-E, E, -E])] + units, extra={3: -A}))
        # cross products a0 n1 - n0 a1 = -+1
        if ab == eb:
            pairs = [((A, A - 1), (E - 1, E - 2)), ((A - 1, A), (E - 2, E - 1))]
        elif ab > eb:
            k = (A - 1) // E
            pairs = [((k * E + 1, k * (E - 1) + 1), (E, E - 1)), ((k * (E - 1) + 1, k * E + 1), (E - 1, E))]
        else:
            k = (E - 1) // A
            pairs = [((A, A - 1), (k * A + 1, k * (A - 1) + 1)), ((A - 1, A), (k * (A - 1) + 1, k * A + 1))]
        for i, (a, n) in enumerate(pairs):
            assert abs(a[0] * n[1] - n[0] * a[1]) == 1
            for sg in (1, -1):
                out.append(scenario("near: cross products differ by 1, pair %d sign %d%s" % (i, sg, sfx), (0, 1), a,
                                    [("p",), ("r", [sg * x for x in n]), ("u", 0), ("u", 1)]))
        out.append(scenario("equal-ratio-large: a and 2a%s" % sfx, (0, 1, 2), (A // 2, 2 * (A // 2), A // 2),
                            [("p",), ("r", (E // 2, 2 * (E // 2), E // 2 + 1)), ("r", (-3, -6, 0))] + units))
    return out


def _wrapping():
    """choose_column_slow only: what the tournament's guard keeps away from it"""
    out = []
    units = [("u", 0), ("u", 1), ("u", 2)]
    for W in (64, 128):
        h, MIN, MAX = 1 << (W // 2), -(1 << (W - 1)), (1 << (W - 1)) - 1
        s = " W%d" % W
        out.append(scenario("wrap: a product of exactly 2^(W-1)" + s, (0, 1, 2), (h, 3, h), [("p",), ("r", (1, h // 2, h // 2)), ("r", (1, 2, 3))] + units))
        out.append(scenario("wrap: both products 2^(W-1)" + s, (0, 1, 2), (h, h // 2, 2), [("p",), ("r", (h, h // 2, 1)), ("r", (3, 2, 1))] + units))
        out.append(scenario("wrap: MIN entries" + s, (0, 1, 2), (3, 2, 1), [("p",), ("r", (MIN, MIN, MAX)), ("r", (MIN, 1, MIN))] + units, extra={3: MIN}))
        out.append(scenario("wrap: MIN entries, MAX candidates" + s, (0, 1, 2), (MAX, MAX - 1, MAX), [("r", (MIN, MAX, MIN)), ("p",), ("r", (1, MIN, -1))] + units))
        # non-zero exactly, zero mod 2^W: the fold moves on to the next row
        out.append(scenario("wrap: cross product 2^W, next row decides (less)" + s, (0, 1), (2 * h, h), [("p",), ("r", (0, h // 2 * 4)), ("r", (4, 1)), ("u", 0), ("u", 1)]))
        out.append(scenario("wrap: cross product 2^W, next row decides (more)" + s, (0, 1), (2 * h, h), [("p",), ("r", (0, 2 * h)), ("r", (1, 4)), ("u", 0), ("u", 1)]))
        out.append(scenario("wrap: cross product -2^W, the unit rows decide" + s, (0, 1), (h, 2 * h), [("p",), ("r", (2 * h, 0)), ("u", 1), ("u", 0)]))
        # unit rows in j's or pivj's column, under candidates whose product with 1 is all there is
        out.append(scenario("wrap: unit row in pivj's column first" + s, (0, 1, 2), (MAX, MAX, MAX), [("u", 0), ("p",), ("u", 1), ("r", (1, 1, 1)), ("u", 2)]))
        out.append(scenario("wrap: unit row in j's column first" + s, (0, 1, 2), (MAX, MAX, 2), [("u", 2), ("u", 1), ("p",), ("r", (MAX, MAX, MIN)), ("u", 0)]))
    return out


_COLUMN_CASES = None


def column_cases(fresh=False):
    """every column-choice case, safe or not; flavour_cases() gives a flavour the ones it admits.  (Built once and kept;
    fresh: built again, the kept list left alone.)"""
    global _COLUMN_CASES
    if _COLUMN_CASES is None or fresh:
        base = _structural()
        out = list(base)
        for i, t in enumerate(base):
            wide = t.W > 130 or t.ni > 40     # the widest and tallest ones: two bands each, in turn
            for k, (ab, eb) in enumerate(BANDS):
                if not wide or k % 4 == i % 4:
                    out.append(scaled(t, ab, eb))
            ab, eb = WRAP_BANDS[i % len(WRAP_BANDS)]
            if not wide or i % 3 == 0:
                out.append(scaled(t, ab, eb, " @wrap a%de%d" % (ab, eb)))
        out += _maxima() + _wrapping()
        if fresh:
            return out
        _COLUMN_CASES = out
    return _COLUMN_CASES


def family(t):
    return t.tag.split(":")[0]


def band(t):
    return t.tag.split(" @")[1] if " @" in t.tag else ""


def required_tags(flavour):
    """the tag families the issue lists, for the flavours they apply to (by the flavour's geometry and widths alone)"""
    f = FLAVOURS[flavour]
    g = f["geom"]
    top = max_candidate_column(flavour)
    need = {"none", "one", "tie2", "tie3", "unit-above", "unit-below", "nel", "knock1", "zero-in-tied", "knocked-only", "first-not-min",
            "several-then-tie", "equal-ratio", "negzero"}
    need |= {"decide%d" % R for R in DECIDERS}
    need |= {"tie%d" % m for m in (64, 65) if top + 1 >= m}
    if g.NM > 1:
        need.add("regs")
    if f.get("slow"):
        need.add("wrap")
    return need


def own_bands(flavour):
    """the magnitude bands at a tournament flavour's admitted maximum"""
    f = FLAVOURS[flavour]
    return [(ab, eb) for ab, eb in BANDS if max(ab, eb) <= f["EB"] and ab + eb == f["PB"] - 2]


# ------------------------------------------------------------------------------------------------ tab_sort_rows
SORT_N = (0, 1, 2, 63, 64, 65, 66, 130)
BIGF = 2147483648.0


def _sort_tab(tag, nvar, sizes, units_at, smax, pad=0):
    """logical rows nvar .. : one real row per entry of `sizes` (None: a unit row there), then `pad` rows of size smax"""
    rng = random.Random(tag)
    n = len(sizes)
    ref = [UNITBIT | j for j in range(nvar)]
    real = [i for i in range(n) if sizes[i] is not None]
    slots = list(range(len(real)))
    rng.shuffle(slots)
    slots += [len(real) + i for i in range(pad)]   # (the padded twin keeps the slots of the first n rows)
    size = [0.0] * len(slots)
    it = iter(slots)
    for i in range(n):
        if sizes[i] is None:
            ref.append(UNITBIT | (i % nvar))
        else:
            s = next(it)
            ref.append(s)
            size[s] = float(np.float32(sizes[i]))
    for _ in range(pad):
        s = next(it)
        ref.append(s)
        size[s] = float(np.float32(smax))
    W = (nvar + 2) & ~1
    rows = [[(s + 1) % 5 - 2] * W for s in range(len(slots))]
    return Tab(tag, nvar, nvar + 1, W, ref, rows, size=size, smax=float(smax))


def sort_cases():
    """(case, padded twin or None): the twin has never-picked rows (size == smax) appended until more than 64 rows are
    sorted, so that sort_rows takes its other branch on the same first n rows"""
    out = []
    rng = random.Random(77)
    for n in SORT_N:
        kinds = [("random", [float(rng.randint(0, 40)) for _ in range(n)]),
                 ("equal sizes", [float(rng.choice((3, 3, 7))) for _ in range(n)]),
                 ("sorted", [float(i) for i in range(n)]),
                 ("reverse", [float(n - i) for i in range(n)]),
                 ("zero and 2^31", [rng.choice((0.0, BIGF, 5.0, 1.5)) for _ in range(n)])]
        for name, sizes in kinds:
            top = max(sizes + [1.0])
            for sname, smax in (("smax the maximum", top), ("smax above all", top + 1), ("smax in the middle", sorted(sizes + [1.0])[len(sizes) // 2]),
                                ("all at or above smax", min(sizes + [1.0]))):
                for uname, where in (("no unit rows", ()), ("unit rows at the ends", (0, n - 1)), ("unit rows in the middle", (n // 2, n // 2 + 1, n // 3))):
                    sz = [None if i in where else s for i, s in enumerate(sizes)]
                    tag = "sort n=%d: %s, %s, %s" % (n, name, sname, uname)
                    t = _sort_tab(tag, 3, sz, where, smax)
                    twin = _sort_tab(tag, 3, sz, where, smax, pad=65 - n) if n <= 64 else None
                    if twin is not None:
                        twin.tag += " (padded)"
                    out.append((t, twin))
    return out


# ------------------------------------------------------------------------------------------------ exam_coef
EXAM_NI = {FN_EXAM1: (1, 63, 64, 65, 192), FN_EXAM4: (1, 63, 64, 65, 192, 256, 257)}


def _exam_tab(tag, ni, rowfn, nparm, big, flags=None, seed=0):
    """nvar = 2 unknowns; rowfn(k, i) -> (constant, [parameter coefficients]) of the i-th real row, at logical row k"""
    rng = random.Random("%s/%d/%d" % (tag, ni, seed))
    nvar = 2
    ncol = nvar + 1 + nparm
    W = (ncol + 1) & ~1
    upos = sorted(rng.sample(range(ni + nvar), nvar))
    slots = list(range(ni))
    rng.shuffle(slots)
    ref, rows, fl = [], [None] * ni, [UNKNOWN] * ni
    i = 0
    for k in range(ni + nvar):
        if k in upos:
            ref.append(UNITBIT | upos.index(k))
            continue
        c, ps = rowfn(k, i)
        row = [rng.randint(-2, 2) for _ in range(nvar)] + [c] + list(ps) + [0] * (W - ncol)
        s = slots[i]
        rows[s] = row
        ref.append(s)
        if flags:
            fl[s] = flags(k, i)
        i += 1
    return Tab("%s, ni=%d" % (tag, ni), nvar, ncol, W, ref, rows, bigparm=(nvar + 1 + big if big is not None else -1), fl=fl)


def exam_cases(fn):
    out = []
    for ni in EXAM_NI[fn]:
        rng = random.Random(ni)
        mid = ni // 2
        late = ni - 1
        # the first big-negative row, after big-positive rows and a big-zero row whose parameters alone say Minus
        for at in sorted({0, mid, late}):
            def rowfn(k, i, at=at):
                if i == at:
                    return 3, (-2, 1)
                if i == at - 1:
                    return -4, (0, -1)          # big zero; parameter rule alone: Minus -- must not be returned
                return (rng.randint(-2, 2), (rng.randint(0, 3), rng.randint(-2, 2))) if i < at else (rng.randint(-3, 3), (rng.randint(-3, 3), rng.randint(-3, 3)))
            out.append(_exam_tab("exam big-negative: row %d after big-positive and big-zero rows" % at, ni, rowfn, 2, 0))
        out.append(_exam_tab("exam no-big-negative: the parameter rule decides", ni,
                             lambda k, i: (rng.randint(-3, 3), (rng.randint(0, 2), rng.randint(-2, 2), rng.randint(-1, 1))), 3, 0))
        out.append(_exam_tab("exam paf: parameters all negative, constant zero", ni, lambda k, i: (0, (-1 - i % 3, -2)), 2, None))
        out.append(_exam_tab("exam both-signs: parameters of both signs", ni, lambda k, i: (rng.randint(-2, 2), (1 + i % 2, -1 - i % 3)), 2, None))
        for c in (-5, 0, 7):
            out.append(_exam_tab("exam no-parameter: constant %d" % c, ni, lambda k, i, c=c: (c if i == mid else abs(c), ()), 0, None))
            out.append(_exam_tab("exam zero-parameter: coefficients zero, constant %d" % c, ni, lambda k, i, c=c: (c if i >= mid else 1, (0, 0)), 2, None))
        out.append(_exam_tab("exam several-minus: the first logical one wins", ni,
                             lambda k, i: ((-1, (0, -1)) if i % 3 == 2 or i == late else (2, (1, 0))), 2, None))
        mixed = (PLUS, ZERO, CRITIC, UNKNOWN, UNKNOWN, MINUS, UNKNOWN)
        for seed in range(12):
            r2 = random.Random(seed * 1000 + ni)
            out.append(_exam_tab("exam mixed-flags: random %d" % seed, ni,
                                 lambda k, i: (r2.randint(-2, 2), (r2.randint(-1, 2) * r2.randint(0, 1), r2.randint(-2, 1) * r2.randint(0, 1))), 2,
                                 (1 if seed % 2 else None), flags=lambda k, i: r2.choice(mixed) if seed % 4 < 3 else (PLUS if i % 2 else UNKNOWN), seed=seed))
    return out


# ------------------------------------------------------------------------------------------------ the kernel's inline guard
GUARD_NVAR, GUARD_NI = 5, 5
CLASS_TOP = (15, 31, 47, 62)   # magnitude classes of 64-bit rows (cls_bits), the last one kept below the sign bit


def guard_tableaux(count_per_pair=8, seed=4242):
    """Small tableaux without parameters for whole solves.  On a fresh tableau the unit rows on top decide every first
    choisir_piv before a real row is reached, so each tableau starts with a harmless pivot.  Row A = (1, -e1 .. -e4 | -1) is
    the only row with a negative constant term and has one candidate, column 0, with pivot 1; it leaves (1, e1 .. e4 | 1)
    as logical row 0.  Row B = (-1, a1 + e1 .. a4 + e4 | 0) becomes (-1, a1 .. a4 | -1) by that pivot: the SECOND pivot row,
    whose candidates a_j are compared on logical row 0 first.  No other row touches column 0.  The a_j are of magnitude
    class ca, the e_j and the other rows' entries of class ce, over all pairs of classes.
    Returns (rows (B, ni, nvar + 1) int64, per tableau (exact column, 64-bit wrapped column, ca, ce) of that choice)."""
    rng = random.Random(seed)
    tabs, seconds = [], []
    for ca in range(4):
        for ce in range(4):
            A, E = (1 << CLASS_TOP[ca]) - 1, (1 << CLASS_TOP[ce]) - 1
            for rep in range(count_per_pair):
                def big(top):
                    return rng.randint(top // 2 + 1, top)
                e = [big(E) for _ in range(GUARD_NVAR - 1)]
                a = [big(A) * rng.choice((1, 1, 1, -1)) for _ in range(GUARD_NVAR - 1)]
                ineq = [[1] + [-x for x in e] + [-1], [-1] + [x + y for x, y in zip(a, e)] + [0]]
                for i in range(GUARD_NI - 2):
                    ineq.append([0] + [big(E) * rng.choice((1, -1, 0)) for _ in range(GUARD_NVAR - 1)] + [rng.randint(1, 50)])
                rng.shuffle(ineq)
                t = nth_choice(ineq, 2)
                if t is None or len(sm.candidates(t)) < 2:
                    continue
                assert not t.ref[0] & UNITBIT and t.rows[t.ref[0]][1:GUARD_NVAR] == e
                assert t.rows[t.ref[t.pivi]][1:GUARD_NVAR] == a
                tabs.append(ineq)
                seconds.append((sm.fold_column(t), sm.fold_column(t, 64), ca, ce))
    return np.array(tabs, dtype=np.int64), seconds


def nth_choice(ineq, n):
    """the tableau as the solve's n-th choisir_piv sees it (bigint_pip's pivot loop, exact: None when an earlier pivot
    leaves 64 bits, or the solve ends before)"""
    import bigint_pip as bp
    nvar, ni = len(ineq[0]) - 1, len(ineq)
    rows = [bp._Row(bp.UNIT, 1, None, i) for i in range(nvar)]
    rows += [bp._Row(bp.UNKNOWN, 1, np.array([int(x) for x in r], dtype=object)) for r in ineq]
    nligne = nvar + ni
    st, det = bp.Stats(64), [1]
    bp.sort_rows(rows, nvar, nligne)
    for step in range(n):
        pivi = next((i for i in range(nligne) if rows[i].flag & bp.MINUS), nligne)
        if pivi >= nligne:
            for i in range(nligne):   # exam_coef without parameters, as bigint_pip.solve
                r = rows[i]
                if r.flag != bp.UNKNOWN:
                    continue
                r.flag = bp._sgn(int(r.v[nvar]))
                if r.flag == bp.MINUS:
                    pivi = i
                    break
        if pivi >= nligne:
            return None
        if step == n - 1:
            break
        try:
            if bp.pivot_step(rows, det, pivi, nvar, ni, st) < 0:
                return None
        except bp.Overflow:
            return None
        if not st.exact:
            return None
    ref, real = [], []
    for r in rows:
        if r.flag & bp.UNIT:
            ref.append(UNITBIT | r.unit)
        else:
            ref.append(len(real))
            real.append([int(x) for x in r.v])
    return Tab("guard", nvar, nvar + 1, nvar + 1, ref, real, pivi=pivi)
