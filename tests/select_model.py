"""Python-int models of the functions that decide WHICH pivot is taken -- choisir_piv, tab_sort_rows, exam_coef -- and of
the per-row summaries (non-zero bitmap, sign summary, magnitude class, constant term) the device functions read, on the
small tableaux of tests/select_cases.py.  TEST INFRASTRUCTURE ONLY; tests/test_gpu_select_probe.py holds the shipped
device functions (through pipamd_debug_select, piplib_amd/csrc/pip_probe.hip) to these, word for word.

A tableau (`Tab`) is what the pivot kernels keep of one: `ref[k]` says what logical row k is -- a slot of `rows`, or
UNITBIT | column for a unit row (the identity on that column) -- and `rows[s]` holds the W entries of the real row in
slot s (unknowns, constant term in column nvar, parameters up to ncol).  Not every column needs a unit row here (the
probe holds at most 256 logical rows); every CANDIDATE column of a column-choice case has one, as in a real tableau.
"""
import struct
from dataclasses import dataclass, field
from fractions import Fraction
from typing import List

import numpy as np

import bigint_pip as bp

UNITBIT, UNITZERO, NOROW, BIG_I = 0x8000, 0x4000, 0xFFFF, 0x7FFFFFFF
UNIT, PLUS, MINUS, ZERO, CRITIC, UNKNOWN = bp.UNIT, bp.PLUS, bp.MINUS, bp.ZERO, bp.CRITIC, bp.UNKNOWN


@dataclass
class Tab:
    tag: str
    nvar: int
    ncol: int
    W: int
    ref: List[int]
    rows: List[List[int]]
    pivi: int = -1
    bigparm: int = -1
    den: List[int] = None
    fl: List[int] = None
    size: List[float] = None     # float32 values, per slot
    smax: float = 0.0
    extra: dict = field(default_factory=dict)

    def __post_init__(self):
        ni = len(self.rows)
        if self.den is None:
            self.den = [1] * ni
        if self.fl is None:
            self.fl = [UNKNOWN] * ni
        if self.size is None:
            self.size = [0.0] * ni
        assert all(len(r) == self.W for r in self.rows) and len(self.den) == len(self.fl) == len(self.size) == ni

    @property
    def ni(self):
        return len(self.rows)

    @property
    def nligne(self):
        return len(self.ref)

    def urow(self):
        """unknown column -> logical row of its unit row (NOROW: none in this tableau)"""
        u = [NOROW] * self.nvar
        for k, rf in enumerate(self.ref):
            if rf & UNITBIT:
                u[rf & 0x3FF] = k
        return u

    def srow(self):
        s = [NOROW] * self.ni
        for k, rf in enumerate(self.ref):
            if not rf & UNITBIT:
                s[rf] = k
        return s

    def nonzeros(self):
        """per slot, the (column, entry) pairs of the non-zero entries (kept: the same case runs on many flavours)"""
        if "nz" not in self.extra:
            self.extra["nz"] = [[(j, x) for j, x in enumerate(r) if x] for r in self.rows]
        return self.extra["nz"]

    def key(self):
        return (self.tag, self.nvar, self.ncol, self.W, tuple(self.ref), tuple(map(tuple, self.rows)), self.pivi, self.bigparm,
                tuple(self.den), tuple(self.fl), tuple(float(x) for x in self.size), float(self.smax))


def signed(x, W):
    x &= (1 << W) - 1
    return x - (1 << W) if x >> (W - 1) else x


def cell(t, k, j):
    """traiter.c valeur(): a unit row is its denominator (1) in its own column"""
    rf = t.ref[k]
    if rf & UNITBIT:
        return 1 if (rf & 0x3FF) == j else 0
    return t.rows[rf][j]


def candidates(t):
    prow = t.rows[t.ref[t.pivi]]
    return [j for j in range(min(t.nvar, t.ncol)) if prow[j] > 0]


# ------------------------------------------------------------------------------------------------ choisir_piv
def fold_column(t, W=None, seen=None):
    """The reference's fold (traiter.c:297-341; bigint_pip.pick_column on this representation): candidate by candidate,
    the first logical row with a non-zero cross product decides.  W: the cross product pivot * v[k][j] - v[k][pivj] * foo
    is formed in signed W-bit wrap-around arithmetic, which is choose_column_slow's definition; None: exactly.  seen: a list
    that takes the bit length of every exact product and difference the fold meets (nothing left W bits while all are
    below W)."""
    if t.pivi < 0:
        return -1
    prow = t.rows[t.ref[t.pivi]]
    pivj, pivot = -1, 0
    for j in candidates(t):
        foo = prow[j]
        if pivj < 0:
            pivj, pivot = j, foo
            continue
        x = 0
        for k in range(t.nligne):
            a, b = pivot * cell(t, k, j), cell(t, k, pivj) * foo
            x = a - b if W is None else signed(signed(a, W) - signed(b, W), W)
            if seen is not None and k != t.pivi:   # (the pivot row's own two products are equal: 0 in any width)
                seen.append(max(abs(a).bit_length(), abs(b).bit_length(), abs(a - b).bit_length()))
            if x != 0:
                break
        if x < 0:
            pivj, pivot = j, foo
    return pivj


def brute_column(t):
    """Independent of the fold: the candidate column j whose column divided by a_j is lexicographically smallest over the
    logical rows, the first such column on a full tie -- row by row, the columns with the minimal Fraction stay."""
    if t.pivi < 0:
        return -1
    prow = t.rows[t.ref[t.pivi]]
    left = candidates(t)
    if not left:
        return -1
    for k in range(t.nligne):
        if len(left) == 1:
            break
        q = [Fraction(cell(t, k, j), prow[j]) for j in left]
        m = min(q)
        left = [j for j, x in zip(left, q) if x == m]
    return left[0]


def magnitudes(t):
    """(bit length of the largest candidate a_j, of the largest |entry| of the other real rows) -- the two factors of the
    tournament's cross products, which skip the pivot row"""
    p = t.ref[t.pivi]
    prow = t.rows[p]
    cs = candidates(t)
    amax = max([prow[j] for j in cs] + [0])
    emax = max([abs(x) for s, r in enumerate(t.rows) if s != p for x in r] + [0])
    return amax.bit_length(), emax.bit_length()


# ------------------------------------------------------------------------------------------------ tab_sort_rows
def sort_ref(t):
    """ref[] after tab_sort_rows' selection loop (traiter.c:591-614) on the given sizes and smax: bigint_pip's loop"""
    ref = list(t.ref)

    def swap(a, b):
        ref[a], ref[b] = ref[b], ref[a]
    bp.selection_sort(t.nvar, t.nligne, float(t.smax), lambda i: ref[i] & UNITBIT, lambda i: float(np.float32(t.size[ref[i]])),
                      swap)
    return ref


# ------------------------------------------------------------------------------------------------ exam_coef
def _sgn(x):
    return MINUS if x < 0 else (PLUS if x > 0 else ZERO)


def exam_coef(t):
    """traiter.c:101-159 as written, on the row values: returns (the row returned -- nligne when no row is proven negative
    -- and the flags per slot afterwards)"""
    fl = list(t.fl)
    n = t.nligne

    def flag(i):
        rf = t.ref[i]
        return UNIT if rf & UNITBIT else fl[rf]
    if t.bigparm >= 0:
        for i in range(n):
            if flag(i) != UNKNOWN:
                continue
            x = t.rows[t.ref[i]][t.bigparm]
            if x < 0:
                fl[t.ref[i]] = MINUS
                return i, fl
            if x > 0:
                fl[t.ref[i]] = PLUS
    for i in range(n):
        if flag(i) != UNKNOWN:
            continue
        row = t.rows[t.ref[i]]
        ff = ZERO
        for j in range(t.nvar + 1, t.ncol):
            fff = _sgn(row[j])
            if fff != ZERO and fff != ff:
                if ff == ZERO:
                    ff = fff
                else:
                    ff = UNKNOWN
                    break
        fff = _sgn(row[t.nvar])
        if ff == PLUS:
            if fff == MINUS:
                ff = UNKNOWN
        elif ff == ZERO:
            ff = fff
        elif ff == MINUS:
            if fff != MINUS:
                ff = UNKNOWN
        fl[t.ref[i]] = ff
        if ff == MINUS:
            return i, fl
    return n, fl


# ------------------------------------------------------------------------------------------------ the row summaries
@dataclass(frozen=True)
class Geometry:
    """where column j sits in a row's non-zero bitmap, and the magnitude classes, of one flavour"""
    BITS: int       # width of the Entier T
    CPL: int        # columns per lane and chunk (general flavours)
    NCH: int
    lean: int = 0   # 0: row_publish; else the packed element's width (lean_publish)

    @property
    def WP(self):
        return {32: 128, 64: 256}[self.lean] if self.lean else self.NCH * 64 * self.CPL

    @property
    def NM(self):
        return {32: 2, 64: 4}[self.lean] if self.lean else self.NCH * self.CPL

    def bit(self, j):
        if self.lean == 32:
            return j & 1, j >> 1
        if self.lean == 64:
            return j >> 6, j & 63
        cw = 64 * self.CPL
        return self.CPL * (j // cw) + j % self.CPL, (j % cw) // self.CPL

    def cls(self, orall):
        if self.lean:
            return 1 if orall >> (self.lean // 2 - 1) else 0
        b4 = self.BITS // 4
        return 3 if orall >> (3 * b4 - 1) else (2 if orall >> (2 * b4 - 1) else (1 if orall >> (b4 - 1) else 0))


def _code(x):
    return 1 if x > 0 else (2 if x < 0 else 0)


def publish(t, g):
    """per slot (sig, rcls, cst, [nzm words]) as row_publish (pip_advance.h) / lean_publish (pip_lean.h) define them, from
    the row values; and the largest class (max_row_class)"""
    out = []
    has_parm = t.ncol > t.nvar + 1 and not g.lean
    for row, nzs in zip(t.rows, t.nonzeros()):
        nz = [0] * g.NM
        orall = 0
        for j, x in nzs:
            w, b = g.bit(j)
            nz[w] |= 1 << b
            orall |= abs(x)
        cst = row[t.nvar] if t.nvar < t.W else 0
        sig = _code(cst)
        if has_parm:
            ps = row[t.nvar + 1:t.ncol]
            sig |= (4 if any(x > 0 for x in ps) else 0) | (8 if any(x < 0 for x in ps) else 0)
            if t.bigparm >= 0:
                sig |= {0: 0, 1: 16, 2: 32}[_code(row[t.bigparm])]
        out.append((sig, g.cls(orall), cst, nz))
    return out, max([o[1] for o in out] + [0])


def float_bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def double_bits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]
