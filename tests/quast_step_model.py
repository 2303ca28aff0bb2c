"""Python-int models of the wave-level steps of the device tree (piplib_amd/csrc/pip_quast.hip): exam_coef
(traiter.c:101-159), tab_sort_rows (traiter.c:556-623), choisir_piv and pivoter (traiter.c:297-548), the cut of
integrer.c:342-400, the deepest cut (integrer.c:417-438) with bezout (integrer.c:98-150), find_parm (integrer.c:258-291),
the sub-problem of compa_test (traiter.c:196-233) and traiter() without parameters.  TEST INFRASTRUCTURE ONLY:
tests/test_gpu_quast_step_probe.py holds the shipped device functions (through pipamd_debug_quast_step,
piplib_amd/csrc/pip_probe.hip) to these, word for word.

Values are exact.  Separately `run(case, Wb)` says which named intermediates leave Wb bits (Wb = 64 or 128: the entry
width of the kernel's instantiation), and with that what the kernel owes on the case:

  fits  no product, sum or difference the step's formulae can form over columns < ncol and rows < nligne leaves Wb
        bits, and the determinant finds a limb: no Q_WHY_* bit beyond the model's, every output word as the model
  must  an intermediate the decision or the result needs leaves Wb bits -- a cross product or difference in a tied column
        of the pivot-column tournament, in an active row of the elimination, in the negated pivot row, lambda * c or a
        Bezout coefficient of the deepest cut, c0 + D - 1 of find_parm -- or the determinant finds no limb
        (traiter.c:424, 442): the return value carries Q_WHY_OVERFLOW; the image may be half rewritten and is not compared
  may   only an intermediate whose result is discarded leaves Wb bits (the cross product of a column that is no longer
        tied, which the tournament's lanes form all the same): a clean exact result or Q_WHY_OVERFLOW, nothing else

What this file takes from the kernel rather than from the reference is layout only: which lanes of `pos` a sort clears,
where `skey` keeps the keys of a tall sort, the result word of solve_plain, and the ORDER in which the tournament meets
its cross products (per row, every tied column against the lowest tied one, then against the lowest smaller one) --
the column it ends on is the lexicographic minimum of traiter.c:297-341, which tests/test_quast_step_cases.py checks by
brute force.
"""
import math
from dataclasses import dataclass
from fractions import Fraction
from typing import List

import numpy as np

import bigint_pip as bp
from select_model import float_bits

UNIT, PLUS, MINUS, ZERO, CRITIC, UNKNOWN = bp.UNIT, bp.PLUS, bp.MINUS, bp.ZERO, bp.CRITIC, bp.UNKNOWN
Q_WHY_OVERFLOW, Q_WHY_ROWS, Q_WHY_TAPE, Q_WHY_STACK, Q_WHY_OTHER = 1, 2, 4, 8, 16
MAXDET = bp.MAXDET
(QS_CLASSIFY, QS_SORT, QS_PIVOT, QS_MAKE_CUT, QS_DEEPEN, QS_CUT_CHAIN, QS_FIND_QUOTIENT, QS_BUILD_SUB,
 QS_SOLVE_PLAIN) = range(9)
FN_NAMES = ["classify_rows", "sort_rows", "pivot_step", "make_cut", "deepen", "make_cut+deepen", "find_quotient", "build_sub",
            "solve_plain"]
QS_HDR, QS_POS, QS_SKEY, QS_SKEY_FILL = 20, 128, 128, -2
OPT_POS, OPT_SKEY, OPT_EXTRA = 1, 2, 4
LDS_MAX = 65536
INT_MIN = -2**31
M64 = (1 << 64) - 1


@dataclass
class Case:
    """one case of pipamd_debug_quast_step: a tableau (flag / ref / den per logical row, val per slot), the determinant,
    and the context, cut vector and `pos` for the steps that read them"""
    tag: str
    fn: int
    nvar: int
    ncol: int
    flag: List[int]
    ref: List[int]
    den: List[int]
    val: List[List[int]]
    nligne: int = -1            # logical rows in use (default: all R)
    ni: int = 0
    bigparm: int = -1
    pivi: int = 0
    det: List[int] = None
    ldet: int = 1
    ctx: List[List[int]] = None
    CW: int = 1
    nc: int = 0
    nparm: int = 0
    cutv: List[int] = None
    deepest: int = 0
    budget: int = 0
    opts: int = 0
    pos: List[int] = None
    nb: int = 1                 # column blocks of the instantiation the case is meant for
    edges: tuple = ()           # names of the edges the case stands on (tests/test_quast_step_cases.py)
    ebw: bool = False           # the determinant walk of the case depends on the width: listed per width

    def __post_init__(self):
        if self.nligne < 0:
            self.nligne = len(self.flag)
        if self.det is None:
            self.det = [1, 0, 0, 0]
        self.det = list(self.det) + [0] * (MAXDET - len(self.det))
        if self.ctx is None:
            self.ctx = []
        if self.cutv is None:
            self.cutv = [0] * (self.CW + 2)
        if self.pos is None:
            self.pos = [0xAA] * QS_POS
        assert len(self.flag) == len(self.ref) == len(self.den) and len(self.cutv) == self.CW + 2
        assert all(len(r) == self.W for r in self.val) and all(len(r) == self.CW for r in self.ctx)

    @property
    def W(self):
        return len(self.val[0])

    @property
    def S(self):
        return len(self.val)

    @property
    def R(self):
        return len(self.flag)

    @property
    def CR(self):
        return len(self.ctx)

    def values(self):
        """every value of the image"""
        for x in self.det + self.den + self.cutv:
            yield x
        for r in self.val + self.ctx:
            for x in r:
                yield x

    def fits(self, Wb):
        return all(-(1 << (Wb - 1)) <= x < (1 << (Wb - 1)) for x in self.values())

    def lds_bytes(self, Wb):
        nv = 4 + self.R + self.S * self.W + self.CR * self.CW + self.CW + 2
        return Wb // 8 * nv + 8 * self.R + 16 + 4 * QS_SKEY + QS_POS

    def header(self):
        return [self.fn, self.W, self.S, self.R, self.nvar, self.ncol, self.nligne, self.ni, self.bigparm, self.pivi, self.CR,
                self.CW, self.nc, self.nparm, self.deepest, self.budget, self.opts, self.ldet, 0, 0]


class Must(Exception):
    """an intermediate the result needs left Wb bits"""


class Trk:
    """the intermediates of one run at width Wb"""

    def __init__(self, Wb):
        self.Wb, self.lo, self.hi, self.may = Wb, -(1 << (Wb - 1)), 1 << (Wb - 1), False
        self.stage = ""      # which step's intermediates are being noted: a Must carries it
        self.max_need = 0    # largest magnitude among the needed intermediates (the case lists aim it at the width's edge)

    def need(self, *vals):
        for x in vals:
            if abs(x) > self.max_need:
                self.max_need = abs(x)
            if not self.lo <= x < self.hi:
                raise Must(self.stage)
        return vals[-1]

    def idle(self, *vals):
        for x in vals:
            if not self.lo <= x < self.hi:
                self.may = True


@dataclass
class Out:
    """what the probe reports of a case: the image as the step left it, and the step's own results"""
    cls: str = "fits"
    ret: int = 0
    aux: int = 0
    ldet: int = 1
    flag: List[int] = None
    ref: List[int] = None
    pos: List[int] = None
    skey: List[int] = None
    det: List[int] = None
    den: List[int] = None
    val: List[List[int]] = None
    ctx: List[List[int]] = None
    cutv: List[int] = None
    cut: List[int] = None
    pivj: int = -1
    max_need: int = 0
    cuts: int = 0
    note: str = ""
    lambda_steps: int = 0


def _image(c, nb):
    return Out(ldet=c.ldet, flag=list(c.flag), ref=list(c.ref), pos=list(c.pos), skey=[QS_SKEY_FILL] * QS_SKEY, det=list(c.det),
               den=list(c.den), val=[list(r) for r in c.val], ctx=[list(r) for r in c.ctx], cutv=list(c.cutv), cut=[0] * (64 * nb))


def _sgn(x):
    return MINUS if x < 0 else (PLUS if x > 0 else ZERO)


# ------------------------------------------------------------------------------------------------ exam_coef
def classify_rows(o, nvar, ncol, bigparm, nligne):
    """traiter.c:101-159: the obvious signs of the Unknown rows; the first row proven negative ends it"""
    if bigparm >= 0:
        for i in range(nligne):
            if o.flag[i] != UNKNOWN:
                continue
            x = o.val[o.ref[i]][bigparm]
            if x < 0:
                o.flag[i] = MINUS
                return i
            if x > 0:
                o.flag[i] = PLUS
    for i in range(nligne):
        if o.flag[i] != UNKNOWN:
            continue
        r = o.val[o.ref[i]]
        ff = ZERO
        for j in range(nvar + 1, ncol):
            fff = _sgn(r[j])
            if fff != ZERO and fff != ff:
                if ff == ZERO:
                    ff = fff
                else:
                    ff = UNKNOWN
                    break
        fff = _sgn(r[nvar])
        if ff == PLUS:
            if fff == MINUS:
                ff = UNKNOWN
        elif ff == ZERO:
            ff = fff
        elif ff == MINUS:
            if fff != MINUS:
                ff = UNKNOWN
        o.flag[i] = ff
        if ff == MINUS:
            return i
    return nligne


# ------------------------------------------------------------------------------------------------ tab_sort_rows
def trunc_int(t):
    """(int)t as cvttsd2si has it: INT_MIN for what no int holds"""
    return INT_MIN if not (-2147483649.0 < t < 2147483648.0) else int(t)


def row_key(r, d, nvar):
    """traiter.c:579-585: max over the unknowns of abs((int)(coefficient / denominator)), in doubles; abs(INT_MIN) is
    INT_MIN and never wins"""
    s = 0.0
    dd = float(d)
    for x in r[:nvar]:
        a = trunc_int(float(x) / dd)
        a = a if a == INT_MIN else abs(a)
        s = max(s, float(a))
    return s


def sort_rows(o, nvar, nligne, want_pos, want_skey):
    """traiter.c:556-623 on the logical rows nvar .. nligne-1 (a row is its flag, slot and denominator; its size travels
    with it).  Returns the step's value: Q_WHY_ROWS | 256 for more rows than the kernel sorts."""
    n = nligne - nvar
    if n > 128 or (n > 64 and not want_skey):
        return Q_WHY_ROWS | 256
    size, ineq, smax = {}, {}, 0.0
    for i in range(nvar, nligne):
        ineq[i] = 0          # (a unit row's is never set: zero, as the oracle has it)
        size[i] = np.float32(0)
        if o.flag[i] & UNIT:
            continue
        s = row_key(o.val[o.ref[i]], o.den[i], nvar)
        size[i] = np.float32(s)
        smax = max(smax, s)
        ineq[i] = i - nvar

    def swap(a, b):
        for arr in (o.flag, o.ref, o.den, size, ineq):
            arr[a], arr[b] = arr[b], arr[a]
    bp.selection_sort(nvar, nligne, smax, lambda i: o.flag[i] & UNIT, lambda i: float(size[i]), swap)
    if n > 64:   # layout: a tall sort keeps the keys in skey, row by row
        for i in range(nvar, nligne):
            o.skey[i - nvar] = float_bits(size[i])
    if want_pos:  # layout: the lanes of pos the sort clears first
        for k in range(128 if n > 64 else 64):
            o.pos[k] = 0
        for i in range(nvar, nligne):
            o.pos[ineq[i]] = i & 0xFF
    return 0


# ------------------------------------------------------------------------------------------------ choisir_piv, pivoter
def cell(o, k, j, ncol):
    """traiter.c:246-252 valeur()"""
    if o.flag[k] & UNIT:
        return o.den[k] if o.ref[k] == j else 0
    return o.val[o.ref[k]][j] if j < ncol else 0


def brute_column(c):
    """choisir_piv by its definition: among the columns with a positive entry in the pivot row, the one whose column
    divided by that entry is lexicographically smallest, the lowest index among equals"""
    o = _image(c, c.nb)
    p = o.val[o.ref[c.pivi]]
    best, bk = -1, None
    for j in range(c.nvar):
        if p[j] <= 0:
            continue
        key = [Fraction(cell(o, k, j, c.ncol), p[j]) for k in range(c.nligne)]
        if best < 0 or key < bk:
            best, bk = j, key
    return best


def tournament(o, pivi, nvar, ncol, nligne, trk):
    """the pivot column, with the cross products noted as the lanes of the tournament form them"""
    trk.stage = "tournament"
    p = o.val[o.ref[pivi]][:ncol]
    tied = [j for j in range(nvar) if p[j] > 0]
    if not tied:
        return -1
    for k in range(nligne):
        if len(tied) <= 1:
            break
        if o.flag[k] & UNIT:
            tied = [j for j in tied if j != o.ref[k]]
            continue
        v = o.val[o.ref[k]][:ncol]
        if all(v[j] == 0 for j in tied):
            continue
        cc = tied[0]
        while True:
            x = {}
            for j in range(ncol):
                a, b = p[cc] * v[j], v[cc] * p[j]
                x[j] = a - b
                (trk.need if j in tied else trk.idle)(a, b, x[j])
            less = [j for j in tied if x[j] < 0]
            if not less:
                tied = [j for j in tied if x[j] == 0]
                break
            cc = less[0]
    return tied[0]


def pivot_step(o, pivi, nvar, ncol, nligne, trk):
    """traiter.c:345-548.  -1: no positive entry in the pivot row; else the Q_WHY_* bits of the step"""
    pivj = tournament(o, pivi, nvar, ncol, nligne, trk)
    o.pivj = pivj
    if pivj < 0:
        return -1
    pslot = o.ref[pivi]
    prow = np.array(o.val[pslot][:ncol], dtype=object)
    pivot, dpiv = int(prow[pivj]), o.den[pivi]
    det = o.det[:o.ldet]
    try:
        bp.det_update(det, pivot, dpiv, trk.Wb)
    except bp.Overflow:
        raise Must("determinant")
    trk.stage = "elimination"
    o.det[:len(det)] = det
    o.ldet = len(det)
    ku = -1
    for k in range(nligne):
        if o.flag[k] & UNIT:
            if o.ref[k] == pivj:
                ku = k
            continue
        if k == pivi:
            continue
        r = o.val[o.ref[k]]
        foo, oden = r[pivj], o.den[k]
        fff = _sgn(foo)
        if foo != 0 or oden != 1:
            d = math.gcd(pivot, foo)
            lpiv, fo = pivot // d, foo // d
            if oden != 1:
                trk.need(lpiv * oden)
            for j in range(ncol):
                if j == pivj:
                    trk.need(dpiv * fo)
                else:
                    trk.need(r[j] * lpiv, int(prow[j]) * fo, r[j] * lpiv - int(prow[j]) * fo)
            z, newden, _, _ = bp.row_update(np.array(r[:ncol], dtype=object), oden, prow, pivot, dpiv, pivj)
            r[:ncol] = [int(x) for x in z]
            o.den[k] = int(newden)
        if fff != ZERO and fff != o.flag[k]:   # traiter.c:518-529, on the sign of the old entry (dpiv > 0)
            o.flag[k] = (UNKNOWN if fff == MINUS else fff) if o.flag[k] == ZERO else UNKNOWN
    if ku < 0:
        return Q_WHY_OTHER
    trk.stage = "role swap"
    for j in range(ncol):
        o.val[pslot][j] = dpiv if j == pivj else trk.need(-int(prow[j]))
    o.flag[ku], o.ref[ku], o.den[ku] = PLUS, pslot, pivot
    o.flag[pivi], o.den[pivi], o.ref[pivi] = UNIT | ZERO, 1, pivj
    return 0


# ------------------------------------------------------------------------------------------------ the cuts
def make_cut(o, i, nvar, ncol, bigparm, width):
    """integrer.c:342-400: the cut of row i, `width` entries (zero beyond ncol), and ok_var | ok_const << 1 | ok_parm << 2"""
    D, r = o.den[i], o.val[o.ref[i]]
    cut = [0] * width
    for j in range(nvar):
        cut[j] = r[j] % D
    for j in range(nvar, ncol):
        cut[j] = 0 if j == bigparm else -((-r[j]) % D)
    ok_var = any(x > 0 for x in cut[:nvar])
    ok_const = cut[nvar] != 0
    ok_parm = any(x != 0 for x in cut[nvar + 1:ncol])
    return cut, (1 if ok_var else 0) | (2 if ok_const else 0) | (4 if ok_parm else 0)


def deepen(cut, D, nvar, trk):
    """integrer.c:417-438 with bezout (integrer.c:98-150), in place: bigint_pip.deepen under this run's width tracker"""
    trk.stage = "deepest cut"
    return bp.deepen(cut, D, nvar, trk.need, lambda k: setattr(trk, "lambda_steps", k))[0]


def find_quotient(o, CW, nc, nparm, trk):
    """integrer.c:258-291 find_parm over has_cut (integrer.c:229-254): the highest parameter that already is the quotient
    the cut cutv = c0 | c_params | D asks for, -1 if none"""
    cut = o.cutv

    def has_cut(p, c0, sign):
        for row in o.ctx[:nc]:
            if row[p] != sign * cut[1 + nparm] or row[nparm] != c0:
                continue
            if any(row[col] != 0 for col in range(p + 1, nparm)):
                continue
            if any(row[col] != sign * cut[1 + col] for col in range(p)):
                continue
            return True
        return False
    if cut[nparm] != 0:
        return -1
    cplus = trk.need(cut[0] + cut[1 + nparm], cut[0] + cut[1 + nparm] - 1)
    trk.need(-cut[0], -cut[1 + nparm])
    for p in range(nparm - 1, -1, -1):
        if cut[1 + p] != 0:
            break
        if has_cut(p, cplus, 1) and has_cut(p, -cut[0], -1):
            return p
    return -1


def build_sub(o, c):
    """traiter.c:196-233: the context under nparm unit rows, the extra row last; -1 where the tableau cannot hold it"""
    nparm, nc = c.nparm, c.nc
    ni = nc + (1 if c.opts & OPT_EXTRA else 0)
    if nparm + ni > c.R or ni > c.S:
        return -1
    for k in range(nparm + ni):
        o.flag[k], o.ref[k], o.den[k] = (UNIT, k, 1) if k < nparm else (UNKNOWN, k - nparm, 1)
    W = min(c.W, 64)
    for r in range(ni):
        src = o.ctx[r] if r < nc else c.cutv
        o.val[r][:W] = [src[j] if j <= nparm else 0 for j in range(W)]
    o.ldet, o.det[0] = 1, 1
    return ni


def solve_plain(o, c, trk):
    """traiter() of a tableau without parameters, integer solve: found | reasons << 1 | pivots << 16"""
    nvar, ni, ncol = c.nvar, c.ni, c.nvar + 1
    bad = sort_rows(o, nvar, nvar + ni, False, False)
    pivots = found = 0
    while not bad:
        nligne = nvar + ni
        pivi = next((i for i in range(nligne) if o.flag[i] & MINUS), nligne)
        if pivi >= nligne:
            pivi = classify_rows(o, nvar, ncol, -1, nligne)
        if pivi >= nligne:
            nil = False
            for i in range(nvar):
                if (o.flag[i] & UNIT) or o.den[i] == 1:
                    continue
                cut, ok = make_cut(o, i, nvar, ncol, -1, c.W)
                if not ok & 2:
                    continue
                if not ok & 1:
                    nil = True
                    o.note = "fractional constant, nothing to cut with"
                    break
                if c.deepest:
                    deepen(cut, o.den[i], nvar, trk)
                if nligne >= c.R or ni >= c.S:
                    bad |= Q_WHY_ROWS | 512
                else:
                    o.val[ni][:] = cut
                    o.flag[nligne], o.ref[nligne], o.den[nligne] = MINUS, ni, o.den[i]
                    o.cuts += 1
                pivi = nligne
                ni += 1
                break
            else:
                found = 1
                break
            if nil or bad:
                break
        pivots += 1
        pr = pivot_step(o, pivi, nvar, ncol, nvar + ni, trk)
        if pr < 0:
            o.note = "no positive entry"
            break
        bad |= pr
        if pivots > c.budget:
            bad |= Q_WHY_OTHER
    return found | (bad << 1) | (pivots << 16)


# ------------------------------------------------------------------------------------------------ a case, run
def run(c, Wb, nb=None):
    """the case at entry width Wb (and nb column blocks): an Out with its class"""
    nb = c.nb if nb is None else nb
    assert c.fits(Wb), c.tag
    o = _image(c, nb)
    trk = Trk(Wb)
    try:
        if c.fn == QS_CLASSIFY:
            o.ret = classify_rows(o, c.nvar, c.ncol, c.bigparm, c.nligne)
        elif c.fn == QS_SORT:
            o.ret = sort_rows(o, c.nvar, c.nligne, c.opts & OPT_POS, c.opts & OPT_SKEY)
        elif c.fn == QS_PIVOT:
            o.ret = pivot_step(o, c.pivi, c.nvar, c.ncol, c.nligne, trk)
        elif c.fn in (QS_MAKE_CUT, QS_DEEPEN, QS_CUT_CHAIN):
            if c.fn == QS_DEEPEN:
                cut = list(c.val[c.ref[c.pivi]]) + [0] * (64 * nb - c.W)
            else:
                cut, o.aux = make_cut(o, c.pivi, c.nvar, c.ncol, c.bigparm, 64 * nb)
            if c.fn != QS_MAKE_CUT:
                deepen(cut, c.den[c.pivi], c.nvar, trk)
            o.cut = cut
        elif c.fn == QS_FIND_QUOTIENT:
            o.ret = find_quotient(o, c.CW, c.nc, c.nparm, trk)
        elif c.fn == QS_BUILD_SUB:
            o.ret = build_sub(o, c)
        elif c.fn == QS_SOLVE_PLAIN:
            o.ret = solve_plain(o, c, trk)
        o.cls = "may" if trk.may else "fits"
    except Must as m:
        o.cls, o.note = "must", "leaves the width in: %s" % (m.args[0] if m.args else "")
    o.max_need, o.lambda_steps = trk.max_need, getattr(trk, "lambda_steps", 0)
    return o


def overflow_reported(c, ret, aux):
    """does what the probe returned carry Q_WHY_OVERFLOW?"""
    if c.fn in (QS_DEEPEN, QS_CUT_CHAIN, QS_FIND_QUOTIENT):
        return bool((aux >> 8) & Q_WHY_OVERFLOW)
    if c.fn == QS_SOLVE_PLAIN:
        return bool((ret >> 1) & Q_WHY_OVERFLOW)
    return ret >= 0 and bool(ret & Q_WHY_OVERFLOW)


# ------------------------------------------------------------------------------------------------ packing
def _words(vals, EW):
    if EW == 1:
        return [v & M64 for v in vals]
    out = []
    for v in vals:
        out += [v & M64, (v >> 64) & M64]
    return out


def pack_in(c, EW):
    """the case as pipamd_debug_quast_step reads it (piplib_amd/csrc/pip_quast.h), uint64 words"""
    w = [x & M64 for x in c.header() + list(c.flag) + list(c.ref) + list(c.pos)]
    vals = list(c.det) + list(c.den) + [x for r in c.val for x in r] + [x for r in c.ctx for x in r] + list(c.cutv)
    return np.array(w + _words(vals, EW), dtype=np.uint64)


def out_words(c, EW, nb):
    nv = 4 + c.R + c.S * c.W + c.CR * c.CW + c.CW + 2
    return 4 + 2 * c.R + QS_POS + QS_SKEY + EW * (nv + 64 * nb)


def pack_out(o, EW):
    """every output word of a case the model calls `fits`"""
    w = [x & M64 for x in [1, o.ret, o.aux, o.ldet] + o.flag + o.ref + o.pos + o.skey]
    vals = o.det + o.den + [x for r in o.val for x in r] + [x for r in o.ctx for x in r] + o.cutv + o.cut
    return np.array(w + _words(vals, EW), dtype=np.uint64)
