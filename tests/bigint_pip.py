"""Exact-arithmetic (Python int) restatement of PipLib's non-parametric pivot loop.

TEST INFRASTRUCTURE ONLY (like oracle/): used by tests/golden/make_bigint_fixtures.py to
produce the fixtures that pin the 128-bit Entier engine, and by tests that cross-check it
against oracle/oraclepip.  Nothing under piplib_amd/ imports it.

What is restated (reference file:line), for problems without parameters (nparm = 0, no big
parameter), exactly as the reference's fixed-width builds run them:

  tab_sort_rows   source/traiter.c:556-623   sort_rows()
  traiter loop    source/traiter.c:628-791   solve()
  chercher        source/traiter.c:39-44
  exam_coef       source/traiter.c:101-159   (nparm = 0: the sign of the constant term)
  choisir_piv     source/traiter.c:297-341   pick_column()
  pivoter         source/traiter.c:345-548   pivot_step(), incl. the multi-limb determinant and its
                                             "Integer overflow" exits (traiter.c:412-446)
  integrer        source/integrer.c:305-486  gomory() (constant cuts)
  deepest cut     source/integrer.c:417-438  deepen(), with `deepest=True` (the reference's -d / Deepest_cut)
  bezout          source/integrer.c:98-150   bezout(), as the reference computes it: the representative of lambda it
                                             arrives at decides how often the loop adds D / delta, and so which cut is built

Integers are Python ints, so nothing wraps.  `bits` is the width of the fixed-width build being
modelled (64 = the reference's `long long` flavour, 128 = the overflow-safe flavour,
include/piplib/piplib.h:42-88): it enters the algorithm only through the determinant limbs
(piplib_lllog2 sums against 8*sizeof(Entier); a limb product passes that test first, so it cannot
wrap).  Every other product, difference and row entry the fixed-width code would form is checked
against that width: `Stats.max_bits` is the largest
magnitude met, and a result is only comparable with a fixed-width run when
`max_bits < bits` (no wrap-around happened) -- callers check `Stats.exact`.  That holds with the deepest cut on: t,
delta, tau, d, Bezout's products and differences, lambda after every round, every lambda * coefficient and D - t are
noted, and `Stats.cut_log` keeps what each deepest cut was made of.

bezout() and deepen() take the callable that is shown every intermediate, so that tests/quast_step_model.py (the device
tree's steps) runs the same statements under its own width tracker.
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

UNIT, PLUS, MINUS, ZERO, CRITIC, UNKNOWN = 1, 2, 4, 8, 16, 32
MAXDET = 4  # reference tab.h:67 MAX_DETERMINANT

ST_SOLUTION, ST_NIL, ST_OVERFLOW = 1, 2, 5  # == PIPAMD_ST_* of include/piplib_amd.h


@dataclass
class Stats:
    bits: int
    max_bits: int = 0          # largest bit length of any intermediate the fixed-width code forms
    max_entry_bits: int = 0    # largest bit length of a stored tableau entry or denominator
    pivots: int = 0
    cuts: int = 0
    rows_changed: List[int] = field(default_factory=list)   # per pivot: rows whose bits change
    entry_bits: List[int] = field(default_factory=list)     # per pivot: max entry bits after it
    nrows: List[int] = field(default_factory=list)          # per pivot: real rows
    det_log: List[tuple] = field(default_factory=list)      # per pivot with a column: (pivot, denominator of the pivot row),
                                                            # what the pivot kernels log for the determinant replay
    cut_log: List[tuple] = field(default_factory=list)      # per deepest cut: (D, delta, lambda, rounds of the lambda += d
                                                            # loop, bit length of the largest lambda * coefficient)
    nil_cut: bool = False      # ended at a fractional constant with no positive coefficient to cut with (integrer.c:482-485)

    @property
    def exact(self):
        return self.max_bits < self.bits


@dataclass
class Result:
    status: int
    pivots: int
    cuts: int
    sol_num: Optional[List[int]]   # per unknown: numerator of the constant term (solution(), traiter.c:255-271)
    sol_den: Optional[List[int]]
    stats: Stats


def _log2(x):
    """integrer.c:51-59 piplib_lllog2: bit length of |x|, 1 for 0."""
    n = abs(x).bit_length()
    return n if n else 1


def _sgn(x):
    return MINUS if x < 0 else (PLUS if x > 0 else ZERO)


class _Row:
    __slots__ = ("flag", "den", "v", "unit", "size")

    def __init__(self, flag, den, v=None, unit=-1):
        self.flag, self.den, self.v, self.unit, self.size = flag, den, v, unit, np.float32(0)


def _note(st, *vals):
    for x in vals:
        b = abs(int(x)).bit_length()
        if b > st.max_bits:
            st.max_bits = b


def _note_arr(st, a):
    if len(a):
        m = max(abs(int(a.max())), abs(int(a.min())))
        b = m.bit_length()
        if b > st.max_bits:
            st.max_bits = b
        return b
    return 0


def sort_rows(rows, nvar, nligne):
    """traiter.c:576-614 for rows with denominator 1 (a freshly loaded tableau)."""
    smax = 0.0
    for i in range(nvar, nligne):
        r = rows[i]
        if r.flag & UNIT:
            continue
        assert r.den == 1
        s = 0.0
        for x in r.v[:nvar]:
            x = int(x)
            # (int)((double)x / 1.0) as cvttsd2si computes it: INT_MIN out of range, and abs(INT_MIN)
            # stays negative so it never wins the max
            if -2**31 < x < 2**31:
                a = float(abs(x))
                if a > s:
                    s = a
        r.size = np.float32(s)
        if s > smax:
            smax = s
    def swap(a, b):
        rows[a], rows[b] = rows[b], rows[a]
    selection_sort(nvar, nligne, smax, lambda i: rows[i].flag & UNIT, lambda i: float(rows[i].size), swap)


def selection_sort(lo, hi, smax, is_unit, size_of, swap):
    """The selection loop of traiter.c:591-614 over the logical rows lo .. hi-1, on given sizes (floats, widened to
    doubles in the comparison as C does) and a given bound smax: for each row that is not Unit, the first row at or after
    it whose size is strictly below the running bound -- smax to begin with -- is swapped into its place."""
    for i in range(lo, hi):
        if is_unit(i):
            continue
        s = smax
        pivi = i
        for j in range(i, hi):
            if is_unit(j):
                continue
            if size_of(j) < s:
                s = size_of(j)
                pivi = j
        if pivi != i:
            swap(pivi, i)


def _cell(rows, k, j):
    """traiter.c valeur(): a unit row is its denominator (1) in its own column."""
    r = rows[k]
    if r.flag & UNIT:
        return r.den if r.unit == j else 0
    return int(r.v[j])


def pick_column(rows, pivi, nvar, nligne, st):
    pivj, pivot = -1, 0
    prow = rows[pivi].v
    for j in range(nvar):
        foo = int(prow[j])
        if foo <= 0:
            continue
        if pivj < 0:
            pivj, pivot = j, foo
            continue
        x = 0
        for k in range(nligne):
            a, b = pivot * _cell(rows, k, j), _cell(rows, k, pivj) * foo
            x = a - b
            _note(st, a, b, x)
            if x != 0:
                break
        if x < 0:
            pivj, pivot = j, foo
    return pivj


class Overflow(Exception):
    pass


def det_update(det, pivot, dpiv, bits):
    """The multi-limb determinant walk of traiter.c:412-446 on the list `det`, in place: the limbs lose the factors
    of dpiv / gcd(pivot, dpiv) (a factor left over: Overflow), then the first limb with room below `bits` takes
    pivot / gcd(pivot, dpiv) (no room and no limb left: Overflow)."""
    d = math.gcd(pivot, dpiv)
    ppivot, dppiv = pivot // d, dpiv // d
    for i in range(len(det)):
        d = math.gcd(det[i], dppiv)
        det[i] //= d
        dppiv //= d
    if dppiv != 1:
        raise Overflow()
    for i in range(len(det)):
        if _log2(det[i]) + _log2(ppivot) < bits:
            det[i] *= ppivot  # below 2^(bits-1) by the test above: never a wrap
            break
    else:
        if len(det) + 1 >= MAXDET:
            raise Overflow()
        det.append(ppivot)


def row_update(v, den, prow, pivot, dpiv, pivj, st=None):
    """The row update of traiter.c:470-501 for the row `v` (object array) under denominator `den`, against the pivot row
    `prow` with pivot entry `pivot` = prow[pivj] and denominator `dpiv`.  Returns (z, newden, lpiv, foo): the new row,
    its denominator and the two multipliers.  z is `v` itself where the reference would multiply by 1 and subtract 0.
    `st`: Stats that note every intermediate the fixed-width code forms."""
    foo = int(v[pivj])
    d = math.gcd(pivot, foo)
    lpiv, foo = pivot // d, foo // d
    g = lpiv * den
    if st is not None:
        _note(st, g)
    if foo == 0 and lpiv == 1:
        z = v  # z = v * 1 - q * 0: same entries; the gcd with g = den may still reduce them
    else:
        a, b = v * lpiv, prow * foo
        z = a - b
        z[pivj] = dpiv * foo
        if st is not None:
            _note_arr(st, a)
            _note_arr(st, b)
            _note_arr(st, z)
    gg = g
    if gg != 1:
        for x in z:
            gg = math.gcd(gg, int(x))
            if gg == 1:
                break
    newden = g
    if gg != 1:
        z = z // gg  # exact: gg divides every entry
        newden = g // gg
    return z, newden, lpiv, foo


def pivot_step(rows, det, pivi, nvar, ni, st):
    ncol = nvar + 1
    nligne = nvar + ni
    st.pivots += 1
    pivj = pick_column(rows, pivi, nvar, nligne, st)
    if pivj < 0:
        return -1
    prow = rows[pivi].v
    pivot, dpiv = int(prow[pivj]), rows[pivi].den
    st.det_log.append((pivot, dpiv))
    det_update(det, pivot, dpiv, st.bits)
    fresh = -prow
    fresh[pivj] = dpiv
    changed = 0
    for k in range(nligne):
        r = rows[k]
        if (r.flag & UNIT) or k == pivi:
            continue
        z, newden, _, _ = row_update(r.v, r.den, prow, pivot, dpiv, pivj, st)
        if newden != r.den or (z is not r.v and bool((z != r.v).any())):
            changed += 1
        r.v, r.den = z, newden
    for k in range(nligne):
        if (rows[k].flag & UNIT) and rows[k].unit == pivj:
            break
    else:
        raise AssertionError("no unit row for the pivot column")
    rows[k] = _Row(PLUS, pivot, fresh)
    rows[pivi] = _Row(UNIT | ZERO, 1, None, pivj)
    mb = 0
    for k in range(nligne):
        r = rows[k]
        if r.flag & UNIT:
            continue
        b = max(abs(int(r.v.max())), abs(int(r.v.min())), r.den).bit_length()
        if b > mb:
            mb = b
        ff, fff = r.flag, _sgn(int(r.v[pivj]))
        if fff != ZERO and fff != ff:
            ff = (UNKNOWN if fff == MINUS else fff) if ff == ZERO else UNKNOWN
        r.flag = ff
    if mb > st.max_entry_bits:
        st.max_entry_bits = mb
    st.rows_changed.append(changed)
    st.entry_bits.append(mb)
    st.nrows.append(ni)
    return 0


def bezout(x, y, delta, need):
    """integrer.c:98-150: z with z * y == x (mod delta) for coprime y and delta, 0 otherwise.  `need(*vals)` is shown every
    value the fixed-width code forms and returns the last of them."""
    a, b, c, d, u, v = 1, 0, 0, 1, y, delta
    while True:
        need(u - u % v)
        q, r = u // v, u % v
        if r == 0:
            break
        u, v = v, r
        e = need(q * c, a - q * c)
        f = need(q * d, b - q * d)
        a, b, c, d = c, d, e, f
    if v != 1:
        return 0
    return need(c * x) % delta


def deepen(cut, D, nvar, need, on_round=None):
    """integrer.c:417-438 on the cut `cut` (unknowns | constant at nvar) under denominator D, in place.  `need` as for
    bezout(); `on_round(k)` is told the rounds of the lambda += d loop as they are spent (0 once Bezout is back).
    Returns (lambda, delta, rounds, bit length of the largest lambda * coefficient)."""
    t = -cut[nvar]
    delta = math.gcd(t, D)
    tau, d = t // delta, D // delta
    lam = bezout(d - 1, tau, d, need)
    rounds = 0
    if on_round:
        on_round(0)
    while math.gcd(lam, D) != 1:
        lam = need(lam + d)
        rounds += 1
        if on_round:
            on_round(rounds)
    big = 0
    for j in range(nvar):
        p = need(lam * cut[j])
        big = max(big, abs(p).bit_length())
        cut[j] = p % D
    p = need(cut[nvar] * lam)
    big = max(big, abs(p).bit_length())
    cut[nvar] = -(D - p % D)
    return lam, delta, rounds, big


def gomory(rows, nvar, ni, st, deepest=False):
    """integrer.c:305-486 for nparm = 0: index of the appended cut row, 0 (all integral), -1 (nil).  `deepest`: the cut is
    scaled as integrer.c:417-438 does under the reference's deepest-cut option."""
    nligne = nvar + ni
    for i in range(nvar):
        r = rows[i]
        D = r.den
        if D == 1 or (r.flag & UNIT):
            continue
        cut = r.v % D  # D > 0: Python's % is piplib_llmod (integrer.c:69-74)
        ok_var = bool((cut[:nvar] > 0).any())
        x = -((-int(r.v[nvar])) % D)
        cut[nvar] = x
        if x == 0:
            continue  # integral row
        if not ok_var:
            st.nil_cut = True
            return -1
        if deepest:
            def need(*vals):
                _note(st, *vals)
                return vals[-1]
            t = -x
            c = [int(y) for y in cut]
            lam, delta, rounds, big = deepen(c, D, nvar, need)
            _note(st, t, delta, t // delta, D // delta, D // delta - 1, D - (x * lam) % D)
            cut = np.array(c, dtype=object)
            st.cut_log.append((D, delta, lam, rounds, big))
        rows.append(_Row(MINUS, D, cut))
        assert len(rows) == nligne + 1
        st.cuts += 1
        return nligne
    return 0


def solve(ineq, integer=True, bits=64, det_out=None, stop_inexact=False, deepest=False) -> Result:
    """ineq: (ni, nvar+1) integers (unknowns | constant).  Returns what traiter() leaves on the
    solution tape for a problem without parameters.  `det_out`: a list that receives the determinant's limbs as the last
    det_update left them (at an Overflow: as it left them when it raised).  `stop_inexact`: give up, with status None,
    before the first pivot that follows an intermediate of `bits` bits or more -- from there on a fixed-width run is
    not comparable, and a caller that only asks about the comparable part need not pay for the rest.  `deepest`: every cut
    is the deepest cut (gomory())."""
    ineq = np.asarray(ineq, dtype=object)
    ni, ncol = ineq.shape
    nvar = ncol - 1
    st = Stats(bits)
    rows = [_Row(UNIT, 1, None, i) for i in range(nvar)]
    rows += [_Row(UNKNOWN, 1, np.array([int(x) for x in ineq[i]], dtype=object)) for i in range(ni)]
    for r in rows[nvar:]:
        _note_arr(st, r.v)
    det = [1]
    sort_rows(rows, nvar, nvar + ni)
    status = None
    try:
        while True:
            nligne = nvar + ni
            pivi = next((i for i in range(nligne) if rows[i].flag & MINUS), nligne)
            if pivi >= nligne:
                # exam_coef with no parameters: an Unknown row gets the sign of its constant term;
                # stop at the first one proven negative
                for i in range(nligne):
                    r = rows[i]
                    if r.flag != UNKNOWN:
                        continue
                    r.flag = _sgn(int(r.v[nvar]))
                    if r.flag == MINUS:
                        pivi = i
                        break
            if pivi >= nligne:
                if not integer:
                    status = ST_SOLUTION
                    break
                pivi = gomory(rows, nvar, ni, st, deepest)
                if pivi == 0:
                    status = ST_SOLUTION
                    break
                if pivi < 0:
                    status = ST_NIL
                    break
                ni += 1
            if stop_inexact and not st.exact:
                break
            if pivot_step(rows, det, pivi, nvar, ni, st) < 0:
                status = ST_NIL
                break
    except Overflow:
        if det_out is not None:
            det_out[:] = det
        return Result(ST_OVERFLOW, st.pivots, st.cuts, None, None, st)
    if det_out is not None:
        det_out[:] = det
    if status == ST_SOLUTION:
        num = [0 if (rows[i].flag & UNIT) else int(rows[i].v[nvar]) for i in range(nvar)]
        den = [1 if (rows[i].flag & UNIT) else int(rows[i].den) for i in range(nvar)]
        return Result(status, st.pivots, st.cuts, num, den, st)
    return Result(status, st.pivots, st.cuts, None, None, st)


def solution_text(num, den):
    """sol_edit text of the solution list (sol.c:335-378), as tests/gpu_common.solution_text."""
    out = ["(list "]
    for n, d in zip(num, den):
        g = math.gcd(n, d)
        out.append("#[ %d]\n" % (n // g) if g == d else "#[ %d/%d]\n" % (n // g, d // g))
    out.append(")\n")
    return "".join(out)
