"""The formulas the host decision trees of layer 3 share (piplib_amd/csrc/pip_tree_steps.h), on the CPU: tests/tree_steps_main.cpp
includes that header alone, is built with the host compiler under the address and undefined-behaviour sanitizers and run as
a child process, in both entry widths.  The expected values come from the model below: Python ints wrapped to the width,
written after the reference line by line (integrer.c:98-150 bezout, 156-227 add_parm, 229-291 has_cut / find_parm, 357-520
integrer; traiter.c:180-237 compa_test, 255-271 solution, 719-757 the fork), not after the header."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S_NIL, S_IF, S_LIST, S_FORM, S_NEW, S_DIV, S_VAL = range(1, 8)         # sol.c:42-50
F_PLUS, F_MINUS, F_ZERO, F_CRITIC, F_UNKNOWN = 2, 4, 8, 16, 32          # include/piplib_amd.h PIPAMD_F_*
CUT_NONE, CUT_CONST, CUT_PARM, CUT_NO_VAR = range(4)


def wrap(x, bits):
    x &= (1 << bits) - 1
    return x - (1 << bits) if x >> (bits - 1) else x


# ------------------------------------------------------------------------------------------------ the model
def bezout(x, y, delta):                      # integrer.c:98-150
    a, b, c, d, u, v = 1, 0, 0, 1, y, delta
    while True:
        q, r = u // v, u % v                  # piplib_int_floor_div_q_r
        if r == 0:
            break
        u, v = v, r
        a, b, c, d = c, d, a - q * c, b - q * d
    return 0 if v != 1 else (c * x) % delta


def has_cut(context, nparm, p, cut):          # integrer.c:229-254; cut: constant | parameters | denominator
    for row in context:
        if row[p] != cut[1 + nparm] or row[nparm] != cut[0]:
            continue
        if any(row[col] != 0 for col in range(p + 1, nparm)):
            continue
        if any(row[col] != cut[1 + col] for col in range(p)):
            continue
        return True
    return False


def find_parm(context, nparm, cut):           # integrer.c:258-291
    if cut[1 + nparm - 1] != 0:
        return -1
    cut = list(cut)
    cut[0] = cut[0] + cut[1 + nparm] - 1
    for p in range(nparm - 1, -1, -1):
        if cut[1 + p] != 0:
            break
        if not has_cut(context, nparm, p, cut):
            continue
        cut[0] = cut[0] + 1 - cut[1 + nparm]
        if has_cut(context, nparm, p, [-x for x in cut]):
            return p
        cut[0] = cut[0] + cut[1 + nparm] - 1
    return -1


def add_parm(context, nparm, cut, cells):     # integrer.c:156-227
    cells += [(S_NEW, nparm, 0), (S_DIV, 0, 0), (S_FORM, nparm + 1, 0)]
    cells += [(S_VAL, -cut[1 + j], 1) for j in range(nparm)]
    cells += [(S_VAL, -cut[0], 1), (S_VAL, cut[1 + nparm], 1)]
    for row in context:
        row.append(row[nparm])
        row[nparm] = 0
    context.append([-cut[1 + j] for j in range(nparm)] + [-cut[1 + nparm], -cut[0]])
    context.append([cut[1 + j] for j in range(nparm)] + [cut[1 + nparm], cut[0] - 1 + cut[1 + nparm]])


def integrer(row, D, nvar, nparm, bigparm, deepest, context):
    """integrer.c:357-520 for one non-integral row -> (kind, nparm, column of the quotient, appended row, cells, spins of
    the deepest cut's while loop); the context is changed in place"""
    ncol = nvar + nparm + 1
    coupure = [x % D for x in row[:nvar]]                       # piplib_int_floor_div_r
    ok_var = any(x > 0 for x in coupure)
    coupure.append(-((-row[nvar]) % D))
    ok_parm = False
    for j in range(nvar + 1, ncol):
        coupure.append(0 if j == bigparm else -((-row[j]) % D))
        ok_parm = ok_parm or coupure[j] != 0
    coupure.append(D)
    cells, spins = [], 0
    if not ok_parm:
        if not ok_var:
            return CUT_NONE, nparm, -1, [], cells, spins         # case (b)
        if deepest:                                              # integrer.c:417-438
            t = -coupure[nvar]
            import math
            delta = math.gcd(t, D)
            tau, d = t // delta, D // delta
            lam = bezout(d - 1, tau, d)
            while math.gcd(lam, D) != 1:
                lam += d
                spins += 1
            for j in range(nvar):
                coupure[j] = (lam * coupure[j]) % D
            coupure[nvar] = -(D - (coupure[nvar] * lam) % D)
        return CUT_CONST, nparm, -1, coupure[:ncol], cells, spins  # case (d)
    parm = find_parm(context, nparm, coupure[nvar:])
    if parm == -1:
        add_parm(context, nparm, coupure[nvar:], cells)
        parm = nparm
        nparm += 1
    if not ok_var:                                               # assert(ok_var), integrer.c:499: the engine's ST_INTERNAL
        return CUT_NO_VAR, nparm, -1, [], cells, spins
    out = coupure[:ncol] + [0] * (nvar + nparm + 1 - ncol)
    out[nvar + 1 + parm] += coupure[ncol]
    return CUT_PARM, nparm, nvar + 1 + parm, out, cells, spins


def fork(cst, parms, integer):                # traiter.c:719-737 -> (cells, context row)
    import math
    com_dem = 0
    for x in parms:
        com_dem = math.gcd(com_dem, x)
    if not integer:
        com_dem = math.gcd(com_dem, cst)
    row = [x // com_dem for x in parms] + [cst // com_dem]       # div_exact; floor_div_q for the integer constant
    assert integer or cst % com_dem == 0
    return [(S_IF, 0, 0), (S_FORM, len(parms) + 1, 0)] + [(S_VAL, x, 1) for x in row], row


# ------------------------------------------------------------------------------------------------ the program
@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("tree_steps") / "tree_steps")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "tree_steps_main.cpp"), "-o", exe], check=True, timeout=300)

    def run(lines):
        """lines: 'bits command integers' -> per line, its ';'-separated lists of ints"""
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [[[int(x) for x in part.split()] for part in ln.split(";")] for ln in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def flat(cells):
    return [x for c in cells for x in c]


def ints(xs):
    return " ".join(str(x) for x in xs)


BITS = [64, 128]


@pytest.mark.parametrize("bits", BITS)
def test_parametric_cut(steps, bits):
    """integrer() on rows of 2 unknowns: every branch of its decision table, the quotient found again, the p-loop of
    find_parm, the big parameter, the sign conventions of the remainders"""
    W = lambda xs: [wrap(x, bits) for x in xs]  # noqa: E731
    lines, want = [], []

    def cut(context, nvar, nparm, bigparm, deepest, D, row, expect_kind, expect_new=None):
        lines.append(f"{bits} ctx {nparm} {len(context)} " + ints(x for r in context for x in r))
        want.append([[len(context)]])
        return cut_again(context, nvar, nparm, bigparm, deepest, D, row, expect_kind, expect_new)

    def cut_again(context, nvar, nparm, bigparm, deepest, D, row, expect_kind, expect_new=None):
        lines.append(f"{bits} cut {nvar} {nparm} {bigparm} {deepest} {D} " + ints(row))
        kind, np2, newcol, out, cells, spins = integrer(row, D, nvar, nparm, bigparm, deepest, context)
        assert kind == expect_kind and (expect_new is None or (np2 > nparm) == expect_new)
        want.append([[kind, np2, newcol], W(out), W(flat(cells)), W([len(context)] + [x for r in context for x in r])])
        return np2, newcol, spins

    # constant cut: the parameter's coefficient is a multiple of D; negative constant, D does not divide it
    cut([], 2, 1, -1, 0, 2, [1, 3, -5, 4], CUT_CONST)
    # ... and the remainders of negative unknowns' entries and of a positive constant (5 -> -3, not -1)
    cut([], 2, 1, -1, 0, 4, [-3, -6, 5, 8], CUT_CONST)
    # parametric cut that defines a quotient: New / Div / Form cells, two context rows, constants moved right
    ctx = [[1, -2]]
    np2, newcol, _ = cut(ctx, 2, 1, -1, 0, 4, [1, 2, -5, 3], CUT_PARM, expect_new=True)
    assert (np2, newcol) == (2, 4) and ctx == [[1, 0, -2], [1, -4, 1], [-1, 4, 2]]
    # the same cut again (the row one parameter wider): find_parm returns the column, no cell, no context row
    np3, newcol, _ = cut_again(ctx, 2, 2, -1, 0, 4, [1, 2, -5, 3, 8], CUT_PARM, expect_new=False)
    assert (np3, newcol) == (2, 4) and len(ctx) == 3
    # ... but with another constant it is another quotient
    cut_again(ctx, 2, 2, -1, 0, 4, [1, 2, -6, 3, 0], CUT_PARM, expect_new=True)
    # trailing zeros, the defining rows only there for an EARLIER column: column 2 has no rows, column 1 has them
    # (the cut's parameter part is (-4, 0, 0), its constant -6, D = 7; the first row is a decoy with the wrong sign)
    ctx = [[4, 7, 0, 0], [-4, 7, 0, 0], [4, -7, 0, 6], [1, 1, 1, 0]]
    np4, newcol, _ = cut(ctx, 2, 3, -1, 0, 7, [2, 3, -6, 3, 14, -7], CUT_PARM, expect_new=False)
    assert (np4, newcol) == (3, 2 + 1 + 1)
    # ... and not found when a column behind it is not zero in the upper row
    ctx = [[-4, 7, 1, 0], [4, -7, 0, 6]]
    cut(ctx, 2, 3, -1, 0, 7, [2, 3, -6, 3, 14, -7], CUT_PARM, expect_new=True)
    # the big parameter inside the parameter columns: its entry is 0 and does not make the cut parametric
    cut([], 2, 2, 3, 0, 4, [1, 2, -5, 3, 8], CUT_CONST)
    cut([], 2, 2, 4, 0, 4, [1, 2, -5, 3, 7], CUT_PARM, expect_new=True)
    # no positive unknown entry and no parameter part: no cut (case (b))
    cut([[1, 0]], 2, 1, -1, 0, 4, [4, -8, -5, 4], CUT_NONE)
    # no positive unknown entry under a parametric part: the quotient is defined first, then assert(ok_var) fails
    cut([[1, 0]], 2, 1, -1, 0, 4, [4, -8, -5, 3], CUT_NO_VAR, expect_new=True)
    # deepest cut: lambda = 2 shares a factor with D = 12 on the first try, the while loop runs
    _, _, spins = cut([], 2, 0, -1, 1, 12, [5, 7, -4], CUT_CONST)
    assert spins >= 1
    cut([], 2, 1, -1, 1, 12, [5, 7, -4, 24], CUT_CONST)
    # ... and the option leaves a parametric cut alone
    cut([], 2, 1, -1, 1, 12, [5, 7, -4, 5], CUT_PARM, expect_new=True)
    assert steps(lines) == want


@pytest.mark.parametrize("bits", BITS)
def test_fork_rows_and_solution(steps, bits):
    """the context row of a fork (integer: floor of a negative constant; rational: the constant inside the gcd), its
    negation for the else branch, and the solution list"""
    lo = -(1 << (bits - 1))
    lines, want = [], []
    for integer, cst, parms in [(1, -7, [4, -6]), (0, -8, [4, -6]), (0, -7, [4, -6]), (1, 5, [0, 0, 6]), (0, 12, [0, -6, 0]),
                                (1, -1, [3]), (1, lo, [2])]:
        np_ = len(parms)
        ctx = [[1] * np_ + [0], [0] * np_ + [3]]
        cells, row = fork(cst, parms, integer)
        lines.append(f"{bits} ctx {np_} 2 " + ints(x for r in ctx for x in r))
        want.append([[2]])
        lines.append(f"{bits} fork {np_} {integer} {cst} " + ints(parms))
        want.append([flat(cells), row, [2]])                 # written behind the rows in use, not yet counted
        lines.append(f"{bits} else {np_}")
        neg = [wrap(-x, bits) for x in row[:-1]] + [wrap(-(row[-1] + 1), bits)]   # traiter.c:751-757
        want.append([[3] + [x for r in ctx for x in r] + neg])
    assert fork(-7, [4, -6], 1)[1] == [2, -3, -4] and fork(-8, [4, -6], 0)[1] == [2, -3, -4]
    assert fork(5, [0, 0, 6], 1)[1] == [0, 0, 1, 0]
    # solution (traiter.c:255-271): List nvar, per unknown Form nparm + 1 and its values over the row's denominator
    num, den = [1, -2, 3, 4, lo, 6], [7, -(lo + 1)]
    lines.append(f"{bits} sol 2 2 " + ints(num + den))
    want.append([[S_LIST, 2, 0, S_FORM, 3, 0, S_VAL, 1, 7, S_VAL, -2, 7, S_VAL, 3, 7,
                  S_FORM, 3, 0, S_VAL, 4, den[1], S_VAL, lo, den[1], S_VAL, 6, den[1]]])
    lines.append(f"{bits} sol 0 3")
    want.append([[S_LIST, 0, 0]])
    assert steps(lines) == want


@pytest.mark.parametrize("bits", BITS)
def test_compa_rows_and_flags(steps, bits):
    """compa_test's two sub-problem rows (traiter.c:193-217) and the flag from their outcomes (traiter.c:228-237)"""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    lines = [f"{bits} rows 2 0 5 3 -4", f"{bits} rows 2 1 5 3 -4", f"{bits} rows 1 0 {lo} {lo}", f"{bits} rows 0 1 -1"]
    want = [[[3, -4, 4], [-3, 4, -6]], [[3, -4, 5], [-3, 4, -6]], [[lo, hi], [lo, hi]], [[-1], [0]]]
    table = {(0, 0, 0): F_UNKNOWN, (0, 0, 1): F_CRITIC, (0, 1, 0): F_PLUS, (0, 1, 1): F_PLUS,   # (plus is Nil, minus is Nil, critic)
             (1, 0, 0): F_MINUS, (1, 0, 1): F_MINUS, (1, 1, 0): F_ZERO, (1, 1, 1): F_ZERO}
    for (p, m, c), f in sorted(table.items()):
        lines.append(f"{bits} flag {p} {m} {c}")
        want.append([[f]])
    assert steps(lines) == want


@pytest.mark.parametrize("bits", BITS)
def test_wrap_edges(steps, bits):
    """the helpers where C's own operators are undefined: divisor 0, divisor -1 at the type's minimum, |minimum|"""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    cases = [("crem", 7, 0, 0), ("crem", lo, -1, 0), ("crem", -7, 2, -1), ("crem", 7, -2, 1),
             ("cquo", 7, 0, 0), ("cquo", lo, -1, lo), ("cquo", -7, 2, -3), ("cquo", hi, -1, -hi),
             ("fmod", 7, 0, 0), ("fmod", lo, -1, 0), ("fmod", -7, 2, 1), ("fmod", -7, -2, 1), ("fmod", lo, hi, hi - 1),
             ("gcd", 0, 0, 0), ("gcd", lo, 0, lo), ("gcd", 0, lo, lo), ("gcd", lo, -1, 1), ("gcd", lo, 6, 2), ("gcd", -12, 18, 6),
             ("floordiv", 7, 0, 0), ("floordiv", lo, -1, lo), ("floordiv", -7, 2, -4), ("floordiv", 7, 2, 3),
             ("floordiv", lo, 2, lo // 2), ("floordiv", hi, 3, hi // 3),
             ("wabs", lo, 0, lo), ("wabs", -5, 0, 5), ("wneg", lo, 0, lo), ("wadd", hi, 1, lo), ("wsub", lo, 1, hi),
             ("wmul", lo, -1, lo), ("wmul", hi, 2, -2)]
    lines = [f"{bits} op {name} {a} {b}" for name, a, b, _ in cases]
    lines.append(f"{bits} op bezout 2 1 3")   # z.1 = 2 (mod 3)
    lines.append(f"{bits} op bezout 4 3 7")   # z.3 = 4 (mod 7): z = 6
    lines.append(f"{bits} op bezout 1 2 4")   # 2 and 4 not coprime: 0
    assert steps(lines) == [[[w]] for _, _, _, w in cases] + [[[2]], [[6]], [[0]]]
