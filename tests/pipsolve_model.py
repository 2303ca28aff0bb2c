"""Test helper: pip_solve(inequnk, ineqpar, Bg, options) (piplib.c:722-880) restated on Python ints.

* plan / build: the integer bookkeeping of piplib.c:758-797 and the two tab_Matrix2Tableau calls (tab.c:292-393), i.e.
  what pipamd_pip_tableaux hands back and what pipamd_pip_info holds;
* quast_text: sol_quast_edit (sol.c:435-734), pip_quast_equalities_dual (piplib.c:651-690) and pip_quast_print
  (piplib.c:198-317) over engine cells, so that an answer can be compared with what the reference prints;
* the seeded problem families of tests/golden/pipsolve (make_pipsolve_fixtures.py) and of the live tests.

TEST INFRASTRUCTURE ONLY.
"""
import json
import math
import os
import re
import subprocess

import numpy as np

import pipbatch as pb
from datfile import matrix_text

GOLDEN = os.path.join(pb.ROOT, "tests", "golden", "pipsolve")
NQ, MAXIMIZE, URS_PARMS, URS_UNKNOWNS, DUAL = 1, 2, 4, 8, 16  # PIPAMD_PIP_*
SOL_SHIFT, SOL_NEGATE, SOL_REMOVE, SOL_MAX, SOL_DUAL = 1, 2, 4, 3, 8  # sol.h:36-50
T_INT, T_DUAL = 1, 2  # TRAITER_*, funcall.h:32-33
S_NIL, S_IF, S_LIST, S_FORM, S_NEW, S_DIV, S_VAL = range(1, 8)  # PIPAMD_SOL_*
INFO_FIELDS = ("nvar", "nparm", "ni", "nc", "bigparm", "flags", "sol_bg", "urs_parms", "sol_flags", "is_void")


def wrap64(x):
    return ((int(x) + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)


def _ints(m):
    return None if m is None else [[int(v) for v in r] for r in m]


def _ncols(m, rows):
    return m.shape[1] if hasattr(m, "shape") else len(rows[0])


def plan(inequnk, ineqpar, bg, options):
    """pipamd_pip_info (without row_off) plus what the build needs: Shift, the matrices' own Np, bignum_is_new"""
    if inequnk is None:  # piplib.c:753-754
        return dict(nvar=0, nparm=0, ni=0, nc=0, bigparm=-1, flags=0, sol_bg=-1, urs_parms=0, sol_flags=0, is_void=1)
    a, c = _ints(inequnk), _ints(ineqpar)
    ncols = _ncols(inequnk, a)
    np0 = 0 if ineqpar is None else _ncols(ineqpar, c) - 2  # piplib.c:758
    nn = ncols - np0 - 2
    nl = len(a) + sum(1 for r in a if r[0] == 0)  # piplib.c:767-770
    nm = 0 if c is None else len(c) + sum(1 for r in c if r[0] == 0)
    npar, shift, urs, sol_flags, isnew = np0, 0, 0, 0, 0
    if options & MAXIMIZE:  # piplib.c:777-783
        sol_flags |= SOL_MAX
        shift = 1
    elif options & URS_UNKNOWNS:
        sol_flags |= SOL_SHIFT
        shift = -1
    if options & URS_PARMS:  # piplib.c:785-788
        urs = npar - (1 if bg >= 0 else 0)
        npar += urs
    if shift and bg < 0:  # piplib.c:791-797
        bg = ncols - 1
        npar += 1
        sol_flags |= SOL_REMOVE
        isnew = 1
    flags = 0
    if options & NQ:  # piplib.c:852-857
        flags = T_INT
    elif options & DUAL:
        flags = T_DUAL
        sol_flags |= SOL_DUAL
    return dict(nvar=nn, nparm=npar, ni=nl, nc=nm, bigparm=bg, flags=flags, sol_bg=bg - nn - 1, urs_parms=urs,
                sol_flags=sol_flags, is_void=0, shift=shift, np0=np0, isnew=isnew)


def matrix_to_tableau(m, ncols, nv, n, shift, bg, urs, wrap=True):
    """tab_Matrix2Tableau (tab.c:292-393) without the unit rows: the rows as lists of Python ints"""
    w = wrap64 if wrap else int
    ctx = n == -1
    nb_columns = ncols - 1
    bignum_is_new = bool(shift) and (bg + ctx > 0) and (bg + ctx > ncols - 2)  # tab.c:311-313
    if bignum_is_new:
        nb_columns += 1
    if ctx:
        shift = 0
        cst = nv + urs
    else:
        cst = nv
    out = []
    for r in m:
        v = [0] * (nb_columns + urs)
        big = 0
        for j in range(nv):
            if bignum_is_new and j == bg:
                continue
            if shift:
                big = w(big + r[1 + j])
            v[j] = w(-r[1 + j]) if shift > 0 else r[1 + j]
        k = nv + 1
        for j in range(nv + 1, nb_columns):
            if bignum_is_new and j == bg:
                continue
            v[j] = r[k]
            k += 1
        for j in range(urs):  # tab.c:358-365
            pos_n = nb_columns - ctx + j
            pos = pos_n - urs
            if pos <= bg:
                pos -= 1
            v[pos_n] = w(-v[pos])
        v[cst] = r[ncols - 1]
        if shift:
            if shift < 0:
                big = w(-big)
            v[bg] = big if bignum_is_new else w(v[bg] + big)
        out.append(v)
        if r[0] == 0:  # tab.c:380-388
            out.append([w(-x) for x in v])
    return out


def build(inequnk, ineqpar, bg, options, wrap=True):
    """(info, domain rows, context rows): what pip_solve hands to traiter() at piplib.c:858 before tab_simplify.
    wrap=False keeps the true integers (to see whether a big column leaves 64 bits)."""
    f = plan(inequnk, ineqpar, bg, options)
    if f["is_void"]:
        return f, [], []
    a, c = _ints(inequnk), _ints(ineqpar)
    nn, npar, urs = f["nvar"], f["nparm"], f["urs_parms"]
    ctx_cols = f["np0"] + 2
    ctx = matrix_to_tableau(c or [], ctx_cols, npar - urs, -1, f["shift"], f["bigparm"] - nn - 1, urs, wrap)
    dom = matrix_to_tableau(a, _ncols(inequnk, a), nn, nn, f["shift"], f["bigparm"], urs, wrap)
    assert all(len(r) == nn + npar + 1 for r in dom) and all(len(r) == npar + 1 for r in ctx)
    assert len(dom) == f["ni"] and len(ctx) == f["nc"]
    return f, dom, ctx


def info_of(f):
    return {k: f[k] for k in INFO_FIELDS}


def as_problem(f, dom, ctx):
    """the built problem as the tableau entries take it (pipamd_problem / oracle batch)"""
    return pb.Problem(f["nvar"], f["nparm"], f["ni"], f["nc"], f["bigparm"], 1 if f["flags"] & T_INT else 0,
                      np.array(dom, dtype=np.int64).reshape(f["ni"], f["nvar"] + f["nparm"] + 1),
                      np.array(ctx, dtype=np.int64).reshape(f["nc"], f["nparm"] + 1))


def context_problem(f, ctx):
    """the context test of piplib.c:818-826 as a problem of its own: traiter(ctxt, NULL, Np, 0, Nm, 0, -1, TRAITER_INT)"""
    return pb.Problem(f["nparm"], 0, f["nc"], 0, -1, 1, np.array(ctx, dtype=np.int64).reshape(f["nc"], f["nparm"] + 1),
                      np.zeros((0, 1), dtype=np.int64))


def simplified(rows, cst):
    """tab_simplify (tab.c:396-427)"""
    out = []
    for r in rows:
        g = 0
        for j, v in enumerate(r):
            if j != cst:
                g = math.gcd(g, v)
        out.append(list(r) if g in (0, 1) else [v // g for v in r])  # floor for the constant, exact elsewhere
    return out


# ------------------------------------------------------------------ the tape to the printed quast
def _vector(cells, i, bg, urs, flags):
    """sol_vector_edit, sol.c:435-512 -> (next cell, [(num, den)])"""
    n = cells[i][1]
    if flags & SOL_REMOVE:
        n -= 1
    n -= urs
    first_urs = urs + (1 if bg >= 0 else 0)
    vec, unbounded, j = [], False, 0
    while len(vec) < n:
        i += 1
        N, D = cells[i][1], cells[i][2]
        d = math.gcd(N, D)
        here = j
        j += 1
        if (flags & SOL_SHIFT) and here == bg:
            N -= D
            if N != 0:
                unbounded = True
        if (flags & SOL_REMOVE) and here == bg:
            continue
        if first_urs <= here < first_urs + urs:
            continue
        num = N // d if d else N
        if flags & SOL_NEGATE:
            num = -num
        vec.append((num, 1 if d == D else D // d))
    if unbounded:
        vec = [(num, 0) for num, _ in vec]
    return i + 1, vec


def _quast(cells, i, bg, urs, flags):
    """sol_quast_edit, sol.c:664-734 -> (next cell, quast); quast = dict(newparm, list, cond, then, else)"""
    q = dict(newparm=[], list=None, cond=None, then=None, orelse=None)
    while cells[i][0] == 0:
        i += 1
    while cells[i][0] == S_NEW:  # sol_newparm_edit, sol.c:525-577
        rank = cells[i][1]
        i, vec = _vector(cells, i + 2, bg, urs, flags & SOL_REMOVE)
        deno = cells[i][1]
        if flags & SOL_REMOVE:
            rank -= 1
        q["newparm"].append((rank - urs, vec, deno))
        i += 1
    kind, a = cells[i][0], cells[i][1]
    i += 1
    if kind == S_LIST:  # sol_list_edit, sol.c:591-638
        q["list"] = []
        for _ in range(a):
            i, vec = _vector(cells, i, bg, urs, flags)
            q["list"].append(vec)
        if flags & SOL_DUAL:
            i, q["then"] = _quast(cells, i, bg, urs, 0)
    elif kind == S_IF:
        i, q["cond"] = _vector(cells, i, bg, urs, flags & SOL_REMOVE)
        i, q["then"] = _quast(cells, i, bg, urs, flags)
        i, q["orelse"] = _quast(cells, i, bg, urs, flags)
    return i, q


def _equalities_dual(s, inequnk):
    """pip_quast_equalities_dual, piplib.c:651-690"""
    if s is None:
        return
    if s["cond"] is not None:
        _equalities_dual(s["then"], inequnk)
        _equalities_dual(s["orelse"], inequnk)
    if not s["list"] or s["then"] is None or not s["then"]["list"]:
        return
    L, k = s["then"]["list"], 0
    for row in inequnk:
        if int(row[0]) == 0:
            if L[k][0][0] != 0:
                k += 1
                del L[k]
            else:
                del L[k]
                L[k][0] = (-L[k][0][0], L[k][0][1])
                k += 1
        else:
            k += 1


def _vec_text(v):
    return "#[" + "".join(f" {n}" if d == 1 else f" {n}/{d}" for n, d in v) + "]"


def _print(q, indent, out):
    """pip_quast_print, piplib.c:198-317"""
    pad = " " * max(indent, 0)
    ni = indent + 1 if indent >= 0 else indent
    if q is None:
        out.append(pad + "void\n")
        return
    for rank, vec, deno in q["newparm"]:
        out.append(f"{pad}(newparm {rank} (div {_vec_text(vec)} {deno}))\n")
    if q["cond"] is None:
        if q["list"] is None:
            out.append(pad + "()\n")
        else:
            out.append(pad + "(list\n")
            for v in q["list"]:
                out.append(" " * max(indent + 1, 0) + _vec_text(v) + "\n")
            out.append(pad + ")\n")
        if q["then"] is not None:
            _print(q["then"], ni, out)
    else:
        out.append(f"{pad}(if {_vec_text(q['cond'])}\n")
        _print(q["then"], ni, out)
        _print(q["orelse"], ni, out)
        out.append(pad + ")\n")


def quast_text(cells, info, inequnk=None):
    """What pip_quast_print prints for pip_solve's answer, from the engine's cells [(kind, param1, param2)] and the
    pipamd_pip_info dict; inequnk (the domain matrix) is needed for Compute_dual with equalities (piplib.c:868-869)."""
    if info["is_void"]:
        return "void\n"
    _, q = _quast(list(cells), 0, info["sol_bg"], info["urs_parms"], info["sol_flags"])
    if (info["sol_flags"] & SOL_DUAL) and inequnk is not None and info["ni"] > len(inequnk):
        _equalities_dual(q, inequnk)
    out = []
    _print(q, 0, out)
    return "".join(out)


# ------------------------------------------------------------------ the front ends' `pip` mode
def option_words(options):
    return "".join(w + "\n" for bit, w in ((MAXIMIZE, "Maximize"), (URS_UNKNOWNS, "Urs_unknowns"), (URS_PARMS, "Urs_parms"))
                   if options & bit) + ("" if options & NQ else "Rational\n") + ("Dual\n" if options & DUAL else "")


def pip_input(inequnk, ineqpar, bg, options):
    """the stdin of `refpip pip` / `oraclepip pip` (example/example.c): the bignum is given in context-matrix columns"""
    dom, ctx = np.asarray(inequnk, dtype=np.int64), np.asarray(ineqpar, dtype=np.int64)
    bignum = bg - (dom.shape[1] - ctx.shape[1]) if bg > 0 else bg
    return (matrix_text(ctx) + f"\n{bignum}\n\n" + matrix_text(dom) + "\n" + option_words(options)).encode()


def quast_part(stdout):
    """the printed quast behind the echo of the input (one empty line ends the echo)"""
    return stdout.split("\n\n", 1)[1]


def run_pip(exe, inequnk, ineqpar, bg, options, timeout=10, env=None):
    """(exit code, printed quast or None, pivots or None: only refpip reports them)"""
    p = subprocess.run([exe, "pip"], input=pip_input(inequnk, ineqpar, bg, options), capture_output=True, timeout=timeout,
                       env=None if env is None else dict(os.environ, **env))
    if p.returncode != 0:
        return p.returncode, None, None
    piv = [int(s.split()[1]) for s in p.stderr.decode().splitlines() if s.startswith("pivots ")]
    return 0, quast_part(p.stdout.decode("latin-1")), piv[0] if piv else None


# ------------------------------------------------------------------ seeded families
FAMILIES = {  # name: (count, Nn range, Np range, rows range, context rows range)
    "p3": (48, (2, 3), (1, 2), (3, 6), (1, 2)),
    "p8": (24, (6, 8), (3, 3), (8, 12), (1, 2)),
}
KINDS = (NQ, 0, DUAL)  # integer, rational, rational + Dual
SHIFTS = (0, MAXIMIZE, URS_UNKNOWNS)


def option_cycle(k):
    """problem k's options and Bg choice (0: -1, 1: the first parameter, 2: the last): the cross product
    {integer, rational, rational+Dual} x {none, Maximize, Urs_unknowns} x {Urs_parms off, on} x {three Bg}, walked so
    that every factor changes often.  Dual is not combined with Urs_parms (the reference itself exits or faults there):
    a Dual problem keeps Dual and drops Urs_parms."""
    kind, shift, urs, bgsel = KINDS[k % 3], SHIFTS[(k // 3) % 3], (k // 9) % 2, (k + k // 18) % 3
    if urs and kind == DUAL:
        urs = 0
    return kind | shift | (URS_PARMS if urs else 0), bgsel


def gen_problem(rng, k, shape):
    """one problem of a family: entries in [-3, 3], constants up to 12 (tests/manual/fuzz_pipsolve.py)"""
    _, nnr, npr, rr, cr = shape
    nn, npar = int(rng.integers(nnr[0], nnr[1] + 1)), int(rng.integers(npr[0], npr[1] + 1))
    nrow, ncrow = int(rng.integers(rr[0], rr[1] + 1)), int(rng.integers(cr[0], cr[1] + 1))
    options, bgsel = option_cycle(k)
    dom = rng.integers(-3, 4, size=(nrow, nn + npar + 2)).astype(np.int64)
    dom[:, 0] = 1
    # (under Maximize the origin stays feasible, so that most of those answers exist -- and are unbounded)
    dom[:, -1] = rng.integers(0 if options & MAXIMIZE else -6, 13, size=nrow)
    eq = k % 8  # equalities in the domain: first row, last row, every row; in the context
    if eq == 1:
        dom[0, 0] = 0
    elif eq == 2:
        dom[-1, 0] = 0
    elif eq == 3 and k % 16 == 3:
        dom[:, 0] = 0
    ctx = rng.integers(-2, 3, size=(ncrow, npar + 2)).astype(np.int64)
    ctx[:, 0] = 1
    ctx[:, -1] = rng.integers(0, 9, size=ncrow)
    if eq == 5:
        ctx[0, 0] = 0
    if k % 6 == 1:  # an empty context: p >= 1 and -p >= 0
        ctx = np.zeros((2, npar + 2), dtype=np.int64)
        ctx[0] = [1] + [1] + [0] * (npar - 1) + [-1]
        ctx[1] = [1] + [-1] + [0] * (npar - 1) + [0]
    bg = -1 if bgsel == 0 else (nn + 1 if bgsel == 1 else nn + npar)
    return dict(inequnk=dom.tolist(), ineqpar=ctx.tolist(), bg=bg, options=options)


def nonzero_dual(text):
    """a Compute_dual answer prints every solution list followed by the list of its dual values: is one of them not 0?"""
    lists = text.split("(list")[1:]
    return any(re.search(r"[ \[]-?[1-9]", part.split(")")[0]) for part in lists[1::2])


def slot_wish(k, p, text):
    """What problem k of a family should show, so that a family has enough of every kind of answer: an unbounded answer
    under Maximize, a non-zero dual value under Dual, a new parameter in every other integer problem, an `if` in every
    other remaining one.  A wish is dropped after 40 draws."""
    o = p["options"]
    if text.strip() == "void" or k % 6 == 1:
        return True
    if o & MAXIMIZE:
        return "/0" in text
    if o & DUAL and not o & NQ:
        return nonzero_dual(text)
    if o & NQ:
        return "(newparm" in text or k % 2 == 1
    return "(if" in text or k % 2 == 1


def defined_answer(p, text):
    """Is the reference's answer to a Compute_dual problem a defined one?  tab_sort_rows (traiter.c:556-623) gets `ineq`
    from malloc, fills it for the rows that are not Unit (traiter.c:581-589) and then scatters `pos` through ALL of it
    (traiter.c:616-618).  In the first call of traiter() no row below the unknowns is Unit; in the calls below a fork of
    the quast some are, and the dual values printed there depend on what the heap held (the engine and the CPU
    restatement read zeros there).  Such an answer is no fixture: a Compute_dual problem whose quast forks is drawn
    again.  The rule comes from the reference's source alone; it does not look at what the engine computes."""
    return "(if" not in text


def gen_family(name, seed, count=None, exe=None):
    """`count` problems the authority `exe` (default: the reference) finishes: [(problem, text, pivots)]; a problem it
    exits on, or does not finish in time, is drawn again, and so are one that does not fulfil its slot's wish and a
    Compute_dual problem to which the reference has no defined answer"""
    shape = FAMILIES[name]
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count or shape[0]):
        for draw in range(90):
            p = gen_problem(rng, k, shape)
            try:
                rc, text, piv = run_pip(exe or pb.REFPIP, p["inequnk"], p["ineqpar"], p["bg"], p["options"], timeout=1)
            except subprocess.TimeoutExpired:
                continue
            if rc == 0 and len(text) <= 2000 and (draw >= 40 or slot_wish(k, p, text)):  # (long answers: fixture size)
                if exe is None and (p["options"] & DUAL) and not (p["options"] & NQ) and not defined_answer(p, text):
                    continue
                out.append((p, text, piv))
                break
        else:
            raise RuntimeError(f"family {name}: no problem {k} that the authority finishes")
    return out


def golden(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)["problems"]
