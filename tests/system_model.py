"""What pip_solve does to a plain system on the way to traiter() and to the dual on the way back, in Python ints: the
expansion of equalities and the shift of tab_Matrix2Tableau (tab.c:328-389), tab_simplify (tab.c:396-427), the reduction
of a dual value (sol_vector_edit with flags 0, sol.c:475-500) and the merge of an equality's two values
(pip_quast_equalities_dual, piplib.c:651-690).  The model the system batch entries (pipamd_batch_load_system,
pipamd_batch_dual_system) are held to; tests/test_system_model.py holds it to the reference.  Test helper only."""
import json
import os
import re
import subprocess
from math import gcd

import numpy as np

import pipbatch as pb
import shift_cases as sc
import shift_model as sm
from datfile import matrix_text

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "system")
# name: equality rows of the family (the shapes and seeds are in the fixture files)
EQ_ROWS = {"s5": (0, 4, 5), "s12": (2, 9)}
# pip_solve's options per case name -> (shift, integer, dual)
OPTIONS = {"": (0, 1, 0), "Rational+Dual": (0, 0, 1), "Maximize": (1, 1, 0), "Maximize+Rational+Dual": (1, 0, 1),
           "Urs_unknowns": (-1, 1, 0), "Urs_unknowns+Rational+Dual": (-1, 0, 1)}


def expand(rows, eq_rows, shift):
    """rows: plain rows a_0 .. a_(n-1) | c; the tableau rows in tab_Matrix2Tableau's order: each row shifted, an equality
    followed by its negation in every column"""
    eq = set(eq_rows)
    out = []
    for r, row in enumerate(rows):
        t = sm.shift_rows([row], shift)[0] if shift else [int(v) for v in row]
        out.append(t)
        if r in eq:
            out.append([-v for v in t])
    return out


def simplify(tab, cst):
    """tab_simplify: per row the gcd of every column but `cst`; beyond 1 those columns are divided by it, the constant
    with the floor"""
    out = []
    for t in tab:
        g = row_gcd(t, cst)
        out.append([v // g for v in t] if g > 1 else list(t))  # (// is the floor; the other columns divide exactly)
    return out


def row_gcd(t, cst):
    g = 0
    for j, v in enumerate(t):
        if j != cst:
            g = gcd(g, v)
    return g


def tableau(rows, eq_rows, shift, simp):
    t = expand(rows, eq_rows, shift)
    return simplify(t, len(rows[0]) - 1) if simp else t


def tableaux(rows, eq_rows, shift, simp):
    """the same for a (batch, nrows, nvar + 1) array: (batch, nrows + len(eq_rows), ncol) int64"""
    return np.array([tableau(r, eq_rows, shift, simp) for r in rows.tolist()], dtype=np.int64)


def reduce_pair(n, d):
    """sol_vector_edit with flags 0 on one value N / D"""
    n, d = int(n), int(d)
    g = gcd(n, d)
    if g == 0:
        return n, d
    return n // g, (1 if g == d else d // g)


def dual(pairs, nrows, eq_rows):
    """pairs: one (numerator, denominator) per TABLEAU row, as solution_dual emits them -> one reduced pair per input
    row; an equality with the values u (its row) and v (the negated row): u if u != 0, else -v"""
    eq = set(eq_rows)
    red = [reduce_pair(n, d) for n, d in pairs]
    assert len(red) == nrows + len(eq)
    out, t = [], 0
    for r in range(nrows):
        if r in eq:
            u, v = red[t], red[t + 1]
            out.append(u if u[0] != 0 else (-v[0], v[1]))
            t += 2
        else:
            out.append(red[t])
            t += 1
    return out


def golden(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def family_rows(g, box, batch=None):
    return sc.plain_rows(g["seed"], g["nvar"], g["ni"], batch or g["batch"], g["kw"], box)


def parse_lists(text):
    """every "(list #[ n/d] ...)" of a printed quast -> [[[n, d], ...], ...] (d = 1 where none is printed)"""
    t = "".join(text.split())
    parts = t.split("(list")[1:]
    return [[[int(n), int(d) if d else 1] for n, d in re.findall(r"#\[(-?\d+)(?:/(-?\d+))?\]", p)] for p in parts]


def pip_text(rows, eq_rows, options):
    """the input of the front ends' `pip` mode: no context, no big parameter, the system with its marker column"""
    marker = np.ones((len(rows), 1), np.int64)
    marker[list(eq_rows), 0] = 0
    dom = np.concatenate([marker, np.asarray(rows, dtype=np.int64)], axis=1)
    opts = "".join(o + "\n" for o in options.split("+") if o)
    return (matrix_text(np.zeros((0, 2), np.int64)) + "\n-1\n\n" + matrix_text(dom) + "\n" + opts).encode()


def oracle_tableau_dual(rows, eq_rows, options):
    """the reduced dual values per TABLEAU row from the CPU oracle's tape with TRAITER_DUAL: its pip front end on the
    system with every equality written out as its two inequalities (the same tableau, nothing to merge); None without
    a solution"""
    eq = set(eq_rows)
    wide = []
    for r, row in enumerate(rows):
        wide.append([int(v) for v in row])
        if r in eq:
            wide.append([-int(v) for v in row])
    p = subprocess.run([pb.ORACLEPIP, "pip"], input=pip_text(wide, (), options), capture_output=True, timeout=60)
    assert p.returncode == 0, p.stderr[:200]
    lists = parse_lists(p.stdout.decode())
    if not lists:
        return None
    assert len(lists) == 2 and len(lists[1]) == len(wide)
    return [tuple(v) for v in lists[1]]
