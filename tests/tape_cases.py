"""Tapes for the evaluator's tests: builders for hand-made ones, the printed text of a tape (what sol_edit, sol.c:291-422,
and engine.tape_text write) turned back into cells, and the parametric problem of the golden family p5 in the tableau form
the layer-3 entries take.  Cells are (kind, param1, param2).  Test helper only."""
import json
import os
import re
from math import gcd

import numpy as np

from tape_model import DIV, FORM, IF, LIST, NEW, NIL, VAL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tape_eval")
MAX64, MIN64 = (1 << 63) - 1, -(1 << 63)
MAX128, MIN128 = (1 << 127) - 1, -(1 << 127)


# ---------------------------------------------------------------- builders
def form(nums, den=1):
    return [(FORM, len(nums), 0)] + [(VAL, int(v), int(den)) for v in nums]


def new(P, coefs, D, item):
    """newparm P = floor((coefs . (theta, 1)) / D), in scope for `item`"""
    return [(NEW, P, 0), (DIV, 0, 0)] + form(coefs) + [(VAL, int(D), 1)] + item


def iff(nums, then, other, den=1):
    return [(IF, 0, 0)] + form(nums, den) + then + other


def leaf(forms, duals=None):
    """forms: (nums, den) per unknown; duals: (num, den) per inequality, or None"""
    out = [(LIST, len(forms), 0)]
    for nums, den in forms:
        out += form(nums, den)
    if duals is not None:
        out.append((LIST, len(duals), 0))
        for n, d in duals:
            out += form([n], d)
    return out


def nil():
    return [(NIL, 0, 0)]


def if_chain(k, nparm=1):
    """k conditions i - theta_0 >= 0 ? () : ..., i = 0 .. k - 1, the last else the list (theta_0): a point theta_0 = t
    with 0 <= t < k jumps over t conditions and ends in the NIL of condition t (ordinal t), whose value is exactly 0;
    t >= k walks the whole chain to the list, ordinal k.  One unknown."""
    cells = []
    zeros = [0] * (nparm - 1)
    for i in range(k):
        cells += [(IF, 0, 0)] + form([-1] + zeros + [i]) + nil()
    return cells + leaf([([1] + zeros + [0], 1)])


def new_chain(nparm, count):
    """`count` new parameters, each floor((previous + 1) / 1) -- the previous one being theta_(nparm-1) for the first --,
    then the list (last new parameter, theta_0): the leaf reads the highest slot"""
    assert nparm >= 1 and count >= 1
    P = nparm + count
    item = leaf([([0] * (P - 1) + [1, 0], 1), ([1] + [0] * P, 1)])
    for q in range(P - 1, nparm - 1, -1):
        item = new(q, [0] * (q - 1) + [1, 1], 1, item)
    return item


# ---------------------------------------------------------------- printed text -> cells
_TOKEN = re.compile(r"\(newparm|\(div|\(if|\(list|\(\)|#\[|\]|\)|-?\d+(?:/-?\d+)?|void")


def cells_from_text(text):
    """the cells of a printed tape.  The printers reduce every value on its own; a form's values are put back over one
    denominator, their least common multiple, which a FORM's cells share.  "void" is the empty tape."""
    toks = _TOKEN.findall(text)
    assert "".join(toks) == "".join(text.split()), "unknown text in a printed tape"
    if toks == ["void"]:
        return []
    out = []
    i = 0

    def value(t):
        n, _, d = t.partition("/")
        return int(n), int(d) if d else 1

    def item():
        nonlocal i
        t = toks[i]
        i += 1
        if t == "()":
            out.append((NIL, 0, 0))
        elif t == "(newparm":
            out.append((NEW, int(toks[i]), 0))
            i += 1
            item()  # the div
            assert toks[i] == ")"
            i += 1
            item()  # what the new parameter is in scope for
        elif t == "(div":
            out.append((DIV, 0, 0))
            item()
            out.append((VAL,) + value(toks[i]))
            i += 1
            assert toks[i] == ")"
            i += 1
        elif t == "(if":
            out.append((IF, 0, 0))
            item(), item(), item()
            assert toks[i] == ")"
            i += 1
        elif t == "(list":
            at = len(out)
            out.append(None)
            k = 0
            while toks[i] != ")":
                item()
                k += 1
            i += 1
            out[at] = (LIST, k, 0)
        elif t == "#[":
            vals = []
            while toks[i] != "]":
                vals.append(value(toks[i]))
                i += 1
            i += 1
            den = 1
            for _, d in vals:
                assert d > 0
                den = den * d // gcd(den, d)
            out.append((FORM, len(vals), 0))
            out.extend((VAL, n * (den // d), den) for n, d in vals)
        else:
            raise ValueError(f"token {t!r} where an item belongs")

    while i < len(toks):
        item()
    return out


def ndual_of(cells, nvar):
    """length of the dual list behind the first solution list of a tape (0: none)"""
    for k, c in enumerate(cells):
        if c[0] == LIST and c[1] == nvar:
            j = k + 1
            for _ in range(nvar):
                j += 1 + cells[j][1]
            return cells[j][1] if j < len(cells) and cells[j][0] == LIST else 0
    return 0


# ---------------------------------------------------------------- the golden family
def golden(name="p5_grid"):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def parametric_tableau(matrix, nvar, nparm, eq_rows):
    """the parametric system (rows unknowns | parameters | constant) as the inequalities of a tableau: unknowns | constant |
    parameters, an equality followed by its negation -> (ni, nvar + nparm + 1) int64"""
    eq = set(eq_rows)
    rows = []
    for r, row in enumerate(matrix):
        t = [int(v) for v in row[:nvar]] + [int(row[-1])] + [int(v) for v in row[nvar:nvar + nparm]]
        rows.append(t)
        if r in eq:
            rows.append([-v for v in t])
    return np.array(rows, dtype=np.int64)


def answers_of(results):
    """the model's (status, leaf, x, dual) per point as the fixture records answers: the x list, None without one"""
    return [[list(p) for p in x] if st == 1 else None for st, _, x, _ in results]
