"""Shared by the tests of the shifted batch entries (Maximize / Urs_unknowns): the plain systems of the families of
tests/golden/shift/ and of the GPU tests, and the reading of a tableau-level solution text.  Test helper only."""
import json
import os
import re
from math import gcd

import numpy as np

from piplib_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shift")
BOX = 12


def plain_rows(seed, nvar, ni, batch, kw, box):
    """synth.lexmin_batch's systems; box: nvar more rows -x_j + BOX >= 0 (every unknown bounded above)"""
    rows = synth.lexmin_batch(seed, batch, nvar, ni, **kw)
    if box:
        B = np.zeros((batch, nvar, nvar + 1), np.int64)
        B[:, np.arange(nvar), np.arange(nvar)] = -1
        B[:, :, -1] = BOX
        rows = np.concatenate([rows, B], axis=1)
    return rows


def shifted(rows, shift):
    """shift_model.shift_rows for a whole (batch, ni, nvar + 1) int64 array, in numpy (values far below 2^63)"""
    A, c = rows[:, :, :-1], rows[:, :, -1:]
    s = A.sum(axis=2, keepdims=True)
    return np.ascontiguousarray(np.concatenate([-A, c, s] if shift > 0 else [A, c, -s], axis=2))


def golden(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def forms(text):
    """tableau-level text "(list #[ b c] ...)" of a solve with one parameter -> [(big, cst, den), ...] over a common
    denominator; None for "()" """
    t = text.strip()
    if "".join(t.split()) == "()":
        return None
    out = []
    for body in re.findall(r"#\[([^\]]*)\]", t):
        (bn, bd), (cn, cd) = [(int(n), int(d) if d else 1) for n, d in re.findall(r"(-?\d+)(?:/(\d+))?", body)]
        den = bd * cd // gcd(bd, cd)
        out.append((bn * (den // bd), cn * (den // cd), den))
    return out
