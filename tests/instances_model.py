"""The instances of one parametric system in Python ints: the substitution pipamd_batch_load_instances does on the device
-- row r of system b is a_r0 .. a_r(nvar-1) | c_r + sum_k p_rk * theta_bk --, which systems fit an entry width, the golden
family of tests/golden/instances/ and hand-built systems at the edges of int64 and __int128.  What the plain systems
become from there on is tests/system_model.py's.  Test helper only."""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instances")


def expand(matrix, points):
    """matrix: nrows x (nvar + nparm + 1), unknowns | parameters | constant; points: batch x nparm.  The dense systems,
    [batch][nrows][nvar + 1], as Python ints: nothing wraps."""
    points = [[int(t) for t in p] for p in points]
    nparm = len(points[0]) if points else 0
    out = []
    for theta in points:
        assert len(theta) == nparm
        system = []
        for row in matrix:
            row = [int(v) for v in row]
            nvar = len(row) - nparm - 1
            assert nvar >= 0
            system.append(row[:nvar] + [row[-1] + sum(p * t for p, t in zip(row[nvar:nvar + nparm], theta))])
        out.append(system)
    return out


def fits(rows, bits):
    """one boolean per system: does every constant fit a signed integer of `bits` bits?  (The unknowns' coefficients are
    the matrix's int64 values as they are.)"""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    return [all(lo <= r[-1] <= hi for r in system) for system in rows]


def golden(name="p5"):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


# ---------------------------------------------------------------- the edges of the entry types
# Two unknowns, four rows, twelve parameters.  The first and the last row are the edge rows,
#   -2 x0 + K0 >= 0,  K0 = 2^62 (t0 - t1) + t2 - 2^63 (t8 + t9)
#   -2 x1 + K3 >= 0,  K3 = 2^62 (t3 - t4) + t5 - 2^63 (t10 + t11)
# between them x0 >= t6 and x1 >= t7.  The gcd of an edge row's unknown columns is 2: tab_simplify halves its constant
# with the floor.  A constant K that is small says x <= K / 2, a K at the top of the type leaves the answer (t6, t7), a K
# at the bottom makes the system infeasible: a wrapped or truncated K shows in the answer.
E62, MIN64, MAX64 = 1 << 62, -(1 << 63), (1 << 63) - 1
EDGE_NVAR = 2
EDGE_MATRIX = [
    [-2, 0, E62, -E62, 1, 0, 0, 0, 0, 0, MIN64, MIN64, 0, 0, 0],
    [1, 0, 0, 0, 0, 0, 0, 0, -1, 0, 0, 0, 0, 0, 0],
    [0, 1, 0, 0, 0, 0, 0, 0, 0, -1, 0, 0, 0, 0, 0],
    [0, -2, 0, 0, 0, E62, -E62, 1, 0, 0, 0, 0, MIN64, MIN64, 0],
]
# name: ((t_a, t_b, t_c, t_d, t_e) of an edge row: K = 2^62 (t_a - t_b) + t_c - 2^63 (t_d + t_e), K)
EDGE_ROWS = {
    "max64": ((2, 0, -1, 0, 0), (1 << 63) - 1),         # 2^63 leaves int64, the sum does not
    "min64": ((-2, 0, 0, 0, 0), -(1 << 63)),
    "cancel": ((4, 4, 5, 0, 0), 5),                     # 2^62 * 4 - 2^62 * 4 + 5: each product leaves int64
    "max64+1": ((2, 0, 0, 0, 0), 1 << 63),
    "min64-1": ((-2, 0, -1, 0, 0), -(1 << 63) - 1),
    "2^64+3": ((4, 0, 3, 0, 0), (1 << 64) + 3),         # wraps to 3 in 64 bits
    "max128": ((0, 0, -1, MIN64, MIN64), (1 << 127) - 1),  # two products of 2^126 and a constant of -1
    "max128+1": ((0, 0, 0, MIN64, MIN64), 1 << 127),
    "min128": ((-4, 0, 0, MAX64, MAX64), -(1 << 127)),  # 2 * -2^63 * (2^63 - 1) - 2^64
    "min128-1": ((-4, 0, -1, MAX64, MAX64), -(1 << 127) - 1),
}
EDGE_BENIGN = (0, 0, 9, 0, 0)  # K = 9


def _edge_point(first, last, t6=2, t7=1):
    return list(first[:3]) + list(last[:3]) + [t6, t7] + list(first[3:]) + list(last[3:])


def edge_cases(bits):
    """(matrix, points, nvar, names): one batch for the entry width `bits` that mixes good and bad systems -- every edge
    row of EDGE_ROWS once as the FIRST row of an otherwise harmless system and once as the LAST, and the harmless system
    itself first, in the middle and last.  Which systems are bad is for fits(expand(matrix, points), bits) to say; the
    expected constants are asserted here against the substitution."""
    assert bits in (64, 128)
    points, names = [_edge_point(EDGE_BENIGN, EDGE_BENIGN)], ["benign"]
    for name, (t, k) in EDGE_ROWS.items():
        points.append(_edge_point(t, EDGE_BENIGN))
        names.append(name + ",first")
        points.append(_edge_point(EDGE_BENIGN, t))
        names.append(name + ",last")
        if name == "2^64+3":
            points.append(_edge_point(EDGE_BENIGN, EDGE_BENIGN, 4, 0))
            names.append("benign")
    points.append(_edge_point(EDGE_BENIGN, EDGE_BENIGN, 0, 3))
    names.append("benign")
    rows = expand(EDGE_MATRIX, points)
    for system, name in zip(rows, names):
        if name != "benign":
            kind, where = name.split(",")
            assert system[0 if where == "first" else 3][-1] == EDGE_ROWS[kind][1], name
            assert system[3 if where == "first" else 0][-1] == 9
    assert all(-(1 << 63) <= t < (1 << 63) for p in points for t in p)
    return EDGE_MATRIX, points, EDGE_NVAR, names
