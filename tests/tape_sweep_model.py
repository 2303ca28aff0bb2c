"""A tape swept over a box of integer points under a context, in Python ints: what pipamd_tape_sweep_plan counts and
what pipamd_tape_sweep computes -- the box in row-major order, the context test, the per-point results on top of
tape_model.evaluate_cells, and the summary.  Test helper only."""
import itertools

import tape_model as tm

ST_OUTSIDE = 11
STATUSES = (("solution", tm.ST_SOLUTION), ("nil", tm.ST_NIL), ("range", tm.ST_RANGE), ("outside", ST_OUTSIDE))
MAX_POINTS = 1 << 38  # a call takes fewer
MIN64, MAX64 = -(1 << 63), (1 << 63) - 1


def box_points(lo, hi):
    """the integer points of lo .. hi (inclusive), the last column fastest: itertools.product's order"""
    assert len(lo) == len(hi)
    return [list(p) for p in itertools.product(*[range(int(a), int(b) + 1) for a, b in zip(lo, hi)])]


def binned(info, bits):
    """per-leaf figures are gathered in LDS: 16 bytes per leaf and 64 for the statuses fit beside the slots, and beside
    the program where it is staged"""
    used = tm.slot_bytes(info["slots"], bits) + (8 * info["words"] if info["staged"] else 0)
    return int(used + 16 * (info["leaves"] + 4) <= tm.LDS_BYTES)


def plan(info, bits, point_cols, lo, hi):
    """what pipamd_tape_sweep_plan fills in, or TapeError with its code"""
    if info is None or bits not in (64, 128) or not 0 <= point_cols <= tm.MAX_SLOTS - 1:
        raise tm.TapeError(tm.E_INVALID, "info, bits or point_cols")
    if point_cols and (lo is None or hi is None):
        raise tm.TapeError(tm.E_INVALID, "no bounds")
    n = 1
    for c in range(point_cols):
        if lo[c] > hi[c]:
            raise tm.TapeError(tm.E_INVALID, f"column {c}: lo above hi")
    for c in range(point_cols):
        n *= hi[c] - lo[c] + 1
    if n >= MAX_POINTS:
        raise tm.TapeError(tm.E_TOOLARGE, f"{n} points")
    return {"n_points": n, "summary_words": 8 + 2 * info["leaves"], "binned": binned(info, bits)}


def inside(point, ctx):
    """the point meets every row (marker, coefficients, constant) of the context: marker 0 an equality, any other >= 0"""
    for row in ctx:
        assert len(row) == len(point) + 2
        v = sum(int(a) * int(t) for a, t in zip(row[1:-1], point)) + int(row[-1])
        if (v != 0) if int(row[0]) == 0 else (v < 0):
            return False
    return True


def apply_context(points, ctx, nvar, ndual, evaluate):
    """per point: evaluate(point) -> (status, leaf, x, dual) where it is inside, (ST_OUTSIDE, -1, zeros, zeros) otherwise"""
    out = (ST_OUTSIDE, -1, [(0, 0)] * nvar, [(0, 0)] * ndual)
    return [evaluate(p) if inside(p, ctx) else out for p in points]


def sweep(cells, nvar, nparm, ndual, lo, hi, ctx=(), bits=64):
    """(results, summary) of an unedited tape over the box"""
    nodes, info = tm.parse(cells, nvar, nparm, ndual, bits)
    res = apply_context(box_points(lo, hi), ctx, nvar, ndual, lambda p: tm.evaluate(nodes, nvar, nparm, ndual, p, bits))
    return res, summarise(res, info["leaves"])


def summarise(results, leaves):
    """the summary as engine.sweep_summary hands it out"""
    s = {"counts": {n: 0 for n, _ in STATUSES}, "first": {n: -1 for n, _ in STATUSES},
         "leaf_count": [0] * leaves, "leaf_first": [-1] * leaves}
    name = {v: n for n, v in STATUSES}
    for k, r in enumerate(results):
        n = name[r[0]]
        s["counts"][n] += 1
        if s["first"][n] < 0:
            s["first"][n] = k
        if r[1] >= 0:
            s["leaf_count"][r[1]] += 1
            if s["leaf_first"][r[1]] < 0:
                s["leaf_first"][r[1]] = k
    return s


def words(summary):
    """the summary dict as the device lays it out"""
    return ([summary["counts"][n] for n, _ in STATUSES] + [summary["first"][n] for n, _ in STATUSES] +
            list(summary["leaf_count"]) + list(summary["leaf_first"]))


# context rows at the edges of the arithmetic: (rows, point, inside?)
def edge_rows():
    c31 = [MIN64] * 31
    return [
        # 31 x (-2^63)^2 = 31 * 2^126 is beyond 128 bits; its sign is right whatever the constant
        ([[1] + c31 + [MIN64]], [MIN64] * 31, True),
        ([[1] + c31 + [0]], [MAX64] * 31, False),
        ([[0] + c31 + [0]], [MIN64] * 31, False),          # an equality whose value leaves 128 bits is not 0
        # an equality met only through cancellation: each product leaves int64
        ([[0, 1 << 62, -(1 << 62), 0]], [7, 7], True),
        ([[0, 1 << 62, -(1 << 62), 0]], [7, 8], False),
        ([[0, 1 << 62, -(1 << 62), 0]], [MAX64, MAX64], True),
        # a marker other than 0 or 1 is an inequality
        ([[-5, 1, 0, -3]], [3, 0], True),
        ([[7, 1, 0, -3]], [2, 0], False),
        ([[2, 0, 0, 0]], [5, 5], True),
    ]
