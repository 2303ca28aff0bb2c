#!/usr/bin/env python3
"""Regenerate tests/golden/instances/p5.json from the reference itself: ONE parametric system -- 5 unknowns, 2 parameters,
7 rows of which two are equalities -- at 8 parameter points, each instance expanded in Python ints
(instances_model.expand) and given to the reference's pip_solve as the plain system it is, under the six option strings
of system_model.OPTIONS (piplib.c:722-880; tab_Matrix2Tableau tab.c:292-393; tab_simplify tab.c:396-427; sol_vector_edit
sol.c:435-512; pip_quast_equalities_dual piplib.c:651-690).

Runs oracle/_ref/refpip pip (the reference library behind oracle/ref_driver.c) and stores the matrix, the points, the
equality rows and, per option string and point, the printed unknowns as [numerator, denominator] pairs (null where no
list is printed), the printed dual pairs (null without Dual or without a list) and the pivot count the driver reports.
A family that does not give the tests enough to hold on to -- solved and infeasible instances, non-zero duals, rows
tab_simplify changes with the floor -- is rejected here.  Only needed when the fixture changes; needs the reference build.
"""
import json, os, re, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
REFPIP = os.path.join(HERE, "..", "..", "oracle", "_ref", "refpip")

NVAR, NPARM, EQ = 5, 2, (0, 3)
# unknowns x0 .. x4 | parameters n, m | constant
MATRIX = [
    [1, 1, 0, 0, 0, -1, 0, 0],     # x0 + x1 == n
    [0, 2, 2, 0, 0, 0, -1, -1],    # 2 x1 + 2 x2 >= m + 1
    [0, -1, -1, 0, 0, 0, 1, 2],    # x1 + x2 <= m + 2
    [0, 0, 0, 1, -2, -1, 1, 0],    # x3 == 2 x4 + n - m
    [0, 0, 0, 0, 3, -1, 0, 3],     # 3 x4 >= n - 3
    [0, 0, 0, -1, -1, 2, 0, 1],    # x3 + x4 <= 2 n + 1
    [0, 0, 1, 1, 0, 0, 0, -3],     # x2 + x3 >= 3
]
POINTS = [[0, 0], [4, 0], [2, 1], [7, 3], [5, 1], [0, 9], [-1, 2], [6, 20]]


def main():
    import instances_model as im
    import system_model as sy
    out_dir = os.path.join(HERE, "instances")
    os.makedirs(out_dir, exist_ok=True)
    rows = im.expand(MATRIX, POINTS)
    assert len(MATRIX) == 7 and all(len(r) == NVAR + NPARM + 1 for r in MATRIX) and len(POINTS) == 8
    doc = {"nvar": NVAR, "nparm": NPARM, "eq_rows": list(EQ), "matrix": MATRIX, "points": POINTS, "cases": {}}
    for opts, (shift, nq, dual) in sy.OPTIONS.items():
        xs, duals, pivots = [], [], []
        for k, system in enumerate(rows):
            p = subprocess.run([REFPIP, "pip"], input=sy.pip_text(system, EQ, opts), capture_output=True, timeout=60)
            assert p.returncode == 0, (opts, k, p.stderr[:200])
            lists = sy.parse_lists(p.stdout.decode("latin-1"))
            assert len(lists) == (2 if dual else 1) * bool(lists), (opts, k, len(lists))
            xs.append(lists[0] if lists else None)
            duals.append(lists[1] if dual and lists else None)
            pivots.append(int(re.search(rb"pivots (\d+)", p.stderr).group(1)))
        doc["cases"][opts] = {"x": xs, "dual": duals, "pivots": pivots}
        solved = [x for x in xs if x is not None]
        print(repr(opts), "lists", len(solved), "of", len(xs), "pivots", pivots)
        assert 3 <= len(solved)
        if not shift:
            assert len(solved) <= len(xs) - 2  # some points make the system infeasible
        if dual:
            got = [d for d in duals if d is not None]
            assert len(got) == len(solved) and all(len(d) == len(MATRIX) for d in got)  # one value per input row
            assert sum(any(n != 0 for n, _ in d) for d in got) >= 3
    changed = floors = 0
    for system in rows:
        for t in sy.tableau(system, EQ, 0, 0):
            g = sy.row_gcd(t, NVAR)
            changed += g > 1
            floors += g > 1 and t[NVAR] % g != 0
    print("tab_simplify changes", changed, "rows, the floor matters in", floors)
    assert changed >= 8 and floors >= 4
    with open(os.path.join(out_dir, "p5.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
