#!/usr/bin/env python3
"""Regenerate tests/golden/tape_eval/p5_grid.json from the reference itself: the parametric system of the golden family
p5 (tests/golden/instances/p5.json: 5 unknowns, 2 parameters, 7 rows of which two are equalities) solved ONCE as the
parametric problem it is, and solved again as a plain system at every point of a grid.

Runs oracle/_ref/refpip (the reference library behind oracle/ref_driver.c) and stores
  * the tape the reference prints for the parametric problem -- the tableau with equalities as twin rows, columns
    unknowns | constant | parameters, no context --, integer (with tab_simplify, as maind.c does) and rational;
  * per flavour and point, the unknowns the reference prints for that instance as a plain system (pip_solve, as
    make_instances_fixtures.py records them): [numerator, denominator] pairs, null where no list is printed.
The points are the grid 0..9 x 0..9, followed by whatever EXTRA_POINTS lists.  A family that gives the tests too little to
hold on to is rejected here: per flavour at least 6 distinct leaves reached, at least 8 points without a solution, at
least one condition that evaluates to exactly 0; at least 20 points through a new parameter (integer), at least 20 with a
non-integer answer (rational).  The printed tapes walked by tests/tape_model.py must give the recorded answers.  Only needed
when the fixture changes; needs the reference build.
"""
import json, os, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
REFPIP = os.path.join(HERE, "..", "..", "oracle", "_ref", "refpip")

GRID = [[n, m] for n in range(10) for m in range(10)]
EXTRA_POINTS = []
FLAVOURS = {"int": ("", 1), "rat": ("Rational", 0)}  # name -> (pip_solve's options for an instance, nq of the tableau)


def main():
    import instances_model as im
    import pipbatch as pb
    import system_model as sy
    import tape_cases as tc
    import tape_model as tm
    g = im.golden()
    nvar, nparm, eq, matrix = g["nvar"], g["nparm"], tuple(g["eq_rows"]), g["matrix"]
    points = GRID + EXTRA_POINTS
    assert len(GRID) == 100 and len(set(map(tuple, points))) == len(points)
    tab = tc.parametric_tableau(matrix, nvar, nparm, eq)
    systems = im.expand(matrix, points)
    doc = {"nvar": nvar, "nparm": nparm, "eq_rows": list(eq), "matrix": matrix, "points": points, "tapes": {}, "answers": {}}
    for name, (opts, nq) in FLAVOURS.items():
        prob = pb.Problem(nvar, nparm, tab.shape[0], 0, -1, nq, tab, [])
        res = pb.run_batch(REFPIP, [prob]).results[0]
        assert res.status == pb.ST_OK, (name, res.status, res.abort_code)
        doc["tapes"][name] = res.text
        xs = []
        for k, system in enumerate(systems):
            p = subprocess.run([REFPIP, "pip"], input=sy.pip_text(system, eq, opts), capture_output=True, timeout=60)
            assert p.returncode == 0, (name, k, p.stderr[:200])
            lists = sy.parse_lists(p.stdout.decode("latin-1"))
            assert len(lists) <= 1, (name, k)
            xs.append(lists[0] if lists else None)
        doc["answers"][name] = xs
        # what the tests can hold on to
        cells = tc.cells_from_text(res.text)
        trace = {}
        got = tm.evaluate_cells(cells, nvar, nparm, 0, points, 64, trace)
        assert tc.answers_of(got) == xs, name  # the printed tape, walked, IS the recorded answers
        leaves = len(set(r[1] for r in got))
        unsolved = sum(x is None for x in xs)
        through_new = sum(bool(t.get("news")) for t in _traces(tm, cells, nvar, nparm, points))
        fractions = sum(x is not None and any(d != 1 for _, d in x) for x in xs)
        print(name, "pivots", res.pivots, "cells", len(cells), "leaves reached", leaves, "unsolved", unsolved,
              "through a new parameter", through_new, "non-integer", fractions, "conditions exactly 0", trace.get("zeros", 0))
        assert leaves >= 6 and unsolved >= 8 and trace.get("zeros", 0) >= 1
        assert through_new >= 20 if name == "int" else fractions >= 20
    out_dir = os.path.join(HERE, "tape_eval")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "p5_grid.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


def _traces(tm, cells, nvar, nparm, points):
    nodes, _ = tm.parse(cells, nvar, nparm, 0, 64)
    for p in points:
        t = {}
        tm.evaluate(nodes, nvar, nparm, 0, p, 64, t)
        yield t


if __name__ == "__main__":
    main()
