#!/usr/bin/env python3
"""Regenerate tests/golden/tape_edit/*.json from the reference itself: per option set one random parametric problem
(3 unknowns, 2 parameters, 5-8 rows, no context rows) solved ONCE by `refpip pip` -- the quast pip_solve returns, i.e.
after sol_quast_edit --, and solved again as a plain system under the same options at every point of a grid.

A fixture holds the problem (inequnk, ineqpar, bg, options as PIPAMD_PIP_* bits), the printed quast, the grid and per
point the unknowns the reference prints for that instance ([numerator, denominator] pairs, denominator 0 for an
unbounded unknown, null where no list is printed).  Urs_parms families use the grid -3..6 x -3..6 (51 points with a
negative coordinate), the others 0..9 x 0..9.

A family is rejected unless the printed quast, walked by tests/tape_edit_model.py, gives every recorded answer (of an
unbounded unknown only the /0 mark is compared: the printed numerators have lost their denominator), at least 4 distinct
leaves are reached and at least 8 points have no solution.  Across the families at least 20 points go through a new
parameter, and one family (maximize) has at least 10 points with an unbounded unknown and at least 10 without.  The
points "without" are points without a solution: the parameters only move the constants of the rows, so the domain's
recession cone -- and with it which unknowns of a lexicographic optimum are unbounded -- is the same at every point
that has a solution (5,000 seeds searched for a family with bounded and unbounded SOLVED points gave none).  What can
vary is held instead: that family also has at least 10 points whose answer holds an unbounded unknown beside a bounded
one, so both kinds of denominator are written within one solution list.  Recorded besides:
how many dropped coefficients of conditions and new-parameter forms were not 0 in the raw tape (the CPU restatement's, on
the tableau tests/pipsolve_model.py builds; exam_coef and integrer.c:373-377 say 0), and whether the reference's instance
numerators of unbounded unknowns agree with the model's (not required).  Seeds the reference does not finish in a second,
or exits on, are passed over.  Only needed when the fixtures change; needs the reference build.
"""
import json, os, subprocess, sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

NVAR, NPARM = 3, 2
FAMILIES = {  # name -> (PIPAMD_PIP_* options, first seed)
    "maximize": (1 | 2, 490),
    "urs_unknowns": (1 | 8, 200),
    "urs_parms": (1 | 4, 300),
    "urs_parms_maximize": (1 | 4 | 2, 400),
    "rational_maximize": (0 | 2, 500),
}
WANT_NEW = {"maximize": 0, "urs_unknowns": 8, "urs_parms": 8, "urs_parms_maximize": 4, "rational_maximize": 0}
WANT_UNBOUNDED = {"maximize": 10}  # at least this many points with an unbounded unknown, as many without, as many mixed


def grid(options):
    lo = -3 if options & 4 else 0
    return [[a, b] for a in range(lo, lo + 10) for b in range(lo, lo + 10)]


def draw(rng, options):
    nrow = int(rng.integers(5, 9))
    dom = rng.integers(-3, 4, size=(nrow, NVAR + NPARM + 2)).astype(np.int64)
    dom[:, 0] = 1
    dom[:, -1] = rng.integers(0 if options & 2 else -6, 13, size=nrow)
    return dom


def main():
    import instances_model as im
    import pipbatch as pb
    import pipsolve_model as pm
    import system_model as sy
    import tape_cases as tc
    import tape_edit_model as te
    ctx = np.zeros((0, NPARM + 2), dtype=np.int64)
    out_dir = os.path.join(HERE, "tape_edit")
    os.makedirs(out_dir, exist_ok=True)
    total_new = 0
    for name, (options, seed0) in FAMILIES.items():
        words = "+".join(w for bit, w in ((2, "Maximize"), (8, "Urs_unknowns"), (4, "Urs_parms")) if options & bit)
        words += "" if options & 1 else "+Rational"
        points = grid(options)
        for seed in range(seed0, seed0 + 400):
            rng = np.random.default_rng(seed)
            dom = draw(rng, options)
            try:
                rc, text, _ = pm.run_pip(pb.REFPIP, dom, ctx, -1, options, timeout=1)
            except subprocess.TimeoutExpired:
                continue
            if rc != 0 or len(text) > 2500 or text.strip() == "void":
                continue
            nodes = te.nodes_from_text(text, NPARM)
            traces = []
            walked = []
            for p in points:
                t = {}
                walked.append(te.evaluate(nodes, NVAR, 0, p, 64, t))
                traces.append(t)
            leaves = len(set(r[1] for r in walked))
            unsolved = sum(r[0] != te.ST_SOLUTION for r in walked)
            through_new = sum(bool(t.get("news")) for t in traces)
            unb = sum(bool(t.get("unbounded")) for t in traces)
            mixed = sum(r[0] == te.ST_SOLUTION and len(set(d == 0 for _, d in r[2])) == 2 for r in walked)
            if leaves < 4 or unsolved < 8 or through_new < WANT_NEW[name]:
                continue
            if name in WANT_UNBOUNDED and min(unb, len(points) - unb, mixed) < WANT_UNBOUNDED[name]:
                continue
            # the reference on every instance, under the same options
            answers, finished = [], True
            for system in im.expand(dom[:, 1:].tolist(), points):
                try:
                    p = subprocess.run([pb.REFPIP, "pip"], input=sy.pip_text(system, (), words), capture_output=True, timeout=5)
                except subprocess.TimeoutExpired:
                    finished = False
                    break
                if p.returncode != 0:
                    finished = False
                    break
                lists = sy.parse_lists(p.stdout.decode("latin-1"))
                assert len(lists) <= 1
                answers.append(lists[0] if lists else None)
            if not finished:
                continue
            bad = [k for k, (r, a) in enumerate(zip(walked, answers)) if not te.same_answer(te.answer_of(r), a)]
            assert not bad, (name, seed, bad[:5], [(points[k], te.answer_of(walked[k]), answers[k]) for k in bad[:3]])
            # the raw tape (the CPU restatement's), edited by the model, prints as the reference's quast
            f, d, c = pm.build(dom, ctx, -1, options)
            res = pb.run_batch(pb.ORACLEPIP, [pm.as_problem(f, d, c)]).results[0]
            assert res.status == pb.ST_OK, (name, seed, res.status)
            raw = tc.cells_from_text(res.text)
            enodes, _, stats = te.edit_nodes(raw, f["nvar"], f["nparm"], 0, pm.info_of(f), 64)
            lines = []
            pm._print(te.quast(enodes), 0, lines)
            assert pb.squash("".join(lines)) == pb.squash(text), (name, seed)
            model = [te.evaluate(enodes, NVAR, 0, p, 64) for p in points]
            assert all(te.same_answer(te.answer_of(r), a) for r, a in zip(model, answers)), (name, seed)
            agree = sum(1 for r, a in zip(model, answers) if a is not None and any(d == 0 for _, d in a)
                        and te.answer_of(r) == a)
            total_new += through_new
            doc = {"name": name, "seed": seed, "nvar": NVAR, "nparm": NPARM, "options": options, "bg": -1,
                   "inequnk": dom.tolist(), "ineqpar": ctx.tolist(), "text": text, "points": points, "answers": answers,
                   "census": {"leaves": leaves, "unsolved": unsolved, "through_new": through_new, "unbounded": unb,
                              "mixed": mixed, "dropped_nonzero": stats["dropped_nonzero"],
                              "unbounded_numerators_agree": agree}}
            print(name, "seed", seed, doc["census"])
            with open(os.path.join(out_dir, name + ".json"), "w") as fh:
                json.dump(doc, fh, separators=(",", ":"), sort_keys=True)
                fh.write("\n")
            break
        else:
            raise RuntimeError(f"family {name}: no seed gives the tests enough to hold on to")
    assert total_new >= 20, total_new


if __name__ == "__main__":
    main()
