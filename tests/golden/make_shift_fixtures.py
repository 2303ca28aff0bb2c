#!/usr/bin/env python3
"""Regenerate tests/golden/shift/*.json from the reference itself: what pip_solve prints for plain systems under
Maximize / Urs_unknowns (piplib.c:777-797, 846-858; tab_Matrix2Tableau tab.c:292-393; sol_vector_edit sol.c:435-512),
integer and Rational, with and without the box x_j <= 12 -- so that bounded and unbounded ("/0") answers both occur.

Runs oracle/_ref/refpip pip (the reference library behind oracle/ref_driver.c) and stores, per family, the inputs (seed
and shape: the rows are synth.lexmin_batch's) and, per problem, the reference's printed list as [numerator, denominator]
pairs, or null where it prints no list.  Only needed when the fixtures change; needs the reference build.
"""
import json, os, re, subprocess, sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
REFPIP = os.path.join(HERE, "..", "..", "oracle", "_ref", "refpip")

# (name, seed, nvar, ni, batch, lexmin_batch keywords)
FAMILIES = [("v5", 31, 5, 8, 40, dict(nnz=3, cmax=3, x0max=5)), ("v12", 32, 12, 10, 24, dict(nnz=3, cmax=4, x0max=6))]

def parse_list(text):
    """"(list #[ n/d] ...)" of sol_vector_edit -> [[n, d], ...] (d = 1 where none is printed); None without a list"""
    t = "".join(text.split())  # (the front end echoes its prompts and the matrices first)
    i = t.find("(list")
    if i < 0:
        return None
    return [[int(n), int(d) if d else 1] for n, d in re.findall(r"#\[(-?\d+)(?:/(-?\d+))?\]", t[i:])]


def main():
    from datfile import matrix_text
    from shift_cases import BOX, plain_rows  # (the tests build the same systems)
    out_dir = os.path.join(HERE, "shift")
    os.makedirs(out_dir, exist_ok=True)
    for name, seed, nvar, ni, batch, kw in FAMILIES:
        doc = {"seed": seed, "nvar": nvar, "ni": ni, "batch": batch, "kw": kw, "box": BOX, "cases": {}}
        for box in (0, 1):
            rows = plain_rows(seed, nvar, ni, batch, kw, box)
            for shift, opt in ((1, "Maximize\n"), (-1, "Urs_unknowns\n")):
                for nq, ropt in ((1, ""), (0, "Rational\n")):
                    lists = []
                    for k in range(batch):
                        dom = np.concatenate([np.ones((rows.shape[1], 1), np.int64), rows[k]], axis=1)
                        txt = (matrix_text(np.zeros((0, 2), np.int64)) + "\n-1\n\n" + matrix_text(dom) + "\n" + opt + ropt).encode()
                        p = subprocess.run([REFPIP, "pip"], input=txt, capture_output=True, timeout=60)
                        assert p.returncode == 0, (name, box, shift, nq, k, p.stderr[:200])
                        lists.append(parse_list(p.stdout.decode("latin-1")))
                    doc["cases"][f"box{box},shift{shift},nq{nq}"] = lists
                    print(name, box, shift, nq, "lists", sum(l is not None for l in lists), "with /0",
                          sum(any(d == 0 for _, d in l) for l in lists if l))
        with open(os.path.join(out_dir, name + ".json"), "w") as f:
            json.dump(doc, f, separators=(",", ":"), sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
