#!/usr/bin/env python3
"""Regenerate tests/golden/matrices/r5.json from the reference itself: what pip_solve prints for the systems of the
ragged family r5 of tests/matrices_cases.py -- every system with its own rows and its own equalities (marker column 0)
-- under the options "", Maximize, Urs_unknowns, each integer and as Rational + Dual, with and without the box x_j <= 12.

Follows make_system_fixtures.py: runs oracle/_ref/refpip pip on system_model.pip_text(kept rows, equalities, options)
per system and stores, per case and system, the printed unknowns as [numerator, denominator] pairs (null where no list
is printed), the printed dual pairs (null without Dual or without a list) and the pivot count the driver reports; the
inputs are stored as the family's seeds, shape and classes (the rows are matrices_cases.family's).  The family is rejected
here unless the reference alone gives the tests enough to hold on to: per case at least 6 solved systems; at least 6
unbounded answers under Maximize without the box; with Dual at least 6 systems with a non-zero dual and at least 6 with a
negative dual value on an equality; every class dealt at least 3 times.  (The seed of the class permutation in
matrices_cases.FAMILIES was changed until they held.)  Only needed when the fixtures change; needs the reference build.
"""
import json, os, re, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
REFPIP = os.path.join(HERE, "..", "..", "oracle", "_ref", "refpip")
NAME = "r5"


def collect(perm_seed=None, verbose=True):
    """the fixture document of r5 with the class permutation of `perm_seed` (None: the family's own); raises
    AssertionError if the family does not meet the conditions above"""
    import matrices_cases as mc
    import system_model as sy
    from shift_cases import BOX
    seed, nvar, n, batch, kw, _, pseed, boxes = mc.FAMILIES[NAME]
    pseed = pseed if perm_seed is None else perm_seed
    doc = {"seed": seed, "nvar": nvar, "n": n, "batch": batch, "kw": kw, "box": BOX, "perm_seed": pseed, "classes": {},
           "cls": {}, "cases": {}}
    for box in boxes:
        fam = mc.family(NAME, box, pseed)
        doc["classes"][str(box)] = [[list(kept), list(eq)] for kept, eq in fam.classes]
        doc["cls"][str(box)] = fam.cls.tolist()
        dealt = [len(mc.members(fam, c)) for c in range(len(fam.classes))]
        if verbose:
            print(NAME, "box", box, "classes dealt", dealt, "room ni", fam.ni)
        assert min(dealt) >= 3
        for opts, (shift, nq, dual) in sy.OPTIONS.items():
            xs, duals, pivots = [], [], []
            for k, (rows, eq) in enumerate(fam.systems):
                p = subprocess.run([REFPIP, "pip"], input=sy.pip_text(rows, eq, opts), capture_output=True, timeout=60)
                assert p.returncode == 0, (NAME, box, opts, k, p.stderr[:200])
                lists = sy.parse_lists(p.stdout.decode("latin-1"))
                assert len(lists) == (2 if dual else 1) * bool(lists), (NAME, box, opts, k, len(lists))
                xs.append(lists[0] if lists else None)
                duals.append(lists[1] if dual and lists else None)
                pivots.append(int(re.search(rb"pivots (\d+)", p.stderr).group(1)))
            doc["cases"][f"box{box},{opts}"] = {"x": xs, "dual": duals, "pivots": pivots}
            solved = [x for x in xs if x is not None]
            unbounded = sum(any(d == 0 for _, d in x) for x in solved)
            if verbose:
                print(NAME, "box", box, repr(opts), "lists", len(solved), "with /0", unbounded)
            assert len(solved) >= 6
            if shift > 0 and not box:
                assert unbounded >= 6
            if dual:
                got = [(d, fam.systems[k]) for k, d in enumerate(duals) if d is not None]
                assert len(got) == len(solved) and all(len(d) == len(rows) for d, (rows, _) in got)  # one value per input row
                nonzero = sum(any(v != 0 for v, _ in d) for d, _ in got)
                negative = sum(any(d[r][0] < 0 for r in eq) for d, (_, eq) in got)
                if verbose:
                    print("   duals: non-zero in", nonzero, "systems, negative on an equality in", negative)
                assert nonzero >= 6 and negative >= 6
    return doc


def main():
    doc = collect()
    out_dir = os.path.join(HERE, "matrices")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, NAME + ".json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
