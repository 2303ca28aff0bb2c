#!/usr/bin/env python3
"""Regenerate tests/golden/system/*.json from the reference itself: what pip_solve prints for plain systems WITH
equalities (marker column 0) under the options "", Maximize, Urs_unknowns, each integer and as Rational + Dual, with and
without the box x_j <= 12 (piplib.c:722-880; tab_Matrix2Tableau tab.c:292-393; tab_simplify tab.c:396-427;
sol_vector_edit sol.c:435-512; pip_quast_equalities_dual piplib.c:651-690).

Runs oracle/_ref/refpip pip (the reference library behind oracle/ref_driver.c) and stores, per family, the inputs (seed
and shape: the rows are shift_cases.plain_rows', the equality rows system_model.EQ_ROWS') and, per case and system, the
printed unknowns as [numerator, denominator] pairs (null where no list is printed), the printed dual pairs (null without
Dual or without a list) and the pivot count the driver reports.  A family that does not give the tests enough to hold on
to -- solved systems, unbounded answers, non-zero and negative duals, rows tab_simplify changes -- is rejected here.
Only needed when the fixtures change; needs the reference build.
"""
import json, os, re, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
REFPIP = os.path.join(HERE, "..", "..", "oracle", "_ref", "refpip")

# (name, seed, nvar, ni, batch, lexmin_batch keywords)
FAMILIES = [("s5", 41, 5, 8, 40, dict(nnz=3, cmax=3, x0max=5)), ("s12", 42, 12, 10, 24, dict(nnz=3, cmax=4, x0max=6))]


def main():
    import system_model as sy
    from shift_cases import BOX, plain_rows  # (the tests build the same systems)
    out_dir = os.path.join(HERE, "system")
    os.makedirs(out_dir, exist_ok=True)
    for name, seed, nvar, ni, batch, kw in FAMILIES:
        eq = sy.EQ_ROWS[name]
        doc = {"seed": seed, "nvar": nvar, "ni": ni, "batch": batch, "kw": kw, "box": BOX, "eq_rows": list(eq), "cases": {}}
        for box in (0, 1):
            rows = plain_rows(seed, nvar, ni, batch, kw, box)
            nrows = rows.shape[1]
            for opts, (shift, nq, dual) in sy.OPTIONS.items():
                xs, duals, pivots = [], [], []
                for k in range(batch):
                    p = subprocess.run([REFPIP, "pip"], input=sy.pip_text(rows[k], eq, opts), capture_output=True, timeout=60)
                    assert p.returncode == 0, (name, box, opts, k, p.stderr[:200])
                    lists = sy.parse_lists(p.stdout.decode("latin-1"))
                    assert len(lists) == (2 if dual else 1) * bool(lists), (name, box, opts, k, len(lists))
                    xs.append(lists[0] if lists else None)
                    duals.append(lists[1] if dual and lists else None)
                    pivots.append(int(re.search(rb"pivots (\d+)", p.stderr).group(1)))
                doc["cases"][f"box{box},{opts}"] = {"x": xs, "dual": duals, "pivots": pivots}
                solved = [x for x in xs if x is not None]
                unbounded = sum(any(d == 0 for _, d in x) for x in solved)
                print(name, "box", box, repr(opts), "lists", len(solved), "with /0", unbounded)
                assert len(solved) >= 6
                if shift > 0 and not box:
                    assert unbounded >= 6
                if dual:
                    got = [d for d in duals if d is not None]
                    assert len(got) == len(solved) and all(len(d) == nrows for d in got)  # one value per input row
                    assert sum(any(n != 0 for n, _ in d) for d in got) >= 6
                    negative = sum(any(d[r][0] < 0 for r in eq) for d in got)
                    print("   duals: negative on an equality in", negative, "systems")
                    if name == "s5":
                        assert negative >= 16
            # what tab_simplify has to do on the box-1 systems (shift 0)
            if box:
                changed = floors = 0
                for r in rows.tolist():
                    for t in sy.tableau(r, eq, 0, 0):
                        g = sy.row_gcd(t, nvar)
                        changed += g > 1
                        floors += g > 1 and t[nvar] % g != 0
                print(name, "tab_simplify changes", changed, "rows, the floor matters in", floors)
                assert changed >= 57 and floors >= 27
        with open(os.path.join(out_dir, name + ".json"), "w") as f:
            json.dump(doc, f, separators=(",", ":"), sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
