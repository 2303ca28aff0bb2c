"""Writes tests/golden/pipsolve/<family>.json: seeded pip_solve inputs (tests/pipsolve_model.py: gen_family) with what
the reference prints for them and its pivot count (oracle/_ref/refpip pip; the count includes the context test).

    python tests/golden/make_pipsolve_fixtures.py

Needs the reference build (oracle/_ref); the tests read only the JSON.  A family is taken from the first seed that
gives the tests something to hold on to: at least 6 quasts with an `if`, 4 with a `newparm`, 4 voids, 6 unbounded
(`/0`) answers under Maximize and 4 Compute_dual answers with a non-zero dual value.  Problems on which the reference
exits are never stored (gen_family draws them again), nor are Compute_dual problems whose quast forks: the dual values
the reference prints below a fork depend on uninitialised memory (pipsolve_model.defined_answer, traiter.c:565-618)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import pipbatch as pb  # noqa: E402
import pipsolve_model as pm  # noqa: E402

NEED = {"if": 6, "newparm": 4, "void": 4, "unbounded": 6, "dual": 4}


def census(fam):
    c = dict.fromkeys(NEED, 0)
    for p, text, _ in fam:
        c["if"] += "(if" in text
        c["newparm"] += "(newparm" in text
        c["void"] += text.strip() == "void"
        c["unbounded"] += bool(p["options"] & pm.MAXIMIZE) and "/0" in text
        c["dual"] += bool(p["options"] & pm.DUAL) and not (p["options"] & pm.NQ) and pm.nonzero_dual(text)
    return c


def main():
    assert pb.have_ref(), "build the reference first (make -C oracle ref)"
    os.makedirs(pm.GOLDEN, exist_ok=True)
    for name in pm.FAMILIES:
        for seed in range(1, 400):
            fam = pm.gen_family(name, seed)
            c = census(fam)
            print(name, "seed", seed, c, flush=True)
            if all(c[k] >= NEED[k] for k in NEED):
                break
        else:
            raise SystemExit(f"family {name}: no seed below 400 meets {NEED}")
        doc = {"family": name, "seed": seed, "census": c,
               "problems": [dict(p, text=text, pivots=piv) for p, text, piv in fam]}
        path = os.path.join(pm.GOLDEN, name + ".json")
        with open(path, "w") as f:
            json.dump(doc, f, separators=(",", ":"))
            f.write("\n")
        print(name, "seed", seed, c, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
