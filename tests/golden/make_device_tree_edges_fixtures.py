#!/usr/bin/env python3
"""Regenerate tests/golden/device_tree_edges/*.json from the reference itself (int64 "dp" build): what oracle/_ref/refpip
answers for every member of tests/device_tree_edges.py -- status (0 answered, 1 void, 2 aborted), the abort's exit code
(26: "The solution is too complex", sol.c:97; 1: "Too much parameters", traiter.c:174), pivot count and the printed
answer without white space.  One file per family.  tests/test_device_tree_edges_model.py holds the CPU oracle to them.
Only needed when the members change; needs oracle/_ref/refpip (built where the reference's sources are)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

import device_tree_edges as dte  # noqa: E402
import pipbatch as pb  # noqa: E402


def family(name):
    return name.rstrip("0123456789_").split("_")[0].rstrip("0123456789")


def main():
    out_dir = os.path.join(HERE, "device_tree_edges")
    os.makedirs(out_dir, exist_ok=True)
    docs = {}
    for name in sorted(dte.MEMBERS):
        r = pb.run_batch(pb.REFPIP, [dte.member(name)]).results[0]
        docs.setdefault(family(name), {})[name] = {"status": r.status, "abort_code": r.abort_code, "pivots": r.pivots,
                                                   "text": pb.squash(r.text)}
    for fam, doc in docs.items():
        with open(os.path.join(out_dir, fam + ".json"), "w") as f:
            json.dump(doc, f, indent=0, sort_keys=True)
            f.write("\n")
        print(fam, sorted(doc))


if __name__ == "__main__":
    main()
