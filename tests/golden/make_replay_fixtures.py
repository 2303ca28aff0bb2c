#!/usr/bin/env python3
"""Generate tests/golden/replay_model.json: what tests/bigint_pip.py (Python ints) says of the determinant bookkeeping of
whole solves, for the GPU tests that hold pipamd_batch_solve's overflow verdicts and job headers to it.

    python tests/golden/make_replay_fixtures.py

(needs oracle/oraclepip; minutes of CPU, which is why the results are stored.  tests/test_replay_fixture.py re-derives a
sample of every family on each run of the suite.)

"screen": per family of 64-bit tableaux the CPU oracle ends in its "Integer overflow" abort, the tableaux on which the
model reaches the SAME abort with every intermediate below 2^63 -- only there is the oracle's pivot count the count of a
determinant that outgrew its limbs, and only there do the tests hold the engine to it.  On the others the oracle's
arithmetic had wrapped before (a denominator then holds a factor no limb has), and what a wrapped run does next is not
the algorithm's to define.  {"aborted": [indices], "exact": {index: pivots}}

"headers": per family and entry width, per tableau the header's determinant after the solve -- the replay of the
run's whole log (tests/replay_model.py) -- where no intermediate reached that width before the run ended, else null.
{"64": [...], "128": [...]} of {"status", "pivots", "ldet", "det": [4 decimal strings]}
"""
import concurrent.futures as cf
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import bigint_pip as bp  # noqa: E402
import pipbatch as pb  # noqa: E402
import replay_model as rm  # noqa: E402
from piplib_amd import synth  # noqa: E402

from replay_fixture import HEADERS, PATH as OUT, SCREEN, rows_of  # noqa: E402


def oracle(rows):
    nvar = rows.shape[2] - 1
    probs = [synth.Problem(nvar, 0, rows.shape[1], 0, -1, 1, rows[b], np.zeros((0, 1), np.int64)) for b in range(rows.shape[0])]
    return pb.run_batch(pb.ORACLEPIP, probs, pb.F_NOSIMPLIFY | pb.F_NOTEXT).results


def screen_one(row):
    """the model's pivot count where it reaches the 64-bit overflow with nothing wrapped before, else None"""
    r = bp.solve(row, integer=True, bits=64, stop_inexact=True)
    return r.pivots if r.status == bp.ST_OVERFLOW and r.stats.exact else None


def header_one(args):
    row, bits = args
    r = bp.solve(row, integer=True, bits=bits, stop_inexact=True)
    if r.status is None or not r.stats.exact:
        return None
    limbs, ldet, npiv, _, _ = rm.replay((1, 0, 0, 0), 1, len(r.stats.det_log), rm.ST_RUN, r.stats.det_log, bits)
    # (a pivot without a column -- the empty answer -- is counted and not logged)
    assert r.status != bp.ST_OVERFLOW or npiv == r.pivots
    return {"status": r.status, "pivots": r.pivots, "ldet": ldet, "det": [str(x) for x in limbs]}


def main():
    doc = {"made_by": "tests/golden/make_replay_fixtures.py (tests/bigint_pip.py, tests/replay_model.py: Python ints)",
           "screen": {}, "headers": {}}
    with cf.ProcessPoolExecutor(max(1, len(os.sched_getaffinity(0)))) as ex:
        for name, spec in SCREEN.items():
            rows = rows_of(spec)
            o = oracle(rows)
            ab = [k for k, r in enumerate(o) if r.status == pb.ST_ABORT and r.abort_code == 2]
            got = list(ex.map(screen_one, [rows[k] for k in ab]))
            exact = {}
            for k, p in zip(ab, got):
                if p is not None:
                    assert p == o[k].pivots, (name, k, p, o[k].pivots)  # the model and the oracle: one abort
                    exact[str(k)] = p
            doc["screen"][name] = {"family": "synth.%s(%d, %d, %d, %d%s)" % (spec[:5] + ("".join(", %s=%s" % kv for kv in spec[5].items()),)),
                                   "aborted": ab, "exact": exact}
            print("%s: %d of %d tableaux aborted, %d of them exact up to the abort (pivots %s .. %s)" % (
                name, len(ab), len(o), len(exact), min(exact.values(), default=None), max(exact.values(), default=None)), flush=True)
        for name, spec in HEADERS.items():
            rows = rows_of(spec)
            doc["headers"][name] = {}
            for bits in (64, 128):
                recs = list(ex.map(header_one, [(rows[k], bits) for k in range(rows.shape[0])]))
                doc["headers"][name][str(bits)] = recs
                print("%s at %d bits: %d of %d tableaux exact, statuses %s" % (
                    name, bits, sum(r is not None for r in recs), len(recs), sorted({r["status"] for r in recs if r})), flush=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
