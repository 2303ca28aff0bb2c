"""The rate of pipamd_tape_eval against the route to the same numbers that solves every point from scratch.

    python tools/tape_eval_rate.py [--points N] [--reps R] [--out FILE]

Input: the parametric system of tests/golden/instances/p5.json (5 unknowns, 2 parameters, 7 rows of which two are
equalities), integer, at N (default 1,000,000) seeded random points of 0..99 x 0..99.
  * quast leg: the problem is solved once (pipamd_solve_tableau, not timed, its pivots reported); Tape.eval of the N
    points, R (default 200) launches between two device events after 3 warm-up launches: the time per launch.
  * instances leg: Batch(instances=True) of the N points with tab_simplify -- load_instances + solve + results, each a
    whole pass between two device events with a synchronise behind it, R' = 3 passes after a warm-up pass; the median.
Before anything is timed the two legs are held against each other: every status, and the reduced values of the first
10,000 points.  One JSON line (and --out): both times, their ratio, the points' memory traffic of the quast leg -- 8 bytes
per parameter in, 8 bytes of status and leaf and 16 bytes per unknown out -- and that traffic over the launch time.
A manual tool, not a test."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--seed", type=int, default=505)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import instances_model as im
    import system_model as sy
    import tape_cases as tc
    from piplib_amd import engine as eng
    g = im.golden()
    nvar, nparm, eq = g["nvar"], g["nparm"], g["eq_rows"]
    e = eng.Engine(0)
    tab = tc.parametric_tableau(g["matrix"], nvar, nparm, eq)
    cells, pivots = eng.solve_tableau_cells(e, nvar, nparm, tab.shape[0], 0, -1, 1, tab, np.zeros((0, nparm + 1), np.int64))
    tape = eng.Tape(e, cells, nvar, nparm)
    points = torch.as_tensor(np.random.default_rng(a.seed).integers(0, 100, (a.points, nparm)), dtype=torch.int64).cuda()
    batch = eng.Batch(e, (np.array(g["matrix"], dtype=np.int64), points), nvar, 0, tflags=eng.T_INT, instances=True, eq_rows=eq,
                      simplify=1)

    def instances_pass():
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        batch.load()
        batch.solve()
        batch.fetch()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end)

    # the two routes give the same numbers
    instances_pass()  # (also the warm-up pass of the instances leg)
    st, leaf, xn, xd = tape.eval(points)
    torch.cuda.synchronize()
    assert torch.equal(st, batch.status), "statuses differ"
    k = min(a.points, 10000)
    num, den, s = batch.sol_num[:k].cpu().tolist(), batch.sol_den[:k].cpu().tolist(), st[:k].cpu().tolist()
    gx, gd = xn[:k].cpu().tolist(), xd[:k].cpu().tolist()
    for i in range(k):
        want = [sy.reduce_pair(num[i][j][0], den[i][j]) if s[i] == eng.ST_SOLUTION else (0, 0) for j in range(nvar)]
        assert list(zip(gx[i], gd[i])) == want, (i, want)
    solved = int((st == eng.ST_SOLUTION).sum())

    out = tape.outputs(a.points, eng.Tape.OUTPUTS[:4])
    for _ in range(3):
        tape.eval_into(points, out)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(a.reps):
        tape.eval_into(points, out)
    end.record()
    torch.cuda.synchronize()
    quast_ms = start.elapsed_time(end) / a.reps
    inst_ms = [instances_pass() for _ in range(3)]
    traffic = a.points * (8 * nparm + 8 + 16 * nvar)
    res = {"system": "p5", "points": a.points, "solved": solved, "quast_pivots_once": int(pivots), "tape_cells": len(cells),
           "tape_info": tape.info, "quast_eval_ms": round(quast_ms, 4), "quast_reps": a.reps,
           "instances_ms": {"median": round(statistics.median(inst_ms), 2), "min": round(min(inst_ms), 2),
                            "max": round(max(inst_ms), 2)},
           "instances_pivots": batch.counters()["pivots"],
           "ratio": round(statistics.median(inst_ms) / quast_ms, 1),
           "quast_points_per_s": round(a.points / quast_ms * 1e3),
           "quast_traffic_MB": round(traffic / 1e6, 1), "quast_traffic_GBps": round(traffic / quast_ms / 1e6, 1),
           "routes_agree": True}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
