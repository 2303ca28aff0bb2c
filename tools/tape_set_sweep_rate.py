"""Many small quasts, each swept over its own parameter box under its own context: one pipamd_tape_set_sweep_run launch
against a pipamd_tape_sweep launch per tape.

    python tools/tape_set_sweep_rate.py [--problems N] [--skip K,K,...] [--out FILE]

Input: the N (default 2,000) seeded `p3` problems of tools/tape_set_rate.py, solved once by pipamd_pip_solve_many (not
timed); every answer that is not void is compiled with its pipamd_pip_info as the edit and becomes one job: the box
[-3, 9]^point_cols under the problem's own ineqpar, summary only.  --skip leaves problems out of the solve; all are drawn, so
the others are what they were (profiles/: 9,225,1470, which the CPU oracle does not finish and which give no tape).
Two timings, each the median of 10 after 3 warm-ups, by device events and by the wall clock (a synchronise behind the
last launch):
  * set:      one TapeSetSweep.run_into launch (a fill and a kernel) for all jobs;
  * single:   one Tape.sweep_into(..., summary=...) per tape -- a fill and a kernel each --, the same compiled tapes, the
              summaries and the device copies of the context rows allocated beforehand.
Before anything is timed every job's words are held against the single sweep's.  One JSON line (and --out): the times,
their ranges and the ratios.  A manual tool, not a test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--skip", default="", help="comma-separated indices of problems left out of the solve")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import pipsolve_model as pm
    from piplib_amd import engine as eng
    e = eng.Engine(0)
    rng = np.random.default_rng(a.seed)
    probs = [pm.gen_problem(rng, k, pm.FAMILIES["p3"]) for k in range(a.problems)]
    left_out = sorted({int(k) for k in a.skip.split(",") if k.strip()})
    probs = [p for k, p in enumerate(probs) if k not in left_out]  # (drawn all the same: the others stay what they were)
    inputs = [eng.PipInput(np.array(p["inequnk"], dtype=np.int64), np.array(p["ineqpar"], dtype=np.int64), p["bg"], p["options"])
              for p in probs]
    tapes, jobs, skipped = [], [], {"failed": 0, "void": 0, "refused": 0, "left_out": left_out}
    t0 = time.perf_counter()
    solved = eng.pip_solve_many(e, inputs)
    solve_s = time.perf_counter() - t0  # (reported, not part of either timing)
    for p, (cells, rc, _, _, info) in zip(probs, solved):
        if rc != 0:
            skipped["failed"] += 1
        elif info["is_void"] or not cells:
            skipped["void"] += 1
        else:
            ndual = info["ni"] if info["sol_flags"] & eng.SOL_DUAL else 0
            try:
                t = eng.Tape(e, cells, info["nvar"], info["nparm"], ndual, 64, edit=info)
            except eng.TapeError:
                skipped["refused"] += 1
                continue
            ctx = np.array(p["ineqpar"], dtype=np.int64).reshape(-1, t.point_cols + 2)
            jobs.append((len(tapes), [-3] * t.point_cols, [9] * t.point_cols, ctx if len(ctx) else None))
            tapes.append(t)
    n = len(tapes)
    tset = eng.TapeSet(e, tapes)
    sweep = tset.sweep_jobs(jobs)
    set_sum = torch.empty(sweep.words, dtype=torch.int64, device="cuda")
    own_sum = [torch.empty(8 + 2 * t.info["leaves"], dtype=torch.int64, device="cuda") for t in tapes]
    own_ctx = [None if c is None else torch.as_tensor(c).cuda() for _, _, _, c in jobs]

    def run_set():
        sweep.run_into(set_sum)

    def run_single():
        for t, (_, lo, hi, _), c, s in zip(tapes, jobs, own_ctx, own_sum):
            t.sweep_into(lo, hi, {}, ctx=c, summary=s)

    # both routes give the same words
    run_set(), run_single()
    torch.cuda.synchronize()
    for j, s in enumerate(own_sum):
        assert torch.equal(set_sum[sweep.summary_off[j]:sweep.summary_off[j + 1]], s), j
    census = sweep.summaries(set_sum)

    def timed(fn):
        dev, wall = [], []
        for rep in range(13):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            start.record()
            fn()
            end.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if rep >= 3:
                dev.append(start.elapsed_time(end))
                wall.append((t1 - t0) * 1e3)
        return {"device_ms": statistics.median(dev), "device_ms_range": [min(dev), max(dev)],
                "wall_ms": statistics.median(wall), "wall_ms_range": [min(wall), max(wall)]}

    plan = eng.set_sweep_plan(jobs, sweep.leaves, [t.point_cols for t in tapes])
    res = {"problems": a.problems, "tapes": n, "jobs": n, "skipped": skipped, "solve_s": solve_s, "set": tset.info,
           "points": sum(plan["points"]), "chunks": plan["chunk_off"][-1], "summary_words": sweep.words,
           "context_rows": sum(0 if c is None else len(c) for _, _, _, c in jobs),
           "counts": {k: sum(s["counts"][k] for s in census) for k in ("solution", "nil", "range", "outside")},
           "one_set_launch": timed(run_set), "launch_per_tape": timed(run_single)}
    for clock in ("device_ms", "wall_ms"):
        res["ratio_per_tape_over_set_" + clock] = res["launch_per_tape"][clock] / res["one_set_launch"][clock]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
