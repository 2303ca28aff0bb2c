"""Many small quasts, each at a handful of points: one pipamd_tape_set_eval launch against a pipamd_tape_eval launch per
tape.

    python tools/tape_set_rate.py [--problems N] [--points K] [--skip K,K,...] [--out FILE]

Input: N (default 2,000) seeded problems of the `p3` shape of tests/pipsolve_model.py (2-3 unknowns, 1-2 parameters, 3-6
rows, all option sets), solved once by pipamd_pip_solve_many (not timed); every answer that is not void is compiled with
its pipamd_pip_info as the edit (Tape(edit=info)) and gets K (default 64) seeded random points of -3..9.
Three timings, each the median of 10 after 3 warm-ups, by device events and by the wall clock (a synchronise behind the
last launch):
  * set:      one TapeSet.eval_into launch, the points sorted by tape;
  * single:   one Tape.eval_into launch per tape, the same compiled tapes and points, outputs allocated beforehand;
  * dealt:    the same points dealt round-robin (point k of tape k mod n) through the set, so every wave serves 64 tapes.
Before anything is timed the set's answers are held against the single tapes', every point, every output.  One JSON
line (and --out): the times, their ranges and the ratios.  A manual tool, not a test."""
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
    ap.add_argument("--points", type=int, default=64)
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
    tapes, skipped = [], {"failed": 0, "void": 0, "refused": 0, "left_out": left_out}
    for cells, rc, _, _, info in eng.pip_solve_many(e, inputs):
        if rc != 0:
            skipped["failed"] += 1
        elif info["is_void"] or not cells:
            skipped["void"] += 1
        else:
            ndual = info["ni"] if info["sol_flags"] & eng.SOL_DUAL else 0
            try:
                tapes.append(eng.Tape(e, cells, info["nvar"], info["nparm"], ndual, 64, edit=info))
            except eng.TapeError:
                skipped["refused"] += 1
    n, K = len(tapes), a.points
    tset = eng.TapeSet(e, tapes)
    cols = tset.point_cols
    pts = torch.as_tensor(rng.integers(-3, 10, (n * K, max(1, cols))), dtype=torch.int64)[:, :cols].contiguous().cuda()
    sorted_idx = torch.arange(n, dtype=torch.int32).repeat_interleave(K).cuda()
    perm = torch.arange(n * K).reshape(n, K).t().reshape(-1).cuda()  # dealt position -> sorted position
    dealt_idx, dealt_pts = sorted_idx[perm].contiguous(), pts[perm].contiguous()
    own_pts = [pts[i * K:(i + 1) * K, :t.point_cols].contiguous() if t.point_cols else K for i, t in enumerate(tapes)]
    own_out = [t.outputs(K) for t in tapes]
    set_out, dealt_out = tset.outputs(n * K), tset.outputs(n * K)

    def run_set():
        tset.eval_into(sorted_idx, pts if cols else None, set_out)

    def run_single():
        for t, p, o in zip(tapes, own_pts, own_out):
            t.eval_into(p, o)

    def run_dealt():
        tset.eval_into(dealt_idx, dealt_pts if cols else None, dealt_out)

    # the three routes give the same numbers
    run_set(), run_single(), run_dealt()
    torch.cuda.synchronize()
    for name in eng.Tape.OUTPUTS:
        assert torch.equal(dealt_out[name], set_out[name][perm]), name
    for i, (t, o) in enumerate(zip(tapes, own_out)):
        rows = slice(i * K, (i + 1) * K)
        assert torch.equal(set_out["status"][rows], o["status"]) and torch.equal(set_out["leaf"][rows], o["leaf"]), i
        for nm, width in (("x_num", t.nvar), ("x_den", t.nvar), ("dual_num", t.ndual), ("dual_den", t.ndual)):
            assert torch.equal(set_out[nm][rows, :width], o[nm]) and not set_out[nm][rows, width:].any(), (i, nm)

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

    res = {"problems": a.problems, "tapes": n, "skipped": skipped, "points_per_tape": K, "points": n * K, "set": tset.info,
           "solved_points": int((set_out["status"] == eng.ST_SOLUTION).sum()),
           "one_set_launch": timed(run_set), "launch_per_tape": timed(run_single), "set_dealt_round_robin": timed(run_dealt)}
    for clock in ("device_ms", "wall_ms"):
        res["ratio_per_tape_over_set_" + clock] = res["launch_per_tape"][clock] / res["one_set_launch"][clock]
        res["ratio_dealt_over_sorted_" + clock] = res["set_dealt_round_robin"][clock] / res["one_set_launch"][clock]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
