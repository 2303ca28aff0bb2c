"""The rate of pipamd_tape_sweep_values against the sweep without values and against the route it replaces.

    python tools/tape_values_rate.py [--side N] [--reps R] [--inner I] [--out FILE]

Input: the integer quast of the golden family p5 (tests/golden/tape_eval/p5_grid.json), solved once, over the box
[0, N-1]^2 (default N = 1000: 10^6 points).  Every leg is timed with device events: R (default 10) windows of I (default
20) launches each after 3 warm-up windows, the median window over I with its minimum and maximum; all legs in one session.
  (a) Tape.sweep_values_into: the fill, the sweep kernel with the value reduction, the fold
  (b) Tape.sweep_into, summary only: the same decode and walk without values -- (a) - (b) is what the reduction costs
  (c) the route (a) replaces: Tape.sweep_into with status, x_num and x_den written out, then the reduction in torch --
      (c) / (a) is what the feature buys
Before anything is timed (a)'s figures are held against (c)'s, every word.  The library is PIPAMD_LIB's where that is set
(an alternative build for an A/B, named in the line).  One JSON line (and --out).  A manual tool, not a test."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import tape_cases as tc
    from piplib_amd import engine as eng
    g = tc.golden()
    nvar, nparm = g["nvar"], g["nparm"]
    e = eng.Engine(0)
    tab = tc.parametric_tableau(g["matrix"], nvar, nparm, g["eq_rows"])
    cells, _ = eng.solve_tableau_cells(e, nvar, nparm, tab.shape[0], 0, -1, 1, tab, np.zeros((0, nparm + 1), np.int64))
    tape = eng.Tape(e, cells, nvar, nparm)
    lo, hi = [0, 0], [a.side - 1, a.side - 1]
    plan = tape.values_plan(lo, hi)
    n = plan["n_points"]

    def timed(fn):
        for _ in range(3 * a.inner):
            fn()
        ms = []
        for _ in range(a.reps):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(a.inner):
                fn()
            end.record()
            torch.cuda.synchronize()
            ms.append(start.elapsed_time(end) / a.inner)
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}

    summary = torch.empty(plan["summary_words"], dtype=torch.int64, device="cuda")
    work = torch.empty(max(1, plan["work_bytes"] // 8), dtype=torch.int64, device="cuda")
    head = torch.empty(tape.sweep_plan(lo, hi)["summary_words"], dtype=torch.int64, device="cuda")
    out3 = tape.outputs(n, ("status", "x_num", "x_den"))
    kk = torch.arange(n, dtype=torch.int64, device="cuda")[:, None]
    top, bottom = torch.iinfo(torch.int64).max, torch.iinfo(torch.int64).min

    def route():
        """sweep with the arrays written out, then the records as torch reduces them (p5's values are far from 2^63 / n:
        an int64 sum is exact here)"""
        tape.sweep_into(lo, hi, out3)
        sol = (out3["status"] == eng.ST_SOLUTION)[:, None]
        num, den = out3["x_num"], out3["x_den"]
        isint = sol & (den == 1)
        vmin = torch.where(isint, num, top).min(0).values
        vmax = torch.where(isint, num, bottom).max(0).values
        return {"n_int": isint.sum(0), "n_frac": (sol & (den > 1)).sum(0), "n_unbounded": (sol & (den == 0)).sum(0),
                "min": vmin, "k_min": torch.where(isint & (num == vmin), kk, n).min(0).values,
                "max": vmax, "k_max": torch.where(isint & (num == vmax), kk, n).min(0).values,
                "sum": torch.where(isint, num, 0).sum(0)}

    # (a) gives (c)'s figures
    tape.sweep_values_into(lo, hi, summary, work)
    got = eng.values_summary(summary, nvar)
    ref = {k: v.tolist() for k, v in route().items()}
    torch.cuda.synchronize()
    for i, rec in enumerate(got["unknowns"]):
        assert rec["n_int"] > 0 and rec == {k: ref[k][i] for k in ref}, (i, rec)
    tape.sweep_into(lo, hi, {}, summary=head)
    torch.cuda.synchronize()
    assert torch.equal(summary[:8], head[:8]), "head words differ from the sweep's"

    legs = {
        "a_sweep_values": lambda: tape.sweep_values_into(lo, hi, summary, work),
        "b_sweep_summary_only": lambda: tape.sweep_into(lo, hi, {}, summary=head),
        "c_sweep_arrays_then_torch": route,
    }
    res = {"system": "p5", "box": [lo, hi], "points": n, "nvar": nvar, "tape_info": tape.info, "plan": plan,
           "library": os.path.basename(os.environ.get("PIPAMD_LIB") or "libpipamd.so"), "reps": a.reps, "launches_per_window": a.inner,
           "values": got, "values_agree_with_the_torch_route": True, "legs": {}}
    for name, fn in legs.items():
        res["legs"][name] = timed(fn)
    m = {k: v["median_ms"] for k, v in res["legs"].items()}
    res["reduction_ms"] = round(m["a_sweep_values"] - m["b_sweep_summary_only"], 4)
    res["a_over_b"] = round(m["a_sweep_values"] / m["b_sweep_summary_only"], 3)
    res["c_over_a"] = round(m["c_sweep_arrays_then_torch"] / m["a_sweep_values"], 2)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
