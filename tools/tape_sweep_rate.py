"""The rate of pipamd_tape_sweep against pipamd_tape_eval at the materialised box.

    python tools/tape_sweep_rate.py [--side N] [--reps R] [--inner I] [--out FILE]

Input: the integer quast of the golden family p5 (tests/golden/tape_eval/p5_grid.json), solved once, over the box
[0, N-1]^2 (default N = 1000: 10^6 points).  Every leg is timed with device events: R (default 10) windows of I (default
20) launches each after 3 warm-up windows, the median window over I; all legs in one session.
  (a) Tape.eval_into on the materialised box, all four outputs      (b) the same with status and leaf only
  (c) sweep, summary only                                           (d) sweep, summary and all four outputs
  (e) (c) under a two-row context
and, to tell what the sweep's own parts cost: (c0) sweep with nothing asked for -- point decode and the walk alone --,
(b') sweep with status and leaf and no summary, (d') sweep with all outputs and no summary.
Many leaves: a chain of k conditions over the LAST of two parameters, box [0, 743] x [0, k] -- every lane of a wave at
another leaf, the worst case of the per-leaf reduction -- at the planner's last binned k and the first unbinned one,
summary only, and each with the summary switched off.  The grid: (c) with the persistent grid capped at 2, 4 and 6 workgroups per
compute unit (pipamd_debug_tape_sweep_blocks) and at its default, the device's occupancy.
Before anything is timed the sweep's summary is held against a reduction of eval's status and leaf, and its arrays
against eval's.  One JSON line (and --out).  A manual tool, not a test."""
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
    import tape_model as tm
    import tape_sweep_model as sm
    from piplib_amd import engine as eng
    g = tc.golden()
    nvar, nparm = g["nvar"], g["nparm"]
    e = eng.Engine(0)
    tab = tc.parametric_tableau(g["matrix"], nvar, nparm, g["eq_rows"])
    cells, _ = eng.solve_tableau_cells(e, nvar, nparm, tab.shape[0], 0, -1, 1, tab, np.zeros((0, nparm + 1), np.int64))
    tape = eng.Tape(e, cells, nvar, nparm)
    lo, hi = [0, 0], [a.side - 1, a.side - 1]
    n = tape.sweep_plan(lo, hi)["n_points"]
    r = torch.arange(a.side, dtype=torch.int64, device="cuda")
    points = torch.stack(torch.meshgrid(r, r, indexing="ij"), dim=-1).reshape(n, 2).contiguous()
    ctx = torch.as_tensor([[1, 1, 1, -8], [1, -1, 2, 4]], dtype=torch.int64, device="cuda")
    four = eng.Tape.OUTPUTS[:4]

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

    def reduced(status, leaf, leaves):
        s = {"counts": {}, "first": {}}
        for name, st in eng.SWEEP_STATUS:
            at = torch.nonzero(status == st).flatten()
            s["counts"][name], s["first"][name] = int(at.numel()), int(at[0]) if at.numel() else -1
        s["leaf_count"] = torch.bincount(leaf[leaf >= 0].long(), minlength=leaves).tolist()
        big = torch.full((leaves,), n, dtype=torch.int64, device=leaf.device)
        k = torch.arange(n, device=leaf.device)[leaf >= 0]
        big.scatter_reduce_(0, leaf[leaf >= 0].long(), k, reduce="amin")
        s["leaf_first"] = [int(v) if v < n else -1 for v in big.tolist()]
        return s

    # the sweep gives eval's numbers
    ev = tape.eval_into(points, tape.outputs(n, four))
    summary, sw = tape.sweep(lo, hi, outputs=four)
    torch.cuda.synchronize()
    for k in four:
        assert torch.equal(ev[k], sw[k]), k
    L = tape.info["leaves"]
    assert eng.sweep_summary(summary, L) == reduced(ev["status"], ev["leaf"], L), "summary differs from eval's reduction"
    inside = (((points[:, None, :] * ctx[None, :, 1:3]).sum(-1) + ctx[:, 3]) >= 0).all(dim=1)
    summary_e, sw_e = tape.sweep(lo, hi, ctx=ctx, outputs=four)
    torch.cuda.synchronize()
    st_e = torch.where(inside, ev["status"], torch.full_like(ev["status"], eng.ST_OUTSIDE))
    leaf_e = torch.where(inside, ev["leaf"], torch.full_like(ev["leaf"], -1))
    assert torch.equal(sw_e["status"], st_e) and torch.equal(sw_e["leaf"], leaf_e)
    assert eng.sweep_summary(summary_e, L) == reduced(st_e, leaf_e, L), "summary under the context differs"

    out4, out2 = tape.outputs(n, four), tape.outputs(n, four[:2])
    buf = torch.empty(8 + 2 * L, dtype=torch.int64, device="cuda")
    legs = {
        "a_eval_all_outputs": lambda: tape.eval_into(points, out4),
        "b_eval_status_leaf": lambda: tape.eval_into(points, out2),
        "c_sweep_summary_only": lambda: tape.sweep_into(lo, hi, {}, summary=buf),
        "d_sweep_summary_all_outputs": lambda: tape.sweep_into(lo, hi, out4, summary=buf),
        "e_sweep_summary_only_two_row_context": lambda: tape.sweep_into(lo, hi, {}, ctx=ctx, summary=buf),
        "c0_sweep_nothing_asked": lambda: tape.sweep_into(lo, hi, {}),
        "b1_sweep_status_leaf_no_summary": lambda: tape.sweep_into(lo, hi, out2),
        "d1_sweep_all_outputs_no_summary": lambda: tape.sweep_into(lo, hi, out4),
    }
    res = {"system": "p5", "box": [lo, hi], "points": n, "tape_info": tape.info, "plan": tape.sweep_plan(lo, hi),
           "reps": a.reps, "launches_per_window": a.inner, "summary": eng.sweep_summary(summary, L),
           "inside_under_context": int(inside.sum()), "sweep_agrees_with_eval": True, "legs": {}}
    for name, fn in legs.items():
        res["legs"][name] = timed(fn)
    res["bytes"] = {"a": n * (8 * nparm + 8 + 16 * nvar), "b": n * (8 * nparm + 8), "c": 8 * (8 + 2 * L),
                    "d": n * (8 + 16 * nvar) + 8 * (8 + 2 * L)}

    # the grid's bound: the summary-only sweep through at most 2, 4 and 6 workgroups per compute unit, and the default
    import ctypes
    knob = eng.lib().pipamd_debug_tape_sweep_blocks
    knob.argtypes = [ctypes.c_int]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res["compute_units"] = cus
    res["grid"] = {}
    for per_cu in (2, 4, 6, 0):
        knob(cus * per_cu)
        res["grid"]["default" if per_cu == 0 else "%d_per_cu" % per_cu] = timed(legs["c_sweep_summary_only"])
    knob(0)

    # many leaves: a chain over the last of two parameters, so that consecutive k are consecutive leaves
    def chain(k):
        cells = []
        for i in range(k):
            cells += [(tm.IF, 0, 0)] + tc.form([0, -1, i]) + tc.nil()
        return cells + tc.leaf([([0, 1, 0], 1)])

    kb = next(k for k in range(1100, 1200) if sm.binned(tm.check(chain(k), 1, 2), 64) and not sm.binned(tm.check(chain(k + 1), 1, 2), 64))
    res["many_leaves"] = {}
    for k in (kb, kb + 1):
        t = eng.Tape(e, chain(k), 1, 2)
        clo, chi = [0, 0], [743, k]
        plan = t.sweep_plan(clo, chi)
        s, o = t.sweep(clo, chi, outputs=("status", "leaf"))
        torch.cuda.synchronize()
        got = eng.sweep_summary(s, k + 1)
        assert got["leaf_count"] == [744] * (k + 1) and got["leaf_first"] == list(range(k + 1)), "chain summary"
        cbuf = torch.empty(8 + 2 * (k + 1), dtype=torch.int64, device="cuda")
        res["many_leaves"]["binned" if plan["binned"] else "unbinned"] = {
            "conditions": k, "tape_info": t.info, "plan": plan,
            "summary_only": timed(lambda: t.sweep_into(clo, chi, {}, summary=cbuf)),
            "nothing_asked": timed(lambda: t.sweep_into(clo, chi, {}))}
        t.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
