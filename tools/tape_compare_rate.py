"""The rate of pipamd_tape_compare_sweep against the route that existed before it: two sweeps with per-point arrays and a
comparison in torch.

    python tools/tape_compare_rate.py [--side N] [--reps R] [--inner I] [--out FILE]

Input: the integer quast of the golden family p5 (tests/golden/tape_eval/p5_grid.json) against its rational quast, each
solved once, over the box [0, N-1]^2 (default N = 1000: 10^6 points), summary only.  Every leg is timed with device
events: R (default 10) windows of I (default 20) launches each after 3 warm-up windows, the median window over I; all
legs in one session.
  (1) compare_sweep, summary only, both tapes of 64-bit cells        (1w) the same, the integer tape 64-bit, the rational 128-bit
  (2) two sweep_into calls with status, x_num and x_den, and the classes, counts and firsts reduced from them in torch
  (2w) the same for the 64 / 128 pair                                  (1l) compare (the list form) at the materialised box
Before anything is timed the summaries of (1) and (2), and of (1w) and (2w), are held equal.  One JSON line (and --out).
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
    none = np.zeros((0, nparm + 1), np.int64)

    def solved(nq, bits):
        cells, _ = eng.solve_tableau_cells(e, nvar, nparm, tab.shape[0], 0, -1, nq, tab, none, bits=bits)
        return eng.Tape(e, cells, nvar, nparm, bits=bits)

    t_int, t_rat, t_rat128 = solved(1, 64), solved(0, 64), solved(0, 128)
    lo, hi = [0, 0], [a.side - 1, a.side - 1]
    n = t_int.compare_plan(t_rat, lo, hi)["n_points"]
    r = torch.arange(a.side, dtype=torch.int64, device="cuda")
    points = torch.stack(torch.meshgrid(r, r, indexing="ij"), dim=-1).reshape(n, 2).contiguous()
    three = ("status", "x_num", "x_den")
    index = torch.arange(n, dtype=torch.int64, device="cuda")

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

    def wide(x, bits):
        """(n, nvar) int64 or (n, nvar, 2) (low, high) -> (n, nvar, 2)"""
        return x if bits == 128 else torch.stack((x, x >> 63), dim=-1)

    def old_route(ta, tb, oa, ob):
        """the summary's ten words from two sweeps' arrays"""
        ta.sweep_into(lo, hi, oa)
        tb.sweep_into(lo, hi, ob)
        sa, sb = oa["status"], ob["status"]
        differ = ((wide(oa["x_num"], ta.bits) != wide(ob["x_num"], tb.bits)) |
                  (wide(oa["x_den"], ta.bits) != wide(ob["x_den"], tb.bits))).flatten(1).any(dim=1)
        cls = torch.where((sa == eng.ST_RANGE) | (sb == eng.ST_RANGE), eng.CMP_RANGE,
                          torch.where(sa != sb, eng.CMP_STATUS,
                                      torch.where((sa == eng.ST_SOLUTION) & differ, eng.CMP_VALUE, eng.CMP_SAME))).long()
        counts = torch.bincount(cls, minlength=5)
        first = torch.full((5,), n, dtype=torch.int64, device=cls.device).scatter_reduce_(0, cls, index, reduce="amin")
        return torch.cat((counts, torch.where(first < n, first, torch.full_like(first, -1))))

    res = {"system": "p5, the integer quast against the rational one", "box": [lo, hi], "points": n,
           "tape_info": {"int": t_int.info, "rat": t_rat.info, "rat128": t_rat128.info}, "reps": a.reps,
           "launches_per_window": a.inner, "legs": {}}
    buf = torch.empty(eng.CMP_WORDS, dtype=torch.int64, device="cuda")
    legs = {}
    for tag, tb in (("", t_rat), ("w", t_rat128)):
        oa, ob = t_int.outputs(n, three), tb.outputs(n, three)
        new, _ = t_int.compare_sweep(tb, lo, hi, outputs=())
        old = old_route(t_int, tb, oa, ob)
        torch.cuda.synchronize()
        assert torch.equal(new, old), (new.tolist(), old.tolist())
        res["summary" + ("_64_128" if tag else "_64_64")] = eng.compare_summary(new)
        res["plan" + ("_64_128" if tag else "_64_64")] = t_int.compare_plan(tb, lo, hi)
        legs["1%s_compare_sweep_summary_only" % tag] = lambda tb=tb: t_int.compare_sweep_into(tb, lo, hi, {}, summary=buf)
        legs["2%s_two_sweeps_and_torch" % tag] = lambda tb=tb, oa=oa, ob=ob: old_route(t_int, tb, oa, ob)
    lst, _ = t_int.compare(t_rat, points, outputs=())
    torch.cuda.synchronize()
    assert eng.compare_summary(lst) == res["summary_64_64"]
    legs["1l_compare_list_summary_only"] = lambda: t_int.compare_into(t_rat, points, {}, summary=buf)
    res["results_agree"] = True
    for name, fn in legs.items():
        res["legs"][name] = timed(fn)
    res["bytes_written"] = {"1": 8 * eng.CMP_WORDS, "2": 2 * n * (4 + 16 * nvar), "2w": n * (4 + 16 * nvar) + n * (4 + 32 * nvar)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
