"""The time of the batch loads from plain rows: pipamd_batch_load_shifted and pipamd_batch_load_system on the same rows.

    python tools/load_system_rate.py [--batch N] [--reps R]

Input: N (default 10,000) plain systems of 126 unknowns and 64 rows (synth.lexmin_batch, the shape of
tools/lexmax_rate.py), loaded under Maximize (shift = +1, 128 columns).  Four legs take turns in one process, R
(default 5) rounds after a warm-up round: the shifted load, the system load without equalities and without tab_simplify
(the same bytes and, since the shifted entry forwards to the system load, the same kernel: the two legs differ in the
host entry alone), the system load with tab_simplify, and the system load with 8 equalities (72 tableau rows).  The
tableau of the second leg is first held to the first one's, bit for bit in what a solve leaves.  Times are device events
round the load alone.  One JSON line: per leg the median, the smallest and the largest time in microseconds.
A manual tool, not a test."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NVAR, NI = 126, 64
EQ8 = tuple(range(3, 64, 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7190)
    a = ap.parse_args()
    import torch
    from piplib_amd import engine as eng, synth
    rows = torch.as_tensor(synth.lexmin_batch(a.seed, a.batch, NVAR, NI)).cuda()
    e = eng.Engine(0)
    legs = {"load_shifted": eng.Batch(e, rows, NVAR, 0, tflags=eng.T_INT, shift=eng.SHIFT_MAX),
            "load_system": eng.Batch(e, rows, NVAR, 0, tflags=eng.T_INT, shift=eng.SHIFT_MAX, system=True),
            "load_system_simplify": eng.Batch(e, rows, NVAR, 0, tflags=eng.T_INT, shift=eng.SHIFT_MAX, system=True, simplify=1),
            "load_system_8_equalities": eng.Batch(e, rows, NVAR, 0, tflags=eng.T_INT, shift=eng.SHIFT_MAX, system=True, eq_rows=EQ8)}
    got = []
    for name in ("load_shifted", "load_system"):
        b = legs[name]
        b.load()
        b.solve()
        b.fetch()
        torch.cuda.synchronize()
        got.append([getattr(b, n).clone() for n in ("status", "pivots", "cuts", "sol_num", "sol_den")])
    assert all(torch.equal(x, y) for x, y in zip(*got))

    def timed(b):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        b.load()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) * 1e3

    us = {name: [] for name in legs}
    for rep in range(a.reps + 1):
        for name, b in legs.items():
            t = timed(b)
            if rep:  # (round 0 warms up)
                us[name].append(t)
    out = {"shape": [NVAR, NI], "batch": a.batch, "reps": a.reps, "system_equals_shifted": True,
           "input_MB": round(rows.numel() * 8 / 1e6, 1)}
    for name, v in us.items():
        out[name + "_us"] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
