"""The rate of a lexmax / free-sign batch with the lean launches on and off.

    python tools/lexmax_rate.py [--batch N] [--reps R] [--inflight K] [--check N] [--lone-batches]

Input: N (default 10,000) integer tableaux of 126 unknowns and 64 inequalities (synth.lexmin_batch) as Batch(shift=+1)
(Maximize) and Batch(shift=-1) (Urs_unknowns): solved under a big parameter, 128 columns.  Statuses and pivot counts of
the first --check tableaux (default: all) are held to the CPU oracle before anything is timed.  Then, in one process
and alternating, the solve with the lean launches (pip_lean_kernel's big-parameter flavour, pipamd_engine_set_lean_big)
and with pipamd_debug_lean(0)
(the launches such a batch took before: pip_advance_kernel throughout) -- one batch at a time, and K (default 8) batches
in flight on K engines and streams.  --lone-batches: the engines are told that their batches run one at a time
(pipamd_engine_set_lone_batches: no second one-wave launch behind the lean one) and only that leg is timed.  Times are device events around the solves, after a warm-up; the load is not timed.
One JSON line per family: pivots/s of both legs (median of R), their spread (min .. max) and the ratio of the medians.
A manual tool, not a test."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NVAR, NI = 126, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inflight", type=int, default=8)
    ap.add_argument("--check", type=int, default=-1, help="tableaux held to the oracle (-1: all)")
    ap.add_argument("--seed", type=int, default=7190)
    ap.add_argument("--lone-batches", action="store_true", help="pipamd_engine_set_lone_batches(1); the lone leg only")
    a = ap.parse_args()
    import numpy as np
    import torch
    import pipbatch as pb
    import shift_cases as sc
    from gpu_common import oracle_batch
    from piplib_amd import engine as eng, synth
    rows = synth.lexmin_batch(a.seed, a.batch, NVAR, NI)
    ncheck = a.batch if a.check < 0 else min(a.check, a.batch)
    for shift, fam in ((eng.SHIFT_MAX, "Maximize"), (eng.SHIFT_URS, "Urs_unknowns")):
        if a.lone_batches:
            a.inflight = 1
        engines = [eng.Engine(0) for _ in range(a.inflight)]
        for e in engines:
            e.set_lone_batches(a.lone_batches)
            e.set_lean_big(True)  # (opt-in; pipamd_debug_lean(0) below switches it off again)
        streams = [torch.cuda.Stream() for _ in range(a.inflight)]
        batches = [eng.Batch(e, rows, NVAR, 0, tflags=eng.T_INT, shift=shift) for e in engines]
        # the results, lean on and off, against the oracle (and each other)
        got = []
        for lean in (1, 0):
            engines[0].debug_lean(lean)
            b = batches[0]
            b.load()
            b.solve()
            b.fetch_shifted()
            torch.cuda.synchronize()
            got.append((b.status.cpu().numpy(), b.pivots.cpu().numpy(), b.x_num.cpu().numpy(), b.x_den.cpu().numpy()))
            launches = engines[0].last_solve_launches()
            if lean:
                launches_on = launches
        same = all((x == y).all() for x, y in zip(*got))
        res = oracle_batch(sc.shifted(rows[:ncheck], shift), NVAR, 1, 1, bigparm=NVAR + 1).results
        wrong = sum(not (r.status == pb.ST_OK and got[0][0][k] in (eng.ST_SOLUTION, eng.ST_NIL) and got[0][1][k] == r.pivots)
                    for k, r in enumerate(res))
        pivots = int(got[0][1].sum())
        assert same and wrong == 0 and (ncheck < a.batch or pivots == sum(r.pivots for r in res)), (same, wrong)

        def timed(k, lean):
            """k batches in flight, each on its own engine and stream: ms from the first solve's start to the last one's end"""
            for e in engines[:k]:
                e.debug_lean(lean)
            for b, s in zip(batches[:k], streams[:k]):
                with torch.cuda.stream(s):
                    b.load()
            torch.cuda.synchronize()
            start = torch.cuda.Event(enable_timing=True)
            ends = [torch.cuda.Event(enable_timing=True) for _ in range(k)]
            start.record(streams[0])
            for s in streams[1:k]:
                s.wait_event(start)
            for b, s in zip(batches[:k], streams[:k]):
                b.solve_async(s.cuda_stream)
            for b, s, ev in zip(batches[:k], streams[:k], ends):
                b.wait()
                ev.record(s)
            torch.cuda.synchronize()
            return max(start.elapsed_time(ev) for ev in ends)

        out = {"family": fam, "shape": [NVAR, NI], "batch": a.batch, "pivots": pivots, "checked_against_oracle": ncheck,
               "lean_on_equals_off": bool(same), "launches_lean_on": launches_on, "launches_lean_off": launches, "reps": a.reps}
        for k, label in ((1, "lone_batches_set"),) if a.lone_batches else ((1, "lone"), (a.inflight, f"inflight{a.inflight}")):
            for lean in (1, 0):  # warm-up
                timed(k, lean)
            ms = {1: [], 0: []}
            for _ in range(a.reps):
                for lean in (1, 0):
                    ms[lean].append(timed(k, lean))
            for lean, leg in ((1, "lean_on"), (0, "lean_off")):
                rate = sorted(k * pivots / (t * 1e-3) for t in ms[lean])
                out[f"{label}_{leg}_Mpivots_per_s"] = {"median": round(statistics.median(rate) / 1e6, 2), "min": round(rate[0] / 1e6, 2),
                                                       "max": round(rate[-1] / 1e6, 2)}
            out[f"{label}_on_vs_off"] = round(statistics.median(ms[0]) / statistics.median(ms[1]), 3)
        print(json.dumps(out), flush=True)
        del batches, engines


if __name__ == "__main__":
    main()
