"""From pinned host memory to a loaded workspace: dense rows through pipamd_batch_load against sparse rows (CSR) through
pipamd_batch_load_sparse.

    python tools/sparse_load_rate.py [--shape headline|cfg4|both] [--reps R] [--no-solve]

Shapes: the headline batch (10,000 systems of 64 rows and 127 unknowns, synth.lexmin_batch, 64-bit entries) and BASELINE
configs[4]'s (1,000 systems of 128 rows and 255 unknowns, 16 non-zeros a row, 128-bit entries).  Six legs take turns in
one process, R (default 10) rounds after a warm-up round, each timed with device events on the stream it runs on:
  dense_total   hipMemcpyAsync of the dense rows from pinned memory, then pipamd_batch_load
  sparse_total  the three CSR copies from pinned memory, then pipamd_batch_load_sparse
  dense_copy / sparse_copy   the copies alone (the host-link rate is the dense copy's bytes over its time)
  dense_load / sparse_load   the load kernels alone, rows resident
The sparse batch is first held to the dense one: the zeroed workspaces after either load hold the same bytes behind the
job headers (tableaux, row tables, spare slots).  Then one solve of the dense-loaded batch is timed, for scale, and on the
headline shape one of the sparse-loaded batch, whose results must be the same.  One JSON line per shape: bytes each way,
per leg the median, the smallest and the largest time in microseconds, the link rate, the solve time.  A manual tool, not
a test."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SHAPES = {"headline": dict(batch=10000, nvar=127, ni=64, bits=64, gen={}, seed=1000, max_rows=64 + 1024, solve_both=True),
          "cfg4": dict(batch=1000, nvar=255, ni=128, bits=128, gen=dict(nnz=16, cmax=30), seed=4000, max_rows=128 + 1280,
                      solve_both=False)}


def measure(name, cfg, reps, solve):
    import torch
    import sparse_cases as sp
    from piplib_amd import engine as eng, synth
    rows = synth.lexmin_batch(cfg["seed"], cfg["batch"], cfg["nvar"], cfg["ni"], **cfg["gen"])
    host_dense = torch.as_tensor(rows).pin_memory()
    host_csr = [torch.as_tensor(a).pin_memory() for a in sp.to_csr(rows)]
    dev_dense = torch.empty(host_dense.shape, dtype=host_dense.dtype, device="cuda:0")
    dev_csr = [torch.empty(a.shape, dtype=a.dtype, device="cuda:0") for a in host_csr]
    e = eng.Engine(0)
    e.set_max_rows(cfg["max_rows"])
    bd = eng.Batch(e, dev_dense, cfg["nvar"], 0, tflags=eng.T_INT, entier_bits=cfg["bits"])
    bs = eng.Batch(e, dev_csr, cfg["nvar"], 0, tflags=eng.T_INT, entier_bits=cfg["bits"], shape=rows.shape, sparse=True)
    assert bd.rows.data_ptr() == dev_dense.data_ptr() and all(x.data_ptr() == y.data_ptr() for x, y in zip(bs.csr, dev_csr))

    def dense_copy():
        dev_dense.copy_(host_dense, non_blocking=True)

    def sparse_copy():
        for d, h in zip(dev_csr, host_csr):
            d.copy_(h, non_blocking=True)

    legs = {"dense_total": lambda: (dense_copy(), bd.load()), "sparse_total": lambda: (sparse_copy(), bs.load_sparse()),
            "dense_copy": dense_copy, "sparse_copy": sparse_copy, "dense_load": bd.load, "sparse_load": bs.load_sparse}

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) * 1e3

    # the two loads build the same workspace (the tableaux, tables and spare slots: everything behind the job headers)
    for b, go in ((bd, legs["dense_total"]), (bs, legs["sparse_total"])):
        b.ws.zero_()
        go()
        torch.cuda.synchronize()
    jobs = (cfg["batch"] * 200 + 255) // 256 * 32  # int64 words of the job headers
    same = bool(torch.equal(bd.ws[jobs:], bs.ws[jobs:]))
    us = {k: [] for k in legs}
    for rep in range(reps + 1):
        for k, fn in legs.items():
            t = timed(fn)
            if rep:  # (round 0 warms up)
                us[k].append(t)
    dense_bytes = host_dense.numel() * 8
    sparse_bytes = sum(a.numel() * a.element_size() for a in host_csr)
    out = {"shape": name, "batch": cfg["batch"], "rows": cfg["ni"], "nvar": cfg["nvar"], "entier_bits": cfg["bits"], "reps": reps,
           "nnz": int(host_csr[1].numel()), "dense_bytes": dense_bytes, "sparse_bytes": sparse_bytes,
           "bytes_ratio": round(dense_bytes / sparse_bytes, 2), "workspaces_equal_behind_headers": same}
    for k, v in us.items():
        out[k + "_us"] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
    out["dense_link_GB_s"] = round(dense_bytes / statistics.median(us["dense_copy"]) / 1e3, 2)
    out["sparse_link_GB_s"] = round(sparse_bytes / statistics.median(us["sparse_copy"]) / 1e3, 2)
    out["total_ratio"] = round(statistics.median(us["dense_total"]) / statistics.median(us["sparse_total"]), 2)
    if solve:
        res = []
        for b, go in ((bd, bd.load), (bs, bs.load_sparse))[:2 if cfg["solve_both"] else 1]:
            go()
            ms = timed(b.solve) / 1e3
            b.fetch()
            torch.cuda.synchronize()
            res.append((ms, [getattr(b, n).clone() for n in ("status", "pivots", "cuts", "sol_num", "sol_den")]))
        out["solve_ms"] = round(res[0][0], 3)
        out["pivots"] = int(res[0][1][1].sum().item())
        if len(res) == 2:
            out["solve_ms_sparse_loaded"] = round(res[1][0], 3)
            out["solves_equal"] = all(bool(torch.equal(x, y)) for x, y in zip(res[0][1], res[1][1]))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["headline", "cfg4", "both"], default="both")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-solve", action="store_true")
    a = ap.parse_args()
    for name in (("headline", "cfg4") if a.shape == "both" else (a.shape,)):
        measure(name, SHAPES[name], a.reps, not a.no_solve)


if __name__ == "__main__":
    main()
