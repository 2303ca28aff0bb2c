"""The load of N instances of one parametric system against the dense load of their expansion by the PARENT commit's library.

    python tools/load_instances_ab.py --parent-lib PATH/libpipamd.so [--batch N] [--rounds R] [--loads K]

Shape: N (default 10,000) systems of 64 rows and 127 unknowns with 4 parameters, int64 entries, shift 0, no tab_simplify:
the headline shape.  The shared matrix is one system of synth.lexmin_batch with four parameter columns put in, the points
are random in [0, 100).  Two legs take turns, R (default 5) rounds, each leg of each round in a process of its own (a
process loads one library):
  dense      pipamd_batch_load_system of the PARENT's library (--parent-lib: a build of the parent commit, which has no
             instances entry) on the dense expansion, batch x 64 x 128 int64, resident on the device;
  instances  pipamd_batch_load_instances of this tree's library on the 64 x 132 matrix and the batch x 4 points; before it
             is timed, its workspace is held to this library's dense load of the expansion, bit for bit.
A leg warms up with 3 loads and then times K (default 100) loads back to back between two device events; its figure is
the time per load.  One JSON line: per leg the per-round times in microseconds with median, smallest and largest, the
input bytes each load reads, the bytes both write, the parent's largest run-to-run difference and the difference of the
medians.  A manual tool, not a test ("instances of one parametric system")."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NVAR, NROWS, NPARM = 127, 64, 4


def family(seed, batch):
    """(matrix (NROWS, NVAR + NPARM + 1), points (batch, NPARM)) as int64 arrays"""
    import numpy as np
    from piplib_amd import synth
    rng = np.random.default_rng(seed)
    plain = synth.lexmin_batch(seed, 1, NVAR, NROWS)[0]
    assert plain.shape == (NROWS, NVAR + 1)
    parms = rng.integers(-3, 4, (NROWS, NPARM))
    matrix = np.concatenate([plain[:, :NVAR], parms, plain[:, NVAR:]], axis=1).astype(np.int64)
    return matrix, rng.integers(0, 100, (batch, NPARM)).astype(np.int64)


def expand_on_device(matrix, points):
    """the dense systems (batch, NROWS, NVAR + 1) on the device (the values are small: nothing leaves int64)"""
    import torch
    m, p = torch.as_tensor(matrix).cuda(), torch.as_tensor(points).cuda()
    rows = torch.empty((p.shape[0], NROWS, NVAR + 1), dtype=torch.int64, device=m.device)
    rows[:, :, :NVAR] = m[None, :, :NVAR]
    rows[:, :, NVAR] = m[None, :, -1] + (m[None, :, NVAR:NVAR + NPARM] * p[:, None, :]).sum(-1)
    return rows


def leg(a):
    import torch
    from piplib_amd import engine as eng
    matrix, points = family(a.seed, a.batch)
    e = eng.Engine(0)
    rows = expand_on_device(matrix, points)
    if a.leg == "dense":
        b = eng.Batch(e, rows, NVAR, 0, tflags=eng.T_INT, system=True)
    else:
        b = eng.Batch(e, (matrix, points), NVAR, 0, tflags=eng.T_INT, instances=True)
        d = eng.Batch(e, rows, NVAR, 0, tflags=eng.T_INT, system=True)
        b.ws.zero_()
        d.ws.zero_()
        b.load()
        d.load()
        torch.cuda.synchronize()
        assert torch.equal(b.ws, d.ws), "the instances load and the dense load of the expansion differ"
        del d, rows
    for _ in range(3):
        b.load()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(a.loads):
        b.load()
    end.record()
    torch.cuda.synchronize()
    print(json.dumps({"leg": a.leg, "lib": eng.LIB_PATH, "us_per_load": start.elapsed_time(end) * 1e3 / a.loads}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "piplib_amd", "libpipamd_parent.so"))
    ap.add_argument("--batch", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loads", type=int, default=100)
    ap.add_argument("--seed", type=int, default=7191)
    ap.add_argument("--leg", choices=["dense", "instances"])
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    if not os.path.exists(a.parent_lib):
        sys.exit(f"{a.parent_lib} missing: build the parent commit's library and name it with --parent-lib")
    us = {"dense": [], "instances": []}
    for _ in range(a.rounds):
        for name in us:
            env = dict(os.environ)
            if name == "dense":
                env["PIPAMD_LIB"] = os.path.abspath(a.parent_lib)
            else:
                env.pop("PIPAMD_LIB", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--batch", str(a.batch), "--loads",
                                str(a.loads), "--seed", str(a.seed)], env=env, capture_output=True, timeout=600)
            if p.returncode != 0:  # (nothing more is started on the device after a leg that failed)
                sys.exit(f"leg {name} failed with status {p.returncode}:\n{p.stderr.decode()[-2000:]}")
            us[name].append(json.loads(p.stdout.decode().strip().splitlines()[-1])["us_per_load"])
    out = {"shape": [NVAR, NROWS, NPARM], "batch": a.batch, "rounds": a.rounds, "loads_per_round": a.loads,
           "dense_input_bytes": a.batch * NROWS * (NVAR + 1) * 8,
           "instances_input_bytes": NROWS * (NVAR + NPARM + 1) * 8 + a.batch * NPARM * 8,
           "tableau_bytes_written": a.batch * NROWS * (NVAR + 1) * 8}
    for name, v in us.items():
        out[name + "_us"] = {"rounds": [round(t, 1) for t in v], "median": round(statistics.median(v), 1), "min": round(min(v), 1),
                             "max": round(max(v), 1)}
    out["parent_largest_difference_us"] = round(max(us["dense"]) - min(us["dense"]), 1)
    out["instances_minus_dense_median_us"] = round(statistics.median(us["instances"]) - statistics.median(us["dense"]), 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
