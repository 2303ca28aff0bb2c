"""Wide parametric problems (65 ... 128 columns) through pipamd_solve_tableaux_lockstep with the device tree on and off,
and through the reference on one CPU core.

    python tools/wide_tree_rate.py [--count N] [--resources]

Families 402 (90 unknowns, 2 parameters, 30 inequalities, 4 context rows) and 406 (110, 1, 30, 2) of
synth.sparse_parametric_problems, screened with the CPU oracle: the problems it finishes (at most 3,000 pivots).  Times
are of the bare C call (median of three for the device tree, one run of the host schedulers), the reference's the
traiter() time of one -O3 process (oracle/_ref/refpip_fast, or the reference's counting build, or the CPU restatement).
--resources: registers and scratch of the kernel's four instantiations as the compiler reports them (no GPU needed).
One JSON line per family."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

FAMILIES = {402: ((90, 2, 30, 4), 1, dict(cmax=1, nnz=2, pmax=1)), 406: ((110, 1, 30, 2), 1, dict(cmax=2, nnz=2, pp=0.15))}


def resources():
    src = os.path.join(ROOT, "piplib_amd", "csrc", "pip_quast.hip")
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-DNDEBUG",
                        "-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True, check=True)
    out, name = {}, None
    for ln in p.stderr.splitlines():
        if "Function Name:" in ln:
            name = ln.split("Function Name:")[1].split("[")[0].strip()
            continue
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", ln)
        if m and name and "pip_quast_kernel" in name:
            out.setdefault(name, {})["vgprs" if m.group(1) == "VGPRs" else "scratch_bytes_per_lane"] = int(m.group(2))
    demangled = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True).stdout.split("\n")
    return {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: v for d, v in zip(demangled, out.values())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1000, help="screened problems per family")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        print(json.dumps({"resource_usage": resources()}), flush=True)
    import pipbatch as pb
    from piplib_amd import engine as eng, synth
    fast = pb.REFPIP + "_fast"
    ref, kind = (fast, "reference -O3") if os.access(fast, os.X_OK) else \
        ((pb.REFPIP, "reference") if pb.have_ref() else (pb.ORACLEPIP, "CPU restatement"))
    e = eng.Engine(0)
    for seed, (shape, nq, kw) in FAMILIES.items():
        keep, drawn = [], 0
        while len(keep) < a.count:  # screen in blocks of 500 problems (the seed moves on by block)
            probs = synth.sparse_parametric_problems(seed * 1000 + drawn // 500, 500, *shape, nq, **kw)
            drawn += 500
            res = pb.run_batch(pb.ORACLEPIP, probs, 0, timeout=600).results
            keep += [(p, r) for p, r in zip(probs, res) if r.status != pb.ST_ABORT and r.pivots <= 3000]
        keep = keep[:a.count]
        probs = [p for p, _ in keep]
        prep = eng.PreparedProblems(probs)
        e.set_device_tree(True)
        eng.solve_prepared(e, prep, lockstep=True)  # warm: buffers, code objects
        on = []
        for _ in range(3):
            prep = eng.PreparedProblems(probs)
            t = time.perf_counter()
            eng.solve_prepared(e, prep, lockstep=True)
            on.append(time.perf_counter() - t)
        served, back = e.last_device_tree()
        got_on = prep.results()
        e.set_device_tree(False)
        prep = eng.PreparedProblems(probs)
        t = time.perf_counter()
        eng.solve_prepared(e, prep, lockstep=True)
        off = time.perf_counter() - t
        got_off = prep.results()
        e.set_device_tree(True)
        wrong = sum(not (rc == 0 and piv == r.pivots and pb.squash(text) == pb.squash("void\n" if r.status == pb.ST_VOID else r.text))
                    for (p, r), (text, rc, st, piv) in zip(keep, got_on))
        cpu = pb.run_batch(ref, probs, pb.F_NOTEXT, timeout=1200).solve_seconds
        on_s = sorted(on)[1]
        print(json.dumps({"family": seed, "shape": shape, "nq": nq, "problems": len(probs), "pivots": sum(r.pivots for _, r in keep),
                          "device_tree_served": served, "handed_back": back, "wrong": wrong, "same_off": got_on == got_off,
                          "device_tree_on_ms": round(on_s * 1e3, 2), "device_tree_off_ms": round(off * 1e3, 2),
                          "cpu_one_core_ms": round(cpu * 1e3, 2), "cpu_kind": kind,
                          "on_vs_off": round(off / on_s, 1), "on_vs_one_core": round(cpu / on_s, 2)}), flush=True)


if __name__ == "__main__":
    main()
