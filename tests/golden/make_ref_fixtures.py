#!/usr/bin/env python3
"""Regenerate tests/golden/ref_dp/ from the reference itself (int64 "dp" build).

Runs oracle/_ref/refpip (the reference library compiled by oracle/Makefile from
/root/reference/source, driven by oracle/ref_driver.c) on the inputs of the
reference's test-suite that have no usable .ll of their own:
  * test/{boulet,bouleti,dirk}.dat  (listed as "pbs with" in test/Makefile.am:17-21;
    their .ll files were produced by another integer flavour)
  * test/challenges/*               (no .ll shipped)
  * example/*.dat                   (only the .pip variants have a .ll)
and stores stdout plus (exit code, first stderr line) in manifest.json.
`--live` writes ref_dp/live.json instead: what the reference prints for the inputs of the *_vs_ref* tests of
tests/test_oracle_golden.py (every test/*.dat, the seeded random batches, the seeded pip_solve inputs), which those
tests compare the oracle with where oracle/_ref is not built.
Only needed when the fixtures change; needs /root/reference (not on the GPU box).
"""
import json, os, subprocess, sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFPIP = os.path.join(HERE, "..", "..", "oracle", "_ref", "refpip")

# test_random_vs_ref: (seed, nvar, nparm, ni, nc, nq) of its seeded batches of 60 problems
RANDOM_CASES = [
    (1, 6, 0, 8, 0, 1), (2, 6, 0, 8, 0, 0), (3, 5, 2, 7, 2, 1), (4, 5, 2, 7, 2, 0),
    (5, 12, 0, 10, 0, 1), (6, 4, 3, 6, 3, 1), (7, 20, 0, 16, 0, 1), (8, 3, 1, 5, 1, 1),
]


def random_case(seed, nvar, nparm, ni, nc, nq):
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    from piplib_amd import synth
    return synth.random_problems(seed, 60, nvar, nparm, ni, nc, nq)


def front_end_inputs():
    """the 80 seeded pip_solve inputs of test_pip_front_end_options_vs_ref_live"""
    from datfile import matrix_text
    rng = np.random.default_rng(9)
    out = []
    for trial in range(80):
        nn, npar = int(rng.integers(1, 4)), int(rng.integers(0, 3))
        nrow, ncrow = int(rng.integers(1, 6)), int(rng.integers(0, 3))
        dom = rng.integers(-3, 4, size=(nrow, nn + npar + 2)).astype(np.int64)
        dom[:, 0] = rng.random(nrow) < 0.85
        dom[:, -1] = rng.integers(-6, 9, size=nrow)
        ctx = rng.integers(-2, 3, size=(ncrow, npar + 2)).astype(np.int64)
        if ncrow:
            ctx[:, 0] = 1
            ctx[:, -1] = rng.integers(0, 9, size=ncrow)
        opt = ["", "Maximize\n", "Urs_unknowns\n", "Urs_parms\n" if npar else "", "Rational\n"][trial % 5]
        out.append((matrix_text(ctx) + "\n-1\n\n" + matrix_text(dom) + "\n" + opt).encode())
    return out


def live():
    """ref_dp/live.json: squashed stdout per .dat; (status, squashed text, pivots) per random problem; (exit code,
    squashed stdout) per pip_solve input"""
    sys.path.insert(0, os.path.join(HERE, ".."))
    import pipbatch as pb
    doc = {"dat": {}, "random": {}, "front_end": []}
    for f in sorted(os.listdir(os.path.join(HERE, "test"))):
        if f.endswith(".dat"):
            p = subprocess.run([REFPIP, "dat", os.path.join(HERE, "test", f)], capture_output=True, timeout=60)
            doc["dat"][f[:-4]] = pb.squash(p.stdout.decode("latin-1"))
    for case in RANDOM_CASES:
        b = pb.run_batch(REFPIP, random_case(*case))
        doc["random"][",".join(map(str, case))] = [[r.status, pb.squash(r.text), r.pivots] for r in b.results]
    for txt in front_end_inputs():
        p = subprocess.run([REFPIP, "pip"], input=txt, capture_output=True, timeout=60)
        doc["front_end"].append([p.returncode, pb.squash(p.stdout.decode("latin-1"))])
    with open(os.path.join(HERE, "ref_dp", "live.json"), "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")

INPUTS = (
    [("test", n + ".dat") for n in ("boulet", "bouleti", "dirk")]
    + [("challenges", n) for n in ("pipFile_0", "system_sysmo_for_pipMP", "vivien32.dat")]
    + [("example", n + ".dat") for n in
       ("big", "cg1", "esced", "ex", "ex2", "fimmel", "max", "small", "square", "square_max", "sven")]
)

def main():
    out_dir = os.path.join(HERE, "ref_dp")
    os.makedirs(out_dir, exist_ok=True)
    manifest = {}
    for sub, name in INPUTS:
        src = os.path.join(HERE, sub, name)
        p = subprocess.run([REFPIP, "dat", src], capture_output=True, timeout=60)
        key = f"{sub}/{name}"
        out_name = key.replace("/", "__") + ".ll"
        with open(os.path.join(out_dir, out_name), "wb") as f:
            f.write(p.stdout)
        err = p.stderr.decode(errors="replace").strip().splitlines()
        manifest[key] = {"rc": p.returncode, "stderr": err[0] if err else "", "ll": out_name}
        print(key, manifest[key])
    # Compute_dual (rational solve + dual variables): non-parametric examples only -- with
    # parameters the reference reads uninitialised memory in tab_sort_rows (traiter.c:576-589
    # skips unit rows before ineq[i] is set) and crashes or prints garbage.
    for name in ("small", "square", "max", "big", "cg1", "sven"):
        src = open(os.path.join(HERE, "example", name + ".pip"), "rb").read() + b"\nRational\nDual\n"
        with open(os.path.join(out_dir, f"dual__{name}.pip"), "wb") as f:
            f.write(src)
        p = subprocess.run([REFPIP, "pip"], input=src, capture_output=True, timeout=60)
        assert p.returncode == 0, name
        with open(os.path.join(out_dir, f"dual__{name}.ll"), "wb") as f:
            f.write(p.stdout)
        print("dual", name, len(p.stdout))
    with open(os.path.join(out_dir, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)

if __name__ == "__main__":
    sys.exit(live() if "--live" in sys.argv else main())
