"""The families of tests/golden/replay_model.json (made by tests/golden/make_replay_fixtures.py, whose text says what the
records mean) and its readers.  TEST INFRASTRUCTURE ONLY."""
import functools
import json
import os

from piplib_amd import synth

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "replay_model.json")

# families the oracle aborts: (generator, seed, batch, nvar, ni, keywords)
SCREEN = {
    "dense-100-rows": ("dense_batch", 7201, 32, 127, 100, dict(cmax=3)),      # tests/test_gpu_lean_prep.py, ..._replay_spare_blocks.py
    "dense-64-rows": ("dense_batch", 7202, 32, 127, 64, dict(cmax=3)),        # tests/test_gpu_replay_spare_blocks.py
    "lean-paths-overflow": ("lexmin_batch", 4072, 160, 127, 64, dict(cmax=40000, x0max=3)),  # tests/test_gpu_parity.py
    # sparse rows of two entries: the entries stay small while the determinant fills its three limbs
    "sparse-100-rows": ("lexmin_batch", 7304, 32, 127, 100, dict(nnz=2, cmax=20)),
    "sparse-64-rows": ("lexmin_batch", 7305, 32, 127, 64, dict(nnz=2, cmax=300)),
}
# The families whose aborts the pivot-count checks are ABOUT: the model must admit three quarters of their aborted
# tableaux (tests/test_replay_fixture.py).  The dense families are not among them: every one of their aborts follows
# wrapped 64-bit arithmetic (entries beyond 2^31 whose products wrap a hundred pivots before the determinant would fill
# its limbs), so the model admits none of them and their counts stay the oracle's word against the engine's.
COUNTED = ("lean-paths-overflow", "sparse-100-rows", "sparse-64-rows")
HEADERS = {
    "dense10": ("dense_batch", 101, 48, 10, 10, {}),
    "dense14": ("dense_batch", 202, 24, 12, 14, {}),
    "headline": ("lexmin_batch", 7101, 64, 127, 64, {}),
}


def rows_of(spec):
    gen, seed, batch, nvar, ni, kw = spec
    return getattr(synth, gen)(seed, batch, nvar, ni, **kw)


@functools.lru_cache(maxsize=None)
def doc():
    with open(PATH) as f:
        return json.load(f)


def exact_aborts(name):
    """{tableau: pivot count} of the aborted tableaux of a SCREEN family that the model holds exact up to the abort"""
    return {int(k): v for k, v in doc()["screen"][name]["exact"].items()}


def family_of(gen, seed, batch, nvar, ni, **kw):
    """the SCREEN family with this generator call, None if there is none"""
    for name, spec in SCREEN.items():
        if spec == (gen, seed, batch, nvar, ni, kw):
            return name
    return None


def headers(name, bits):
    """per tableau of a HEADERS family None or (status, pivots, ldet, [4 limbs]) by the model at `bits` bits"""
    return [None if r is None else (r["status"], r["pivots"], r["ldet"], [int(x) for x in r["det"]])
            for r in doc()["headers"][name][str(bits)]]
