"""The determinant replay in Python ints: what pip_det_replay_kernel, pip_det_replay_lanes_kernel and the lean kernel's
spare blocks (csrc/pip_kernels.hip, det_replay_lane of csrc/pip_advance.h) leave in a job header after they have walked
the job's log of (pivot, denominator of the pivot row) pairs -- traiter.c:394-446 for the pivots the launches logged.

TEST INFRASTRUCTURE ONLY, like bigint_pip.py, whose det_update is the one place the walk over the limbs is stated.

A header's determinant is four limbs and `ldet`, the count of those in use; the limbs beyond `ldet` are not part of the
number and stay whatever they are.  `bits` is the width of the engine's entries (64 or 128).
"""
import math

import bigint_pip as bp

ST_RUN, ST_SOLUTION, ST_NIL, ST_CAPACITY, ST_OVERFLOW = 0, 1, 2, 3, 5  # PIPAMD_ST_* of include/piplib_amd.h
DETLOG = 512  # PIPAMD_DETLOG of csrc/pip_job.h: the pairs a job's log holds
AUX_NOCOLUMN = -1  # PIPAMD_AUX_NOCOLUMN: the header's aux of a job that ended ST_NIL in a pivot without a column


def det_model(limbs, ldet, ppivot, dppiv, W):
    """det_step's outputs by bigint_pip.det_update: the limbs in use walk, the others stay as they are.
    -> (limb0, limb1, limb2, limb3, ldet, ok)"""
    det = list(limbs[:ldet])
    ok = 1
    try:
        bp.det_update(det, ppivot, dppiv, W)
    except bp.Overflow:
        ok = 0
        if len(det) == ldet:
            # det_update raises before it appends; det_step has counted the fourth limb by then (ldet++ before its test)
            d = dppiv
            for x in limbs[:ldet]:
                d //= math.gcd(x, d)
            if d == 1:
                det = det + [None]
    n = len(det)
    out = [det[i] if i < n and det[i] is not None else limbs[i] for i in range(4)]
    return tuple(out) + (n, ok)


def replay(limbs, ldet, npiv, status, log, bits, aux=0):
    """-> (limbs, ldet, npiv, status, nlog = 0) after the replay of `log`, a list of (pivot, dpiv) with both >= 1, on a
    header that holds `limbs` (four), `ldet`, the pivot count `npiv` (every pivot of the log counted) and `status`.
    A job that went on pivoting behind an overflow its deferred replay had not found yet may have ended in a pivot
    that found no column: ST_NIL with aux = AUX_NOCOLUMN, that pivot counted in `npiv` and not logged.
    The first entry that overflows ends the walk: the limbs stay as det_step leaves them at that step, the status is
    "Integer overflow" whatever it was, and the pivot count is that of the overflowing pivot (the reference exits inside
    that call of pivoter)."""
    limbs = tuple(limbs)
    assert len(limbs) == 4
    for k, (pivot, dpiv) in enumerate(log):
        d = math.gcd(pivot, dpiv)
        *limbs, ldet, ok = det_model(limbs, ldet, pivot // d, dpiv // d, bits)
        if not ok:
            unlogged = 1 if (status, aux) == (ST_NIL, AUX_NOCOLUMN) else 0
            return tuple(limbs), ldet, npiv - unlogged - len(log) + k + 1, ST_OVERFLOW, 0
    return tuple(limbs), ldet, npiv, status, 0


def first_overflow(limbs, ldet, log, bits):
    """index of the first entry of `log` that overflows, None if none does; and why: "factor" (dppiv keeps a factor no
    limb holds) or "limb" (a fourth limb)"""
    limbs = tuple(limbs)
    for k, (pivot, dpiv) in enumerate(log):
        d = math.gcd(pivot, dpiv)
        before = ldet
        *limbs, ldet, ok = det_model(limbs, ldet, pivot // d, dpiv // d, bits)
        if not ok:
            return k, ("limb" if ldet == before + 1 else "factor")
    return None, None


def header_after_solve(log, bits):
    """(limbs in use, ldet) of a job header once every launch's log has been replayed, for a tableau whose whole run
    logged `log` (bigint_pip's Stats.det_log): a fresh header holds the one limb 1 (pip_batch_load kernels)"""
    limbs, ldet, _, _, _ = replay((1, 0, 0, 0), 1, len(log), ST_RUN, log, bits)
    return list(limbs[:min(ldet, 4)]), ldet
