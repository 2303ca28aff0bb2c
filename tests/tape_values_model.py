"""A sweep's values reduced per unknown, in Python ints: what pipamd_tape_sweep_values_plan counts and what
pipamd_tape_sweep_values computes -- on top of tape_sweep_model's per-point results, the head words of the sweep's summary
and, per unknown, the record of include/piplib_amd.h (PIPAMD_VALUES_*).  Test helper only."""
import tape_model as tm
import tape_sweep_model as sm

MAX_NVAR, HEAD, REC = 64, 8, 16
PART_BYTES = 96      # a partial record in the work buffer (csrc/pip_tape.h, TAPE_VALUES_PART words)
MAX_BLOCKS = 2048    # the grid's cap (TAPE_VALUES_MAX_BLOCKS)
FIELDS = ("n_int", "n_frac", "n_unbounded", "min", "k_min", "max", "k_max", "sum")


def work_bytes(n_points, nvar):
    """a partial record per unknown and wave, two waves a workgroup, a workgroup per chunk of BLOCK points up to the cap"""
    return PART_BYTES * nvar * 2 * min(-(-n_points // tm.BLOCK), MAX_BLOCKS)


def staged(info, bits):
    """the program is copied to LDS: info says so, and it fits beside the slots (the reduction itself takes no LDS)"""
    return int(bool(info["staged"]) and info["words"] > 0 and
               tm.slot_bytes(max(info["slots"], 1), bits) + 8 * info["words"] <= tm.LDS_BYTES)


def plan(info, bits, nvar, point_cols, lo, hi):
    """what pipamd_tape_sweep_values_plan fills in, or TapeError with its code"""
    if nvar is None or nvar < 0:
        raise tm.TapeError(tm.E_INVALID, "nvar")
    p = sm.plan(info, bits, point_cols, lo, hi)   # its refusals come first
    if nvar > MAX_NVAR:
        raise tm.TapeError(tm.E_TOOLARGE, f"{nvar} unknowns")
    return {"n_points": p["n_points"], "summary_words": HEAD + REC * nvar, "work_bytes": work_bytes(p["n_points"], nvar),
            "staged": staged(info, bits)}


def empty_record():
    return {"n_int": 0, "n_frac": 0, "n_unbounded": 0, "min": 0, "k_min": -1, "max": 0, "k_max": -1, "sum": 0}


def summarise(results, nvar):
    """the summary as engine.values_summary hands it out, from per-point (status, leaf, x, dual): only SOLUTION points
    take part; a pair over 1 enters n_int, min, max and sum, over more n_frac, over 0 n_unbounded"""
    head = {"counts": {n: 0 for n, _ in sm.STATUSES}, "first": {n: -1 for n, _ in sm.STATUSES}}
    name = {v: n for n, v in sm.STATUSES}
    for k, r in enumerate(results):
        head["counts"][name[r[0]]] += 1
        if head["first"][name[r[0]]] < 0:
            head["first"][name[r[0]]] = k
    recs = [empty_record() for _ in range(nvar)]
    for k, r in enumerate(results):
        if r[0] != tm.ST_SOLUTION:
            continue
        assert len(r[2]) == nvar
        for rec, (num, den) in zip(recs, r[2]):
            if den == 0:
                rec["n_unbounded"] += 1
            elif den > 1:
                rec["n_frac"] += 1
            else:
                assert den == 1
                if rec["n_int"] == 0 or num < rec["min"]:
                    rec["min"], rec["k_min"] = num, k
                if rec["n_int"] == 0 or num > rec["max"]:
                    rec["max"], rec["k_max"] = num, k
                rec["n_int"] += 1
                rec["sum"] += num
    return {"counts": head["counts"], "first": head["first"], "unknowns": recs}


def sweep(cells, nvar, nparm, ndual, lo, hi, ctx=(), bits=64):
    """(results, summary) of an unedited tape over the box"""
    res, _ = sm.sweep(cells, nvar, nparm, ndual, lo, hi, ctx, bits)
    return res, summarise(res, nvar)


def _limbs(v, n):
    """the n little-endian int64 limbs of v in two's complement"""
    assert -(1 << (64 * n - 1)) <= v < (1 << (64 * n - 1))
    v &= (1 << (64 * n)) - 1
    out = [(v >> (64 * i)) & ((1 << 64) - 1) for i in range(n)]
    return [w - (1 << 64) if w >> 63 else w for w in out]


def words(summary):
    """the summary dict as the device lays it out: signed int64 words"""
    w = [summary["counts"][n] for n, _ in sm.STATUSES] + [summary["first"][n] for n, _ in sm.STATUSES]
    for r in summary["unknowns"]:
        w += [r["n_int"], r["n_frac"], r["n_unbounded"], 0] + _limbs(r["min"], 2) + [r["k_min"]] + _limbs(r["max"], 2) + \
             [r["k_max"]] + _limbs(r["sum"], 3) + [0, 0, 0]
    return w
