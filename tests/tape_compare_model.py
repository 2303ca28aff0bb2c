"""Two solution tapes compared point by point, in Python ints: what pipamd_tape_compare_plan counts and what
pipamd_tape_compare / pipamd_tape_compare_sweep compute -- the class of a point, `where`, the two statuses and the
summary -- on top of tape_edit_model.evaluate_cells (each tape in its own width, with its own edit) and
tape_sweep_model (the box and the context).  A tape is a dict: cells, nvar, nparm and, optionally, ndual, edit, bits.
Test helper only."""
import tape_edit_model as te
import tape_model as tm
import tape_sweep_model as sm

SAME, STATUS, VALUE, RANGE, OUTSIDE = range(5)
CLASSES = ("same", "status", "value", "range", "outside")
WORDS = 10
DUAL = 1


def tape(cells, nvar, nparm, ndual=0, edit=None, bits=64):
    return dict(cells=cells, nvar=nvar, nparm=nparm, ndual=ndual, edit=edit, bits=bits)


def point_cols(t):
    return te.point_cols(t["nparm"], t.get("edit"))


def info(t):
    return te.check(t["cells"], t["nvar"], t["nparm"], t.get("ndual", 0), t.get("edit"), t.get("bits", 64))


def evaluate(t, points):
    """[(status, leaf, x, dual)] as pipamd_tape_eval hands them out for the tape"""
    return te.evaluate_cells(t["cells"], t["nvar"], t["nparm"], t.get("ndual", 0), points, t.get("edit"), t.get("bits", 64))


def classify(ra, rb, dual=False):
    """(class, where, sa, sb) of one point from the two evaluations there"""
    sa, sb = ra[0], rb[0]
    if sa == tm.ST_RANGE or sb == tm.ST_RANGE:
        return RANGE, -1, sa, sb
    if sa != sb:
        return STATUS, -1, sa, sb
    if sa == tm.ST_SOLUTION:
        pairs_a, pairs_b = list(ra[2]), list(rb[2])
        assert len(pairs_a) == len(pairs_b)
        if dual:
            assert len(ra[3]) == len(rb[3])
            pairs_a, pairs_b = pairs_a + list(ra[3]), pairs_b + list(rb[3])
        for i, (p, q) in enumerate(zip(pairs_a, pairs_b)):
            if tuple(p) != tuple(q):
                return VALUE, i, sa, sb
    return SAME, -1, sa, sb


def check_pair(a, b, flags=0):
    """what both entries refuse of a pair before they look at the points"""
    if flags & ~DUAL:
        raise tm.TapeError(tm.E_INVALID, "flags")
    if a["nvar"] != b["nvar"] or point_cols(a) != point_cols(b):
        raise tm.TapeError(tm.E_INVALID, "nvar or point columns differ")
    if flags & DUAL and a.get("ndual", 0) != b.get("ndual", 0):
        raise tm.TapeError(tm.E_INVALID, "ndual differs")


def compare(a, b, points, flags=0):
    """the list form: [(class, where, sa, sb)] per point; no context, never OUTSIDE"""
    check_pair(a, b, flags)
    return [classify(ra, rb, bool(flags & DUAL)) for ra, rb in zip(evaluate(a, points), evaluate(b, points))]


def compare_sweep(a, b, lo, hi, ctx=(), flags=0):
    """the sweep form over the box lo .. hi under the rows of ctx: (results, summary)"""
    check_pair(a, b, flags)
    points = sm.box_points(lo, hi)
    ins = [sm.inside(p, ctx) for p in points]
    inner = iter(compare(a, b, [p for p, i in zip(points, ins) if i], flags))
    res = [next(inner) if i else (OUTSIDE, -1, sm.ST_OUTSIDE, sm.ST_OUTSIDE) for i in ins]
    return res, summarise(res)


def summarise(results):
    """the summary as engine.compare_summary hands it out"""
    s = {"counts": {n: 0 for n in CLASSES}, "first": {n: -1 for n in CLASSES}}
    for k, r in enumerate(results):
        n = CLASSES[r[0]]
        s["counts"][n] += 1
        if s["first"][n] < 0:
            s["first"][n] = k
    return s


def words(summary):
    """the summary dict as the device lays it out"""
    return [summary["counts"][n] for n in CLASSES] + [summary["first"][n] for n in CLASSES]


# ---------------------------------------------------------------- the planner's arithmetic
def lds(info_a, bits_a, info_b, bits_b):
    """(bytes of the two slot areas, staged): the pair is served when the areas fit LDS_BYTES; both programs are staged
    when they fit beside them too"""
    slots = tm.slot_bytes(max(info_a["slots"], 1), bits_a) + tm.slot_bytes(max(info_b["slots"], 1), bits_b)
    return slots, int(slots + 8 * (info_a["words"] + info_b["words"]) <= tm.LDS_BYTES)


def plan(info_a, bits_a, info_b, bits_b, point_cols, lo, hi):
    """what pipamd_tape_compare_plan fills in, or TapeError with its code"""
    if info_a is None or info_b is None or bits_a not in (64, 128) or bits_b not in (64, 128):
        raise tm.TapeError(tm.E_INVALID, "info or bits")
    n = sm.plan(info_a, bits_a, point_cols, lo, hi)["n_points"]
    slots, staged = lds(info_a, bits_a, info_b, bits_b)
    if slots > tm.LDS_BYTES:
        raise tm.TapeError(tm.E_TOOLARGE, f"{slots} bytes of slots")
    return {"n_points": n, "staged": staged}


# ---------------------------------------------------------------- hand-made pairs the tests share
def equivalents():
    """[(name, tape a, tape b, lo, hi)]: pairs of different shape that mean the same at every point"""
    import tape_cases as tc
    one = tc.leaf([([2, 1, 3], 2), ([0, -1, 5], 3)])
    two = tc.leaf([([1, 1, 0], 1), ([1, 0, -4], 7)])
    base = tc.iff([1, -1, 2], one, tc.iff([1, 1, -7], tc.nil(), two))
    # n . theta + c >= 0 ? X : Y  is  -(n . theta + c) - 1 >= 0 ? Y : X  over the integers: ordinals 0 1 2 become 2 1 0
    swapped = tc.iff([-1, 1, -3], tc.iff([-1, -1, 6], two, tc.nil()), one)
    scaled = tc.iff([1, -1, 2], tc.leaf([([6, 3, 9], 6), ([0, -3, 15], 9)]),
                    tc.iff([1, 1, -7], tc.nil(), tc.leaf([([3, 3, 0], 3), ([3, 0, -12], 21)])))
    lo, hi = [-6, -5], [8, 7]
    return [("negated condition, items swapped", tape(base, 2, 2), tape(swapped, 2, 2), lo, hi),
            ("forms scaled by 3", tape(base, 2, 2), tape(scaled, 2, 2), lo, hi),
            ("both", tape(swapped, 2, 2), tape(scaled, 2, 2), lo, hi)]


def widths(a, b):
    """the pair in the four width pairs: [(bits_a, bits_b, a, b)]"""
    return [(wa, wb, dict(a, bits=wa), dict(b, bits=wb)) for wa in (64, 128) for wb in (64, 128)]
