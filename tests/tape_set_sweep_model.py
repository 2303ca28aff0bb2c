"""Every tape of a set swept over its own box, in Python ints: what pipamd_tape_set_sweep_plan counts -- points, summary
offsets, chunk offsets, refusals in the order the planner finds them -- and the per-job summary, which is
tape_sweep_model's for that job's tape, box and context.  A job is a dict: cells, nvar, nparm, ndual (the tape), lo, hi,
ctx (its box and context) and optionally bits.  Test helper only."""
import tape_model as tm
import tape_sweep_model as sm

CHUNK = 128              # consecutive k of one job a workgroup takes at a time
MAX_JOBS = 1 << 20
MAX_LEAVES = 1 << 31     # a program stays below 2^31 words, and a leaf is a word at least


def words_of(leaves):
    return 8 + 2 * leaves


def plan(jobs, leaves, point_cols):
    """jobs: [(lo, hi, n_ctx, has_ctx)] -> {"points", "summary_off", "chunk_off"}, or TapeError(code, job) with the
    first refusal: jobs are checked in order, a job's own shape before the running sum of points"""
    n = len(jobs)
    if n > MAX_JOBS:
        raise tm.TapeError(tm.E_TOOLARGE, "jobs")
    points, summary_off, chunk_off, total = [], [0], [0], 0
    for j, (lo, hi, n_ctx, has_ctx) in enumerate(jobs):
        where = f"job {j}"
        if n_ctx < 0 or (n_ctx > 0 and not has_ctx) or not 0 <= leaves[j] < MAX_LEAVES:
            raise tm.TapeError(tm.E_INVALID, where)
        try:
            p = sm.plan({"leaves": leaves[j], "slots": 1, "words": 0, "staged": 0}, 64, point_cols[j], lo, hi)["n_points"]
        except tm.TapeError as e:
            raise tm.TapeError(e.code, where)
        total += p
        if total >= sm.MAX_POINTS:
            raise tm.TapeError(tm.E_TOOLARGE, where)
        points.append(p)
        summary_off.append(summary_off[-1] + words_of(leaves[j]))
        chunk_off.append(chunk_off[-1] + -(-p // CHUNK))
    return {"points": points, "summary_off": summary_off, "chunk_off": chunk_off}


def job_summary(job):
    """(summary dict, leaves) of one job: the single sweep's"""
    bits = job.get("bits", 64)
    _, info = tm.parse(job["cells"], job["nvar"], job["nparm"], job["ndual"], bits)
    _, summary = sm.sweep(job["cells"], job["nvar"], job["nparm"], job["ndual"], job["lo"], job["hi"], job.get("ctx") or (), bits)
    return summary, info["leaves"]


def sweep(jobs):
    """(per-job summary dicts, all words as the device lays them out, summary_off)"""
    out, words, off = [], [], [0]
    for job in jobs:
        summary, leaves = job_summary(job)
        w = sm.words(summary)
        assert len(w) == words_of(leaves)
        out.append(summary)
        words += w
        off.append(len(words))
    return out, words, off


def census(answers, leaf_of, leaves):
    """a summary counted directly over recorded answers (None: no solution) and the leaf each point reached"""
    s = {"counts": {n: 0 for n, _ in sm.STATUSES}, "first": {n: -1 for n, _ in sm.STATUSES},
         "leaf_count": [0] * leaves, "leaf_first": [-1] * leaves}
    for k, (a, l) in enumerate(zip(answers, leaf_of)):
        name = "nil" if a is None else "solution"
        s["counts"][name] += 1
        if s["first"][name] < 0:
            s["first"][name] = k
        s["leaf_count"][l] += 1
        if s["leaf_first"][l] < 0:
            s["leaf_first"][l] = k
    return s


def merge_tiles(tiles):
    """tiles: [(summary, k offset of the tile's point 0 in the whole box's order, or a function tile k -> whole k)] of
    tiles that partition a box -> the whole box's summary: counts add, a first is the smallest tile first moved to the
    whole box's k"""
    def moved(first, to):
        return -1 if first < 0 else (to(first) if callable(to) else first + to)

    def least(a, b):
        return b if a < 0 else (a if b < 0 else min(a, b))

    L = len(tiles[0][0]["leaf_count"])
    s = {"counts": {n: 0 for n, _ in sm.STATUSES}, "first": {n: -1 for n, _ in sm.STATUSES},
         "leaf_count": [0] * L, "leaf_first": [-1] * L}
    for t, to in tiles:
        for n, _ in sm.STATUSES:
            s["counts"][n] += t["counts"][n]
            s["first"][n] = least(s["first"][n], moved(t["first"][n], to))
        for i in range(L):
            s["leaf_count"][i] += t["leaf_count"][i]
            s["leaf_first"][i] = least(s["leaf_first"][i], moved(t["leaf_first"][i], to))
    return s
