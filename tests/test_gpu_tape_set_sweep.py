"""-m gpu: engine.TapeSet.sweep_jobs -- every tape of a set swept over its own box in one launch, a summary per job
(pipamd_tape_set_sweep_create / pipamd_tape_set_sweep_run, pip_tape_set_sweep_kernel of csrc/pip_tape.hip), both widths.

Authorities: engine.Tape.sweep_into of each tape alone with the job's box and context (held to the reference's recorded
answers and to the models by tests/test_gpu_tape_sweep.py); tests/tape_set_sweep_model.py (held to the recorded answers
by tests/test_tape_set_sweep_model.py); the golden grid's records.  Every word of every job is compared."""
import ctypes as C

import numpy as np
import pytest

import tape_cases as tc
import tape_model as tm
import tape_set_sweep_model as ssm
import tape_sweep_model as sm
import tape_values_cases as vc
from tape_cases import MAX64, MIN64
from test_gpu_tape_eval import _engine
from test_gpu_tape_set import UNBOUNDED
from test_gpu_tape_sweep import set_blocks

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]


def single(t, lo, hi, ctx):
    """the words pipamd_tape_sweep writes for the tape alone"""
    import torch
    s, _ = t.sweep_into(lo, hi, {}, ctx=ctx, summary=True)
    torch.cuda.synchronize()
    return s.cpu().tolist()


def run(w, **kw):
    import torch
    got = w.run(**kw)
    torch.cuda.synchronize()
    return got.cpu().tolist()


def hold(tapes, jobs, blocks=(0,)):
    """the set of `tapes` swept over `jobs` [(tape index, lo, hi, ctx)], with the grid capped to each of `blocks`: every
    job's words are the tape's own sweep's.  Returns (TapeSetSweep, words, the single sweeps' words per job)"""
    from piplib_amd import engine as eng
    tset = eng.TapeSet(_engine(), tapes)
    w = tset.sweep_jobs(jobs)
    want = [single(tapes[i], lo, hi, ctx) for i, lo, hi, ctx in jobs]
    assert w.summary_off == [0] + list(np.cumsum([len(x) for x in want]))
    assert w.leaves == [tapes[i].info["leaves"] for i, _, _, _ in jobs]
    words = None
    try:
        for b in blocks:
            set_blocks(b)
            words = run(w)
            assert len(words) == w.summary_off[-1]
            for j, (a, z) in enumerate(zip(w.summary_off, w.summary_off[1:])):
                assert words[a:z] == want[j], (b, j, jobs[j][:3])
    finally:
        set_blocks(0)
    return w, words, want


# ---------------------------------------------------------------- 1. the golden tapes
@pytest.mark.parametrize("bits", [64, 128])
def test_golden_tapes(bits):
    from piplib_amd import engine as eng
    g = tc.golden()
    names = list(g["tapes"])
    cells = [tc.cells_from_text(g["tapes"][n]) for n in names]
    tapes = [eng.Tape(_engine(), c, g["nvar"], g["nparm"], 0, bits) for c in cells]
    w, words, _ = hold(tapes, [(i, [0, 0], [9, 9], None) for i in range(len(tapes))])
    got = w.summaries(words)
    for i, n in enumerate(names):
        res = tm.evaluate_cells(cells[i], g["nvar"], g["nparm"], 0, g["points"], bits)
        assert tc.answers_of(res) == g["answers"][n]
        assert got[i] == ssm.census(g["answers"][n], [r[1] for r in res], tapes[i].info["leaves"]), n
    info = w.set.tape_info(1)
    assert info == dict(tapes[1].info, point_cols=2, nvar=g["nvar"], ndual=0)
    with pytest.raises(eng.TapeError):
        w.set.tape_info(len(tapes))


# ---------------------------------------------------------------- 2. job sizes and the grid
def test_job_sizes_and_grids():
    """jobs around the wave and the chunk, neighbours on different tapes; with 1, 2 and 3 workgroups one workgroup
    crosses many jobs and flushes its status figures at every change"""
    from piplib_amd import engine as eng
    e = _engine()
    tapes = [eng.Tape(e, tc.if_chain(5), 1, 1, 0, 64),
             eng.Tape(e, tc.iff([1, 1, -5], tc.leaf([([1, 0, 0], 1), ([0, 1, 0], 1)]), tc.nil()), 2, 2, 0, 64),
             eng.Tape(e, tc.nil(), 1, 1, 0, 64)]
    jobs = []
    for rep, at in ((0, -2), (1, 3)):
        for k, n in enumerate((1, 63, 64, 65, 127, 128, 129, 257)):
            i = (k + rep) % 3
            jobs.append((i, [at, 3], [at + n - 1, 3], [[1, 1, 0, -at - 1]]) if i == 1 else (i, [at], [at + n - 1], None))
    w, words, _ = hold(tapes, jobs, blocks=(1, 2, 3, 0))
    assert [sum(s["counts"].values()) for s in w.summaries(words)] == [1, 63, 64, 65, 127, 128, 129, 257] * 2


# ---------------------------------------------------------------- 3. slot rows, marks, the empty tape, tiles
@pytest.mark.parametrize("bits", [64, 128])
def test_slot_rows_marks_empty_tape_and_tiles(bits):
    from piplib_amd import engine as eng
    e = _engine()
    g = tc.golden()
    cells, nvar, nparm, ndual, edit = UNBOUNDED
    tapes = [eng.Tape(e, tc.new_chain(1, 30), 2, 1, 0, bits),                                    # 0: 32 slots
             eng.Tape(e, tc.iff([1, -2], tc.leaf([([3, 1], 2)]), tc.nil()), 1, 1, 0, bits),      # 1: 2 slots
             eng.Tape(e, cells, nvar, nparm, ndual, bits, edit=edit),                           # 2: both marks
             eng.Tape(e, [], 1, 3, 0, bits),                                                     # 3: empty
             eng.Tape(e, tc.iff([-3], tc.nil(), tc.leaf([([7], 2)])), 1, 0, 0, bits),            # 4: no point column
             eng.Tape(e, tc.cells_from_text(g["tapes"]["int"]), g["nvar"], g["nparm"], 0, bits)]  # 5: tiled
    assert (tapes[0].info["slots"], tapes[1].info["slots"], tapes[2].point_cols, tapes[4].point_cols) == (32, 2, 1, 0)
    ctx = [[1, 1, 1, -4]]
    jobs = [(0, [-40], [109], None), (1, [-40], [109], None), (0, [200], [349], None), (1, [-3], [146], None),
            (2, [-3], [7], None), (1, [0], [10], None), (3, [0, 1, 2], [3, 4, 5], [[1, 1, 0, 0, -2]]), (4, [], [], None),
            (5, [0, 0], [3, 9], ctx), (5, [4, 0], [6, 9], ctx), (5, [7, 0], [9, 9], ctx), (5, [0, 0], [9, 9], ctx)]
    w, words, _ = hold(tapes, jobs, blocks=(1, 0))
    got = w.summaries(words)
    assert got[6]["counts"] == {"solution": 0, "nil": 32, "range": 0, "outside": 32} and got[6]["leaf_count"] == []
    assert got[7]["counts"]["solution"] == 1 and got[7]["leaf_first"] == [-1, 0]
    assert ssm.merge_tiles([(got[8], 0), (got[9], 40), (got[10], 70)]) == got[11]
    assert got[11]["counts"]["outside"] > 0 and got[11]["counts"]["solution"] > 0


# ---------------------------------------------------------------- 4. contexts, ragged over the jobs
@pytest.mark.parametrize("bits", [64, 128])
def test_contexts(bits):
    from piplib_amd import engine as eng
    e = _engine()
    one = eng.Tape(e, tc.if_chain(5), 1, 1, 0, bits)
    two = eng.Tape(e, tc.iff([1, 1, -5], tc.leaf([([1, 0, 0], 1), ([0, 1, 0], 1)]), tc.nil()), 2, 2, 0, bits)
    wide = eng.Tape(e, tc.nil(), 1, 31, 0, bits)
    edge = sm.edge_rows()
    jobs = [(0, [-4], [200], None), (1, [-1, -2], [11, 10], [[1, 1, -1, -1]]), (0, [-4], [200], [[1, -1, 100]]),
            (1, [-1, -2], [11, 10], [[0, 1, -1, 0]]), (0, [-4], [200], [[0, 1, -7]]),
            (1, [-1, -2], [11, 10], [[1, 0, 0, -1]]), (0, [-4], [200], [[1, 0, -1]]),
            (1, [-1, -2], [11, 10], [[1, 1, 1, -4], [0, 1, -2, 0]])]
    for rows, point, inside in (edge[0], edge[1], edge[2]):  # rows of INT64_MIN coefficients over 31 columns
        jobs.append((2, point, point, rows))
    w, words, _ = hold([one, two, wide], jobs, blocks=(2, 0))
    got = w.summaries(words)
    assert got[0]["counts"]["outside"] == 0 and 0 < got[1]["counts"]["outside"] < 169 and got[4]["counts"]["outside"] == 204
    assert got[5]["counts"]["outside"] == 169 and got[6]["counts"]["outside"] == 205 and sum(got[6]["leaf_count"]) == 0
    for s, (_, _, inside) in zip(got[8:], edge[:3]):
        assert s["counts"] == {"solution": 0, "nil": int(inside), "range": 0, "outside": int(not inside)}


# ---------------------------------------------------------------- 5. RANGE points
@pytest.mark.parametrize("bits", [64, 128])
def test_range_points(bits):
    from piplib_amd import engine as eng
    e = _engine()
    if bits == 64:  # theta >= 2 and theta <= -3: the new parameter 2^62 theta leaves int64
        tapes = [eng.Tape(e, tc.new(1, [1 << 62, 0], 1, tc.leaf([([0, 1, 3], 2), ([1, 0, 0], 1)])), 2, 1, 0, 64)]
    else:           # theta >= 4: 2^63 times the new parameter leaves 128 bits in the second unknown
        tapes = [eng.Tape(e, tc.new(1, [1 << 62, 0], 1, tc.leaf([([1, 0, 0], 1), ([0, 1 << 63, 3], 2)])), 2, 1, 0, 128)]
    jobs = [(0, [-5], [6], None), (0, [2], [300], None)]
    for name, (case, widths) in vc.edges().items():
        if bits in widths:
            cells, nvar, nparm, lo, hi, ctx, edit = case
            tapes.append(eng.Tape(e, cells, nvar, nparm, 0, bits, edit=edit))
            jobs.append((len(tapes) - 1, lo, hi, list(ctx) or None))
    jobs.append((0, [-5], [6], None))
    w, words, _ = hold(tapes, jobs, blocks=(1, 0))
    got = w.summaries(words)
    assert 0 < got[0]["counts"]["range"] < 12 and got[0]["counts"]["solution"] > 0 and got[1]["counts"]["range"] >= 297
    assert sum(s["counts"]["range"] > 0 for s in got) >= 4 and got[-1] == got[0]


# ---------------------------------------------------------------- 6. many leaves
def test_many_leaves():
    """a chain whose first wave reaches 64 distinct leaves, one whose rows are each at another leaf, and a chain of 2016
    conditions, next to a job of two leaves"""
    from piplib_amd import engine as eng
    e = _engine()
    tapes = [eng.Tape(e, tc.if_chain(70), 1, 1, 0, 64), eng.Tape(e, vc.leaf_chain(40), 1, 2, 0, 64),
             eng.Tape(e, tc.if_chain(2016), 1, 1, 0, 64), eng.Tape(e, tc.iff([1, -2], tc.leaf([([3, 1], 2)]), tc.nil()), 1, 1, 0, 64)]
    jobs = [(0, [0], [199], None), (3, [0], [5], None), (1, [0, 0], [3, 63], None), (2, [-5], [2100], None), (3, [-9], [200], None)]
    w, words, _ = hold(tapes, jobs, blocks=(1, 0))
    got = w.summaries(words)
    assert got[0]["leaf_count"] == [1] * 70 + [130] and got[0]["leaf_first"] == list(range(71))
    assert sum(c > 0 for c in got[2]["leaf_count"]) == 41 and sum(c > 0 for c in got[3]["leaf_count"]) == 2017


# ---------------------------------------------------------------- 7. streams, reuse, no jobs, refusals
def test_streams_reuse_and_refusals():
    import torch
    from piplib_amd import engine as eng
    e = _engine()
    g = tc.golden()
    tapes = [eng.Tape(e, tc.cells_from_text(g["tapes"]["int"]), g["nvar"], g["nparm"], 0, 64), eng.Tape(e, tc.if_chain(5), 1, 1, 0, 64)]
    jobs = [(0, [-5, -5], [58, 58], [[1, 1, 1, -3]]), (1, [0], [999], None), (0, [0, 0], [9, 9], None)] * 3
    w, words, _ = hold(tapes, jobs)
    a, b = torch.full((w.words,), 7, dtype=torch.int64, device="cuda"), torch.full((w.words + 5,), -9, dtype=torch.int64, device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    w.run_into(a, stream=s1.cuda_stream)
    w.run_into(b, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert a.cpu().tolist() == words and b.cpu().tolist() == words + [-9] * 5
    w.run_into(a)  # again into the same words: the call initialises them, nothing accumulates
    torch.cuda.synchronize()
    assert a.cpu().tolist() == words
    tset = w.set
    none = tset.sweep_jobs([])
    assert none.summary_off == [0] and run(none) == [] and none.summaries([]) == []
    ok = (1, [0], [9], None)
    for bad, job in (([(-1, [0], [9], None)], 0), ([ok, (2, [0], [9], None)], 1), ([ok, ok, ok, (1, [5], [4], None), ok], 3)):
        with pytest.raises(eng.TapeError) as err:
            tset.sweep_jobs(bad)
        assert err.value.code == tm.E_INVALID and f"tape_set_sweep_create: job {job}" in str(err.value), str(err.value)
    # a null ctx with n_ctx > 0, through the C entry itself
    fn = eng.lib().pipamd_tape_set_sweep_create
    arr = (eng.TapeSweepJob * 2)()
    box = (C.c_int64 * 1)(3)
    for q in arr:
        q.tape, q.lo, q.hi = 1, C.addressof(box), C.addressof(box)
    arr[1].n_ctx = 2
    out = C.c_void_p()
    assert fn(e._h, tset._h, 2, arr, C.byref(out), None) == tm.E_INVALID and not out.value
    assert "tape_set_sweep_create: job 1" in eng.lib().pipamd_last_error().decode()
    assert run(w) == words  # (refusals leave the set and its sweeps as they were)


# ---------------------------------------------------------------- 8. end to end
def test_pip_solve_many_end_to_end():
    """40 seeded problems of the p3 shape solved by pip_solve_many, compiled with their infos, each swept under its own
    ineqpar over [-3, 9]^point_cols: every job is the tape's own sweep.  (The family is drawn as
    test_gpu_pipsolve.py draws its fresh seeds: a problem the CPU oracle does not finish in a second is drawn again --
    the raw stream of seed 1 has one, its tenth, on which the host tree spends minutes.)"""
    import pipbatch as pb
    import pipsolve_model as pm
    from piplib_amd import engine as eng
    e = _engine()
    probs = [p for p, _, _ in pm.gen_family("p3", 1, count=40, exe=pb.ORACLEPIP)]
    inputs = [eng.PipInput(np.array(p["inequnk"], dtype=np.int64), np.array(p["ineqpar"], dtype=np.int64), p["bg"], p["options"])
              for p in probs]
    tapes, jobs = [], []
    for p, (cells, rc, _, _, info) in zip(probs, eng.pip_solve_many(e, inputs)):
        if rc != 0 or info["is_void"] or not cells:
            continue
        ndual = info["ni"] if info["sol_flags"] & eng.SOL_DUAL else 0
        t = eng.Tape(e, cells, info["nvar"], info["nparm"], ndual, 64, edit=info)
        ctx = np.array(p["ineqpar"], dtype=np.int64).reshape(-1, t.point_cols + 2)
        tapes.append(t)
        jobs.append((len(tapes) - 1, [-3] * t.point_cols, [9] * t.point_cols, ctx if len(ctx) else None))
    assert len(tapes) >= 20
    w, words, _ = hold(tapes, jobs)
    got = w.summaries(words)
    assert sum(s["counts"]["solution"] for s in got) > 0 and sum(s["counts"]["outside"] for s in got) > 0
