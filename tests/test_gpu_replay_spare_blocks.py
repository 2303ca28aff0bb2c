"""-m gpu: the determinant replay in the spare blocks of pipamd_batch_solve's second lean launch (csrc/pip_lean.h,
lean_spare_replay; pipamd_engine_set_spare_replay) and the one-wave-per-job catch-all behind the launches.

The second lean launch has a block per tableau of the batch over the list of the tableaux the first launch paused; its
blocks beyond the list replay the logs of the finished tableaux that are not on the list.  Every case runs with
pipamd_engine_set_bulk_min low enough for the two lean launches to go out, and after every solve the `nlog` of every job
header must be 0: no log is left unreplayed, whoever replayed it.  Who did is seen with the solve stopped behind the two
lean launches without the catch-all (debug_single_launch(3), test_spare_blocks_do_the_replaying)."""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
NLOG, STATUS, NPIV, LDET, DET = 42, 18, 20, 22, 24  # PipJob (csrc/pip_job.h) as 50 ints; det[]: 8 int64 from int 24


def solve(rows, nvar, spare=True, lean=1, round_pivots=0, round_rows=0, single=0, bits=64, lone=False):
    """(status, pivots, cuts, sol_num, sol_den), the job headers as ints, the launches of the solve"""
    import torch
    from piplib_amd import engine as eng
    batch, ni = rows.shape[0], rows.shape[1]
    e = eng.Engine(0)
    e.set_bulk_min(1)
    e.set_max_rows(ni + 1024)
    e.set_spare_replay(spare)
    e.debug_lean(lean)
    if round_pivots:
        e.set_round_pivots(round_pivots)
    if round_rows:
        e.set_round_rows(round_rows)
    e.debug_single_launch(single)
    if lone:
        e.set_lone_batches(True)
    b = eng.Batch(e, rows, nvar, 0, tflags=eng.T_INT | (eng.T_ROWS_STAY if bits == 64 else 0), entier_bits=bits)
    b.load()
    b.solve()
    b.fetch()
    torch.cuda.synchronize()
    jobs = b.ws[:25 * batch].view(torch.int32).view(batch, 50).cpu().numpy().copy()
    out = tuple(t.cpu().numpy() for t in (b.status, b.pivots, b.cuts, b.sol_num, b.sol_den))
    return out, jobs, e.last_solve_launches()


def same(a, b):
    from piplib_amd import engine as eng
    for x, y in zip(a[:3], b[:3]):
        assert (x == y).all()
    done = a[0] == eng.ST_SOLUTION
    assert (a[3][done] == b[3][done]).all() and (a[4][done] == b[4][done]).all()


def against_oracle(rows, nvar, out, exact=None):
    """exact: {tableau: pivots} of the aborted tableaux the model holds exact up to the abort (tests/replay_fixture.py):
    on them the "Integer overflow" is the determinant's, found by the replay, and its pivot count is the oracle's"""
    from gpu_common import oracle_batch, solution_text
    import pipbatch as pb
    from piplib_amd import engine as eng
    st, pv, _, num, den = out
    o = oracle_batch(rows, nvar, 0, 1).results
    assert len(o) == rows.shape[0]
    aborted = agree = 0
    for k, r in enumerate(o):
        if r.status == pb.ST_ABORT:  # mapped as tests/test_gpu_lean_prep.py maps it
            assert st[k] == {2: eng.ST_OVERFLOW, 4: eng.ST_MAXCOL}.get(r.abort_code, eng.ST_OVERFLOW), (k, st[k], r.abort_code)
            aborted += 1
            agree += int(pv[k] == r.pivots)
            if r.abort_code == 2 and exact and k in exact:
                assert pv[k] == r.pivots == exact[k], (k, pv[k], r.pivots, exact[k])
            continue
        assert st[k] in (eng.ST_SOLUTION, eng.ST_NIL), (k, st[k])
        assert pv[k] == r.pivots, (k, pv[k], r.pivots)
        got = "()" if st[k] == eng.ST_NIL else pb.squash(solution_text(num[k], den[k]))
        assert got == pb.squash(r.text), k
    if aborted:
        print("aborted %d, held to the oracle's pivot count %d, same count on %d of all aborted" % (
            aborted, len([k for k in (exact or ()) if o[k].status == pb.ST_ABORT]), agree))
    return aborted


@pytest.fixture(scope="module")
def headline():
    """the batch of cases (b) and (c), and its solve with the part switched off and without the lean kernel"""
    from piplib_amd import synth
    rows = synth.lexmin_batch(7101, 64, 127, 64)
    ref, jobs, _ = solve(rows, 127, spare=False, lean=0)
    assert (jobs[:, NLOG] == 0).all()
    return rows, ref


@pytest.mark.parametrize("seed,ni", [(7201, 100), (7202, 64)])
def test_overflow_found_by_the_replay(seed, ni):
    """(a) dense tableaux (screened on the CPU: the oracle ends every one in its "Integer overflow" abort within a
    second): the replay is what finds the overflow.  100 rows: the family of tests/test_gpu_lean_prep.py, whose second
    launch has no lean class (the catch-all in its one-lane form does the work); 64 rows: the two lean launches."""
    from piplib_amd import synth
    import replay_fixture as rf
    rows = synth.dense_batch(seed, 32, 127, ni, cmax=3)
    out, jobs, launches = solve(rows, 127)
    assert launches >= 3, launches
    assert (jobs[:, NLOG] == 0).all()
    # (the model admits none of these: every abort of the family follows wrapped arithmetic, replay_fixture.COUNTED)
    assert against_oracle(rows, 127, out, rf.exact_aborts(rf.family_of("dense_batch", seed, 32, 127, ni, cmax=3))) == 32
    off, jobs, _ = solve(rows, 127, spare=False)
    assert (jobs[:, NLOG] == 0).all()
    same(out, off)


@pytest.mark.parametrize("budget", [0, 64])
def test_headline_against_the_oracle(headline, budget):
    """(b) every tableau of a headline-shaped batch: status, pivots, solution text -- with the engine's own first-launch
    budget, which may leave the second launch's list of so small a batch empty, and with a budget of 64 pivots, under
    which the first launch finishes some tableaux and pauses others: list blocks and spare blocks both have work"""
    rows, ref = headline
    out, jobs, launches = solve(rows, 127, round_pivots=budget)
    assert launches >= 3, launches
    assert (jobs[:, NLOG] == 0).all()
    assert against_oracle(rows, 127, out) == 0
    same(out, ref)
    _, j1, _ = solve(rows, 127, round_pivots=budget, single=2, spare=False)
    running = int((j1[:, STATUS] == 0).sum())
    print("first launch alone, budget %d: %d of %d tableaux still running" % (budget, running, len(j1)))
    if budget:
        assert 0 < running < len(j1)


@pytest.mark.parametrize("batch", [64, 130])
def test_spare_blocks_do_the_replaying(batch):
    """the solve stopped behind the two lean launches WITHOUT the catch-all replay (debug_single_launch(3)), first-launch
    budget 64: the logs are as the launches left them.  With the part on, every tableau the first launch finished (it is
    not on the second launch's list) has an empty log -- only the spare blocks can have emptied it; with the part off the
    same tableaux still carry their logs, so the check can tell the two apart.  130: the last replay block is partly filled"""
    from piplib_amd import engine as eng, synth
    rows = synth.lexmin_batch(7101, batch, 127, 64)
    _, j1, _ = solve(rows, 127, round_pivots=64, single=2, spare=False)
    finished = np.isin(j1[:, STATUS], (eng.ST_SOLUTION, eng.ST_NIL))
    assert 0 < finished.sum() < batch
    _, joff, _ = solve(rows, 127, round_pivots=64, single=3, spare=False)
    left = int((joff[finished, NLOG] > 0).sum())
    print("batch %d: the first launch finished %d tableaux, %d of them with a log to replay" % (batch, finished.sum(), left))
    assert left > 0
    _, jon, _ = solve(rows, 127, round_pivots=64, single=3)
    assert (jon[finished, NLOG] == 0).all(), np.nonzero(finished & (jon[:, NLOG] != 0))[0]
    assert (jon[finished, STATUS] == j1[finished, STATUS]).all()


def test_every_tableau_on_the_list(headline):
    """(c) a first-launch budget of one pivot: every tableau pauses, the list is the whole batch, no spare block"""
    rows, ref = headline
    _, j1, _ = solve(rows, 127, round_pivots=1, single=2)
    assert (j1[:, STATUS] == 0).all()
    out, jobs, _ = solve(rows, 127, round_pivots=1)
    assert (jobs[:, NLOG] == 0).all()
    same(out, ref)


def test_empty_list(headline):
    """(c) the tableaux the first launch finishes under a budget of 352 pivots and an image of 96 spare rows, as a batch
    of their own under the same settings: nothing pauses, the list is empty, every block of the second launch is spare"""
    rows, ref = headline
    _, j1, _ = solve(rows, 127, round_pivots=352, round_rows=96, single=2)
    keep = np.nonzero(j1[:, STATUS] != 0)[0]
    print("finished by the first launch (352 pivots, 96 spare rows): %d of %d" % (len(keep), len(j1)))
    assert len(keep) >= 32
    sub = np.ascontiguousarray(rows[keep])
    _, j2, _ = solve(sub, 127, round_pivots=352, round_rows=96, single=2)
    assert (j2[:, STATUS] != 0).all()
    out, jobs, _ = solve(sub, 127, round_pivots=352, round_rows=96)
    assert (jobs[:, NLOG] == 0).all()
    same(out, tuple(x[keep] for x in ref))


@pytest.mark.parametrize("batch", [1, 65, 130])
def test_partly_filled_last_block(batch):
    """(c) batches that end inside a replay block of 64"""
    from piplib_amd import synth
    rows = synth.lexmin_batch(7101, batch, 127, 64)
    ref, jobs, _ = solve(rows, 127, spare=False, lean=0)
    assert (jobs[:, NLOG] == 0).all()
    out, jobs, _ = solve(rows, 127)
    assert (jobs[:, NLOG] == 0).all()
    same(out, ref)


# ---- the overflow's pivot count and the determinant the replays leave in the job header, against the model
# (tests/golden/replay_model.json, made by tests/bigint_pip.py and tests/replay_model.py in Python ints)

VARIANTS = [dict(), dict(lean=0), dict(spare=False), dict(round_pivots=1), dict(round_pivots=64),
            dict(round_pivots=64, spare=False), dict(lone=True)]  # lone: the wave-per-job catch-all does the replaying
# (the lean kernel and its spare blocks take 64-bit batches only: with 128-bit entries those switches select nothing)
VARIANTS_128 = [dict(), dict(round_pivots=1), dict(round_pivots=64), dict(lone=True)]


def header_det(jobs, bits):
    """per job (ldet, [4 limbs]) of the header, the limbs as signed integers of `bits` bits"""
    w = np.ascontiguousarray(jobs[:, DET:DET + 16]).view(np.uint64)
    ew = bits // 64
    out = []
    for k in range(len(jobs)):
        limbs = [sum(int(w[k, ew * i + h]) << (64 * h) for h in range(ew)) for i in range(4)]
        out.append((int(jobs[k, LDET]), [x - (1 << bits) if x >> (bits - 1) else x for x in limbs]))
    return out


@pytest.mark.parametrize("name,budgets", [("sparse-100-rows", (0, 64)), ("sparse-64-rows", (0, 1, 16))])
def test_overflow_pivot_count(name, budgets):
    """tableaux whose determinant outgrows its three limbs in EXACT arithmetic (sparse rows of two entries; screened on
    the CPU: the model reaches the oracle's abort with nothing wrapped, tests/test_replay_fixture.py): the replay is the
    only source of their "Integer overflow", and the pivot count it writes -- npiv - nlog + k + 1 over a log that may
    span launches -- is the oracle's.  100 rows: the aborts come after 70 .. 97 pivots, around the first launch's
    budgets; 64 rows: after 27 .. 37, in the first lean launch's log or, under a budget of 1 or 16, the second's"""
    import replay_fixture as rf
    rows = rf.rows_of(rf.SCREEN[name])
    exact = rf.exact_aborts(name)
    assert len(exact) >= 15
    ref = None
    for budget in budgets:
        for kw in (dict(), dict(spare=False), dict(lean=0), dict(lone=True)):
            out, jobs, _ = solve(rows, 127, round_pivots=budget, **kw)
            assert (jobs[:, NLOG] == 0).all()
            assert (jobs[:, NPIV] == out[1]).all()
            if ref is None:
                ref = out
                assert against_oracle(rows, 127, out, exact) == len(exact)
            same(out, ref)


@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("name", ["dense10", "dense14", "headline"])
def test_header_determinant(name, bits):
    """the limbs and ldet a solve leaves in the job headers -- carried from one replay to the next, as two words a limb
    with 128-bit entries, and read by nothing but the next replay -- are the model's final determinant on every
    tableau it follows to the end at this width (an overflow included: the limbs as the failing step left them),
    whoever replayed: lean kernel on and off, spare blocks on and off, first-launch budgets of 1 and 64 pivots, and an
    engine of lone batches, whose catch-all goes out a wave per job.  All variants agree on every tableau"""
    import replay_fixture as rf
    from piplib_amd import engine as eng
    rows = rf.rows_of(rf.HEADERS[name])
    nvar = rows.shape[2] - 1
    recs = rf.headers(name, bits)
    first = None
    for kw in (VARIANTS if bits == 64 else VARIANTS_128):
        out, jobs, _ = solve(rows, nvar, bits=bits, **kw)
        assert (jobs[:, NLOG] == 0).all(), kw
        det = header_det(jobs, bits)
        if first is None:
            first = (out, det)
            held = 0
            for k, r in enumerate(recs):
                if r is None or out[0][k] == eng.ST_CAPACITY:
                    continue
                assert (out[0][k], out[1][k]) == r[:2], (k, out[0][k], out[1][k], r[:2])
                assert det[k] == (r[2], r[3]), (k, det[k], r[2:])
                held += 1
            print("%s at %d bits: %d of %d headers held to the model" % (name, bits, held, len(recs)))
            assert held >= (4 if (name, bits) == ("dense14", 64) else len(recs) // 2)
        same(out, first[0])
        assert det == first[1], kw
