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
NLOG, STATUS = 42, 18  # PipJob (csrc/pip_job.h) as 50 ints


def solve(rows, nvar, spare=True, lean=1, round_pivots=0, round_rows=0, single=0):
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
    b = eng.Batch(e, rows, nvar, 0, tflags=eng.T_INT | eng.T_ROWS_STAY)
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


def against_oracle(rows, nvar, out):
    from gpu_common import oracle_batch, solution_text
    import pipbatch as pb
    from piplib_amd import engine as eng
    st, pv, _, num, den = out
    o = oracle_batch(rows, nvar, 0, 1).results
    assert len(o) == rows.shape[0]
    aborted = 0
    for k, r in enumerate(o):
        if r.status == pb.ST_ABORT:  # mapped as tests/test_gpu_lean_prep.py maps it
            assert st[k] == {2: eng.ST_OVERFLOW, 4: eng.ST_MAXCOL}.get(r.abort_code, eng.ST_OVERFLOW), (k, st[k], r.abort_code)
            aborted += 1
            continue
        assert st[k] in (eng.ST_SOLUTION, eng.ST_NIL), (k, st[k])
        assert pv[k] == r.pivots, (k, pv[k], r.pivots)
        got = "()" if st[k] == eng.ST_NIL else pb.squash(solution_text(num[k], den[k]))
        assert got == pb.squash(r.text), k
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
    rows = synth.dense_batch(seed, 32, 127, ni, cmax=3)
    out, jobs, launches = solve(rows, 127)
    assert launches >= 3, launches
    assert (jobs[:, NLOG] == 0).all()
    assert against_oracle(rows, 127, out) == 32
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
