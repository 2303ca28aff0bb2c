"""-m gpu: the pivot budget of pipamd_batch_solve's first bulk launch (pipamd_engine_set_round_pivots; the engine's default
is PIPAMD_ROUND_PIVOTS, csrc/pip_host.cpp).  A tableau leaves the first lean launch when it is finished, has spent the
budget, has no room left in the launch's LDS image, or holds a row beyond ints; whatever the budget, the launches behind
it take the tableau from where it stopped, so status, pivots, cuts and solutions may not depend on it.

Batch: 256 tableaux of the headline shape (127 unknowns, 64 rows) with pipamd_engine_set_bulk_min(64), budgets 96 (the
default of rounds 3 to 5), the engine's default and one above it, all against the CPU oracle.  With the larger budgets
tableaux must leave the first launch for "no room in the image" (PipJob.pad_ == 5 behind pipamd_debug_single_launch(2)):
the path a larger budget makes more common is exercised, not assumed.  The family's tableaux seldom need more than the
image's 48 spare rows, so the image is lowered to ROUND_ROWS spare rows (pipamd_engine_set_round_rows) for every solve of
this test."""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEFAULT = 128     # PIPAMD_ROUND_PIVOTS
ROUND_ROWS = 32   # spare rows of the first launch's image in this test
STATUS, PAD = 18, 43  # PipJob (csrc/pip_job.h) as 50 ints


def solve(rows, budget, single=0):
    import torch
    from piplib_amd import engine as eng
    e = eng.Engine(0)
    e.set_bulk_min(64)
    e.set_max_rows(rows.shape[1] + 1024)
    e.set_round_rows(ROUND_ROWS)
    if budget:
        e.set_round_pivots(budget)
    e.debug_single_launch(single)
    b = eng.Batch(e, rows, 127, 0, tflags=eng.T_INT | eng.T_ROWS_STAY)
    b.load()
    b.solve()
    b.fetch()
    torch.cuda.synchronize()
    jobs = b.ws[:25 * rows.shape[0]].view(torch.int32).view(rows.shape[0], 50).cpu().numpy().copy()
    return tuple(t.cpu().numpy() for t in (b.status, b.pivots, b.cuts, b.sol_num, b.sol_den)), jobs, e.last_solve_launches()


def test_first_launch_budgets():
    from gpu_common import oracle_batch, solution_text
    import pipbatch as pb
    from piplib_amd import engine as eng, synth
    rows = synth.lexmin_batch(1000, 256, 127, 64)
    budgets = sorted({96, DEFAULT, DEFAULT + 64})
    outs = {}
    for bud in [0] + budgets:  # 0: the engine's own default
        outs[bud], _, launches = solve(rows, bud)
        assert launches >= 3, (bud, launches)
    for bud in budgets:
        for x, y in zip(outs[0][:3], outs[bud][:3]):
            assert (x == y).all(), bud
        done = outs[0][0] == eng.ST_SOLUTION
        assert (outs[0][3][done] == outs[bud][3][done]).all() and (outs[0][4][done] == outs[bud][4][done]).all(), bud
    st, pv, _, num, den = outs[0]
    o = oracle_batch(rows, 127, 0, 1).results
    assert len(o) == 256
    for k, r in enumerate(o):
        assert r.status != pb.ST_ABORT and st[k] in (eng.ST_SOLUTION, eng.ST_NIL), (k, st[k])
        assert pv[k] == r.pivots, (k, pv[k], r.pivots)
        got = "()" if st[k] == eng.ST_NIL else pb.squash(solution_text(num[k], den[k]))
        assert got == pb.squash(r.text), k
    # who leaves the first launch, and why (1: budget spent, 5: no room in the image)
    left = {}
    for bud in budgets:
        _, jobs, _ = solve(rows, bud, single=2)
        run = jobs[:, STATUS] == 0
        left[bud] = {w: int(((jobs[:, PAD] == w) & run).sum()) for w in (1, 2, 3, 5)}
        print("budget %d: %d tableaux leave the first launch unfinished, by reason %s" % (bud, run.sum(), left[bud]))
    assert left[budgets[-1]][5] > 0, left
    assert left[budgets[-1]][1] <= left[budgets[0]][1], left
