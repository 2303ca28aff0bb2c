"""-m gpu: the lean bulk kernel with its rows prepared one per lane (csrc/pip_lean.h: lean_prepare_rows, the reductions
that start from a folded gcd, the cut kept in registers) against the same batch without the lean kernel
(pipamd_debug_lean) and against the CPU oracle: statuses, pivot and cut counts, solutions of EVERY tableau.

Shapes: the headline's (127 unknowns, 64 rows) with the rows left in the caller's array and copied; dense tableaux of
100 rows, where nearly every row is non-zero in the pivot column -- more than 64 work rows a pivot, so a second batch of
64 is prepared inside one pivot; and the instantiation with run-time column counts.  The seeds were screened on the CPU:
the oracle finishes every tableau within a second (the dense ones all end in its "Integer overflow" abort, which the
kernels answer with PIPAMD_ST_OVERFLOW, mapped as test_lean_kernel_paths maps it)."""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]


def _rows(gen, seed, batch, nvar, ni):
    from piplib_amd import synth
    if gen == "dense":
        return synth.dense_batch(seed, batch, nvar, ni, cmax=3)
    return synth.lexmin_batch(seed, batch, nvar, ni)


@pytest.mark.parametrize("name,gen,seed,batch,nvar,ni,stay", [
    ("headline-rows-stay", "lexmin", 7101, 64, 127, 64, True),
    ("headline-rows-copied", "lexmin", 7101, 64, 127, 64, False),
    ("dense-second-batch", "dense", 7201, 32, 127, 100, True),
    ("run-time-width-63", "lexmin", 7301, 64, 63, 32, True),
    ("run-time-width-100", "lexmin", 7401, 64, 100, 60, False),
])
def test_lean_prepared_rows(name, gen, seed, batch, nvar, ni, stay):
    import torch
    from gpu_common import oracle_batch, solution_text
    import pipbatch as pb
    from piplib_amd import engine as eng
    rows = _rows(gen, seed, batch, nvar, ni)
    outs, launches = [], []
    for lean in (0, 1):
        e = eng.Engine(0)
        e.set_bulk_min(batch // 2)
        e.set_max_rows(ni + 1024)
        e.debug_lean(lean)
        b = eng.Batch(e, rows, nvar, 0, tflags=eng.T_INT | (eng.T_ROWS_STAY if stay else 0))
        for _ in range(2):  # the second load + solve reuses the workspace
            b.load()
            b.solve()
        launches.append(e.last_solve_launches())
        b.fetch()
        torch.cuda.synchronize()
        outs.append((b.status.cpu().numpy(), b.pivots.cpu().numpy(), b.cuts.cpu().numpy(), b.sol_num.cpu().numpy(),
                     b.sol_den.cpu().numpy()))
    assert launches[1] > launches[0], launches  # the lean launch went out
    # the lean launch on its own (PipJob of csrc/pip_job.h as 50 ints: status 18, pivots 20, rows rewritten 23)
    e.debug_single_launch(2)
    b.load()
    b.solve()
    e.debug_single_launch(0)
    j = b.ws[:25 * batch].view(torch.int32).view(batch, 50).cpu().numpy()
    npiv, nupd = j[:, 20], j[:, 23]
    print("%s: lean launch alone: pivots %d, rows rewritten %d, most rows a pivot (mean of a tableau) %.1f" % (
        name, npiv.sum(), nupd.sum(), (nupd / np.maximum(npiv, 1)).max()))
    assert (npiv > 0).all(), npiv  # pivots ran in the lean kernel, on every tableau
    if gen == "dense":
        # a tableau whose pivots rewrote more than 64 rows on average had a pivot with more than 64 work rows: the
        # preparation's second batch of 64
        assert (nupd > 64 * npiv).any(), (nupd / np.maximum(npiv, 1)).max()
    for x, y in zip(*outs):
        assert (x == y).all()
    st, pv, _, num, den = outs[1]
    o = oracle_batch(rows, nvar, 0, 1).results
    assert len(o) == batch
    # an "Integer overflow" the model follows in exact arithmetic is the determinant's, and its pivot count the oracle's
    # (tests/replay_fixture.py; the dense family has none: every abort of it follows wrapped arithmetic)
    import replay_fixture as rf
    fam = rf.family_of(gen + "_batch", seed, batch, nvar, ni, **(dict(cmax=3) if gen == "dense" else {}))
    exact = rf.exact_aborts(fam) if fam else {}
    for k, r in enumerate(o):
        if r.status == pb.ST_ABORT:
            assert st[k] == {2: eng.ST_OVERFLOW, 4: eng.ST_MAXCOL}.get(r.abort_code, eng.ST_OVERFLOW), (k, st[k], r.abort_code)
            if r.abort_code == 2 and k in exact:
                assert pv[k] == r.pivots == exact[k], (k, pv[k], r.pivots)
            continue
        assert st[k] in (eng.ST_SOLUTION, eng.ST_NIL), (k, st[k])
        assert pv[k] == r.pivots, (k, pv[k], r.pivots)
        got = "()" if st[k] == eng.ST_NIL else pb.squash(solution_text(num[k], den[k]))
        assert got == pb.squash(r.text), k
