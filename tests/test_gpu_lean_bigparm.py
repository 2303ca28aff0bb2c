"""The lean bulk kernel's big-parameter flavour (csrc/pip_lean.h, pip_lean_kernel<SC, false, true>): batches whose one
parameter is the big one (lexicographic maxima, unknowns of either sign), loaded as shifted rows with the plain
pipamd_batch_load.  The same batch with and without the lean launches (pipamd_debug_lean) gives identical statuses, pivot
and cut counts, numerators (both) and denominators on every tableau, and status, pivots and solution text equal the
CPU oracle's; the lean launch really serves the batch.  One more test: without pipamd_engine_set_lean_big such a batch
takes the launches it took before the flavour existed."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BATCH = 160
SEEDS = {(126, 64): 7190, (125, 64): 7189, (62, 32): 7094, (5, 8): 7013, (126, 100): 7226, (127, 64): 7191}
KW = {(5, 8): dict(nnz=3, cmax=3, x0max=5, pneg=0.5)}  # (small systems on which every tableau still needs a pivot)


@functools.lru_cache(maxsize=None)
def _rows(nvar, ni, shift, scale):
    import shift_cases as sc
    from piplib_amd import synth
    rows = sc.shifted(synth.lexmin_batch(SEEDS[nvar, ni], BATCH, nvar, ni, **KW.get((nvar, ni), {})), shift)
    if scale:  # every other tableau: one inequality multiplied through (same polyhedron, large entries, big column too)
        rows[::2, ni // 2, :] *= scale
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def _oracle(nvar, ni, shift, nq, scale):
    """computed once per family, shared by the cases that solve it"""
    from gpu_common import oracle_batch
    return oracle_batch(_rows(nvar, ni, shift, scale), nvar, 1, nq, bigparm=nvar + 1).results


# name, nvar, ni, what else
CASES = [
    ("w128-exactly", 126, 64, {}),                 # W = 128: the big entry is the last value of lane 63
    ("padded-column", 125, 64, {}),                # 127 columns + a zero column; constant and big entry in different lanes
    ("narrow-62", 62, 32, {}),                     # idle lanes stay zero
    ("narrow-5", 5, 8, {}),
    ("class-160", 126, 100, {}),                   # the second lean launch resumes what the first paused
    ("round-pivots-8", 126, 64, dict(round_pivots=8)),   # summaries (big sign included) cross between the two kernels
    ("scaled-rows", 126, 64, dict(scale=40000)),   # the mid path; rows that leave ints mid-run, with a big column
    ("spare-rows-spent", 126, 64, dict(cap=6)),    # PIPAMD_ST_CAPACITY inside the flavour, then expanser
    ("rows-stay", 126, 64, dict(stay=True)),       # the kernel fetches the caller's nvar + 2 wide rows
    ("not-taken-127", 127, 64, {}),                # 129 columns: the general kernel does it all
]


@pytest.mark.parametrize("nq", [1, 0], ids=["integer", "rational"])
@pytest.mark.parametrize("shift", [1, -1], ids=["maximize", "urs"])
@pytest.mark.parametrize("name,nvar,ni,opt", CASES, ids=[c[0] for c in CASES])
def test_lean_bigparm_paths(name, nvar, ni, opt, shift, nq):
    import torch
    from gpu_common import solution_text
    import pipbatch as pb
    from piplib_amd import engine as eng
    rows = _rows(nvar, ni, shift, opt.get("scale", 0))
    tflags = (eng.T_INT if nq else 0) | (eng.T_ROWS_STAY if opt.get("stay") else 0)
    outs, launches = [], []
    for lean in (0, 1):
        e = eng.Engine(0)
        e.set_bulk_min(64)
        e.set_max_rows(ni + 1024)
        e.set_lean_big(True)   # (opt-in; pipamd_debug_lean(0) switches it off like the plain flavour)
        if "round_pivots" in opt:
            e.set_round_pivots(opt["round_pivots"])
        e.debug_lean(lean)
        b = eng.Batch(e, rows, nvar, 1, bigparm=nvar + 1, tflags=tflags, cap_cuts=opt.get("cap"))
        for _ in range(2):  # the second load + solve reuses the workspace
            b.load()
            b.solve()
        launches.append(e.last_solve_launches())
        b.fetch()
        torch.cuda.synchronize()
        outs.append((b.status.cpu().numpy(), b.pivots.cpu().numpy(), b.cuts.cpu().numpy(), b.sol_num.cpu().numpy(),
                     b.sol_den.cpu().numpy()))
    print(name, shift, nq, "launches (lean off, on)", launches, "pivots", int(outs[1][1].sum()))
    if name == "not-taken-127":
        assert launches[1] == launches[0], launches
    else:
        assert launches[1] > launches[0], launches  # the lean launch went out (one more launch than without)
        # the lean launch on its own (PipJob of csrc/pip_job.h, 200 bytes: status at byte 72, pivots at 80, the lean
        # kernel's exit reason at 172 -- 1 pivot budget)
        e.debug_single_launch(2)
        b.load()
        b.solve()
        e.debug_single_launch(0)
        j = b.ws[:25 * BATCH].view(torch.int32).view(BATCH, 50).cpu().numpy()
        status, npiv, why = j[:, 18], j[:, 20], j[:, 43]
        running = status == eng.ST_RUN
        print("  after the lean launch alone: running", int(running.sum()), "reasons", np.bincount(why[running], minlength=6))
        assert (npiv > 0).all(), np.nonzero(npiv == 0)
        if "round_pivots" in opt:
            assert (running & (why == 1)).any()  # paused on the budget: they resume, several times
        elif name == "class-160" and shift < 0 and nq:
            assert (running & (why == 1)).sum() > BATCH // 2  # most spend the first launch's pivot budget
        else:   # (a tableau out of spare rows has left the launch too: PIPAMD_ST_CAPACITY, then expanser)
            assert (~running).sum() > BATCH // 2, running.sum()
        if name == "spare-rows-spent" and nq:
            assert (status == eng.ST_CAPACITY).any()
    for x, y in zip(*outs):
        assert x.shape == y.shape and (x == y).all()
    st, pv, _, num, den = outs[1]
    for k, r in enumerate(_oracle(nvar, ni, shift, nq, opt.get("scale", 0))):
        assert r.status == pb.ST_OK, (k, r.status, r.abort_code)
        assert st[k] in (eng.ST_SOLUTION, eng.ST_NIL), (k, st[k])
        assert pv[k] == r.pivots, (k, pv[k], r.pivots)
        got = "()" if st[k] == eng.ST_NIL else pb.squash(solution_text(num[k], den[k]))
        assert got == pb.squash(r.text), k


def test_flavour_is_opt_in():
    """default engine: a big-parameter batch takes no lean launch (as many launches as with pipamd_debug_lean(0)); with
    pipamd_engine_set_lean_big one more, and the same results"""
    import torch
    from piplib_amd import engine as eng
    nvar, ni = 126, 64
    rows = _rows(nvar, ni, -1, 0)
    launches, outs = [], []
    for big, lean in ((0, 1), (0, 0), (1, 1)):
        e = eng.Engine(0)
        e.set_bulk_min(64)
        e.set_lean_big(big)
        e.debug_lean(lean)
        b = eng.Batch(e, rows, nvar, 1, bigparm=nvar + 1, tflags=eng.T_INT)
        b.load()
        b.solve()
        launches.append(e.last_solve_launches())
        b.fetch()
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in (b.status, b.pivots, b.cuts, b.sol_num, b.sol_den)])
    assert launches[0] == launches[1] and launches[2] > launches[0], launches
    for x, y, z in zip(*outs):
        assert (x == y).all() and (x == z).all()
