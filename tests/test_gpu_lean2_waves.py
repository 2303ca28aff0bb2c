"""-m gpu: the second lean launch of pipamd_batch_solve with four waves per tableau (csrc/pip_lean.h, pip_lean_kernel<SC, FULL,
false, 4>; pipamd_engine_set_lean2_waves) against the same launch with one wave, and both against the CPU oracle.

The rows of a pivot, the entry pass and the epilogue are spread over the waves; a row's new value does not depend on the
wave that computes it, so status, pivots, cuts and solutions -- and, behind the two lean launches alone, the job headers --
may not depend on the number of waves.  Small batches make the second launch do most of the work: a first-launch budget
of 8 pivots (pipamd_engine_set_round_pivots) pauses nearly every tableau, and the second launch resumes it."""
import functools

import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
# PipJob (csrc/pip_job.h) as 50 ints: ni, status, npiv, ncut, nupd, maxabs (two ints), nlog, pad_
NI, STATUS, NPIV, NCUT, NUPD, MAXABS, NLOG, PAD = 12, 18, 20, 21, 23, 40, 42, 43
HEADER = [STATUS, NI, NPIV, NCUT, NUPD, NLOG, PAD, MAXABS, MAXABS + 1]


def solve(rows, nvar, waves, budget=8, nq=1, stay=True, cap=None, single=0):
    """one load + solve with `waves` waves per tableau in the second lean launch: (status, pivots, cuts, sol_num,
    sol_den), the job headers, the number of launches"""
    import torch
    from piplib_amd import engine as eng
    ni = rows.shape[1]
    e = eng.Engine(0)
    e.set_bulk_min(64)
    e.set_round_pivots(budget)
    e.set_max_rows(ni + 1024)
    e.set_lean2_waves(waves)
    e.debug_single_launch(single)
    b = eng.Batch(e, rows, nvar, 0, tflags=(eng.T_INT if nq else 0) | (eng.T_ROWS_STAY if stay else 0), cap_cuts=cap)
    b.load()
    b.solve()
    b.fetch()
    torch.cuda.synchronize()
    n = rows.shape[0]
    jobs = b.ws[:25 * n].view(torch.int32).view(n, 50).cpu().numpy().copy()
    out = tuple(t.cpu().numpy() for t in (b.status, b.pivots, b.cuts, b.sol_num, b.sol_den))
    return out, jobs, e.last_solve_launches()


def same_results(a, b, what):
    from piplib_amd import engine as eng
    for x, y in zip(a[:3], b[:3]):
        assert (x == y).all(), what
    done = a[0] == eng.ST_SOLUTION
    assert (a[3][done] == b[3][done]).all() and (a[4][done] == b[4][done]).all(), what


def against_oracle(out, o, exact=None):
    """as test_lean_kernel_paths (tests/test_gpu_parity.py) compares: aborts mapped to statuses, else pivots and the text"""
    from gpu_common import solution_text
    import pipbatch as pb
    from piplib_amd import engine as eng
    st, pv, _, num, den = out
    held = 0
    for k, r in enumerate(o):
        if r.status == pb.ST_ABORT:
            assert st[k] == {2: eng.ST_OVERFLOW, 4: eng.ST_MAXCOL}.get(r.abort_code, eng.ST_OVERFLOW), (k, st[k], r.abort_code)
            if exact and r.abort_code == 2 and k in exact:
                assert pv[k] == r.pivots == exact[k], (k, pv[k], r.pivots)
                held += 1
            continue
        assert st[k] in (eng.ST_SOLUTION, eng.ST_NIL), (k, st[k])
        assert pv[k] == r.pivots, (k, pv[k], r.pivots)
        got = "()" if st[k] == eng.ST_NIL else pb.squash(solution_text(num[k], den[k]))
        assert got == pb.squash(r.text), k
    return held


@functools.lru_cache(maxsize=None)
def headline():
    """the batch of tests/test_gpu_first_launch_budget.py and what the oracle says about it (it finishes every tableau)"""
    from gpu_common import oracle_batch
    from piplib_amd import synth
    rows = synth.lexmin_batch(1000, 256, 127, 64)
    return rows, oracle_batch(rows, 127, 0, 1).results


@pytest.mark.parametrize("budget", [8, 32])
def test_headline_shape(budget):
    import pipbatch as pb
    rows, o = headline()
    assert len(o) == 256 and all(r.status != pb.ST_ABORT for r in o)
    outs = {}
    for waves in (1, 4):
        outs[waves], _, launches = solve(rows, 127, waves, budget)
        assert launches >= 3, (waves, launches)
    same_results(outs[1], outs[4], budget)
    against_oracle(outs[1], o)
    against_oracle(outs[4], o)
    # the two lean launches on their own: the headers they leave, and what the second one did
    _, first, _ = solve(rows, 127, 4, budget, single=2)
    heads = {waves: solve(rows, 127, waves, budget, single=1)[1] for waves in (1, 4)}
    for i in HEADER:
        assert (heads[1][:, i] == heads[4][:, i]).all(), (budget, i)
    gained = heads[4][:, NPIV] > first[:, NPIV]
    print("budget %d: %d of 256 tableaux gained pivots in the second launch" % (budget, gained.sum()))
    assert gained.sum() >= 64, gained.sum()


@pytest.mark.parametrize("name,ni,nq,kw,cap,stay", [
    ("rational", 64, 0, dict(), None, True),
    ("headline-copied-rows", 64, 1, dict(), None, False),
    ("class-1-at-entry", 64, 1, dict(scale=40000), None, True),   # the mid path, on every wave
    ("class-2-mid-run", 64, 1, dict(scale=1 << 24), None, True),  # a row stored wide mid-pivot by whichever wave has it
    ("overflow", 64, 1, dict(cmax=40000, x0max=3), None, True),   # the row gcd's overflow flag, raised by any wave
    ("spare-rows-spent", 64, 1, dict(), 6, True),                 # PIPAMD_ST_CAPACITY inside the launch, then expanser
    ("class-160", 100, 1, dict(), None, True),
])
def test_families_of_lean_kernel_paths(name, ni, nq, kw, cap, stay):
    """the batches of test_lean_kernel_paths (same seeds and keywords), every tableau paused after 8 pivots"""
    from gpu_common import oracle_batch
    from piplib_amd import synth
    nvar, batch = 127, 160
    kw = dict(kw)
    scale = kw.pop("scale", 0)
    rows = synth.lexmin_batch(4000 + ni + len(name), batch, nvar, ni, **kw)
    if scale:
        rows[::2, ni // 2, :] *= scale
    outs, launches = {}, {}
    for waves in (1, 4):
        outs[waves], _, launches[waves] = solve(rows, nvar, waves, nq=nq, stay=stay, cap=cap)
    assert launches[1] == launches[4] >= 3, launches
    same_results(outs[1], outs[4], name)
    import replay_fixture as rf
    exact = rf.exact_aborts("lean-paths-overflow") if name == "overflow" else {}
    o = oracle_batch(rows, nvar, 0, nq).results
    for waves in (1, 4):
        held = against_oracle(outs[waves], o, exact)
        if name == "overflow":
            assert held == len(exact) >= 120, (held, len(exact))


@pytest.mark.parametrize("nvar,ni,stay,four", [
    (100, 60, False, True),   # 102 columns: pip_lean_kernel<160, false, false, 4>
    (41, 16, True, False),    # 112 row slots in the second launch: no four-wave kernel for that class, one wave
])
def test_run_time_widths(nvar, ni, stay, four):
    from gpu_common import oracle_batch
    from piplib_amd import synth
    rows = synth.lexmin_batch(5000 + nvar, 200, nvar, ni)
    outs, launches = {}, {}
    for waves in (1, 4):
        outs[waves], _, launches[waves] = solve(rows, nvar, waves, stay=stay)
    # (the class without a four-wave kernel: the same sequence of launches, whatever was asked for)
    assert launches[1] == launches[4] >= 3, (four, launches)
    same_results(outs[1], outs[4], (nvar, ni))
    o = oracle_batch(rows, nvar, 0, 1).results
    against_oracle(outs[1], o)
    against_oracle(outs[4], o)
