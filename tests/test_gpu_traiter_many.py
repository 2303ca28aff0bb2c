"""-m gpu: pipamd_traiter_many -- traiter() for many problems in one call, flags per problem -- and Compute_dual on the
device-resident traiter() for calls that sort 65 ... 128 rows (piplib_amd/csrc/pip_quast.hip, sort_rows_tall).

The authority for cells and pivot counts is the per-problem host tree (pipamd_traiter on an engine with the device tree
off), which test_gpu_golden.py::test_compute_dual_on_gpu[host] pins to the reference's own dual fixtures; for flags 0 and
T_INT the CPU oracle's text is compared too (text only: its pivot count includes the context test's, which traiter() does
not run).  The tall families are sparse_parametric_problems screened by the oracle (ST_OK within 400 pivots, so the
one-at-a-time host side stays at seconds): every kept problem has at least one solution list, so the dual is emitted."""
import functools
import subprocess

import pytest

import pipbatch as pb

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

E_INVALID, E_SOLVER = -1, -5
K = dict(cmax=2, nnz=2, pp=0.15)
Z = dict(cmax=3, nnz=3)
# seed: (nvar, nparm, ni, nc), count, generator arguments, problems the screen keeps at least
TALL = {511: ((8, 1, 64, 2), 16, K, 14),     # last one-row-per-lane sort
        512: ((8, 1, 65, 2), 16, K, 11),     # smallest tall sort
        503: ((10, 0, 100, 0), 16, Z, 16),   # tall, no parameters
        513: ((20, 1, 104, 2), 16, K, 4),    # tallest shape in the box
        505: ((30, 1, 65, 2), 16, K, 6),     # many forks, each with its own `pos`
        506: ((75, 1, 80, 2), 12, K, 9),     # two column blocks and tall
        507: ((100, 0, 70, 0), 12, Z, 12)}   # two column blocks and tall, no parameters


def _oracle(p, nq):
    q = pb.Problem(p.nvar, p.nparm, p.ni, p.nc, p.bigparm, nq, p.ineq, p.ctx)
    try:
        return pb.run_batch(pb.ORACLEPIP, [q], pb.F_NOSIMPLIFY, timeout=10).results[0]
    except subprocess.TimeoutExpired:
        return None


@functools.lru_cache(maxsize=None)
def _tall(seed):
    """the family's problems the oracle finishes (ST_OK) within 400 pivots"""
    from piplib_amd import synth
    shape, count, kw, _ = TALL[seed]
    keep = []
    for p in synth.sparse_parametric_problems(seed, count, *shape, 0, **kw):
        r = _oracle(p, 0)
        if r is not None and r.status == pb.ST_OK and r.pivots <= 400:
            keep.append(p)
    return keep


@functools.lru_cache(maxsize=None)
def _mixed():
    from piplib_amd import engine as eng, synth
    probs = synth.random_problems(92, 40, 5, 2, 7, 2, 0) + synth.random_problems(145, 40, 8, 2, 10, 2, 0)
    return probs, [(0, eng.T_INT, eng.T_DUAL)[i % 3] for i in range(len(probs))]


@pytest.fixture(scope="module")
def engines():
    from piplib_amd import engine as eng
    on, off = eng.Engine(0), eng.Engine(0)
    off.set_device_tree(False)
    return on, off


_host_cache = {}


def _host(off, key, probs, flags, bits):
    """what pipamd_traiter returns problem by problem on the host tree, in traiter_many's form (computed once per key)"""
    from piplib_amd import engine as eng
    if (key, bits) not in _host_cache:
        out = []
        for p, f in zip(probs, flags):
            try:
                cells, piv = eng.traiter(off, p.nvar, p.nparm, p.ni, p.nc, p.bigparm, f, p.ineq, p.ctx, bits=bits)
                out.append((cells, 0, 0, piv))
            except eng.SolverError as x:
                out.append((None, E_SOLVER, x.status, x.pivots))
        _host_cache[(key, bits)] = out
    return _host_cache[(key, bits)]


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if w[1] == E_SOLVER:
            assert g[0] is None and g[1] == E_SOLVER and g[2] == w[2], (i, g[1:], w[1:])
        else:
            assert g[1] == 0 and g[3] == w[3], (i, g[1:], w[1:])
            assert g[0] == w[0], i


@pytest.mark.parametrize("bits", [64, 128])
def test_many_equals_one_at_a_time_mixed_flags(engines, bits):
    from piplib_amd import engine as eng
    on, off = engines
    probs, flags = _mixed()
    got = eng.traiter_many(on, probs, flags, bits=bits)
    served, back = on.last_device_tree()
    assert 0 < served and served + back <= len(probs)
    _same(got, _host(off, "mixed", probs, flags, bits))


def test_against_the_oracle():
    """flags 0 and T_INT: the text of every problem the oracle finishes (no tab_simplify on either side)"""
    from piplib_amd import engine as eng, synth
    e = eng.Engine(0)
    probs, _ = _mixed()
    ints = synth.random_problems(141, 60, 5, 2, 7, 2, 1)
    compared = 0
    for ps, flag in ((probs, 0), (ints, eng.T_INT)):
        got = eng.traiter_many(e, ps, [flag] * len(ps))
        for p, (cells, rc, st, piv) in zip(ps, got):
            r = _oracle(p, 1 if flag else 0)
            if r is None or r.status != pb.ST_OK:
                continue
            assert rc == 0, (rc, st)
            assert pb.squash(eng.tape_text(cells)) == pb.squash(r.text)
            compared += 1
    assert compared >= 100, compared  # (the oracle finishes all 140 of them on the CPU)


def _lists(results):
    from piplib_amd import engine as eng
    return [c[1] for cells, rc, _, _ in results if rc == 0 for c in cells if c[0] == eng.SOL_LIST]


@pytest.mark.parametrize("seed,bits", [(s, 64) for s in sorted(TALL)] + [(512, 128), (503, 128)])
def test_tall_duals_on_the_device(engines, seed, bits):
    """Compute_dual for calls that sort up to 128 rows: cells and pivots as the host tree has them, the device tree
    serving exactly the problems it serves without the dual (the dual adds no arithmetic that could overflow) and at
    least half of them; twice the lists of the plain solve, every second one with an entry per inequality."""
    from piplib_amd import engine as eng
    on, off = engines
    keep = _tall(seed)
    ni = TALL[seed][0][2]
    assert len(keep) >= TALL[seed][3], len(keep)
    dual = eng.traiter_many(on, keep, [eng.T_DUAL] * len(keep), bits=bits)
    served_dual = on.last_device_tree()[0]
    plain = eng.traiter_many(on, keep, None, bits=bits)
    served_plain = on.last_device_tree()[0]
    print(f"family {seed}, {bits} bits: kept {len(keep)}, device tree served {served_dual} with the dual, {served_plain} without")
    _same(dual, _host(off, seed, keep, [eng.T_DUAL] * len(keep), bits))
    assert served_dual == served_plain
    assert 2 * served_dual >= len(keep), (served_dual, len(keep))
    ld, lp = _lists(dual), _lists(plain)
    assert lp and len(ld) == 2 * len(lp)
    assert all(a == ni for a in ld[1::2])


def test_outside_the_box_goes_to_the_host_tree(engines):
    """110 inequalities: not a shape for the device tree, with or without the dual"""
    from piplib_amd import engine as eng, synth
    on, off = engines
    probs = synth.sparse_parametric_problems(514, 8, 6, 1, 110, 2, 0, **K)
    flags = [eng.T_DUAL] * len(probs)
    got = eng.traiter_many(on, probs, flags)
    assert on.last_device_tree() == (0, 0)
    _same(got, _host(off, 514, probs, flags, 64))


@pytest.mark.parametrize("bad", [3, 4])
def test_bad_flag_fails_its_problem_only(engines, bad):
    from piplib_amd import engine as eng
    on, off = engines
    probs, flags = _mixed()
    want = _host(off, "mixed", probs, flags, 64)
    n, at = 12, 4
    fl = list(flags[:n])
    fl[at] = bad
    got = eng.traiter_many(on, probs[:n], fl)
    assert got[at][0] is None and got[at][1] == E_INVALID
    _same(got[:at] + got[at + 1:], want[:at] + want[at + 1:n])


def test_nthreads_and_device_tree_off(engines):
    from piplib_amd import engine as eng
    on, off = engines
    keep = _tall(512)
    flags = [eng.T_DUAL] * len(keep)
    want = eng.traiter_many(on, keep, flags)
    assert on.last_device_tree()[0] > 0
    for nthreads in (1, 4):
        assert eng.traiter_many(off, keep, flags, nthreads=nthreads) == want
        assert off.last_device_tree() == (0, 0)
