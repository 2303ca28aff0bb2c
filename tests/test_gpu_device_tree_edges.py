"""-m gpu: the device-resident traiter() (piplib_amd/csrc/pip_quast.hip) exactly at every capacity reserve of its box
(quast_caps, piplib_amd/csrc/pip_tree.cpp) and one past it, on the deterministic families of tests/device_tree_edges.py.

Every member runs alone in its call (quast_caps_max lets a roomier sibling enlarge a problem's box), through
solve_tableaux(lockstep=True) and solve_tableaux_lockstep128, with the device tree on and off.  The authority is the CPU
oracle of that width: text, pivot count, rc == -5 where the reference abandons the problem.  On top of that the device
tree's own record of the problem (Engine.debug_device_tree_records) must say served, or handed back with exactly the
Q_WHY_* bit of the reserve that ran out.  The flip points are the documented reserves, not the kernel's checks; the figures
each member rests on are held to the oracle and the reference in tests/test_device_tree_edges_model.py."""
import pytest

import device_tree_edges as dte
import pipbatch as pb

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

_ENGINES, _ORACLE = {}, {}


def _engine(tree=True):
    """two engines for the whole module, both recording: device tree on / off"""
    from piplib_amd import engine as eng
    if tree not in _ENGINES:
        e = eng.Engine(0)
        e.set_device_tree(tree)
        e.debug_device_tree_record(True)
        _ENGINES[tree] = e
    return _ENGINES[tree]


def _oracle(key, probs, bits):
    """the CPU oracle's results for probs, computed once per (key, bits)"""
    if (key, bits) not in _ORACLE:
        _ORACLE[key, bits] = pb.run_batch(pb.ORACLEPIP if bits == 64 else pb.ORACLEPIP128, probs).results
    return _ORACLE[key, bits]


def _run(e, probs, bits):
    from piplib_amd import engine as eng
    if bits == 128:
        return eng.solve_tableaux_lockstep128(e, probs)
    return eng.solve_tableaux(e, probs, lockstep=True)


def _same(probs, want, got):
    assert len(got) == len(want) == len(probs)
    for k, (r, (text, rc, st, piv)) in enumerate(zip(want, got)):
        if r.status == pb.ST_ABORT:
            assert rc == -5, (k, rc, st)
            continue
        assert rc == 0, (k, rc, st)
        assert pb.squash(text) == pb.squash("void\n" if r.status == pb.ST_VOID else r.text), k
        assert piv == r.pivots, (k, piv, r.pivots)


def _check_record(rec, why, r, cells):
    """one problem's record: served (why == 0) with the oracle's cells and pivots, or handed back for exactly `why`"""
    result, ncell, piv, bits = int(rec[0]), int(rec[1]), int(rec[2]), int(rec[3])
    if why == 0:
        assert (result, bits) == (dte.Q_DONE, 0), rec.tolist()
        assert (ncell, piv, int(rec[5])) == (cells, r.pivots, cells), rec.tolist()
    else:
        assert (result, bits & dte.Q_WHY_MASK, ncell) == (dte.Q_FALLBACK, why, 0), rec.tolist()
        assert int(rec[5]) < dte.SOL_SIZE  # (cells written before it left: within its own tape)


def _alone(name, bits, why):
    """member `name` alone in its call: the oracle's answer with the device tree on and off; the record as `why` says
    (None: any outcome, returned)"""
    from piplib_amd import engine as eng
    p = dte.member(name)
    assert eng.device_tree_fits(p, bits) == 1
    r = _oracle(name, [p], bits)[0]
    e = _engine(True)
    got = _run(e, [p], bits)
    rec = e.debug_device_tree_records()
    _same([p], [r], got)
    assert rec.shape == (1, 6)
    if why is not None:
        _check_record(rec[0], why, r, dte.oracle_figures(p, bits)["cells"])
    assert e.last_device_tree() == ((1, 0) if int(rec[0][0]) != dte.Q_FALLBACK else (0, 1))
    off = _engine(False)
    assert _run(off, [p], bits) == got
    assert off.last_device_tree() == (0, 0)
    assert (off.debug_device_tree_records() == dte.NOT_GIVEN).all()
    return rec[0]


@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("name", sorted(dte.DEVICE))
def test_edge_member_alone(name, bits):
    """fork depth 24 | 25;  new parameters 10 | 11, 4 | 5 at 60 columns, 8 | 9 at 120, 1 | 2 at 127;  cut rows 24 | 25 at 24,
    40, 57 and 104 inequalities, 8 | 9 at 56;  all reserves at once;  49 | 50 parameters;  the tape well clear, at 4088 and
    4095 cells, at 4096 and beyond.
    (Found by this test: the host schedulers answered wide(49, 0, 1), wide(48, 0, 2) and wide(50, 0, 0), which the reference
    abandons with "Too much parameters" -- Tree::node and Forest::advance now fail a solution or a parametric cut at
    PIPAMD_MAXPARM parameters as compa_test does;  and every hand-back carried Q_WHY_OTHER besides its reason.)"""
    _alone(name, bits, dte.DEVICE[name])


@pytest.mark.parametrize("bits", [64, 128])
def test_full_context_member(bits):
    """chain(24, nnew=10, nc=17): CR + 1 == SS == 64, the compa_test sub-problems (up to 62 rows) have two spare slots and
    cut (197 cuts in all).  The answer is the oracle's; a hand-back must carry Q_WHY_ROWS.  Measured on an MI355X: served,
    no why bits, in both widths (no sub-problem needs more than its two spare slots)."""
    rec = _alone("chain24_new10_nc17", bits, None)
    result, why = int(rec[0]), int(rec[3]) & dte.Q_WHY_MASK
    assert (result == dte.Q_DONE and why == 0) or (result == dte.Q_FALLBACK and why & dte.Q_WHY_ROWS), rec.tolist()
    assert (result, why) == (dte.Q_DONE, 0)


def test_recording_is_off_by_default():
    from piplib_amd import engine as eng
    e = eng.Engine(0)
    p = dte.member("new9")
    got = eng.solve_tableaux(e, [p], lockstep=True)
    assert e.last_device_tree() == (1, 0)
    assert e.debug_device_tree_records().shape == (0, 6)
    e.debug_device_tree_record(True)
    assert eng.solve_tableaux(e, [p], lockstep=True) == got
    assert e.debug_device_tree_records().shape == (1, 6)
    e.debug_device_tree_record(False)
    assert eng.solve_tableaux(e, [p], lockstep=True) == got
    assert e.debug_device_tree_records().shape == (0, 6)


@pytest.mark.parametrize("bits", [64, 128])
def test_neighbours_in_one_call(bits):
    """66 members in one call, at its reserve / one past it taking turns (fork depth, cut rows, tape; frames and tapes of
    one launch lie back to back in HBM): every answer its own oracle answer, the records served / handed back alternately
    with the reason of each family, the served count that of the at-reserve members run alone"""
    nb = dte.neighbours()
    probs = [p for p, _ in nb]
    assert len(probs) >= 64
    want = _oracle("neighbours", probs, bits)
    e = _engine(True)
    at = [k for k, (_, a) in enumerate(nb) if a]
    _same([probs[k] for k in at], [want[k] for k in at], _run(e, [probs[k] for k in at], bits))
    alone = e.last_device_tree()
    assert alone == (len(at), 0)
    got = _run(e, probs, bits)
    rec = e.debug_device_tree_records()
    _same(probs, want, got)
    assert rec.shape == (len(probs), 6)
    reason = [dte.Q_WHY_STACK, dte.Q_WHY_ROWS, dte.Q_WHY_TAPE]
    for k, (p, a) in enumerate(nb):
        if a:
            assert (int(rec[k][0]), int(rec[k][3]), int(rec[k][2])) == (dte.Q_DONE, 0, want[k].pivots), (k, rec[k].tolist())
            assert int(rec[k][1]) == dte.oracle_figures(p, bits)["cells"], (k, rec[k].tolist())
        else:
            assert (int(rec[k][0]), int(rec[k][3]) & dte.Q_WHY_MASK) == (dte.Q_FALLBACK, reason[(k % 6) // 2]), (k, rec[k].tolist())
    assert e.last_device_tree() == (alone[0], len(probs) - len(at))
    off = _engine(False)
    assert _run(off, probs, bits) == got
    assert off.last_device_tree() == (0, 0)


@pytest.mark.parametrize("bits", [64, 128])
def test_neighbours_through_traiter_many_dual(bits):
    """pipamd_traiter_many with T_DUAL on rational chains (nq = 0), 24 and 25 forks deep taking turns: cells and pivot
    counts as the host tree has them, the records served / handed back for the fork depth alternately"""
    from piplib_amd import engine as eng
    probs = [dte.chain(24 + (k % 2), nq=0, v=1 + k // 2) for k in range(64)]
    flags = [eng.T_DUAL] * len(probs)
    want = eng.traiter_many(_engine(False), probs, flags, bits=bits)
    assert all(rc == 0 for _, rc, _, _ in want)
    e = _engine(True)
    got = eng.traiter_many(e, probs, flags, bits=bits)
    rec = e.debug_device_tree_records()
    assert got == want
    assert len({str(c) for c, _, _, _ in got}) == len(probs)  # (every tape its own)
    assert rec.shape == (len(probs), 6)
    for k in range(len(probs)):
        want_rec = (dte.Q_DONE, 0) if k % 2 == 0 else (dte.Q_FALLBACK, dte.Q_WHY_STACK)
        assert (int(rec[k][0]), int(rec[k][3]) & dte.Q_WHY_MASK) == want_rec, (k, rec[k].tolist())
        if k % 2 == 0:
            assert int(rec[k][2]) == got[k][3] and int(rec[k][1]) == len(got[k][0]), (k, rec[k].tolist())
    assert e.last_device_tree() == (len(probs) // 2, len(probs) // 2)


@pytest.mark.parametrize("bits", [64, 128])
def test_neighbours_through_pip_solve_many(bits):
    """the 66 neighbours as PolyLib matrices through pipamd_pip_solve_many (tableaux built on the device, the device tree
    run from that buffer): cells, rc, pivots and info as with the device tree off, text and pivots the oracle's, the
    records by input index served / handed back alternately"""
    from piplib_amd import engine as eng
    nb = dte.neighbours()
    probs = [p for p, _ in nb]
    inputs = [eng.PipInput(*dte.pip_matrices(p), -1, eng.PIP_NQ) for p in probs]
    oracle = _oracle("neighbours", probs, bits)
    off = _engine(False)
    want = eng.pip_solve_many(off, inputs, bits=bits)
    assert off.last_device_tree() == (0, 0)
    assert (off.debug_device_tree_records() == dte.NOT_GIVEN).all() and off.debug_device_tree_records().shape == (len(probs), 6)
    e = _engine(True)
    got = eng.pip_solve_many(e, inputs, bits=bits)
    rec = e.debug_device_tree_records()
    assert got == want
    assert rec.shape == (len(probs), 6)
    reason = [dte.Q_WHY_STACK, dte.Q_WHY_ROWS, dte.Q_WHY_TAPE]
    for k, ((p, a), r, (cells, rc, st, piv, info)) in enumerate(zip(nb, oracle, got)):
        assert (info["nvar"], info["nparm"], info["ni"], info["nc"]) == (p.nvar, p.nparm, p.ni, p.nc), k
        if r.status == pb.ST_ABORT:
            assert rc == -5 and not a, (k, rc, st)
        else:
            assert rc == 0 and piv == r.pivots, (k, rc, st, piv, r.pivots)
            assert pb.squash(eng.tape_text(cells)) == pb.squash(r.text), k
        if a:
            assert (int(rec[k][0]), int(rec[k][3]), int(rec[k][2]), int(rec[k][1])) == (dte.Q_DONE, 0, piv, len(cells)), (k, rec[k].tolist())
        else:
            assert (int(rec[k][0]), int(rec[k][3]) & dte.Q_WHY_MASK) == (dte.Q_FALLBACK, reason[(k % 6) // 2]), (k, rec[k].tolist())
    assert e.last_device_tree() == (len(probs) // 2, len(probs) // 2)
