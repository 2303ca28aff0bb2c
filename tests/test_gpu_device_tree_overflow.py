"""-m gpu: the device-resident traiter() (piplib_amd/csrc/pip_quast.hip) on whole problems at its 64-bit overflow line, the
pairs of tests/device_tree_overflow.py: at the flip point the chain of step models leaves 64 bits in the pivot-column
tournament, in the elimination, or in the determinant's limbs; one below it nothing does.

Every member runs alone in its call, as in tests/test_gpu_device_tree_edges.py.  At 64 bits the device tree's record says
served, or handed back with exactly Q_WHY_OVERFLOW, as the chain predicts; at 128 bits every member is served.  Text and
pivot count are the CPU oracle's of that width, and the same with the device tree off.  The chain itself is held to the
128-bit oracle without a device in tests/test_device_tree_overflow_model.py."""
import pytest

import device_tree_edges as dte
import device_tree_overflow as dto
import pipbatch as pb

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

MEMBERS = dto.members()
_ENGINES, _ORACLE = {}, {}


def _engine(tree):
    from piplib_amd import engine as eng
    if tree not in _ENGINES:
        e = eng.Engine(0)
        e.set_device_tree(tree)
        e.debug_device_tree_record(True)
        _ENGINES[tree] = e
    return _ENGINES[tree]


def _oracle(bits):
    """the CPU oracle's results for every member, computed once per width"""
    if bits not in _ORACLE:
        names = sorted(MEMBERS)
        res = pb.run_batch(pb.ORACLEPIP if bits == 64 else pb.ORACLEPIP128, [MEMBERS[n][0] for n in names]).results
        _ORACLE[bits] = dict(zip(names, res))
    return _ORACLE[bits]


def _run(e, probs, bits):
    from piplib_amd import engine as eng
    if bits == 128:
        return eng.solve_tableaux_lockstep128(e, probs)
    return eng.solve_tableaux(e, probs, lockstep=True)


@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("name", sorted(MEMBERS))
def test_overflow_member_alone(name, bits):
    from piplib_amd import engine as eng
    p, family, M, at = MEMBERS[name]
    c = dto.chain(p, bits)
    assert c.cls == ("must" if at and bits == 64 else "fits")
    assert eng.device_tree_fits(p, bits) == 1
    r = _oracle(bits)[name]
    e = _engine(True)
    got = _run(e, [p], bits)
    rec = e.debug_device_tree_records()
    assert rec.shape == (1, 6)
    result, ncell, piv, why = int(rec[0][0]), int(rec[0][1]), int(rec[0][2]), int(rec[0][3])
    print("%s at %d bits: record %s, chain %s %s" % (name, bits, rec[0].tolist(), c.cls, c.stage))
    if c.cls == "must":
        assert (result, why & dte.Q_WHY_MASK, ncell) == (dte.Q_FALLBACK, dte.Q_WHY_OVERFLOW, 0), rec[0].tolist()
        assert e.last_device_tree() == (0, 1)
    else:
        assert (result, why, piv) == (dte.Q_DONE, 0, c.pivots), rec[0].tolist()
        assert e.last_device_tree() == (1, 0)
    (text, rc, st, pv), = got
    if r.status == pb.ST_ABORT:
        assert rc == -5, (rc, st)
    else:
        assert rc == 0 and pv == r.pivots, (rc, st, pv, r.pivots)
        assert pb.squash(text) == pb.squash("void\n" if r.status == pb.ST_VOID else r.text)
        if c.cls == "fits":
            assert pv == c.pivots
    off = _engine(False)
    assert _run(off, [p], bits) == got
    assert off.last_device_tree() == (0, 0)
