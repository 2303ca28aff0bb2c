"""CPU: the replay model against the CPU oracle on tableaux the oracle ends in its "Integer overflow" abort, and the
stored records of tests/golden/replay_model.json against the model that made them (a sample a family; the whole file
takes minutes, tests/golden/make_replay_fixtures.py).

bigint_pip.solve(bits=64) walks the same determinant as the oracle's long long build; its pivot count at the abort must
be the oracle's wherever nothing had wrapped before (Stats.exact).  On dense10 / dense14 (tests/golden/
make_bigint_fixtures.FAMILIES) that is the case on NO aborted tableau: their entries pass 2^63 long before three limbs
are full, and the oracle's abort is the wrapped arithmetic's (a denominator with a factor no limb holds).  The sparse
families of tests/replay_fixture.py are the ones whose determinant outgrows its limbs in exact arithmetic."""
import math
import os
import sys

import numpy as np
import pytest

import bigint_pip as bp
import pipbatch as pb
import replay_fixture as rf
import replay_model as rm
from piplib_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))


def oracle(rows):
    nvar = rows.shape[2] - 1
    probs = [synth.Problem(nvar, 0, rows.shape[1], 0, -1, 1, rows[b], np.zeros((0, 1), np.int64)) for b in range(rows.shape[0])]
    return pb.run_batch(pb.ORACLEPIP, probs, pb.F_NOSIMPLIFY | pb.F_NOTEXT).results


@pytest.mark.parametrize("family", ["dense10", "dense14"])
def test_model_counts_the_oracles_pivots_up_to_the_abort(family):
    from make_bigint_fixtures import FAMILIES, rows_of
    assert family in FAMILIES
    rows = rows_of(family)
    o = oracle(rows)
    aborted = [k for k, r in enumerate(o) if r.status == pb.ST_ABORT]
    assert len(aborted) >= 10 and all(o[k].abort_code == 2 for k in aborted)
    held = 0
    for k in aborted:
        m = bp.solve(rows[k], integer=True, bits=64, stop_inexact=True)
        if m.stats.exact:  # nothing wrapped up to here: the model is where the oracle is
            assert m.status == bp.ST_OVERFLOW and m.pivots == o[k].pivots, (family, k, m.status, m.pivots, o[k].pivots)
            held += 1
        else:
            assert m.pivots <= o[k].pivots, (family, k)  # ... the oracle went on with wrapped values
    print("%s: %d of %d aborted tableaux exact up to the abort" % (family, held, len(aborted)))


@pytest.mark.parametrize("name", sorted(rf.SCREEN))
def test_screen_records(name):
    rec = rf.doc()["screen"][name]
    rows = rf.rows_of(rf.SCREEN[name])
    o = oracle(rows)
    aborted = [k for k, r in enumerate(o) if r.status == pb.ST_ABORT and r.abort_code == 2]
    assert aborted == rec["aborted"] and len(aborted) >= 15
    exact = rf.exact_aborts(name)
    assert set(exact) <= set(aborted)
    for k, p in exact.items():
        assert o[k].pivots == p, (name, k)
    if name in rf.COUNTED:  # a condition on the families the pivot-count checks are about, not a measurement
        assert 4 * len(exact) >= 3 * len(aborted), (name, len(exact), len(aborted))
    # re-derived: the first admitted tableaux, and the first one left out (the dense ones take seconds each)
    for k in sorted(exact)[:3]:
        m = bp.solve(rows[k], integer=True, bits=64, stop_inexact=True)
        assert m.status == bp.ST_OVERFLOW and m.stats.exact and m.pivots == exact[k], (name, k)
        # ... and the replay of its log ends where it ended
        limbs, ldet, npiv, status, _ = rm.replay((1, 0, 0, 0), 1, len(m.stats.det_log), rm.ST_RUN, m.stats.det_log, 64)
        assert (status, npiv) == (rm.ST_OVERFLOW, m.pivots) and rm.first_overflow((1, 0, 0, 0), 1, m.stats.det_log, 64)[1] == "limb"
    out = [k for k in aborted if k not in exact][:1]
    for k in out:
        m = bp.solve(rows[k], integer=True, bits=64, stop_inexact=True)
        assert m.status is None and not m.stats.exact, (name, k)
    print("%s: %d aborted, %d held to the pivot count, %d left out by the exactness screen" % (
        name, len(aborted), len(exact), len(aborted) - len(exact)))


@pytest.mark.parametrize("name", sorted(rf.HEADERS))
def test_header_records(name):
    rows = rf.rows_of(rf.HEADERS[name])
    for bits in (64, 128):
        recs = rf.headers(name, bits)
        assert len(recs) == rows.shape[0] and sum(r is not None for r in recs) >= 4
        for k in sorted((k for k, r in enumerate(recs) if r is not None), key=lambda k: recs[k][1])[:2]:  # the shortest runs
            det = []
            m = bp.solve(rows[k], integer=True, bits=bits, det_out=det, stop_inexact=True)
            status, pivots, ldet, limbs = recs[k]
            assert m.stats.exact and (m.status, m.pivots) == (status, pivots), (name, bits, k)
            # the limbs solve() itself walked are the replay's of the log it kept
            n = 3 if status == bp.ST_OVERFLOW else ldet  # (the fourth limb that overflows is counted and never stored)
            assert det == limbs[:n] and limbs[n:] == [0] * (4 - n), (name, bits, k)
    # the two widths walk one log: where both are exact the determinant is one number, split differently
    both = [(a, b) for a, b in zip(rf.headers(name, 64), rf.headers(name, 128)) if a and b and a[0] != bp.ST_OVERFLOW]
    assert both
    for a, b in both:
        assert a[:2] == b[:2] and math.prod(a[3][:a[2]]) == math.prod(b[3][:b[2]])
