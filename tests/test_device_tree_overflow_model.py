"""The overflow families of tests/device_tree_overflow.py on the CPU: at its flip point M each family's chain of step models
leaves 64 bits first in the step the family is named after, with M - 1 nothing leaves 64 bits, at 128 bits nothing does
either way; and the chain's answer and pivot count are the 128-bit oracle's on every member.  No GPU."""
import math

import pytest

import bigint_pip as bp
import device_tree_overflow as dto
import pipbatch as pb

MEMBERS = dto.members()


def test_a_dozen_members_in_pairs():
    assert len(MEMBERS) == 2 * len(dto.FAMILIES) == 12
    assert {f[3] for f in dto.FAMILIES.values()} == {"tournament", "elimination", "determinant"}
    for name, (p, family, M, at) in MEMBERS.items():
        assert p.nparm == 0 and p.nc == 0 and p.nvar <= 4 and p.ni <= 4
        assert max(abs(int(x)) for x in p.ineq.ravel()) == M, name
        if p.nq:   # tab_simplify (integer problems) must find nothing to divide: the chain starts from the rows as given
            assert all(math.gcd(*[int(x) for x in r[:-1]]) == 1 for r in p.ineq), name


@pytest.mark.parametrize("name", sorted(MEMBERS))
def test_chain_classes(name):
    p, family, M, at = MEMBERS[name]
    c64, c128 = dto.chain(p, 64), dto.chain(p, 128)
    assert c128.cls == "fits"
    if at:
        assert (c64.cls, c64.stage) == ("must", dto.FAMILIES[family][3])
    else:
        assert c64.cls == "fits"
        assert (c64.status, c64.pivots, c64.cuts, c64.num, c64.den) == (c128.status, c128.pivots, c128.cuts, c128.num, c128.den)


def test_chain_equals_the_128_bit_oracle():
    names = sorted(MEMBERS)
    want = pb.run_batch(pb.ORACLEPIP128, [MEMBERS[n][0] for n in names]).results
    for name, r in zip(names, want):
        c = dto.chain(MEMBERS[name][0], 128)
        assert r.status != pb.ST_ABORT and r.pivots == c.pivots, (name, r.pivots, c.pivots)
        text = "()" if c.status == bp.ST_NIL else bp.solution_text(c.num, c.den)
        assert pb.squash(r.text) == pb.squash(text), name
