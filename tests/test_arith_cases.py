"""What tests/test_gpu_arith_probe.py rests on, checked without a device: bigint_pip's lifted row_update / det_update are
pivot_step's arithmetic, the wrap-around addition to the model agrees with the plain model wherever nothing wraps, and
the row-case lists are deterministic, within their cap, inside every path's preconditions and on every width threshold."""
import math

import numpy as np
import pytest

import bigint_pip as bp
import test_gpu_arith_probe as P

LISTS = sorted({(fam, WP) for _, _, WP, fam, _ in P.PATHS.values()})


def test_row_and_det_update_are_pivot_steps_arithmetic(monkeypatch):
    """on seeded tableaux, every row and every limb pivot_step leaves is what row_update / det_update give on the state
    before the pivot"""
    real = bp.pivot_step
    seen = [0, 0]

    def spy(rows, det, pivi, nvar, ni, st):
        nligne = nvar + ni
        before = [(r.flag, r.den, None if r.v is None else r.v.copy()) for r in rows[:nligne]]
        det0 = list(det)
        pivj = bp.pick_column(rows, pivi, nvar, nligne, bp.Stats(st.bits))
        over = False
        try:
            rc = real(rows, det, pivi, nvar, ni, st)
        except bp.Overflow:
            over = True
        if pivj < 0:
            assert rc == -1
            return rc
        prow, dpiv = before[pivi][2], before[pivi][1]
        pivot = int(prow[pivj])
        try:
            bp.det_update(det0, pivot, dpiv, st.bits)
            assert not over and det0 == list(det)
        except bp.Overflow:
            assert over
            raise
        for k in range(nligne):
            flag, den, v = before[k]
            if (flag & bp.UNIT) or k == pivi:
                continue
            z, newden, lpiv, foo = bp.row_update(v.copy(), den, prow, pivot, dpiv, pivj)
            d = math.gcd(pivot, int(v[pivj]))
            assert (lpiv, foo) == (pivot // d, int(v[pivj]) // d)
            assert newden == rows[k].den and [int(x) for x in z] == [int(x) for x in rows[k].v]
            seen[0] += 1
        seen[1] += 1
        return rc
    monkeypatch.setattr(bp, "pivot_step", spy)
    rng = np.random.default_rng(5)
    for trial in range(12):
        nvar, ni = int(rng.integers(2, 7)), int(rng.integers(3, 9))
        ineq = rng.integers(-9, 10, size=(ni, nvar + 1))
        ineq[:, nvar] = rng.integers(-30, 60, size=ni)
        bp.solve(ineq, integer=True, bits=64)
    assert seen[1] > 30 and seen[0] > 150


@pytest.mark.parametrize("fam,WP", LISTS)
def test_row_case_lists(fam, WP):
    f = P.FAMILY[fam]
    W = f["W"]
    cases = P.cases_of(fam, WP)
    assert 200 <= len(cases) <= P.ROW_CASE_CAP
    if WP == min(wp for fm, wp in LISTS if fm == fam):
        again = P.row_cases(fam, WP)   # deterministic: plain functions of fixed seeds
        assert [(c["v"], c["prow"], c["den"], c["dpiv"], c["pivj"]) for c in again] == \
               [(c["v"], c["prow"], c["den"], c["dpiv"], c["pivj"]) for c in cases]
    seen_B, seen_gb, fitting, wrapping, not_ok, rounds = set(), set(), 0, 0, 0, set()
    pivjs, seen_g0 = set(), set()
    for c in cases:
        assert len(c["v"]) == WP and len(c["prow"]) == WP
        assert P.preconditions_hold(c, fam), c["tag"]
        lpiv, foo = P.multipliers(c)
        assert math.gcd(lpiv, foo) == 1 and lpiv >= 1
        ok, nd, z, B = P.wrap_row_model(c, W)
        g0 = P.signed(lpiv * c["den"], W)
        # the model's own identities: one positive g with g z' == z (the W-bit z before the division) and g newden == g0,
        # and nothing left to divide
        zpre = [P.signed(P.signed(a * lpiv, W) - P.signed(b * foo, W), W) for a, b in zip(c["v"], c["prow"])]
        zpre[c["pivj"]] = P.signed(c["dpiv"] * foo, W)
        assert B == max(abs(x) for x in zpre).bit_length()
        if ok:
            g = math.gcd(g0, *zpre)
            assert g >= 1 and [g * x for x in z] == zpre and g * nd == g0
            assert math.gcd(nd, *z) == 1
        else:
            not_ok += 1
            assert g0 == 0 and not any(zpre) and nd == 0 and not any(z)
        if P.case_fits(c, W):
            fitting += 1
            pok, pnd, pz, plpiv, pfoo = P.plain_row_model(c)   # the authority: bigint_pip.row_update
            assert (pok, pnd, pz) == (ok, nd, z) and (plpiv, pfoo) == (lpiv, foo), c["tag"]
            assert P.row_model(c, W) == (ok, nd, z)
        else:
            wrapping += 1
        seen_B.add(B)
        gstart = math.gcd(abs(g0), abs(zpre[c["pivj"]]))
        seen_gb.add((B, gstart.bit_length()))
        if foo:
            seen_g0.add((B, abs(g0).bit_length() > 32, abs(g0).bit_length() > 64))
        pivjs.add(c["pivj"])
        if c["wantB"] is not None and "grid" in c["tag"]:
            rounds.add(c["tag"].split(" r")[-1][:1])
    # every threshold holds a case with B exactly there
    assert set(f["thresholds"]) <= seen_B, sorted(set(f["thresholds"]) - seen_B)
    # ... crossed with the bit length of the starting g at 32 / 33 (64 / 65 for 128-bit entries), wherever the path's
    # operands can hold such a g: within the entries (g <= |z|), or as a denominator over foo = 0
    for B in f["thresholds"]:
        for gb in (32, 33) + ((64, 65) if W == 128 else ()):
            full = B > min(f["row"], W - 1) + min(f["mul"], W - 1)   # both products at full size: g0 = lpiv * den has mul + gb bits
            if (gb < B and not (full and min(f["mul"], W - 1) + gb > min(f["g0"], W - 1))) or \
                    (f["g0"] >= gb + 1 and B <= min(f["row"], W - 1)):
                assert (B, gb) in seen_gb, (B, gb)
        # ... and with a denominator product beyond 32 (64) bits over a full update's entries
        assert any(b == B and w32 for b, w32, _ in seen_g0), B
        assert W == 64 or f["g0"] < 66 or any(b == B and w64 for b, _, w64 in seen_g0), B
    assert set(P.lane_positions(W, WP)) <= pivjs
    assert not_ok >= 1 and fitting > 100
    if f["row"] == W or fam in ("LI_M", "LL_M"):
        assert wrapping >= 20
    else:
        assert wrapping == 0
    assert {"0", "1", "2", "3", "4"} <= rounds


def test_ladder_cases_meet_the_general_paths_preconditions():
    """a case of a specialised path is a case of every path it is also run through"""
    for path, (_, W, WP, fam, ladder) in P.PATHS.items():
        for other in ladder:
            _, W2, WP2, fam2, _ = P.PATHS[other]
            assert (W2, WP2) == (W, WP)
            assert all(P.preconditions_hold(c, fam2) for c in P.cases_of(fam, WP)), (path, other)


def test_scalar_case_lists():
    for W, sv in ((32, False), (64, False), (64, True), (128, False), (128, True)):
        ps = P.pair_cases(W, sv, 1)
        assert ps == P.pair_cases(W, sv, 1)
        firsts = {a for a, _ in ps}
        for k in range(W if sv else W + 1):
            for x in ((1 << k) - 1, 1 << k, (1 << k) + 1):
                if (x < (1 << (W - 1))) if sv else (x < (1 << W)):
                    assert x in firsts, (W, sv, k)
        if sv:
            assert -(1 << (W - 1)) in firsts and (-(1 << (W - 1)), -1) in ps
    cs = P.tiny_cases(2, 3)
    assert cs.shape == (12 * ((1 << 20) - 2), 2) and (cs[:, 0] < (1 << 20)).all()
