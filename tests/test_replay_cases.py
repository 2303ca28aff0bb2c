"""CPU: the case lists of the determinant-replay probe (tests/replay_cases.py) hold every class they promise -- by what
tests/replay_model.py says of each case, not by what the builder meant -- and the model classifies every admitted case,
so that tests/test_gpu_det_replay_probe.py drops none at run time."""
import math

import pytest

import replay_cases as rc
import replay_model as rm


def walked(c):
    """the pairs of a case a replay walks: up to and including the first overflow"""
    k, _ = rm.first_overflow(c["limbs"], c["ldet"], c["log"], c["bits"])
    return c["log"] if k is None else c["log"][:k + 1]


@pytest.mark.parametrize("W", [64, 128])
def test_every_case_is_admitted_and_classified(W):
    for c in rc.pool(W):
        assert c["bits"] == W and len(c["limbs"]) == 4 and 1 <= c["ldet"] <= 3
        assert all(-(1 << (W - 1)) <= x < (1 << (W - 1)) for x in c["limbs"])
        assert len(c["log"]) + len(c["tail"]) <= rm.DETLOG and c["npiv"] >= len(c["log"])
        assert all(0 < pp < (1 << (W - 1)) and 0 < dp < (1 << (W - 1)) for pp, dp in c["log"] + c["tail"])
        limbs, ldet, npiv, status, nlog = rm.replay(c["limbs"], c["ldet"], c["npiv"], c["status"], c["log"], W, c["aux"])
        assert nlog == 0 and 1 <= ldet <= 4 and len(limbs) == 4
        assert all(-(1 << (W - 1)) <= x < (1 << (W - 1)) for x in limbs)
        assert limbs[min(ldet, 4):] == tuple(c["limbs"][min(ldet, 4):])  # what is not in use stays
        if status != rm.ST_OVERFLOW or c["status"] == rm.ST_OVERFLOW:
            assert (npiv, status) == (c["npiv"], c["status"])
        else:
            unlogged = (c["status"], c["aux"]) == (rm.ST_NIL, rm.AUX_NOCOLUMN)
            k, _ = rm.first_overflow(c["limbs"], c["ldet"], c["log"], W)
            assert npiv == c["npiv"] - unlogged - len(c["log"]) + k + 1 >= 1
        assert len(rc.job_words(c)) == rc.HDR + rc.LOGWORDS


@pytest.mark.parametrize("W", [64, 128])
def test_log_lengths_and_overflow_places(W):
    cs = rc.pool(W)
    clean = [c for c in cs if rm.first_overflow(c["limbs"], c["ldet"], c["log"], W)[0] is None]
    assert {len(c["log"]) for c in clean} >= set(rc.LENGTHS)
    seen = set()
    for c in cs:
        k, why = rm.first_overflow(c["limbs"], c["ldet"], c["log"], W)
        if k is None:
            continue
        n = len(c["log"])
        seen.add((k, why))
        if k == n - 1:
            seen.add(("last", why))
            if n == rm.DETLOG:
                seen.add(("last of a full log", why))
        if n - k > 3:
            # the state at the failing step; walking the next pair from it would change the limbs (a missing stop shows),
            # and a later pair would overflow again (the LAST overflow winning shows in the pivot count)
            limbs, ldet, _, _, _ = rm.replay(c["limbs"], c["ldet"], c["npiv"], c["status"], c["log"][:k + 1], W)
            nxt = rm.replay(limbs, min(ldet, 3), 0, 0, c["log"][k + 1:k + 2], W)
            later = [j for j in range(k + 1, n) if rm.first_overflow(limbs, min(ldet, 3), c["log"][j:j + 1], W)[0] == 0]
            if later and (nxt[0] != limbs or nxt[1] != min(ldet, 3)):
                seen.add((k, why, "pairs behind it"))
    for at in rc.OVERFLOW_AT:
        for why in ("factor", "limb"):
            assert (at, why) in seen, (at, why)
            if at != "last":
                assert (at, why, "pairs behind it") in seen, (at, why)
    assert ("last of a full log", "factor") in seen and ("last of a full log", "limb") in seen


@pytest.mark.parametrize("W", [64, 128])
def test_starting_states_and_pairs(W):
    cs = rc.pool(W)
    edges = {(c["ldet"], c["limbs"][c["ldet"] - 1].bit_length()) for c in cs if c["log"]}
    assert edges >= {(n, b) for n in (1, 2, 3) for b in (W - 2, W - 1)}
    # a pivot of one bit fits a last limb of W - 2 bits and one of W - 1 bits no more, a pivot of two bits neither
    # (log2 + log2 < B): limbs grown behind the first pair, behind the second
    grew = {(c["ldet"], c["limbs"][c["ldet"] - 1].bit_length() - W) +
            tuple(rm.replay(c["limbs"], c["ldet"], 0, 0, c["log"][:n], W)[1] - c["ldet"] for n in (1, 2))
            for c in cs if len(c["log"]) == 9 and c["log"][:2] == [(1, 1), (2, 1)]}
    assert grew == {(1, -2, 0, 1), (1, -1, 1, 1), (2, -2, 0, 1), (2, -1, 1, 1), (3, -2, 0, 1), (3, -1, 1, 1)}, grew
    over = {(c["status"], rm.replay(c["limbs"], c["ldet"], c["npiv"], c["status"], c["log"], W)[3] == rm.ST_OVERFLOW)
            for c in cs if c["log"]}
    assert over == {(s, o) for s in rc.STATUSES for o in (False, True)}
    # the last pivot counted and not logged (ST_NIL, aux -1) with an overflow in the log and without; the same aux under
    # another status, where it means nothing; ST_NIL without it
    marks = {(c["status"] == rm.ST_NIL, c["aux"] == rm.AUX_NOCOLUMN,
              rm.first_overflow(c["limbs"], c["ldet"], c["log"], W)[0] is not None) for c in cs if c["log"]}
    assert marks == {(n, a, o) for n in (False, True) for a in (False, True) for o in (False, True)}, marks
    for o in (False, True):  # a pivot count beyond the log, as earlier, already replayed launches leave it
        assert any(c["npiv"] > len(c["log"]) + 1 and c["log"] and
                   (rm.first_overflow(c["limbs"], c["ldet"], c["log"], W)[0] is not None) == o for c in cs)
    kinds = set()
    for c in cs:
        for pp, dp in walked(c):
            g = math.gcd(pp, dp)
            if dp == 1:
                kinds.add("dp 1")
            elif g == 1:
                kinds.add("coprime")
            elif g == dp:
                kinds.add("gcd dp")
            elif g == pp:
                kinds.add("gcd pp")
            else:
                kinds.add("gcd other")
            for x in (pp, dp):
                if W == 128:
                    kinds.add("low word 0" if x & rc.M64 == 0 else ("high word 0" if x >> 64 == 0 else "both words"))
    want = {"dp 1", "coprime", "gcd dp", "gcd pp", "gcd other"}
    assert kinds >= (want | {"low word 0", "high word 0", "both words"} if W == 128 else want), kinds


@pytest.mark.parametrize("W", [64, 128])
def test_launches(W):
    ls = rc.launches(W)
    assert {len(l["jobs"]) for l in ls if l["list"] is None} == set(rc.JOBS)
    used = {id(c) for l in ls if l["list"] is None for c in l["jobs"] if c["bits"] == W}
    assert used == {id(c) for c in rc.pool(W)}  # no case dropped
    alien = [c for l in ls for c in l["jobs"] if c["bits"] != W]
    assert any(c["log"] and rm.first_overflow(c["limbs"], c["ldet"], c["log"], c["bits"])[0] is not None for c in alien)
    listed = [l for l in ls if l["list"] is not None]
    assert {len(l["jobs"]) for l in listed} == {65, 130}
    for l in listed:
        lst = l["list"]
        assert len(set(lst)) == len(lst) < len(l["jobs"]) and lst != sorted(lst) and lst != sorted(lst, reverse=True)
        off = [c for j, c in enumerate(l["jobs"]) if j not in lst and c["bits"] == W and c["log"]]
        on = [c for j, c in enumerate(l["jobs"]) if j in lst and c["bits"] == W and c["log"]]
        assert off and on
        assert any(rm.first_overflow(c["limbs"], c["ldet"], c["log"], W)[0] is not None for c in off)
    for l in ls:
        want = rc.expected(l)
        assert len(want) == len(l["jobs"]) and all(len(w) == rc.NOUT for w in want)
        changed = sum(w != rc.untouched(c) for w, c in zip(want, l["jobs"]))
        assert changed or len(l["jobs"]) == 1


@pytest.mark.parametrize("W", [64, 128])
def test_carry_pairs(W):
    ps = rc.carry_pairs(W)
    ends = set()
    for a, b, tail in ps:
        assert rm.first_overflow(a["limbs"], a["ldet"], a["log"], W)[0] is None
        assert 0 < len(b) and len(b) + len(tail) <= rm.DETLOG
        assert all(0 < pp < (1 << (W - 1)) and 0 < dp < (1 << (W - 1)) for pp, dp in b + tail)
        k, why = rm.first_overflow(a["limbs"], a["ldet"], a["log"] + b, W)
        assert k is None or k >= len(a["log"])
        ends.add(why)
        # the limbs A leaves are not the ones it found: the second replay starts from what the first one stored
        mid = rm.replay(a["limbs"], a["ldet"], a["npiv"], a["status"], a["log"], W)
        assert mid[0] != tuple(a["limbs"]) or mid[1] != a["ldet"] or len(a["log"]) < 2
    assert ends == {None, "factor", "limb"}
    assert any(len(a["log"]) == rm.DETLOG for a, _, _ in ps) and any(len(a["log"]) + len(b) == rm.DETLOG for a, b, _ in ps)
