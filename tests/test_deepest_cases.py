"""What tests/test_gpu_deepest_cut.py rests on, checked without a device: the case list of tests/deepest_cases.py is
deterministic and inside its search space, every tag holds a case (and a case exact at 64 bits where the tag allows one),
every case's first deepest cut is another row than the plain cut of the same state, the embedding in wide rows leaves the
model's pivots, cuts and solution alone, and the model -- tests/bigint_pip.py with deepest=True -- is the CPU oracles' and,
where it is built, the reference's own answer on every case at every width of the list."""
import numpy as np
import pytest

import bigint_pip as bp
import deepest_cases as dc
import pipbatch as pb

FLAGS = pb.F_DEEPEST | pb.F_NOSIMPLIFY
IDS = range(len(dc.cases()))
IDS64 = [k for k in IDS if dc.cases()[k].exact64]


def _small(k):
    s = dc.cases()[k]
    r = s.res
    return r.status, r.pivots, r.cuts, list(r.stats.cut_log), None if r.sol_num is None else (r.sol_num, r.sol_den)


def test_the_list_is_deterministic_small_and_inside_the_search_space():
    cs = dc.cases()
    assert 16 <= len(cs) <= 64
    dc.cases.cache_clear()
    again = dc.cases()
    assert [(s.ineq, s.tags, s.exact64) for s in again] == [(s.ineq, s.tags, s.exact64) for s in cs]
    for s in cs:
        assert dc.in_search_space(s.ineq), s.ineq
        assert s.res.stats.exact and s.res.stats.bits == 128 and s.res.cuts >= 1 and len(s.res.stats.cut_log) == s.res.cuts
        assert s.res.status in (bp.ST_SOLUTION, bp.ST_NIL)
    # a pinned draw is a draw: inside the space, kept, and in the list
    for m in dc.PINNED:
        assert dc.in_search_space(m) and dc.keep(m) is not None and any(s.ineq == m for s in cs)
    # the 64-bit verdict is the whole run's, not the truncated one's
    for s in cs:
        assert bp.solve(s.ineq, bits=64, deepest=True).stats.exact == s.exact64


@pytest.mark.parametrize("tag", dc.TAGS)
def test_every_tag_holds_a_case(tag):
    have = [s for s in dc.cases() if tag in s.tags]
    assert have, tag
    if tag in dc.TAGS_64:
        assert any(s.exact64 for s in have), tag
    else:
        assert not any(s.exact64 for s in have), tag


def test_tags_say_what_the_cut_log_says():
    for s in dc.cases():
        log = s.res.stats.cut_log
        for D, delta, lam, rounds, big in log:
            assert D > 1 and D % delta == 0 and 0 < lam and __import__("math").gcd(lam, D) == 1
        assert ("prod>63" in s.tags) == any(big > 63 for *_, big in log)
        assert ("delta>1" in s.tags) == any(delta > 1 for _, delta, *_ in log)
        assert ("rounds>=2" in s.tags) == any(r >= 2 for *_, r, _ in log)
        assert ("rounds=1" in s.tags) == any(r == 1 for *_, r, _ in log)
        assert ("cuts>=2" in s.tags) == (len(log) >= 2)
        assert ("nil" in s.tags) == (s.res.status == bp.ST_NIL)
        if s.exact64:
            assert "prod>63" not in s.tags


def test_integrers_own_nil_exit_is_out_of_reach():
    """integrer.c:482-485 case (b) cannot happen without parameters (deepest_cases' docstring has the argument): no draw
    of the search ends there, so the list's "nil" cases are the pivot rows without a positive coefficient"""
    ends = 0
    for m in dc.draws():
        r = bp.solve(m, bits=128, deepest=True, stop_inexact=True)
        assert not r.stats.nil_cut, m
        ends += r.status == bp.ST_NIL and r.cuts >= 1
    assert ends >= 20


def test_the_first_deepest_cut_is_not_the_plain_cut(monkeypatch):
    """up to its first cut a solve is the same with and without the option; there the deepest cut is another row in every
    case, and for most cases the pivot or cut count of the whole solve differs too: a kernel that ignored PIPAMD_T_DEEPEST
    cannot pass"""
    real = bp.deepen
    seen = []

    def spy(cut, D, nvar, need, on_round=None):
        before = list(cut)
        out = real(cut, D, nvar, need, on_round)
        seen.append((before, list(cut), D, out[0]))
        return out
    monkeypatch.setattr(bp, "deepen", spy)
    counts_differ = 0
    for s in dc.cases():
        del seen[:]
        r = bp.solve(s.ineq, bits=128, deepest=True)
        before, after, D, lam = seen[0]
        assert lam % D != 1 and before != after, s.ineq
        assert all(0 <= x < D for x in after[:dc.NV]) and -D <= after[dc.NV] < 0
        plain = bp.solve(s.ineq, bits=128, deepest=False)
        assert not plain.stats.cut_log
        counts_differ += (plain.pivots, plain.cuts) != (r.pivots, r.cuts)
    assert counts_differ >= len(dc.cases()) // 4


@pytest.mark.parametrize("bits", (64, 128))
def test_embedding_leaves_the_model_alone(bits):
    """in every nvar of the list: status, pivot count, cut count, cut log and the active unknowns' solution are those of
    the small tableau, the unknowns of the zero columns stay 0, and the width verdict is the small tableau's"""
    for nvar in dc.NVAR[bits]:
        cols = dc.columns(nvar, dc.CW[bits])
        assert sorted(set(cols)) == list(cols) and cols[0] == 0 and cols[3] == nvar - 1 and cols[2] == cols[1] + 1
        for k in (IDS64 if bits == 64 else IDS):
            r = dc.model(k, nvar, bits)
            assert r.stats.exact, (k, nvar)
            assert dc.project(r, nvar, dc.CW[bits]) == _small(k), (k, nvar)
    # the block boundary is used wherever the row has one that leaves the four columns apart
    assert dc.columns(255, 128) == (0, 127, 128, 254) and dc.columns(510, 128) == (0, 383, 384, 509)
    assert dc.columns(127, 64) == (0, 63, 64, 126) and dc.columns(510, 64) == (0, 447, 448, 509)


def test_the_widest_row_is_the_engines():
    """NVAR_MAX is read off the code: integrer() refuses nvar + 1 >= PIPAMD_MAXCOL columns"""
    import os
    import re
    src = open(os.path.join(pb.ROOT, "piplib_amd", "csrc", "pip_job.h")).read()
    assert int(re.search(r"#define PIPAMD_MAXCOL (\d+)", src).group(1)) == dc.MAXCOL
    adv = open(os.path.join(pb.ROOT, "piplib_amd", "csrc", "pip_advance.h")).read()
    assert "if (ncol >= PIPAMD_MAXCOL) {\n          status = PIPAMD_ST_MAXCOL;" in adv
    assert dc.NVAR[64][-1] == dc.NVAR[128][-1] == dc.MAXCOL - 2


def _problems(ids, nvar, bits):
    from piplib_amd import synth
    return [synth.Problem(nvar, 0, dc.NI, 0, -1, 1, dc.embed(dc.cases()[k].ineq, nvar, dc.CW[bits]), np.zeros((0, 1), np.int64))
            for k in ids]


def _same(results, ids, nvar, bits):
    assert len(results) == len(ids)
    for k, r in zip(ids, results):
        m = dc.model(k, nvar, bits)
        assert r.status == pb.ST_OK, (k, nvar, r.status, r.abort_code)
        assert r.pivots == m.pivots, (k, nvar, r.pivots, m.pivots)
        want = "()" if m.status == bp.ST_NIL else pb.squash(bp.solution_text(m.sol_num, m.sol_den))
        assert pb.squash(r.text) == want, (k, nvar)


@pytest.mark.parametrize("nvar", dc.NVAR[64])
def test_model_is_the_64_bit_oracle_and_the_reference(nvar):
    """every case exact at 64 bits: status, pivot count and solution text of oraclepip, and of the reference's own 64-bit
    build where it is here, under the deepest-cut option"""
    assert len(IDS64) >= 8
    probs = _problems(IDS64, nvar, 64)
    _same(pb.run_batch(pb.ORACLEPIP, probs, FLAGS).results, IDS64, nvar, 64)
    if pb.have_ref():
        _same(pb.run_batch(pb.REFPIP, probs, FLAGS).results, IDS64, nvar, 64)


@pytest.mark.parametrize("nvar", dc.NVAR[128])
def test_model_is_the_128_bit_oracle(nvar):
    """every case: exact at 128 bits, and oraclepip128's status, pivot count and solution text"""
    _same(pb.run_batch(pb.ORACLEPIP128, _problems(IDS, nvar, 128), FLAGS).results, list(IDS), nvar, 128)


def test_the_small_tableaux_themselves_are_the_oracles():
    """... and so are the unembedded tableaux (4 unknowns)"""
    from piplib_amd import synth
    for exe, ids in ((pb.ORACLEPIP, IDS64), (pb.ORACLEPIP128, list(IDS))) + (((pb.REFPIP, IDS64),) if pb.have_ref() else ()):
        probs = [synth.Problem(dc.NV, 0, dc.NI, 0, -1, 1, np.array(dc.cases()[k].ineq, np.int64), np.zeros((0, 1), np.int64))
                 for k in ids]
        for k, r in zip(ids, pb.run_batch(exe, probs, FLAGS).results):
            m = dc.cases()[k].res
            assert r.status == pb.ST_OK and r.pivots == m.pivots, (k, r.pivots, m.pivots)
            want = "()" if m.status == bp.ST_NIL else pb.squash(bp.solution_text(m.sol_num, m.sol_den))
            assert pb.squash(r.text) == want, k
