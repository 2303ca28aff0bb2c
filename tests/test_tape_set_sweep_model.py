"""tests/tape_set_sweep_model.py held to the reference: every job's summary is a direct census of the recorded answers of
tests/golden/tape_eval (what the reference printed, not the code under test), tiles of a box merge to the whole box's
summary, and the planner's arithmetic.  Host only, Python ints only."""
import pytest

import tape_cases as tc
import tape_model as tm
import tape_set_sweep_model as ssm
import tape_sweep_model as sm


def golden_job(name, lo=(0, 0), hi=(9, 9), ctx=None, bits=64):
    g = tc.golden()
    return {"cells": tc.cells_from_text(g["tapes"][name]), "nvar": g["nvar"], "nparm": g["nparm"], "ndual": 0,
            "lo": list(lo), "hi": list(hi), "ctx": ctx, "bits": bits}


@pytest.mark.parametrize("bits", [64, 128])
def test_every_job_is_a_census_of_the_recorded_answers(bits):
    g = tc.golden()
    jobs = [golden_job("int", bits=bits), golden_job("rat", bits=bits), golden_job("int", bits=bits)]
    summaries, words, off = ssm.sweep(jobs)
    assert len(summaries) == 3 and off[0] == 0 and off[-1] == len(words)
    for job, name, s, a, b in zip(jobs, ("int", "rat", "int"), summaries, off, off[1:]):
        answers = g["answers"][name]
        res = tm.evaluate_cells(job["cells"], job["nvar"], job["nparm"], 0, g["points"], bits)
        assert tc.answers_of(res) == answers  # (the leaf a point reached is the only figure the fixture does not print)
        leaves = tm.check(job["cells"], job["nvar"], job["nparm"], 0, bits)["leaves"]
        want = ssm.census(answers, [r[1] for r in res], leaves)
        assert s == want and words[a:b] == sm.words(want) and b - a == ssm.words_of(leaves)
        assert want["counts"]["solution"] == sum(x is not None for x in answers) > 0
        assert sum(want["leaf_count"]) == 100 and sum(c > 0 for c in want["leaf_count"]) >= 6


def test_tiles_merge_to_the_whole_box():
    whole, _ = ssm.job_summary(golden_job("int", ctx=[[1, 1, 1, -4]]))
    assert whole["counts"]["outside"] > 0 and whole["counts"]["solution"] > 0
    # rows of the box: a tile's k are consecutive k of the whole box, its first moves by an offset
    rows = [(0, 3), (4, 6), (7, 9)]
    tiles = [(ssm.job_summary(golden_job("int", (a, 0), (b, 9), [[1, 1, 1, -4]]))[0], 10 * a) for a, b in rows]
    assert ssm.merge_tiles(tiles) == whole
    assert ssm.merge_tiles(tiles[::-1]) == whole
    # columns of the box: tile k = (row, column - a) is whole k = 10 row + column
    cols = [(0, 0), (1, 6), (7, 9)]
    tiles = [(ssm.job_summary(golden_job("int", (0, a), (9, b), [[1, 1, 1, -4]]))[0],
              (lambda k, a=a, w=b - a + 1: 10 * (k // w) + a + k % w)) for a, b in cols]
    assert ssm.merge_tiles(tiles) == whole
    # a tile that is left out is missed
    assert ssm.merge_tiles(tiles[:2]) != whole


def test_plan_arithmetic():
    box = lambda n: ([5], [5 + n - 1], 0, False)
    sizes = [1, 127, 128, 129, 257]
    leaves = [0, 3, 7, 1, 40]
    p = ssm.plan([box(n) for n in sizes] + [([], [], 2, True)], leaves + [2], [1] * 5 + [0])
    assert p["points"] == sizes + [1]
    assert p["chunk_off"] == [0, 1, 2, 3, 5, 8, 9]
    assert p["summary_off"] == [0, 8, 22, 44, 54, 142, 154]
    assert ssm.plan([], [], []) == {"points": [], "summary_off": [0], "chunk_off": [0]}
    big = ([0, 0], [(1 << 19) - 1, (1 << 19) - 2], 0, False)  # 2^38 - 2^19 points
    assert ssm.plan([big], [1], [2])["points"] == [(1 << 38) - (1 << 19)]
    refusals = [
        ([box(3), ([1], [0], 0, False)], [1, 1], [1, 1], tm.E_INVALID, 1),
        ([box(3), box(3), ([0], [1], -1, False)], [1] * 3, [1] * 3, tm.E_INVALID, 2),
        ([([0], [1], 2, False)], [1], [1], tm.E_INVALID, 0),
        ([box(1), ([0], [1], 0, False)], [1, 1], [1, 32], tm.E_INVALID, 1),
        ([box(1), ([0], [1], 0, False)], [1, -1], [1, 1], tm.E_INVALID, 1),
        ([box(1), ([0, 0], [(1 << 19) - 1, (1 << 19) - 1], 0, False)], [1, 1], [1, 2], tm.E_TOOLARGE, 1),
        ([big, box((1 << 19) - 1), box(1)], [1] * 3, [2, 1, 1], tm.E_TOOLARGE, 2),
        ([([sm.MIN64], [sm.MAX64], 0, False)], [1], [1], tm.E_TOOLARGE, 0),
    ]
    for jobs, lv, pc, code, job in refusals:
        with pytest.raises(tm.TapeError) as e:
            ssm.plan(jobs, lv, pc)
        assert e.value.code == code and str(job) in str(e.value), (jobs, e.value)
    assert ssm.plan([big, box((1 << 19) - 1)], [1] * 2, [2, 1])["chunk_off"][-1] == 1 << 31  # (beyond 32 bits signed)
