"""tests/tape_edit_model.py against the CPU authorities, no GPU: (a) for the golden pip_solve problems (tests/golden/
pipsolve) the raw tape of the CPU restatement, edited by the model with the model's pipamd_pip_info, prints vector by
vector as the quast the reference printed -- the caller's own Bg first, last and new, with and without Urs_parms --;
(b) the fixtures of tests/golden/tape_edit, their printed quasts walked, equal the answers the reference recorded per
point."""
import json
import os

import numpy as np
import pytest

import pipbatch as pb
import pipsolve_model as pm
import tape_cases as tc
import tape_edit_model as te

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tape_edit")
FAMILIES = ("maximize", "urs_unknowns", "urs_parms", "urs_parms_maximize", "rational_maximize")


def family(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def vectors(text):
    """a printed quast as its lines, every vector a list of "n" / "n/d" strings"""
    return [ln.split() for ln in text.strip().splitlines()]


@pytest.mark.parametrize("name", sorted(pm.FAMILIES))
def test_edited_raw_tapes_print_as_the_reference_quasts(name):
    g = [p for p in pm.golden(name) if p["text"].strip() != "void" and not (p["options"] & pm.DUAL and not p["options"] & pm.NQ)]
    built = [pm.build(np.array(p["inequnk"], dtype=np.int64), np.array(p["ineqpar"], dtype=np.int64), p["bg"], p["options"])
             for p in g]
    res = pb.run_batch(pb.ORACLEPIP, [pm.as_problem(*b) for b in built]).results
    for k, (p, (f, _, _), r) in enumerate(zip(g, built, res)):
        assert r.status == pb.ST_OK, k
        raw = tc.cells_from_text(r.text)
        nodes, info, _ = te.edit_nodes(raw, f["nvar"], f["nparm"], 0, pm.info_of(f), 64)
        lines = []
        pm._print(te.quast(nodes), 0, lines)
        assert vectors("".join(lines)) == vectors(p["text"]), k
        assert info["slots"] >= te.point_cols(f["nparm"], pm.info_of(f)) + 1


def test_golden_problems_cover_every_place_of_the_big_parameter():
    """the caller's own Bg as the first and as the last parameter, and a new one, each with and without Urs_parms, among
    the problems the test above edits"""
    seen = set()
    for name in sorted(pm.FAMILIES):
        for p in pm.golden(name):
            if p["text"].strip() == "void" or (p["options"] & pm.DUAL and not p["options"] & pm.NQ):
                continue
            f = pm.plan(p["inequnk"], p["ineqpar"], p["bg"], p["options"])
            given = p["bg"] >= 0
            seen.add((given and f["sol_bg"] == 0, given and f["sol_bg"] == f["nparm"] - f["urs_parms"] - 1,
                      bool(f["sol_flags"] & pm.SOL_REMOVE), f["urs_parms"] > 0))
    for urs in (False, True):
        assert any(s[0] and s[3] == urs for s in seen) and any(s[1] and s[3] == urs for s in seen), urs
        assert any(s[2] and s[3] == urs for s in seen), urs


@pytest.mark.parametrize("name", FAMILIES)
def test_fixture_quasts_walked_give_the_recorded_answers(name):
    g = family(name)
    assert len(g["points"]) >= 100 and len(g["answers"]) == len(g["points"])
    nodes = te.nodes_from_text(g["text"], g["nparm"])
    traces, got = [], []
    for p in g["points"]:
        t = {}
        got.append(te.evaluate(nodes, g["nvar"], 0, p, 64, t))
        traces.append(t)
    for k, (r, a) in enumerate(zip(got, g["answers"])):
        assert te.same_answer(te.answer_of(r), a), (k, g["points"][k])
    assert len(set(r[1] for r in got)) >= 4 and sum(a is None for a in g["answers"]) >= 8
    if g["options"] & pm.URS_PARMS:
        assert sum(min(p) < 0 for p in g["points"]) >= 30
    c = g["census"]
    assert c["through_new"] == sum(bool(t.get("news")) for t in traces)
    assert c["unbounded"] == sum(a is not None and any(d == 0 for _, d in a) for a in g["answers"])


def test_fixtures_together_give_the_tests_something_to_hold_on_to():
    gs = [family(n) for n in FAMILIES]
    assert sum(g["census"]["through_new"] for g in gs) >= 20
    # (which unknowns are unbounded is the same at every point that has a solution -- the parameters only move the rows'
    # constants --, so the points "without" are the unsolved ones; bounded and unbounded unknowns meet within an answer)
    assert any(g["census"]["unbounded"] >= 10 and len(g["points"]) - g["census"]["unbounded"] >= 10 and
               g["census"]["mixed"] >= 10 for g in gs)
    assert {g["options"] for g in gs} == {3, 9, 5, 7, 2}


def test_model_without_an_edit_is_the_plain_model():
    import tape_model as tm
    g = tc.golden()
    cells = tc.cells_from_text(g["tapes"]["int"])
    nodes, info, _ = te.edit_nodes(cells, g["nvar"], g["nparm"])
    assert info == tm.check(cells, g["nvar"], g["nparm"])
    want = tm.evaluate_cells(cells, g["nvar"], g["nparm"], 0, g["points"])
    assert [te.evaluate(nodes, g["nvar"], 0, p) for p in g["points"]] == want
