"""tests/pipsolve_model.py against the CPU authorities, no GPU: the model's tableaux for every golden pip_solve input
(tests/golden/pipsolve, printed and counted by the reference) give, through `oraclepip batch`, the golden pivot count and
void-ness; hand-written rows pin the column layout of tab_Matrix2Tableau (tab.c:292-393) and quast_text's reading of
the tape; the CPU restatement's `pip` mode prints the golden texts.  (quast_text over whole answers is held to the
goldens by the GPU tests: the cells come from the engine.)"""
import numpy as np
import pytest

import pipbatch as pb
import pipsolve_model as pm

FAMILIES = sorted(pm.FAMILIES)


def _arrays(p):
    return np.array(p["inequnk"], dtype=np.int64), np.array(p["ineqpar"], dtype=np.int64)


@pytest.mark.parametrize("name", FAMILIES)
def test_family_gives_the_tests_something_to_hold_on_to(name):
    g = pm.golden(name)
    assert len(g) == pm.FAMILIES[name][0]
    assert sum("(if" in p["text"] for p in g) >= 6
    assert sum("(newparm" in p["text"] for p in g) >= 4
    assert sum(p["text"].strip() == "void" for p in g) >= 4
    assert sum(bool(p["options"] & pm.MAXIMIZE) and "/0" in p["text"] for p in g) >= 6
    opts = {p["options"] for p in g}
    for bit in (pm.NQ, pm.MAXIMIZE, pm.URS_PARMS, pm.URS_UNKNOWNS, pm.DUAL):
        assert any(o & bit for o in opts), bit
    assert {p["bg"] == -1 for p in g} == {True, False}
    assert any(all(r[0] == 0 for r in p["inequnk"]) for p in g)      # every row an equality
    assert any(p["inequnk"][0][0] == 0 and p["inequnk"][-1][0] != 0 for p in g)
    assert any(p["inequnk"][-1][0] == 0 and p["inequnk"][0][0] != 0 for p in g)
    assert any(any(r[0] == 0 for r in p["ineqpar"]) for p in g)      # an equality in the context


@pytest.mark.parametrize("name", FAMILIES)
def test_model_tableaux_give_golden_pivots_and_voids(name):
    g = pm.golden(name)
    probs = []
    for p in g:
        f, dom, ctx = pm.build(*_arrays(p), p["bg"], p["options"])
        probs.append(pm.as_problem(f, dom, ctx))
    res = pb.run_batch(pb.ORACLEPIP, probs).results  # (tab_simplify for the integer ones, the context test, traiter())
    for k, (p, r) in enumerate(zip(g, res)):
        assert r.status != pb.ST_ABORT, k
        assert (r.status == pb.ST_VOID) == (p["text"].strip() == "void"), k
        assert r.pivots == p["pivots"], (k, r.pivots, p["pivots"])


@pytest.mark.parametrize("name", FAMILIES)
def test_oracle_pip_mode_prints_the_golden_text(name):
    """the CPU restatement's `pip` mode against the reference's stored text, Compute_dual lists included (the families
    hold no Compute_dual problem whose quast forks: the reference's dual values are heap-dependent there, see
    pipsolve_model.defined_answer)"""
    for k, p in enumerate(pm.golden(name)):
        rc, text, _ = pm.run_pip(pb.ORACLEPIP, p["inequnk"], p["ineqpar"], p["bg"], p["options"])
        assert rc == 0 and pb.squash(text) == pb.squash(p["text"]), k
        assert not ((p["options"] & pm.DUAL) and not (p["options"] & pm.NQ) and "(if" in p["text"]), k


A1, A2, P1, P2, P3, CST = 2, -3, 5, 7, 11, 13
WIDE = [[1, A1, A2, P1, P2, P3, CST]]
WCTX = [[1, 1, 2, 3, 4]]
NARROW = [[1, A1, A2, P1, CST]]
NCTX = [[1, 6, 4]]
# (inequnk, ineqpar, bg, options) -> domain rows, context rows, the info fields that matter
LAYOUT = {
    "Urs_parms, Bg the first parameter": (
        (WIDE, WCTX, 3, pm.NQ | pm.URS_PARMS),
        [[A1, A2, CST, P1, P2, P3, -P2, -P3]], [[1, 2, 3, -2, -3, 4]],
        dict(nvar=2, nparm=5, ni=1, nc=1, bigparm=3, sol_bg=0, urs_parms=2, sol_flags=0, flags=1)),
    "Urs_parms, Bg the last parameter": (
        (WIDE, WCTX, 5, pm.NQ | pm.URS_PARMS),
        [[A1, A2, CST, P1, P2, P3, -P1, -P2]], [[1, 2, 3, -1, -2, 4]],
        dict(nvar=2, nparm=5, ni=1, nc=1, bigparm=5, sol_bg=2, urs_parms=2, sol_flags=0, flags=1)),
    "Urs_parms without Bg": (
        (WIDE, WCTX, -1, pm.URS_PARMS),
        [[A1, A2, CST, P1, P2, P3, -P1, -P2, -P3]], [[1, 2, 3, -1, -2, -3, 4]],
        dict(nvar=2, nparm=6, ni=1, nc=1, bigparm=-1, sol_bg=-4, urs_parms=3, sol_flags=0, flags=0)),
    "Maximize makes a big parameter in domain and context": (
        (NARROW, NCTX, -1, pm.NQ | pm.MAXIMIZE),
        [[-A1, -A2, CST, P1, A1 + A2]], [[6, 0, 4]],
        dict(nvar=2, nparm=2, ni=1, nc=1, bigparm=4, sol_bg=1, urs_parms=0, sol_flags=7, flags=1)),
    "Urs_unknowns makes one too, with the sum negated": (
        (NARROW, NCTX, -1, pm.URS_UNKNOWNS | pm.DUAL),
        [[A1, A2, CST, P1, -(A1 + A2)]], [[6, 0, 4]],
        dict(nvar=2, nparm=2, ni=1, nc=1, bigparm=4, sol_bg=1, urs_parms=0, sol_flags=1 | 4 | 8, flags=2)),
    "an equality under Maximize, the sum added to the given Bg": (
        ([[0, A1, A2, P1, CST]], NCTX, 3, pm.MAXIMIZE | pm.URS_UNKNOWNS),
        [[-A1, -A2, CST, P1 + A1 + A2], [A1, A2, -CST, -(P1 + A1 + A2)]], [[6, 4]],
        dict(nvar=2, nparm=1, ni=2, nc=1, bigparm=3, sol_bg=0, urs_parms=0, sol_flags=3, flags=0)),
    "Urs_parms and a new big parameter: the copies skip it": (
        (NARROW, [[0, 6, 4]], -1, pm.NQ | pm.MAXIMIZE | pm.URS_PARMS),
        [[-A1, -A2, CST, P1, A1 + A2, -P1]], [[6, 0, -6, 4], [-6, 0, 6, -4]],
        dict(nvar=2, nparm=3, ni=1, nc=2, bigparm=4, sol_bg=1, urs_parms=1, sol_flags=7, flags=1)),
}


@pytest.mark.parametrize("case", sorted(LAYOUT))
def test_column_layout(case):
    args, dom, ctx, info = LAYOUT[case]
    f, d, c = pm.build(*args)
    assert d == dom and c == ctx
    assert {k: f[k] for k in info} == info


def test_sums_wrap_in_64_bits():
    top = (1 << 63) - 1
    f, d, c = pm.build([[1, top, 1, 0]], None, -1, pm.MAXIMIZE)
    assert d == [[-top, -1, 0, -(1 << 63)]]
    f, d, c = pm.build([[1, top, 1, 0]], None, -1, pm.MAXIMIZE, wrap=False)
    assert d == [[-top, -1, 0, 1 << 63]]


def test_void_without_a_domain_matrix():
    f, d, c = pm.build(None, None, -1, pm.NQ)
    assert f["is_void"] == 1 and pm.quast_text([], f) == "void\n"


def test_quast_text_on_hand_written_tapes():
    """(list #[..]) with SOL_MAX | SOL_REMOVE: the big parameter's column is dropped, the values negated; an unbounded
    answer prints /0 throughout (sol.c:476-507)"""
    info = dict(is_void=0, sol_bg=1, urs_parms=0, sol_flags=7, ni=1)
    V = pm.S_VAL
    cells = [(pm.S_LIST, 1, 0), (pm.S_FORM, 3, 0), (V, 4, 2), (V, 3, 3), (V, -5, 1)]
    assert pm.quast_text(cells, info) == "(list\n #[ -2 5]\n)\n"
    cells = [(pm.S_LIST, 1, 0), (pm.S_FORM, 3, 0), (V, 4, 2), (V, 2, 1), (V, -5, 1)]
    assert pm.quast_text(cells, info) == "(list\n #[ -2/0 5/0]\n)\n"
    cells = [(pm.S_IF, 0, 0), (pm.S_FORM, 2, 0), (V, 1, 1), (V, -3, 1), (pm.S_NIL, 0, 0), (pm.S_NIL, 0, 0)]
    assert pm.quast_text(cells, dict(is_void=0, sol_bg=-1, urs_parms=0, sol_flags=0, ni=1)) == "(if #[ 1 -3]\n ()\n ()\n)\n"
