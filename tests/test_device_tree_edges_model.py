"""The edge families of tests/device_tree_edges.py on the CPU: every member the GPU tests run has the structural figures
its edge rests on -- nested-if depth, new parameters, cuts, tape cells, the abort -- asserted against the CPU oracle
(liboracle64.so / liboracle128.so through ctypes, and the oraclepip CLI for the text), and the oracle's text, status and
pivot count against the reference's: the fixtures of tests/golden/device_tree_edges/ always, oracle/_ref/refpip too where
it is built.  No GPU."""
import glob
import json
import os

import pytest

import device_tree_edges as dte
import pipbatch as pb

_FIX = {}
for _f in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_tree_edges", "*.json"))):
    _FIX.update(json.load(open(_f)))
_CLI = {}


def _cli(name, bits=64):
    """the oracle CLI's answer for a member (computed once)"""
    if (name, bits) not in _CLI:
        _CLI[name, bits] = pb.run_batch(pb.ORACLEPIP if bits == 64 else pb.ORACLEPIP128, [dte.member(name)]).results[0]
    return _CLI[name, bits]


def test_every_member_has_its_tables():
    assert set(dte.FIGURES) == set(dte.MEMBERS) == set(_FIX)
    assert set(dte.DEVICE) == set(dte.MEMBERS) - {"chain24_new10_nc17"}  # (the full context: no flip point fixed in advance)
    assert set(dte.TAPE) <= set(dte.MEMBERS)


@pytest.mark.parametrize("name", sorted(dte.MEMBERS))
@pytest.mark.parametrize("bits", [64, 128])
def test_structural_figures(name, bits):
    status, depth, newp, ncuts, cells, pivots = dte.FIGURES[name]
    f = dte.oracle_figures(dte.member(name), bits)
    assert f["status"] == status
    r = _cli(name, bits)
    if status != dte.ORA_OK:
        assert r.status == pb.ST_ABORT and r.abort_code == status
        if cells is not None:
            assert f["cells"] == cells
        return
    assert r.status == pb.ST_OK
    assert (dte.if_depth(r.text), dte.newparms(r.text), f["cuts"], f["cells"], f["pivots"]) == (depth, newp, ncuts, cells, pivots)
    assert r.pivots == pivots


@pytest.mark.parametrize("name", sorted(dte.MEMBERS))
def test_oracle_vs_reference(name):
    """text, status and pivot count: the fixtures, and the reference itself where it is built"""
    r = _cli(name)
    refs = [_FIX[name]]
    if pb.have_ref():
        rr = pb.run_batch(pb.REFPIP, [dte.member(name)]).results[0]
        refs.append({"status": rr.status, "abort_code": rr.abort_code, "pivots": rr.pivots, "text": pb.squash(rr.text)})
    for ref in refs:
        assert r.status == ref["status"]
        if r.status == pb.ST_ABORT:
            assert ref["abort_code"] == dte.REF_EXIT[r.abort_code]
            continue
        assert r.pivots == ref["pivots"]
        assert pb.squash(r.text) == ref["text"]
    r128 = _cli(name, 128)
    assert (r128.status, r128.abort_code, r128.pivots, r128.text) == (r.status, r.abort_code, r.pivots, r.text)


def test_tape_members_by_the_formula():
    """cells of a tree: (2^k - 1)(nparm + 3) + 2^k (1 + nvar (nparm + 2)); the reference refuses SOL_SIZE cells and more"""
    for name, cells in dte.TAPE.items():
        p = dte.member(name)
        k = p.ni
        assert dte.tree_cells(k, p.nvar - k, p.nparm - k) == cells
        f = dte.oracle_figures(p)
        assert (f["status"], f["cells"]) == ((dte.ORA_OK, cells) if cells < dte.SOL_SIZE else (dte.ORA_ERR_SOLSIZE, dte.SOL_SIZE))
    assert sorted(c for c in dte.TAPE.values() if c <= 3600) and max(dte.TAPE.values()) >= dte.SOL_SIZE
    assert any(4088 <= c < dte.SOL_SIZE for c in dte.TAPE.values())


def test_full_context_member_cuts_in_its_sub_problems():
    """chain(24, nnew=10, nc=17): 197 cuts against 10 without the context rows -- the compa_test sub-problems cut"""
    assert dte.oracle_figures(dte.member("chain24_new10_nc17"))["cuts"] == 197
    assert dte.oracle_figures(dte.member("chain24_new10"))["cuts"] == 10


def test_neighbours_keep_their_figures_and_differ():
    """the members of the neighbours call: same depth / cuts / cells as their base member, every tape text its own"""
    base = {(True, 0): "chain24", (False, 0): "chain25", (True, 1): "cuts24_ni40", (False, 1): "cuts25_ni40",
            (True, 2): "tree5_12_0", (False, 2): "tree5_13_0"}
    nb = dte.neighbours()
    assert len(nb) >= 64
    res = pb.run_batch(pb.ORACLEPIP, [p for p, _ in nb]).results
    ref = pb.run_batch(pb.REFPIP, [p for p, _ in nb]).results if pb.have_ref() else res
    texts = set()
    for k, ((p, at), r, rr) in enumerate(zip(nb, res, ref)):
        assert at == (k % 2 == 0)
        status, depth, newp, ncuts, cells, pivots = dte.FIGURES[base[at, (k % 6) // 2]]
        f = dte.oracle_figures(p)
        assert f["status"] == status and (r.status == pb.ST_ABORT) == (status != dte.ORA_OK)
        assert (r.status, r.pivots, pb.squash(r.text)) == (rr.status, rr.pivots, pb.squash(rr.text))
        if status == dte.ORA_OK:
            assert (dte.if_depth(r.text), f["cuts"], f["cells"]) == (depth, ncuts, cells)
            texts.add(r.text)
    assert len(texts) == sum(r.status == pb.ST_OK for r in res)


def test_neighbours_as_polylib_matrices():
    """pip_matrices: tab_Matrix2Tableau (tests/pipsolve_model.py) builds every neighbour's own rows from its matrices"""
    import pipsolve_model as pm
    for p, _ in dte.neighbours(2) + [(dte.member("chain24_new10_nc17"), True)]:
        dom, ctx = dte.pip_matrices(p)
        assert dom.shape == (p.ni, p.nvar + p.nparm + 2) and ctx.shape == (p.nc, p.nparm + 2)
        info, rows, crow = pm.build(dom, ctx, -1, pm.NQ)
        assert (info["nvar"], info["nparm"], info["ni"], info["nc"], info["bigparm"]) == (p.nvar, p.nparm, p.ni, p.nc, -1)
        assert rows == p.ineq.tolist() and crow == p.ctx.tolist()
