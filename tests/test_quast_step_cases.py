"""What tests/test_gpu_quast_step_probe.py rests on, checked without a device: the case lists of
tests/quast_step_cases.py are deterministic and stay inside what the probe's host entry admits; every case has a class at
each width; `may` cases are at most a tenth of a function's list; every named edge has a `fits` case and, where it is a
magnitude, a `must` case one step beyond; the 64-bit `fits` cases stand in the 128-bit list with the same expected values;
and the model agrees with tests/bigint_pip.py wherever the two restate the same operation."""
import numpy as np
import pytest

import bigint_pip as bp
import quast_step_cases as qc
import quast_step_model as qm

WIDTHS = (64, 128)
GROUPS = list(qc.FUNCTIONS)


def _runs(name, Wb):
    return [(c, qm.run(c, Wb, c.nb)) for c in qc.all_cases(name, Wb)]


@pytest.mark.parametrize("name", GROUPS)
def test_lists_are_deterministic_and_admitted(name):
    for Wb in WIDTHS:
        cases = qc.all_cases(name, Wb)
        qc.all_cases.cache_clear(), qc._free.cache_clear(), qc._edge.cache_clear()
        again = qc.all_cases(name, Wb)
        assert [c.tag for c in cases] == [c.tag for c in again]
        assert all((qm.pack_in(a, Wb // 64) == qm.pack_in(b, Wb // 64)).all() for a, b in zip(cases, again))
        assert len({c.tag for c in cases}) == len(cases)
        assert 10 <= len(cases) <= 400
        for c in cases:
            # what pipamd_debug_quast_step's host entry asks of a case (piplib_amd/csrc/pip_probe.hip)
            assert c.fn in qc.FUNCTIONS[name] and c.fits(Wb) and c.lds_bytes(Wb) <= qm.LDS_MAX, c.tag
            assert 1 <= c.W <= 64 * c.nb and 1 <= c.nvar < c.ncol <= c.W and c.nligne <= c.R <= 256 and c.ni <= c.S <= 256, c.tag
            assert -1 <= c.bigparm < c.ncol and c.nc <= c.CR and 0 <= c.nparm < c.CW <= 64 and 1 <= c.ldet <= qm.MAXDET, c.tag
            for k in range(c.R):
                assert 0 <= c.ref[k] < (c.nvar if c.flag[k] & qm.UNIT else c.S) and c.den[k] >= 1 and 0 <= c.flag[k] < 64, c.tag
            if c.fn in (qm.QS_PIVOT, qm.QS_MAKE_CUT, qm.QS_DEEPEN, qm.QS_CUT_CHAIN):
                assert c.pivi < c.nligne and not c.flag[c.pivi] & qm.UNIT, c.tag
            if c.fn == qm.QS_SOLVE_PLAIN:
                assert c.ncol == c.nvar + 1 and c.nvar + c.ni == c.nligne and c.budget <= 4096, c.tag
            if name in qc.ONE_BLOCK:
                assert c.nb == 1, c.tag
        for nb in (1, 2):
            got = qc.cases(name, Wb, nb)
            assert got == ([] if nb == 2 and name in qc.ONE_BLOCK else [c for c in cases if c.nb <= nb])


@pytest.mark.parametrize("name", GROUPS)
def test_classes_and_the_cap_on_may(name):
    for Wb in WIDTHS:
        runs = _runs(name, Wb)
        n = {k: sum(1 for _, o in runs if o.cls == k) for k in ("fits", "must", "may")}
        assert sum(n.values()) == len(runs)
        assert 10 * n["may"] <= len(runs), (name, Wb, n)
        for c, o in runs:   # a one-block case has the same class and values on two blocks, but for the cut vector's length
            if c.nb == 1 and name not in qc.ONE_BLOCK:
                o2 = qm.run(c, Wb, 2)
                assert (o2.cls, o2.ret, o2.aux, o2.val, o2.den, o2.flag, o2.cut[:64]) == (o.cls, o.ret, o.aux, o.val, o.den, o.flag, o.cut), c.tag


@pytest.mark.parametrize("name", GROUPS)
def test_every_edge_has_its_cases(name):
    for Wb in WIDTHS:
        runs = _runs(name, Wb)
        for cls, table in (("fits", qc.EDGES_FITS), ("must", qc.EDGES_MUST)):
            for edge in table.get(name, []):
                hit = [c.tag for c, o in runs if edge in c.edges and o.cls == cls and (Wb == 64 or not c.tag.startswith("[B = 2^63]"))]
                assert hit, "%s at %d bits: no `%s` case on the edge %r" % (name, Wb, cls, edge)
        if Wb == 128:
            for edge in qc.EDGES_128.get(name, []):
                assert any(edge in c.edges and o.cls == "fits" for c, o in runs), edge
        # a name nobody asks for is a typing error
        asked = set(qc.EDGES_FITS.get(name, []) + qc.EDGES_MUST.get(name, []) + qc.EDGES_128.get(name, []))
        loose = {"W=ncol", "cross untied", "nc0", "nparm0", "fits32 -2^31-1"}
        for c, _ in runs:
            assert all(e.startswith(("ncol", "nligne", "nvar")) for e in set(c.edges) - asked - loose), (c.tag, c.edges)
    # the one `may` the lists hold by design: an untied column's cross product
    if name == "pivot_step":
        for Wb in WIDTHS:
            assert any("cross untied" in c.edges and o.cls == "may" for c, o in _runs(name, Wb))


@pytest.mark.parametrize("name", GROUPS)
def test_64_bit_fits_cases_stand_in_the_128_bit_list(name):
    wide = {c.tag: (c, o) for c, o in _runs(name, 128)}
    for c, o in _runs(name, 64):
        if o.cls != "fits" or c.ebw:
            continue   # (Case.ebw: the determinant's limbs are placed by the width; such a case is listed per width)
        assert c.tag in wide, c.tag
        c2, o2 = wide[c.tag]
        assert (qm.pack_in(c, 2) == qm.pack_in(c2, 2)).all() and o2.cls == "fits", c.tag
        assert (qm.pack_out(o, 2) == qm.pack_out(o2, 2)).all(), c.tag
    assert any(c.ebw for c, _ in _runs("pivot_step", 64)) and all(not c.ebw for c, _ in _runs(name, 64) if c.fn != qm.QS_PIVOT)


def test_pivot_column_is_the_lexicographic_minimum():
    """the tournament's trace ends on choisir_piv's column: brute force over the columns divided by the pivot row's entry"""
    n = 0
    for Wb in WIDTHS:
        for c, o in _runs("pivot_step", Wb):
            if o.cls == "must" and o.pivj < 0:
                continue
            assert o.pivj == qm.brute_column(c), c.tag
            n += 1
    assert n >= 150


def _bp_rows(c, o=None):
    src = c if o is None else o
    rows = []
    for k in range(c.nligne):
        if src.flag[k] & qm.UNIT:
            rows.append(bp._Row(src.flag[k], src.den[k], None, src.ref[k]))
        else:
            rows.append(bp._Row(src.flag[k], src.den[k], np.array(src.val[src.ref[k]][:c.ncol], dtype=object)))
    return rows


def test_pivot_step_equals_bigint_pip_where_they_overlap():
    """bigint_pip.pivot_step is the non-parametric loop's: on every `fits` case with a unit row for its column the rows,
    denominators, flags and determinant it leaves are the model's (ncol is free there: the row update walks what it is given)"""
    n = 0
    for c, o in _runs("pivot_step", 64):
        if o.cls != "fits" or o.ret != 0:
            continue
        rows = _bp_rows(c)
        det = list(c.det[:c.ldet])
        st = bp.Stats(64)
        prow = rows[c.pivi].v
        assert bp.pick_column(rows, c.pivi, c.nvar, c.nligne, st) == o.pivj, c.tag
        pivot, dpiv = int(prow[o.pivj]), rows[c.pivi].den
        bp.det_update(det, pivot, dpiv, 64)
        assert det == o.det[:o.ldet], c.tag
        for k in range(c.nligne):
            r = rows[k]
            if (r.flag & qm.UNIT) or k == c.pivi:
                continue
            z, newden, _, _ = bp.row_update(r.v, r.den, prow, pivot, dpiv, o.pivj)
            assert [int(x) for x in z] == o.val[o.ref[k]][:c.ncol] and int(newden) == o.den[k], (c.tag, k)
        n += 1
    assert n >= 60


def test_sort_equals_bigint_pip_where_they_overlap():
    """bigint_pip.sort_rows sorts rows over a denominator of 1: the same order of rows"""
    n = 0
    for c, o in _runs("sort_rows", 64):
        if o.ret != 0 or any(c.den[k] != 1 for k in range(c.nvar, c.nligne)):
            continue
        rows = _bp_rows(c)
        was = {id(r): c.ref[k] for k, r in enumerate(rows)}
        bp.sort_rows(rows, c.nvar, c.nligne)
        assert [was[id(r)] for r in rows] == o.ref[:c.nligne], c.tag
        n += 1
    assert n >= 10


def test_plain_solves_equal_bigint_pip():
    """solve_plain's chain without the deepest cut is bigint_pip.solve: found or nil, the pivots, the answer"""
    n = 0
    for c, o in _runs("solve_plain", 64):
        if c.deepest or o.ret & 0xFFFE or c.flag[:c.nvar] != [qm.UNIT] * c.nvar:
            continue
        ineq = [c.val[s][:c.ncol] for s in range(c.ni)]
        r = bp.solve(ineq, integer=True, bits=64)
        assert r.stats.exact and (r.status == bp.ST_SOLUTION) == bool(o.ret & 1) and r.pivots == o.ret >> 16 and r.cuts == o.cuts, c.tag
        if o.ret & 1:
            num = [0 if o.flag[i] & qm.UNIT else o.val[o.ref[i]][c.nvar] for i in range(c.nvar)]
            den = [1 if o.flag[i] & qm.UNIT else o.den[i] for i in range(c.nvar)]
            assert (num, den) == (r.sol_num, r.sol_den), c.tag
        n += 1
    assert n >= 12


def test_named_cases_do_what_their_tags_say():
    runs = {c.tag: (c, o) for name in GROUPS for c, o in _runs(name, 64)}
    c, o = runs["no positive entry"]
    assert o.ret == -1 and qm.pack_out(o, 1)[4:].tolist() == qm.pack_out(qm._image(c, 1), 1)[4:].tolist()
    assert runs["tie never resolved ends on the lowest column; no unit row for it"][1].ret == qm.Q_WHY_OTHER
    assert runs["tie never resolved ends on the lowest column; no unit row for it"][1].pivj == 0
    assert runs["the tournament moves within block 0, then on to block 1"][1].pivj == 70
    assert runs["the tournament stays tied through block 1 and ends back in block 0"][1].pivj == 3
    assert runs["n = 65 without skey"][1].ret == runs["n = 129"][1].ret == qm.Q_WHY_ROWS | 256
    c, o = runs["keys at 2^24 +- 1: the float key rounds, the bound does not"]
    assert o.ref[c.nvar:] == [3, 2, 1, 0]   # 2^24 + 1 keys as 2^24, below the bound 2^24 + 1.0 like its equal: it moves
    c, o = runs["a swap across the 64 boundary, pos"]
    assert o.ref[c.nvar] == 70 and o.pos[70] == c.nvar and o.pos[0] != c.nvar
    assert runs["a fractional constant with nothing to cut with"][1].note.startswith("fractional")
    assert runs["a row without a positive entry"][1].note == "no positive entry"
    assert runs["two candidates: the highest parameter"][1].ret == 3 and runs["both defining rows"][1].ret == 2
    assert runs["a nonzero coefficient ends the search before the rows' parameter"][1].ret == -1
    assert runs["the rows of a lower parameter only"][1].ret == 1
    budget = [(c, o) for c, o in runs.values() if "budget met" in c.edges]
    assert budget and all(o.ret & 1 and not (o.ret >> 1) & 0x7FFF and o.ret >> 16 == c.budget for c, o in budget)
    assert all((o.ret >> 1) & 0x7FFF == qm.Q_WHY_OTHER for c, o in runs.values() if "budget 0" in c.edges or "budget short" in c.edges)
    assert all((o.ret >> 1) & 0x7FFF == qm.Q_WHY_ROWS | 512 for c, o in runs.values() if "rows cap" in c.edges)
    assert all(o.ret == -1 for c, o in runs.values() if "refusal" in c.edges)
