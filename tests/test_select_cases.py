"""What tests/test_gpu_select_probe.py rests on, checked without a device: the case lists of tests/select_cases.py are
deterministic, hold every tag for every flavour it applies to, stay inside each function's domain and drop nothing from
it; the fold model of choisir_piv is bigint_pip.pick_column and equals a brute-force lexicographic minimum; the wrap
model equals the exact one wherever nothing leaves W bits; the sort model is bigint_pip.sort_rows' loop; the exam model's
named cases do what their tags say."""
import numpy as np
import pytest

import bigint_pip as bp
import select_cases as sc
import select_model as sm

ALL = sc.column_cases()


def test_lists_are_deterministic():
    again = sc.column_cases(fresh=True)
    assert again is not ALL
    assert [t.key() for t in again] == [t.key() for t in ALL]
    assert [(t.key(), w and w.key()) for t, w in sc.sort_cases()] == [(t.key(), w and w.key()) for t, w in sc.sort_cases()]
    for fn in sc.EXAM_NI:
        assert [t.key() for t in sc.exam_cases(fn)] == [t.key() for t in sc.exam_cases(fn)]
    a, fa = sc.guard_tableaux()
    b, fb = sc.guard_tableaux()
    assert (a == b).all() and fa == fb


def test_every_case_is_a_tableau_the_probe_holds():
    for t in ALL:
        assert t.W % 2 == 0 and t.nvar <= t.ncol <= t.W and t.ni <= sc.SLOTS and t.nligne <= sc.ROWS, t.tag
        assert 0 <= t.pivi < t.nligne and not t.ref[t.pivi] & sm.UNITBIT, t.tag
        real = sorted(rf for rf in t.ref if not rf & sm.UNITBIT)
        assert real == list(range(t.ni)), t.tag                      # every slot is one logical row
        units = [rf & 0x3FF for rf in t.ref if rf & sm.UNITBIT]
        assert len(set(units)) == len(units) and all(j < t.nvar for j in units), t.tag
        assert any(sc.admits(t, f) for f in sc.FLAVOURS), t.tag       # nobody's case is nobody's test


@pytest.mark.parametrize("flavour", list(sc.FLAVOURS))
def test_flavour_gets_its_cases(flavour):
    f = sc.FLAVOURS[flavour]
    g = f["geom"]
    cases = sc.flavour_cases(flavour)
    ids = {id(t) for t in cases}
    assert len(cases) >= 300
    # condition, not a measurement: nothing a flavour's precondition admits is dropped -- the precondition recomputed here
    for t in ALL:
        prow = t.rows[t.ref[t.pivi]]
        cands = [j for j in range(t.nvar) if prow[j] > 0]
        shape = (t.W <= g.WP and t.nvar <= g.WP and all(-(1 << (g.BITS - 1)) <= x < (1 << (g.BITS - 1)) for r in t.rows for x in r))
        if g.lean:
            shape = shape and t.nvar < t.W and t.ncol == t.nvar + 1
        ok = shape
        if ok and not f.get("slow"):
            amax = max([prow[j] for j in cands] + [0])
            others = [abs(x) for s, r in enumerate(t.rows) if s != t.ref[t.pivi] for x in r]
            everything = others + [abs(x) for x in prow]
            ok = (amax.bit_length() + max(others + [0]).bit_length() <= f["PB"] - 2 and max(everything).bit_length() <= f["EB"] and
                  all(sm.UNITBIT | j in t.ref for j in cands))
        assert ok == (id(t) in ids), (flavour, t.tag)
    # every tag family the flavour is due
    fams = {sc.family(t) for t in cases}
    assert sc.required_tags(flavour) <= fams, sorted(sc.required_tags(flavour) - fams)
    top = sc.max_candidate_column(flavour)
    seen_cols = set()
    for t in cases:
        seen_cols.update(sm.candidates(t))
    for c in sc.COLS:
        if c <= top:
            assert c in seen_cols, (flavour, c)
            assert any(sm.fold_column(t) == c and len(sm.candidates(t)) > 1 for t in cases if c in sm.candidates(t)), (flavour, c)
    assert top in seen_cols
    if flavour == "C128_8":
        assert {448, 449, 510, 511} <= seen_cols
    if g.NM > 1:   # tied columns in different registers / chunks
        assert any(len({g.bit(j)[0] for j in sm.candidates(t)}) == min(g.NM, len(sm.candidates(t))) > 1 for t in cases if sc.family(t) == "regs")
    # both sides of the pivot row, at every deciding row
    for R in sc.DECIDERS:
        sides = {t.pivi < R for t in cases if sc.family(t) == "decide%d" % R}
        assert sides == ({False} if R == 0 else {False, True}), (flavour, R)
        assert all(not t.ref[R] & sm.UNITBIT and R != t.pivi for t in cases if sc.family(t) == "decide%d" % R)
    if not f.get("slow"):
        # magnitudes at the flavour's admitted maximum: entries AT the maximum, cross products that differ by 1, equal ratios
        mine = sc.own_bands(flavour)
        assert mine, flavour
        for ab, eb in mine:
            b = "a%de%d" % (ab, eb)
            got = {sc.family(t) for t in cases if sc.band(t) == b}
            assert {"max", "near", "equal-ratio-large"} <= got and len(got) > 15, (flavour, b, sorted(got))
            assert any(sm.magnitudes(t) == (ab, eb) for t in cases if sc.band(t) == b and sc.family(t) == "max")
        for t in cases:   # inside the domain: no cross product of the fold leaves the arithmetic's width
            seen = []
            sm.fold_column(t, None, seen)
            assert max(seen + [0]) <= f["PB"] - 1, t.tag
    else:
        W = g.BITS
        wrapped = [t for t in cases if sm.fold_column(t, W) != sm.fold_column(t)]
        assert len(wrapped) >= 20 and any(sc.family(t) == "wrap" for t in wrapped)
        assert any("MIN" in t.tag for t in cases) and any("2^(W-1)" in t.tag for t in cases)


def test_fold_model_is_pick_column_and_the_lexicographic_minimum():
    for t in ALL:
        col = sm.fold_column(t)
        assert col == sm.brute_column(t), t.tag
        # bigint_pip.pick_column on the same tableau
        rows = []
        for rf in t.ref:
            rows.append(bp._Row(bp.UNIT, 1, None, rf & 0x3FF) if rf & sm.UNITBIT else bp._Row(bp.UNKNOWN, 1, np.array(t.rows[rf], dtype=object)))
        if t.ni * t.nvar <= 4000:
            assert bp.pick_column(rows, t.pivi, t.nvar, t.nligne, bp.Stats(64)) == col, t.tag
    assert sum(1 for t in ALL if sm.fold_column(t) != (sm.candidates(t) + [-1])[0]) > 300   # (the first candidate is no answer)


@pytest.mark.parametrize("W", [64, 128])
def test_wrap_model_is_the_exact_model_where_nothing_wraps(W):
    fits = differs = 0
    for t in ALL:
        if max(abs(x) for r in t.rows for x in r) >> (W - 1):
            continue
        seen = []
        exact = sm.fold_column(t, None, seen)
        if max(seen + [0]) < W:
            fits += 1
            assert sm.fold_column(t, W) == exact, t.tag
        elif sm.fold_column(t, W) != exact:
            differs += 1
    assert fits > 500 and differs >= 20
    # the named wrap cases do what they say
    for t in ALL:
        if t.tag.startswith("wrap: cross product") and t.tag.endswith("W%d" % W):
            prow = t.rows[t.ref[t.pivi]]
            x = prow[0] * sm.cell(t, t.pivi + 1, 1) - sm.cell(t, t.pivi + 1, 0) * prow[1]
            assert x != 0 and x % (1 << W) == 0, t.tag


def test_sort_model_is_bigint_pips_loop():
    """on freshly loaded tableaux: the sizes and smax bigint_pip.sort_rows computes, given to the model, order the rows as
    bigint_pip.sort_rows does"""
    rng = np.random.default_rng(11)
    for trial in range(40):
        nvar, ni = int(rng.integers(1, 5)), int(rng.integers(0, 80))
        ineq = rng.integers(-6, 7, size=(ni, nvar + 1))
        rows = [bp._Row(bp.UNIT, 1, None, i) for i in range(nvar)]
        rows += [bp._Row(bp.UNKNOWN, 1, np.array([int(x) for x in r], dtype=object)) for r in ineq]
        for k in rng.integers(nvar, nvar + ni, size=ni // 8):       # a few unit rows inside the range
            rows[k] = bp._Row(bp.UNIT, 1, None, 0)
        mine = list(rows)
        bp.sort_rows(rows, nvar, nvar + ni)
        real = [r for r in mine if not r.flag & bp.UNIT]
        smax = max([float(r.size) for r in real] + [0.0])
        ref = [sm.UNITBIT | r.unit if r.flag & bp.UNIT else real.index(r) for r in mine]
        W = (nvar + 2) & ~1
        t = sm.Tab("fresh", nvar, nvar + 1, W, ref, [[int(x) for x in r.v] + [0] * (W - nvar - 1) for r in real],
                   size=[float(r.size) for r in real], smax=smax)
        want = [sm.UNITBIT | r.unit if r.flag & bp.UNIT else real.index(r) for r in rows]
        assert sm.sort_ref(t) == want


def test_sort_cases():
    pairs = sc.sort_cases()
    ns = {t.nligne - t.nvar for t, _ in pairs}
    assert ns == set(sc.SORT_N)
    moved = 0
    for t, twin in pairs:
        n = t.nligne - t.nvar
        assert t.ni <= sc.SLOTS and t.nligne <= sc.ROWS
        assert (twin is not None) == (n <= 64)
        ref = sm.sort_ref(t)
        assert sorted(ref) == sorted(t.ref) and [rf for rf in ref if rf & sm.UNITBIT] == [rf for rf in t.ref if rf & sm.UNITBIT]
        assert all((ref[k] == t.ref[k]) for k in range(t.nligne) if t.ref[k] & sm.UNITBIT)      # unit rows stay where they are
        moved += ref != t.ref
        if twin is not None:
            assert twin.nligne - twin.nvar == 65 and twin.ref[:t.nligne] == t.ref and twin.size[:t.ni] == t.size
            assert all(twin.size[s] == np.float32(twin.smax) for s in twin.ref[t.nligne:])
            tref = sm.sort_ref(twin)
            assert tref[:t.nligne] == ref and tref[t.nligne:] == twin.ref[t.nligne:], twin.tag
        if "all at or above smax" in t.tag:
            assert ref == t.ref
        if "sorted" in t.tag and "above all" in t.tag and "no unit" in t.tag:
            assert ref == t.ref
    assert moved > 150
    tags = " | ".join(t.tag for t, _ in pairs)
    for word in ("equal sizes", "smax the maximum", "smax above all", "all at or above smax", "zero and 2^31", "unit rows at the ends",
                 "unit rows in the middle", "sorted", "reverse"):
        assert word in tags
    assert any(sc.BIGF in t.size and 0.0 in t.size for t, _ in pairs)


@pytest.mark.parametrize("fn", list(sc.EXAM_NI))
def test_exam_cases(fn):
    cases = sc.exam_cases(fn)
    slots, rows = (sc.SLOTS_NW4, sc.ROWS_NW4) if fn == sc.FN_EXAM4 else (sc.SLOTS, sc.ROWS)
    assert {t.ni for t in cases} == set(sc.EXAM_NI[fn])
    fams = set()
    for t in cases:
        assert t.ni <= slots and t.nligne <= rows and t.W % 2 == 0 and t.ncol <= t.W
        assert t.srow() != sorted(t.srow()) or t.ni < 3            # slots permuted against logical order
        i, fl = sm.exam_coef(t)
        fam = t.tag.split(":")[0]
        fams.add((fam, t.ni))
        changed = [s for s in range(t.ni) if fl[s] != t.fl[s]]
        assert all(t.fl[s] == sm.UNKNOWN for s in changed), t.tag          # only Unknown rows may change
        srow = t.srow()
        if i < t.nligne:
            assert fl[t.ref[i]] == sm.MINUS and t.fl[t.ref[i]] == sm.UNKNOWN
            assert all(srow[s] <= i or t.bigparm >= 0 for s in changed), t.tag      # rows behind the one returned keep their flag
        big = [(srow[s], r[t.bigparm]) for s, r in enumerate(t.rows) if t.fl[s] == sm.UNKNOWN] if t.bigparm >= 0 else []
        if fam == "exam big-negative":
            first = min(k for k, b in big if b < 0)
            assert i == first
            if first > min(srow):   # the big-zero row before it, Minus by its parameters alone, is not returned and stays Unknown
                zs = [s for s in range(t.ni) if srow[s] < first and t.rows[s][t.bigparm] == 0 and t.rows[s][t.nvar] < 0]
                assert t.ni == 1 or (zs and all(fl[s] == sm.UNKNOWN for s in zs)), t.tag
        if fam == "exam no-big-negative":
            assert not any(b < 0 for _, b in big)
        if fam == "exam paf":
            assert i == t.nligne and fl == t.fl
        if fam == "exam several-minus":
            minus = sorted(srow[s] for s in range(t.ni) if t.rows[s][t.nvar] < 0)
            assert i == minus[0] and all(fl[t.ref[k]] == sm.UNKNOWN for k in minus[1:])
    for ni in sc.EXAM_NI[fn]:
        for fam in ("exam big-negative", "exam no-big-negative", "exam paf", "exam both-signs", "exam no-parameter", "exam zero-parameter",
                    "exam several-minus", "exam mixed-flags"):
            assert (fam, ni) in fams, (fam, ni)
    assert any(len(set(t.fl)) >= 4 for t in cases)


def test_publish_model_by_hand():
    """the summaries' geometry on one row, worked out by hand from the comments of Shared<T> and the lean flavours"""
    row = [0] * 72
    row[5], row[70], row[3] = -(1 << 15), 7, 2      # column 3: the constant term
    t = sm.Tab("hand", 3, 4, 72, [0], [row])
    #                                         sig  cls  cst  bitmap words
    assert sm.publish(t, sm.Geometry(64, 2, 1))[0] == [(1, 1, 2, [1 << 35, (1 << 2) | (1 << 1)])]             # word h, bit j / 2
    assert sm.publish(t, sm.Geometry(128, 1, 4))[0] == [(1, 0, 2, [(1 << 5) | (1 << 3), 1 << 6, 0, 0])]       # word j / 64, bit j % 64
    assert sm.publish(t, sm.Geometry(64, 2, 1, lean=32))[0] == [(1, 1, 2, [1 << 35, (1 << 2) | (1 << 1)])]
    assert sm.publish(t, sm.Geometry(128, 1, 4, lean=64))[0] == [(1, 0, 2, [(1 << 5) | (1 << 3), 1 << 6, 0, 0])]
    g = sm.Geometry(64, 2, 1)
    assert [g.cls(x) for x in ((1 << 15) - 1, 1 << 15, (1 << 31) - 1, 1 << 31, (1 << 47) - 1, 1 << 47, 1 << 63)] == [0, 1, 1, 2, 2, 3, 3]
    g = sm.Geometry(128, 1, 1)
    assert [g.cls(x) for x in ((1 << 31) - 1, 1 << 31, (1 << 63) - 1, 1 << 63, (1 << 95) - 1, 1 << 95)] == [0, 1, 1, 2, 2, 3]
    # parameters and the big one: bits 2-3 and 4-5
    t = sm.Tab("parm", 1, 4, 4, [0], [[1, -1, 0, -3], [1, 0, 2, 0], [0, 0, 2, -1]], bigparm=3)
    assert [p[0] for p in sm.publish(t, sm.Geometry(64, 2, 1))[0]] == [2 | 8 | 32, 4, 4 | 8 | 32]


def test_guard_tableaux_need_the_slow_fold():
    """the end-to-end batch holds every pair of magnitude classes, and at least 8 tableaux on which the first pivot's
    wrapped fold -- what the reference's 64-bit build computes -- picks another column than the exact one"""
    rows, firsts = sc.guard_tableaux()
    assert len(rows) >= 40 and rows.shape[1:] == (sc.GUARD_NI, sc.GUARD_NVAR + 1) and len(firsts) == len(rows)
    assert {(ca, ce) for _, _, ca, ce in firsts} == {(a, e) for a in range(4) for e in range(4)}
    differ = [(ex, wr, ca, ce) for ex, wr, ca, ce in firsts if ex != wr]
    assert len(differ) >= 8
    # the guard's own rule, on the classes: they all lie where it rejects the tournament
    bits = (15, 31, 47, 64)
    assert all(bits[ca] + bits[ce] > 62 for _, _, ca, ce in differ)
    # where the rule admits the tournament the two folds agree
    assert all(ex == wr for ex, wr, ca, ce in firsts if bits[ca] + bits[ce] <= 62)


def test_the_oracle_solves_the_guard_tableaux():
    """the oracle library's 64-bit wrap-around build runs every tableau of the batch past its second pivot, or ends it with
    the reference's overflow exit -- what tests/test_gpu_select_probe.py compares the kernel with"""

    import pipbatch as pb
    from piplib_amd import synth
    rows, firsts = sc.guard_tableaux()
    probs = [synth.Problem(sc.GUARD_NVAR, 0, rows.shape[1], 0, -1, 1, rows[b], np.zeros((0, 1), np.int64)) for b in range(len(rows))]
    res = pb.run_batch(pb.ORACLEPIP, probs, pb.F_NOSIMPLIFY).results
    assert len(res) == len(rows) and all(r.status == pb.ST_ABORT or r.pivots >= 2 for r in res)
