"""-m gpu: Batch(matrices=True) -- PolyLib matrices with a row count and equalities per system for the batch layer
(pipamd_batch_load_matrices, pipamd_batch_dual_matrices; pip_batch_load_system_kernel and pip_batch_dual_kernel with the
PipEqMarkers policy, csrc/pip_kernels.hip).

The ragged batches of tests/matrices_cases.py are compared with the authorities that exist:
  (a) the CPU oracle on the model's tableau of every system (system_model.tableau on its kept rows and equalities):
      status, pivot count and solution;
  (b) the uniform path: every class's systems as one Batch(system=True, eq_rows=...) through pipamd_batch_load_system --
      status, pivots, cuts, sol_num / sol_den, x_num / x_den and the dual pairs of the ragged batch equal that batch's bit
      for bit, system by system (those batches have another ni, so another number of spare rows: a tableau's spare room
      does not leak into its result);
  (c) for r5 the reference's printed answers, duals and pivot counts of tests/golden/matrices/r5.json.
No system is left out of a comparison; the bulk case compares with (a) alone."""
import functools

import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

MODES = {"int-simplify": (1, 1, 0), "int-plain": (1, 0, 0), "rational-dual": (0, 0, 1)}  # nq, simplify, dual
OPTS = {0: "", 1: "Maximize", -1: "Urs_unknowns"}
SHIFTS = dict(argvalues=[0, 1, -1], ids=["plain", "maximize", "urs"])
ARRAYS = ("status", "pivots", "cuts", "sol_num", "sol_den")


@functools.lru_cache(maxsize=None)
def _expected(name, box, shift, nq, simp):
    """(a): the oracle's result per system, run class by class (a class's tableaux have one shape); once per case"""
    import matrices_cases as mc
    import pipbatch as pb
    from gpu_common import oracle_batch
    fam = mc.family(name, box)
    res = [None] * len(fam.systems)
    for c in range(len(fam.classes)):
        out = oracle_batch(mc.tableaux(fam, c, shift, simp), fam.nvar, 1 if shift else 0, nq, bigparm=fam.nvar + 1 if shift else -1)
        for b, r in zip(mc.members(fam, c), out.results):
            assert r.status == pb.ST_OK
            res[b] = r
    assert all(r is not None for r in res)
    return res


def _engine(lean_big=False):
    from piplib_amd import engine as eng
    e = eng.Engine(0)
    e.set_lean_big(lean_big)
    return e


def _tflags(nq, dual):
    from piplib_amd import engine as eng
    return (eng.T_INT if nq else 0) | (eng.T_DUAL if dual else 0) | eng.T_ROWS_STAY  # (ROWS_STAY is ignored)


def _finish(b, dual=None):
    import torch
    b.solve()
    b.fetch()
    if b.shift:
        b.fetch_shifted()
    if dual is not None:
        b.dual_pair = dual(b)
    torch.cuda.synchronize()
    return b


def _solve_ragged(room, nrows, nvar, ni, shift, nq, simp, dual, bits=64, halves=False, e=None):
    """room: (batch, max_rows, nvar + 2) matrices; nrows: (batch,) int32 or None; ni: the room for the tallest tableau"""
    import torch
    from piplib_amd import engine as eng
    b = eng.Batch(e or _engine(), None if halves else room, nvar, 0, tflags=_tflags(nq, dual), entier_bits=bits, shift=shift,
                  shape=room.shape, matrices=True, nrows=None if halves else nrows, ni=ni, simplify=simp)
    assert b.desc.ni == ni and b.matrices.max_rows == room.shape[1]
    if not halves:
        b.load_matrices()
        return _finish(b, (lambda b: b.dual_matrices()) if dual else None)
    h = room.shape[0] // 2 + 3
    dev = torch.as_tensor(room, dtype=torch.int64).to(b.dev)
    cnt = torch.as_tensor(nrows, dtype=torch.int32).to(b.dev)
    parts = [(dev[:h].contiguous(), cnt[:h].contiguous()), (dev[h:].contiguous(), cnt[h:].contiguous())]
    b.load_matrices_part(parts[0][0], parts[0][1], 0)
    b.load_matrices_part(parts[1][0], parts[1][1], h)

    def two(b):
        out = b.dual_matrices_part(parts[0][0], parts[0][1], 0)
        return b.dual_matrices_part(parts[1][0], parts[1][1], h, out=out)
    return _finish(b, two if dual else None)


def _solve_family(fam, shift, nq, simp, dual, bits=64, halves=False, e=None):
    return _solve_ragged(fam.room, fam.nrows, fam.nvar, fam.ni, shift, nq, simp, dual, bits, halves, e)


def _solve_uniform(rows, nvar, eq, shift, nq, simp, dual, bits=64, e=None):
    """(b): same-shaped plain systems through pipamd_batch_load_system / pipamd_batch_dual_system"""
    from piplib_amd import engine as eng
    b = eng.Batch(e or _engine(), rows, nvar, 0, tflags=_tflags(nq, dual), entier_bits=bits, shift=shift, system=True, eq_rows=eq,
                  simplify=simp)
    assert b.desc.ni == rows.shape[1] + len(eq)
    b.load_system()
    return _finish(b, (lambda b: b.dual_system()) if dual else None)


def _ints(t, bits):
    from piplib_amd import engine as eng
    a = t.cpu().numpy()
    return eng.wide_to_int(a) if bits == 128 else a.astype(object)


def _same(a, b, names=ARRAYS):
    import torch
    for name in names:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    if a.shift:
        assert torch.equal(a.x_num, b.x_num) and torch.equal(a.x_den, b.x_den)
    if hasattr(a, "dual_pair"):
        assert torch.equal(a.dual_pair[0], b.dual_pair[0]) and torch.equal(a.dual_pair[1], b.dual_pair[1])


def _against_oracle(b, res, bits=64, members=None):
    """(a) every system (or the listed ones, res in their order): status, pivots and the solution as the oracle has them"""
    import pipbatch as pb
    from gpu_common import solution_text
    from piplib_amd import engine as eng
    st, pv = b.status.cpu().numpy(), b.pivots.cpu().numpy()
    num, den = _ints(b.sol_num, bits), _ints(b.sol_den, bits)
    solved = 0
    for k, r in zip(members if members is not None else range(len(res)), res):
        want = pb.squash(r.text)
        assert st[k] == (eng.ST_NIL if want == "()" else eng.ST_SOLUTION), (k, st[k], want[:60])
        assert pv[k] == r.pivots, (k, pv[k], r.pivots)
        if want != "()":
            assert pb.squash(solution_text(num[k], den[k])) == want, (k, want[:120])
            solved += 1
        else:
            assert not num[k].any() and not den[k].any(), k
    return solved


def _against_uniform(b, fam, shift, nq, simp, dual, bits, e):
    """(b) class by class: every array of the ragged batch, at the class's systems, equals the uniform batch's"""
    import matrices_cases as mc
    import torch
    seen = 0
    for c, (kept, eq) in enumerate(fam.classes):
        rows, eq = mc.class_rows(fam, c)
        u = _solve_uniform(rows, fam.nvar, eq, shift, nq, simp, dual, bits, e)
        idx = torch.as_tensor(mc.members(fam, c), device=b.dev)
        for name in ARRAYS + (("x_num", "x_den") if shift else ()):
            assert torch.equal(getattr(b, name)[idx], getattr(u, name)), (c, name)
        if dual:
            for got, want in zip(b.dual_pair, u.dual_pair):
                assert got.shape[1] == fam.max_rows and want.shape[1] == len(kept)
                assert torch.equal(got[idx][:, :len(kept)], want), c
                assert not got[idx][:, len(kept):].any(), c  # (0, 0) from the system's row count on
        seen += len(idx)
    assert seen == len(fam.systems)


def _answers(b, bits):
    """pip_solve's list per system, [[numerator, denominator], ...] in lowest terms, None without a solution"""
    import system_model as sy
    from piplib_amd import engine as eng
    st = b.status.cpu().numpy()
    if b.shift:
        xn, xd = _ints(b.x_num, bits), _ints(b.x_den, bits)
        return [[[int(n), int(d)] for n, d in zip(xn[k], xd[k])] if st[k] == eng.ST_SOLUTION else None for k in range(len(st))]
    sn, sd = _ints(b.sol_num, bits), _ints(b.sol_den, bits)
    return [[list(sy.reduce_pair(sn[k][i][0], sd[k][i])) for i in range(sd.shape[1])] if st[k] == eng.ST_SOLUTION else None
            for k in range(len(st))]


def _duals(b, bits):
    n, d = _ints(b.dual_pair[0], bits), _ints(b.dual_pair[1], bits)
    return [[[int(x), int(y)] for x, y in zip(nr, dr)] for nr, dr in zip(n, d)]


@functools.lru_cache(maxsize=None)
def _golden():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matrices", "r5.json")) as f:
        return json.load(f)


def _against_golden(b, fam, shift, nq, simp, dual, bits):
    """(c) the reference's printed answers, duals and pivot counts"""
    opts = OPTS[shift] + ("+" if shift and dual else "") + ("Rational+Dual" if dual else "")
    want = _golden()["cases"][f"box{fam.box},{opts}"]
    got_x = _answers(b, bits)
    assert got_x == want["x"]
    if simp or not nq:  # (the reference's pivot counts are those of the simplified tableau)
        assert b.pivots.cpu().tolist() == want["pivots"]
    if dual:
        got_d = _duals(b, bits)
        for k, (rows, eq) in enumerate(fam.systems):
            w = want["dual"][k]
            assert (w is None) == (got_x[k] is None), k
            pad = [[0, 0]] * (fam.max_rows - len(rows))
            assert got_d[k] == (w if w is not None else [[0, 0]] * len(rows)) + pad, (k, got_d[k], w)


def _check_case(name, box, shift, mode, bits=64, golden=False):
    import matrices_cases as mc
    nq, simp, dual = MODES[mode]
    fam = mc.family(name, box)
    e = _engine()
    b = _solve_family(fam, shift, nq, simp, dual, bits, e=e)
    solved = _against_oracle(b, _expected(name, box, shift, nq, simp), bits)
    _against_uniform(b, fam, shift, nq, simp, dual, bits, e)
    if golden:
        _against_golden(b, fam, shift, nq, simp, dual, bits)
    return b, solved


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shift", **SHIFTS)
@pytest.mark.parametrize("box", [0, 1])
def test_r5(box, shift, mode):
    b, solved = _check_case("r5", box, shift, mode, golden=True)
    assert solved >= 6


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shift", **SHIFTS)
@pytest.mark.parametrize("box", [0, 1])
def test_r5_128_bit_entries(box, shift, mode):
    """(low, high) pairs; the values fit 64 bits, so everything equals the goldens too"""
    b, solved = _check_case("r5", box, shift, mode, bits=128, golden=True)
    assert solved >= 6


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shift", **SHIFTS)
@pytest.mark.parametrize("name,bits", [("t3", 64), ("w70", 64), ("w131", 64), ("w131", 128)])
def test_mask_word_edge_and_wide_rows(name, bits, shift, mode):
    """t3: 63, 64, 65 and 70 rows with equalities on both sides of a mask word's edge; w70 / w131: a row spans more than
    64 lanes / takes the load's eight-columns-a-lane instantiation"""
    b, solved = _check_case(name, 1, shift, mode, bits=bits)
    assert solved >= 4


@pytest.mark.parametrize("shift,lean_big", [(0, False), (1, True), (1, False)], ids=["plain", "maximize-lean", "maximize-general"])
def test_bulk_through_the_lean_launches(shift, lean_big):
    """2,048 systems of six classes, integer with tab_simplify: every system against the oracle, (a) alone"""
    import matrices_cases as mc
    fam = mc.family("bulk12", 1)
    b = _solve_family(fam, shift, 1, 1, 0, e=_engine(lean_big))
    assert b.e.last_solve_launches() >= 2
    solved = _against_oracle(b, _expected("bulk12", 1, shift, 1, 1))
    assert 100 <= solved < len(fam.systems)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shift", [0, -1], ids=["plain", "urs"])
def test_parts_equal_one_call(shift, mode):
    """the batch loaded in two parts and the dual fetched in two parts, each part with its own rows and row counts"""
    import matrices_cases as mc
    nq, simp, dual = MODES[mode]
    fam = mc.family("r5", 1)
    a = _solve_family(fam, shift, nq, simp, dual)
    h = _solve_family(fam, shift, nq, simp, dual, halves=True)
    _same(a, h)
    _against_oracle(h, _expected("r5", 1, shift, nq, simp))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shift", **SHIFTS)
def test_no_row_counts_as_the_system_entry(shift, mode):
    """d_nrows == NULL: every system has max_rows rows; with s5's equalities written as markers the batch equals
    pipamd_batch_load_system on the same rows in every array and in the dual"""
    import numpy as np
    import system_model as sy
    nq, simp, dual = MODES[mode]
    g = sy.golden("s5")
    rows, nvar, eq = sy.family_rows(g, 1), g["nvar"], sy.EQ_ROWS["s5"]
    marker = np.ones(rows.shape[:2] + (1,), np.int64)
    marker[:, list(eq), 0] = 0
    room = np.ascontiguousarray(np.concatenate([marker, rows], axis=2))
    a = _solve_ragged(room, None, nvar, rows.shape[1] + len(eq), shift, nq, simp, dual)
    u = _solve_uniform(rows, nvar, eq, shift, nq, simp, dual)
    _same(a, u)
    assert (a.status == 1).sum().item() >= 6


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shift", [0, 1], ids=["plain", "maximize"])
def test_bad_systems_end_badinput(shift, mode):
    """eight systems of r5, four of them bad -- a row count of 0, of -1, of max_rows + 1, and an all-equality system under
    a d->ni one row too small for it --: those end ST_BADINPUT with zeros in every result and dual entry, the other four
    equal their results in a batch without the bad ones, and solve() ends as it does for that batch"""
    import matrices_cases as mc
    import numpy as np
    import torch
    from piplib_amd import engine as eng
    nq, simp, dual = MODES[mode]
    fam = mc.family("r5", 0)
    alleq = [c for c, (kept, eq) in enumerate(fam.classes) if len(eq) == len(kept) and 2 * len(kept) == fam.ni][0]
    ni = fam.ni - 1
    fits = [b for b in range(len(fam.systems)) if fam.nrows[b] + len(fam.systems[b][1]) <= ni]
    good = [mc.members(fam, c)[0] for c in (0, 1, 3, 5)]  # one row, one equality, the full system, a mid-sized one
    assert all(b in fits for b in good)
    spoil = [b for b in fits if b not in good][:3]
    pick = [spoil[0], good[0], spoil[1], good[1], good[2], spoil[2], mc.members(fam, alleq)[0], good[3]]
    bad, ok = [0, 2, 5, 6], [1, 3, 4, 7]
    room = np.ascontiguousarray(fam.room[pick])
    nrows = fam.nrows[pick].copy()
    nrows[[0, 2, 5]] = [0, -1, fam.max_rows + 1]
    a = _solve_ragged(room, nrows, fam.nvar, ni, shift, nq, simp, dual)  # (solve() raises unless it returns PIPAMD_OK)
    c = _solve_ragged(np.ascontiguousarray(room[ok]), nrows[ok], fam.nvar, ni, shift, nq, simp, dual)
    names = ARRAYS + (("x_num", "x_den") if shift else ())
    assert a.status[bad].cpu().tolist() == [eng.ST_BADINPUT] * 4
    for name in names[1:]:
        assert not getattr(a, name)[bad].any(), name
    for name in names:
        assert torch.equal(getattr(a, name)[ok], getattr(c, name)), name
    if dual:
        for got, want in zip(a.dual_pair, c.dual_pair):
            assert not got[bad].any()
            assert torch.equal(got[ok], want)
    res = _expected("r5", 0, shift, nq, simp)
    assert _against_oracle(a, [res[pick[k]] for k in ok], members=ok) >= 1
