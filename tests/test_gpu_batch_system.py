"""-m gpu: Batch(system=True) -- pip_solve's plain system for the batch layer (pipamd_batch_load_system,
pipamd_batch_dual_system; pip_batch_load_system_kernel and pip_batch_dual_kernel<T, PipEqMask>, csrc/pip_kernels.hip).

Authorities: tests/system_model.py (Python ints; tests/test_system_model.py holds it to the reference's pip_solve), the CPU
oracle on the model's tableau (status, pivots, solution), the same tableau loaded with pipamd_batch_load (cuts and the
solution arrays bit for bit), and the reference's printed answers and duals of tests/golden/system/.  No system is left
out of any comparison."""
import functools

import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

KW = dict(nnz=3, cmax=4, x0max=6)
# families beyond the golden ones: name -> (seed, nvar, nrows, batch, keywords, equality rows)
WIDE = {"w70": (43, 70, 12, 16, KW, (0, 11)),     # a row spans more than 64 lanes; the last row's negation ends the tableau
        "w131": (44, 131, 8, 8, KW, (3,)),        # more than 128 columns: the load's eight-columns-a-lane instantiation
        "bulk12": (42, 12, 10, 2048, KW, (2, 9))}  # s12's generator with batch 2,048: the lean launches
MODES = {"int-simplify": (1, 1, 0), "int-plain": (1, 0, 0), "rational-dual": (0, 0, 1)}  # nq, simplify, dual
OPTS = {0: "", 1: "Maximize", -1: "Urs_unknowns"}


@functools.lru_cache(maxsize=None)
def _family(name, box):
    """(plain rows (read-only), nvar, equality rows)"""
    import shift_cases as sc
    import system_model as sy
    if name in WIDE:
        seed, nvar, nrows, batch, kw, eq = WIDE[name]
        rows = sc.plain_rows(seed, nvar, nrows, batch, kw, box)
    else:
        g = sy.golden(name)
        rows, nvar, eq = sy.family_rows(g, box), g["nvar"], sy.EQ_ROWS[name]
    rows.setflags(write=False)
    return rows, nvar, eq


@functools.lru_cache(maxsize=None)
def _expected(name, box, shift, nq, simp):
    """(the model's tableaux, the oracle's results on them); computed once per case"""
    import pipbatch as pb
    import system_model as sy
    from gpu_common import oracle_batch
    rows, nvar, eq = _family(name, box)
    tab = sy.tableaux(rows, eq, shift, simp)
    res = oracle_batch(tab, nvar, 1 if shift else 0, nq, bigparm=nvar + 1 if shift else -1).results
    assert all(r.status == pb.ST_OK for r in res)
    return tab, res


def _engine(lean_big=False, bulk_min=None):
    from piplib_amd import engine as eng
    e = eng.Engine(0)
    if bulk_min:
        e.set_bulk_min(bulk_min)
    e.set_lean_big(lean_big)
    return e


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


def _solve_system(rows, nvar, eq, shift, nq, simp, dual, bits=64, halves=False, e=None):
    import torch
    from piplib_amd import engine as eng
    tflags = (eng.T_INT if nq else 0) | (eng.T_DUAL if dual else 0) | eng.T_ROWS_STAY  # (ROWS_STAY is ignored)
    b = eng.Batch(e or _engine(), None if halves else rows, nvar, 0, tflags=tflags, entier_bits=bits, shift=shift, shape=rows.shape,
                  system=True, eq_rows=eq, simplify=simp)
    assert b.desc.ni == rows.shape[1] + len(eq)
    if not halves:
        b.load_system()
        return _finish(b, (lambda b: b.dual_system()) if dual else None)
    h = rows.shape[0] // 2 + 3
    dev = torch.as_tensor(rows, dtype=torch.int64).to(b.dev)
    parts = [dev[:h].contiguous(), dev[h:].contiguous()]
    b.load_system_part(parts[0], 0)
    b.load_system_part(parts[1], h)

    def two(b):
        out = b.dual_system_part(parts[0], 0)
        return b.dual_system_part(parts[1], h, out=out)
    return _finish(b, two if dual else None)


def _solve_tableau(tab, nvar, shift, nq, bits=64, e=None, loader_shift=0):
    """the existing loads: pipamd_batch_load on a finished tableau, or pipamd_batch_load_shifted on plain rows"""
    from piplib_amd import engine as eng
    big = bool(shift) and not loader_shift
    b = eng.Batch(e or _engine(), tab, nvar, 1 if big else 0, bigparm=nvar + 1 if big else -1, tflags=eng.T_INT if nq else 0,
                  entier_bits=bits, shift=loader_shift)
    b.load()
    return _finish(b)


def _ints(t, bits):
    from piplib_amd import engine as eng
    a = t.cpu().numpy()
    return eng.wide_to_int(a) if bits == 128 else a.astype(object)


def _same(a, b, names=("status", "pivots", "cuts", "sol_num", "sol_den")):
    import torch
    for name in names:
        assert torch.equal(getattr(a, name), getattr(b, name)), name


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


def _against_oracle(b, res, nvar, bits=64):
    """every system: status, pivots and the solution as the oracle has them on the model's tableau"""
    import pipbatch as pb
    from gpu_common import solution_text
    from piplib_amd import engine as eng
    st, pv = b.status.cpu().numpy(), b.pivots.cpu().numpy()
    num, den = _ints(b.sol_num, bits), _ints(b.sol_den, bits)
    solved = 0
    for k, r in enumerate(res):
        want = pb.squash(r.text)
        assert st[k] == (eng.ST_NIL if want == "()" else eng.ST_SOLUTION), (k, st[k], want[:60])
        assert pv[k] == r.pivots, (k, pv[k], r.pivots)
        if want != "()":
            assert pb.squash(solution_text(num[k], den[k])) == want, (k, want[:120])
            solved += 1
        else:
            assert not num[k].any() and not den[k].any(), k
    return solved


def _check_case(name, box, shift, mode, bits=64, halves=False, golden=True):
    import system_model as sy
    nq, simp, dual = MODES[mode]
    rows, nvar, eq = _family(name, box)
    tab, res = _expected(name, box, shift, nq, simp)
    b = _solve_system(rows, nvar, eq, shift, nq, simp, dual, bits, halves)
    solved = _against_oracle(b, res, nvar, bits)
    # the model's tableau through pipamd_batch_load: cuts and the solution arrays, bit for bit
    _same(b, _solve_tableau(tab, nvar, shift, nq, bits))
    got_x = _answers(b, bits)
    opts = OPTS[shift] + ("+" if shift and dual else "") + ("Rational+Dual" if dual else "")
    if golden:
        want = sy.golden(name)["cases"][f"box{box},{opts}"]
        assert got_x == want["x"]
        if simp or not nq:  # (the reference's pivot counts are those of the simplified tableau)
            assert b.pivots.cpu().tolist() == want["pivots"]
    if dual:
        got_d = _duals(b, bits)
        nrows = rows.shape[1]
        for k in range(len(rows)):
            if golden:
                w = want["dual"][k]
            else:
                t = sy.oracle_tableau_dual(rows[k], eq, opts)
                w = None if t is None else [list(p) for p in sy.dual(t, nrows, eq)]
            assert (w is None) == (got_x[k] is None), k
            assert got_d[k] == (w if w is not None else [[0, 0]] * nrows), (k, got_d[k], w)
    return b, solved


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shift", [0, 1, -1], ids=["plain", "maximize", "urs"])
@pytest.mark.parametrize("box", [0, 1])
@pytest.mark.parametrize("name", ["s5", "s12"])
def test_golden_families(name, box, shift, mode):
    b, solved = _check_case(name, box, shift, mode)
    assert solved >= 6


@pytest.mark.parametrize("nq", [1, 0], ids=["integer", "rational"])
@pytest.mark.parametrize("shift", [0, 1, -1], ids=["plain", "maximize", "urs"])
def test_without_equalities_as_the_existing_loads(shift, nq):
    """neq == 0, simplify == 0: the tableau of pipamd_batch_load (shift 0) / pipamd_batch_load_shifted on the same rows"""
    rows, nvar, _ = _family("s12", 1)
    b = _solve_system(rows, nvar, (), shift, nq, 0, 0)
    c = _solve_tableau(rows, nvar, shift, nq, loader_shift=shift)
    _same(b, c)
    if shift:
        _same(b, c, ("x_num", "x_den"))
    assert (b.status == 1).sum().item() >= 6


def test_dual_without_equalities_as_the_plain_dual():
    """neq == 0, shift 0, rational with dual: dual_system() is dual() of the same rows loaded with pipamd_batch_load,
    each pair reduced -- one comparison over the whole batch"""
    import system_model as sy
    from piplib_amd import engine as eng
    rows, nvar, _ = _family("s12", 1)
    b = _solve_system(rows, nvar, (), 0, 0, 0, 1)
    c = eng.Batch(_engine(), rows, nvar, 0, tflags=eng.T_DUAL)
    c.load()
    c = _finish(c, lambda c: c.dual())
    _same(b, c)
    assert (b.status == 1).sum().item() >= 6
    assert _duals(b, 64) == [[list(sy.reduce_pair(n, d)) for n, d in t] for t in _duals(c, 64)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shift", [0, -1], ids=["plain", "urs"])
def test_parts_equal_one_call(shift, mode):
    """the batch loaded in two parts and the dual fetched in two parts"""
    nq, simp, dual = MODES[mode]
    rows, nvar, eq = _family("s5", 1)
    a = _solve_system(rows, nvar, eq, shift, nq, simp, dual)
    h = _solve_system(rows, nvar, eq, shift, nq, simp, dual, halves=True)
    _same(a, h)
    if dual:
        import torch
        assert torch.equal(a.dual_pair[0], h.dual_pair[0]) and torch.equal(a.dual_pair[1], h.dual_pair[1])
    _against_oracle(h, _expected("s5", 1, shift, nq, simp)[1], nvar)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shift", [0, 1, -1], ids=["plain", "maximize", "urs"])
@pytest.mark.parametrize("box", [0, 1])
def test_128_bit_entries(box, shift, mode):
    """(low, high) pairs; the values fit 64 bits, so everything equals the goldens and the 64-bit results"""
    _check_case("s5", box, shift, mode, bits=128)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shift", [0, 1, -1], ids=["plain", "maximize", "urs"])
@pytest.mark.parametrize("name,bits", [("w70", 64), ("w131", 64), ("w131", 128)])
def test_wide_rows(name, bits, shift, mode):
    b, solved = _check_case(name, 1, shift, mode, bits=bits, golden=False)
    assert solved >= 4


@pytest.mark.parametrize("shift,lean_big", [(0, False), (1, True), (1, False)], ids=["plain", "maximize-lean", "maximize-general"])
def test_bulk_through_the_lean_launches(shift, lean_big):
    """2,048 systems of s12's shape, integer with tab_simplify: every system against the oracle"""
    rows, nvar, eq = _family("bulk12", 1)
    tab, res = _expected("bulk12", 1, shift, 1, 1)
    b = _solve_system(rows, nvar, eq, shift, 1, 1, 0, e=_engine(lean_big))
    assert b.e.last_solve_launches() >= 2
    solved = _against_oracle(b, res, nvar)
    assert 100 <= solved < len(rows)
