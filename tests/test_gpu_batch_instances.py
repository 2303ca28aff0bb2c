"""-m gpu: Batch(instances=True) -- one parametric system at many parameter points (pipamd_batch_load_instances,
pipamd_batch_dual_instances; the PipInstanceRows source policy of pip_batch_load_system_kernel and pip_batch_dual_kernel,
csrc/pip_kernels.hip).

Authorities: tests/instances_model.py's expansion in Python ints (tests/test_instances_model.py holds it to the
reference) given to the dense entry, byte for byte in the workspace (pipamd_batch_load_system, itself held to
tests/system_model.py by tests/test_gpu_batch_system.py); the reference's printed answers, duals and pivot counts of
tests/golden/instances/p5.json; tests/bigint_pip.py where a constant leaves int64; the CPU oracle.  The helpers that hold
a solved batch to those are the dense test's own (tests/test_gpu_batch_system.py).  No system is left out of any
comparison."""
import functools

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

SHIFTS = [0, 1, -1]
JOB_WORDS, JOB_NI, JOB_S, JOB_W, JOB_STATUS = 25, 12, 16, 17, 18  # PipJob (csrc/pip_job.h): 200 bytes; int32 indices


def _tbs():
    import test_gpu_batch_system as tbs
    return tbs


def _flags(nq, dual):
    from piplib_amd import engine as eng
    return (eng.T_INT if nq else 0) | (eng.T_DUAL if dual else 0) | eng.T_ROWS_STAY  # (ROWS_STAY is ignored)


def _inst_batch(e, matrix, points, nvar, eq, shift, tflags, simp, bits=64):
    from piplib_amd import engine as eng
    m = np.array(matrix, dtype=np.int64).reshape(len(matrix), -1)
    p = points if isinstance(points, int) else np.array(points, dtype=np.int64).reshape(len(points), m.shape[1] - nvar - 1)
    b = eng.Batch(e, (m, p), nvar, 0, tflags=tflags, entier_bits=bits, shift=shift, instances=True, eq_rows=eq, simplify=simp)
    assert b.desc.ni == len(matrix) + len(eq) and b.desc.nparm == (1 if shift else 0)
    return b


def _solve_instances(matrix, points, nvar, eq, shift, nq, simp, dual, bits=64, e=None):
    tbs = _tbs()
    b = _inst_batch(e or tbs._engine(), matrix, points, nvar, eq, shift, _flags(nq, dual), simp, bits)
    b.load_instances()
    return tbs._finish(b, (lambda b: b.dual_instances()) if dual else None)


def _dense(matrix, points):
    import instances_model as im
    return np.array(im.expand(matrix, points), dtype=np.int64)


def _slices(b):
    """per system (its PipJob words, its block's words) of a batch's workspace; the layout of pipamd_batch_layout"""
    B = b.desc.batch
    jobs = ((B * 8 * JOB_WORDS + 255) & ~255) // 8
    words, rest = divmod(b.ws.numel() - 1 - jobs, B)
    assert rest == 0
    return [(slice(JOB_WORDS * k, JOB_WORDS * (k + 1)), slice(jobs + words * k, jobs + words * (k + 1))) for k in range(B)]


def _jobs(b):
    return b.ws[:JOB_WORDS * b.desc.batch].cpu().numpy().view(np.int32).reshape(b.desc.batch, 2 * JOB_WORDS)


# ---------------------------------------------------------------- the workspace, byte for byte

# the parameter block and the constant at the lane-block edges of the matrix row (columns 64, 128, ...), the tableau's own
# width crossing its edges; (129, 382) is a row of 512 columns
PAIRS = [(3, 0), (3, 1), (3, 2), (60, 3), (60, 4), (63, 64), (64, 65), (127, 1), (129, 63), (129, 382)]


def _eq_variants(nrows):
    return [(), (0,), (nrows - 1,), tuple(range(nrows))]


def _edge_family(nvar, nparm, nrows, combo):
    """(matrix, points) of 3 systems: rows that are all zero, the constant alone, the parameters alone, full and sparse,
    in an order that moves with `combo`; the first point is zero for every second combo; values up to 2^40 in the
    matrix and 2^20 in the points, so that no constant leaves int64"""
    rng = np.random.default_rng(7919 * nvar + 31 * nparm + combo)
    m = np.zeros((nrows, nvar + nparm + 1), np.int64)
    kinds = []
    for r in range(nrows):
        kind = (combo + r) % 5
        kinds.append(kind)
        if kind == 1 or kind >= 3:
            m[r, -1] = rng.integers(-50, 51) or 7
        if kind >= 2:
            m[r, nvar:nvar + nparm] = rng.integers(-9, 10, nparm)
            if nparm:
                m[r, nvar + rng.integers(0, nparm)] = (1 << 40) + 1
                m[r, nvar + nparm - 1] = m[r, nvar + nparm - 1] or -3  # the last parameter, next to the constant
                m[r, nvar] = m[r, nvar] or 5                           # the first one, next to the unknowns
        if kind == 3:
            m[r, :nvar] = rng.integers(-9, 10, nvar)
            m[r, nvar - 1] = m[r, nvar - 1] or 2
        if kind == 4:
            cols = rng.choice(nvar, min(nvar, 3), replace=False)
            m[r, cols] = 6 * rng.integers(1, 5, len(cols))  # a gcd for tab_simplify
    p = rng.integers(-(1 << 20), 1 << 20, (3, nparm))
    if combo % 2 == 0:
        p[0] = 0
    return m, p, kinds


@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("nvar,nparm", PAIRS)
def test_workspace_equals_the_dense_load(nvar, nparm, bits):
    """every column of every row, row tables, spare slots and headers: the zeroed workspace after load_instances() against
    the zeroed workspace after load_system() on the model's expansion -- same engine, same descriptor.  3 systems of 2 .. 6
    rows; no equality, the first row, the last row, every row; the three shifts; tab_simplify on and off."""
    import torch
    from piplib_amd import engine as eng
    e = eng.Engine(0)
    combo, seen, zero_points = 0, set(), 0
    for shift in SHIFTS:
        for simp in (0, 1):
            for v in range(4):
                nrows = 6 - combo % 5  # 6, 5, 4, 3, 2, 6, ...
                eq = _eq_variants(nrows)[v]
                m, p, kinds = _edge_family(nvar, nparm, nrows, combo)
                seen |= set(kinds)
                zero_points += not p[0].any()
                a = _dense(m, p)
                assert a.shape == (3, nrows, nvar + 1)
                kw = dict(tflags=eng.T_INT, entier_bits=bits, shift=shift, eq_rows=eq, simplify=simp)
                s = eng.Batch(e, (m, p), nvar, 0, instances=True, **kw)
                d = eng.Batch(e, a, nvar, 0, system=True, **kw)
                assert bytes(s.desc) == bytes(d.desc) and s.ws.shape == d.ws.shape
                s.ws.zero_()
                d.ws.zero_()
                s.load_instances()
                d.load_system()
                torch.cuda.synchronize()
                assert torch.equal(s.ws, d.ws), (shift, simp, eq, nrows)
                assert d.ws.any()
                combo += 1
    assert combo == 24 and seen == {0, 1, 2, 3, 4} and zero_points == (12 if nparm else 24)


@pytest.mark.parametrize("bits", [64, 128])
def test_rows_beyond_the_kept_constants(bits):
    """520 rows: the load kernel keeps the constants of a system's first 512 rows between its two passes and forms the
    later ones again.  Three systems; row 515 of the third has the constant 2^62 * 4 + c: a bad system with 64-bit
    entries -- decided by a row of the second kind --, and with 128-bit entries a good one whose entry is read back from
    the workspace, every row of it.  The other two systems equal the dense load's, job header and block."""
    import torch
    import instances_model as im
    from piplib_amd import engine as eng
    nvar, nparm, nrows, far = 3, 2, 520, 515
    rng = np.random.default_rng(520)
    m = rng.integers(-9, 10, (nrows, nvar + nparm + 1))
    m[far, nvar] = 1 << 62
    p = np.array([[1, -3], [0, 0], [4, 5]], dtype=np.int64)
    rows = im.expand(m.tolist(), p.tolist())
    want = rows[2][far][-1]
    assert want == (1 << 64) + 5 * int(m[far, nvar + 1]) + int(m[far, -1])
    assert im.fits(rows, 64) == [True, True, False] and im.fits(rows, 128) == [True] * 3
    a = np.array([rows[0], rows[1], rows[1]], dtype=np.int64)
    e = eng.Engine(0)
    kw = dict(tflags=eng.T_INT, entier_bits=bits)
    s = eng.Batch(e, (m, p), nvar, 0, instances=True, **kw)
    d = eng.Batch(e, a, nvar, 0, system=True, **kw)
    assert bytes(s.desc) == bytes(d.desc) and s.ws.shape == d.ws.shape
    s.ws.zero_()
    d.ws.zero_()
    s.load_instances()
    d.load_system()
    torch.cuda.synchronize()
    sl, jobs = _slices(s), _jobs(s)
    for k in (0, 1):
        assert torch.equal(s.ws[sl[k][0]], d.ws[sl[k][0]]) and torch.equal(s.ws[sl[k][1]], d.ws[sl[k][1]]), k
    ew, W = bits // 64, int(jobs[2, JOB_W])
    vals = sl[0][1].start + int(s.ws[sl[2][0]][0].item())  # PipJob.vals_off, in words from the arena's start
    block = s.ws[vals:vals + nrows * W * ew].cpu().numpy().reshape(nrows, W, ew)
    if bits == 64:
        assert jobs[2, JOB_STATUS] == eng.ST_BADINPUT and jobs[2, JOB_NI] == 0 and not block.any()
    else:
        assert jobs[2, JOB_STATUS] == eng.ST_RUN and jobs[2, JOB_NI] == nrows
        got = eng.wide_to_int(block)
        assert got[:, :nvar + 1].tolist() == rows[2]
        assert got[far, nvar] == want and not got[:, nvar + 1:].any()


# ---------------------------------------------------------------- exact constants, bad systems among good ones

EDGE_MODES = {"int-plain": (1, 0, 0), "int-simplify": (1, 1, 0), "rational-dual": (0, 0, 1)}  # nq, simplify, dual


@pytest.mark.parametrize("mode", list(EDGE_MODES))
@pytest.mark.parametrize("bits", [64, 128])
def test_exact_constants_and_bad_systems(bits, mode):
    """one batch of instances_model.edge_cases: constants at the top and the bottom of the entry type and one beyond
    either, sums whose products leave 64 bits and cancel, 2^64 + 3 (a wrapped 3 in 64 bits), two products of 2^126; the
    edge row first or last in its system.
    - status PIPAMD_ST_BADINPUT exactly where the model's constants do not fit; such a system has an empty tableau, none
      of its rows stored, and after the solve zero pivots, results and duals;
    - a good system whose constants fit int64: job header and block equal the dense load's, byte for byte;
    - a good system, those with a constant beyond int64 (128-bit entries) among them: status, pivots and solution as
      tests/bigint_pip.py computes them in Python ints from the model's tableau -- every good system but those whose
      constant is the smallest value of the entry type and stays it (no tab_simplify), which bigint_pip does not call
      exact for that width (a bit length of 64 or 128: the fixed-width solve negates it);
    - every good system: the results it has in a batch without the bad ones."""
    import torch
    import bigint_pip as bp
    import instances_model as im
    import pipbatch as pb
    import system_model as sy
    from gpu_common import solution_text
    from piplib_amd import engine as eng
    tbs = _tbs()
    nq, simp, dual = EDGE_MODES[mode]
    matrix, points, nvar, names = im.edge_cases(bits)
    rows = im.expand(matrix, points)
    fit, fit64 = im.fits(rows, bits), im.fits(rows, 64)
    B = len(points)
    good = [k for k in range(B) if fit[k]]
    bad = [k for k in range(B) if not fit[k]]
    wide = [k for k in good if not fit64[k]]
    assert len(good) >= 7 and len(bad) >= 4 and (bits == 64) == (not wide)

    e = tbs._engine()
    b = _inst_batch(e, matrix, points, nvar, (), 0, _flags(nq, dual), simp, bits)
    b.ws.zero_()
    b.load_instances()
    # the dense load of the same batch, the harmless system in the place of those whose constants leave int64
    a = np.array([rows[k] if fit64[k] else rows[0] for k in range(B)], dtype=np.int64)
    d = eng.Batch(e, a, nvar, 0, tflags=_flags(nq, dual), entier_bits=bits, system=True, simplify=simp)
    assert bytes(b.desc) == bytes(d.desc) and b.ws.shape == d.ws.shape
    d.ws.zero_()
    d.load_system()
    torch.cuda.synchronize()
    jobs = _jobs(b)
    ew = bits // 64
    for k, (job, blk) in enumerate(_slices(b)):
        if not fit[k]:
            assert jobs[k, JOB_STATUS] == eng.ST_BADINPUT and jobs[k, JOB_NI] == 0, names[k]
            vals = int(b.ws[job][0].item())  # PipJob.vals_off, in words from the arena's start
            room = jobs[k, JOB_S] * jobs[k, JOB_W] * ew
            start = _slices(b)[0][1].start + vals
            assert blk.start <= start and start + room <= blk.stop and room > 0
            assert not b.ws[start:start + room].any(), names[k]  # nothing of it was stored
        else:
            assert jobs[k, JOB_STATUS] == eng.ST_RUN and jobs[k, JOB_NI] == len(matrix), names[k]
            if fit64[k]:
                assert torch.equal(b.ws[job], d.ws[job]) and torch.equal(b.ws[blk], d.ws[blk]), names[k]

    tbs._finish(b, (lambda b: b.dual_instances()) if dual else None)
    st = b.status.cpu().numpy()
    assert [k for k in range(B) if st[k] == eng.ST_BADINPUT] == bad
    outs = ("pivots", "cuts", "sol_num", "sol_den")
    for k in bad:
        for name in outs:
            assert not getattr(b, name)[k].any(), (names[k], name)
        if dual:
            assert not b.dual_pair[0][k].any() and not b.dual_pair[1][k].any(), names[k]
    # the same systems without the bad ones
    g = _solve_instances(matrix, [points[k] for k in good], nvar, (), 0, nq, simp, dual, bits)
    for name in ("status",) + outs:
        assert torch.equal(getattr(b, name)[good], getattr(g, name)), name
    if dual:
        assert torch.equal(b.dual_pair[0][good], g.dual_pair[0]) and torch.equal(b.dual_pair[1][good], g.dual_pair[1])
    assert (g.status == eng.ST_SOLUTION).sum().item() >= 3
    # Python ints: every good system whose solve stays within the entry type, those beyond int64 among them
    pv, num, den = b.pivots.cpu().numpy(), tbs._ints(b.sol_num, bits), tbs._ints(b.sol_den, bits)
    inexact, nil = [], 0
    for k in good:
        r = bp.solve(sy.tableau(rows[k], (), 0, simp), integer=bool(nq), bits=bits)
        if not r.stats.exact:
            inexact.append(k)
            continue
        nil += r.status == bp.ST_NIL
        assert st[k] == r.status and pv[k] == r.pivots, (names[k], st[k], r.status, pv[k], r.pivots)
        if r.status == bp.ST_SOLUTION:
            assert pb.squash(solution_text(num[k], den[k])) == pb.squash(bp.solution_text(r.sol_num, r.sol_den)), names[k]
        else:
            assert not num[k].any() and not den[k].any(), names[k]
    assert set(names[k].split(",")[0] for k in inexact) <= {"min64" if bits == 64 else "min128"}
    assert bits == 64 or len(set(wide) - set(inexact)) >= 8
    assert nil >= (2 if bits == 128 or simp else 0)


# ---------------------------------------------------------------- the golden family

@functools.lru_cache(maxsize=None)
def _p5():
    import instances_model as im
    g = im.golden()
    return g, g["matrix"], g["points"], g["nvar"], tuple(g["eq_rows"])


def _p5_options():
    import system_model as sy
    return list(sy.OPTIONS)


@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("opts", ["", "Rational+Dual", "Maximize", "Maximize+Rational+Dual", "Urs_unknowns",
                                  "Urs_unknowns+Rational+Dual"])
def test_golden_family(opts, bits):
    """p5 at its 8 points: answers, duals and pivot counts as the reference's pip_solve printed them for each instance;
    cuts and the solution arrays bit for bit as from the dense load of the expansion"""
    import torch
    import system_model as sy
    tbs = _tbs()
    assert _p5_options() == ["", "Rational+Dual", "Maximize", "Maximize+Rational+Dual", "Urs_unknowns",
                             "Urs_unknowns+Rational+Dual"]
    g, matrix, points, nvar, eq = _p5()
    shift, nq, dual = sy.OPTIONS[opts]
    want = g["cases"][opts]
    b = _solve_instances(matrix, points, nvar, eq, shift, nq, nq, dual, bits)  # integer cases simplified, as pip_solve does
    got_x = tbs._answers(b, bits)
    assert got_x == want["x"]
    assert b.pivots.cpu().tolist() == want["pivots"]
    d = tbs._solve_system(_dense(matrix, points), nvar, eq, shift, nq, nq, dual, bits)
    tbs._same(b, d, ("status", "pivots", "cuts", "sol_num", "sol_den") + (("x_num", "x_den") if shift else ()))
    if dual:
        nrows = len(matrix)
        got_d = tbs._duals(b, bits)
        for k in range(len(points)):
            w = want["dual"][k]
            assert (w is None) == (got_x[k] is None), k
            assert got_d[k] == (w if w is not None else [[0, 0]] * nrows), (k, got_d[k], w)
        assert torch.equal(b.dual_pair[0], d.dual_pair[0]) and torch.equal(b.dual_pair[1], d.dual_pair[1])
    assert sum(x is not None for x in got_x) >= 3


# ---------------------------------------------------------------- parts

@pytest.mark.parametrize("shift", [0, -1], ids=["plain", "urs"])
@pytest.mark.parametrize("middle", ["same-matrix", "other-matrix"])
def test_parts_equal_one_call(middle, shift):
    """9 points loaded as parts of 1, 5 and 3 (a non-zero `first`, points of the part's own): the workspace after the
    loads and, after the solve, results and duals equal the one-call load's -- or, where the middle part has another
    matrix of the same shape, the dense load's of the three expansions"""
    import torch
    from piplib_amd import engine as eng
    tbs = _tbs()
    g, matrix, points, nvar, eq = _p5()
    points = points + [[3, 1]]
    other = [list(r) for r in matrix]
    if middle == "other-matrix":
        other[1][nvar] = 1      # a parameter coefficient
        other[2][-1] += 3       # a constant
        other[4][4] = 2         # an unknown's coefficient
        other[6][nvar + 1] = -1
    e = tbs._engine()
    tflags = eng.T_DUAL
    parts = _inst_batch(e, matrix, len(points), nvar, eq, shift, tflags, 0)
    parts.ws.zero_()
    other_dev = torch.as_tensor(np.array(other, dtype=np.int64)).to(parts.dev)
    dev, at, dense = [], 0, []
    for i, n in enumerate((1, 5, 3)):
        pts = torch.as_tensor(np.array(points[at:at + n], dtype=np.int64)).to(parts.dev)
        mat = other_dev if i == 1 else None
        parts.load_instances_part(pts, at, matrix=mat)
        dev.append((pts, at, mat))
        dense.append(_dense(other if i == 1 else matrix, points[at:at + n]))
        at += n
    assert at == len(points) == 9
    if middle == "same-matrix":
        one = _inst_batch(e, matrix, points, nvar, eq, shift, tflags, 0)
        one.ws.zero_()
        one.load_instances()
        dual_one = lambda b: b.dual_instances()  # noqa: E731
    else:
        a = np.concatenate(dense)
        assert (a[1:6] != _dense(matrix, points[1:6])).any()
        one = eng.Batch(e, a, nvar, 0, tflags=tflags, shift=shift, system=True, eq_rows=eq)
        one.ws.zero_()
        one.load_system()
        dual_one = lambda b: b.dual_system()  # noqa: E731
    torch.cuda.synchronize()
    assert torch.equal(one.ws, parts.ws)
    tbs._finish(one, dual_one)

    def by_parts(b):
        out = None
        for pts, first, mat in dev:
            out = b.dual_instances_part(pts, first, out=out, matrix=mat)
        return out
    tbs._finish(parts, by_parts)
    tbs._same(one, parts, ("status", "pivots", "cuts", "sol_num", "sol_den") + (("x_num", "x_den") if shift else ()))
    assert torch.equal(one.dual_pair[0], parts.dual_pair[0]) and torch.equal(one.dual_pair[1], parts.dual_pair[1])
    assert (one.status == eng.ST_SOLUTION).sum().item() >= 3 and one.dual_pair[1].any()


# ---------------------------------------------------------------- the bulk path

BULK_MATRIX = [  # x0 .. x3 | n, m | constant
    [1, 1, 0, 0, -1, 0, 0],     # x0 + x1 >= n
    [0, -2, 1, 0, 0, 1, 3],     # 2 x1 <= x2 + m + 3
    [0, 0, -1, 3, 1, -1, 0],    # x2 <= 3 x3 + n - m
    [-3, 0, 0, -2, -1, 2, 7],   # 3 x0 + 2 x3 <= 2 m + 7 - n
    [0, 2, 0, 2, 0, -1, -1],    # 2 x1 + 2 x3 >= m + 1
    [0, 0, 2, -1, -1, 0, 4],    # 2 x2 >= x3 + n - 4
]


def test_bulk_sized_batch():
    """2,048 points of a 4-unknown, 2-parameter, 6-row system, integer with tab_simplify: a batch of the size that takes
    the bulk launch sequence.  Status, pivots, cuts and solutions bit for bit as from the dense load of the expansion; 16
    systems across the batch against the CPU oracle on the model's tableau"""
    import pipbatch as pb
    import system_model as sy
    from gpu_common import oracle_batch, solution_text
    from piplib_amd import engine as eng
    tbs = _tbs()
    nvar = 4
    points = [[n, m] for n in range(64) for m in range(32)]
    assert len(points) == 2048
    b = _solve_instances(BULK_MATRIX, points, nvar, (), 0, 1, 1, 0)
    a = _dense(BULK_MATRIX, points)
    d = tbs._solve_system(a, nvar, (), 0, 1, 1, 0)
    tbs._same(b, d)
    st, pv = b.status.cpu().numpy(), b.pivots.cpu().numpy()
    num, den = b.sol_num.cpu().numpy(), b.sol_den.cpu().numpy()
    sample = list(range(5, 2048, 131))
    assert len(sample) == 16
    res = oracle_batch(sy.tableaux(a[sample], (), 0, 1), nvar, 0, 1).results
    solved = 0
    for k, r in zip(sample, res):
        assert r.status == pb.ST_OK
        want = pb.squash(r.text)
        assert st[k] == (eng.ST_NIL if want == "()" else eng.ST_SOLUTION), (k, st[k], want[:60])
        assert pv[k] == r.pivots, (k, pv[k], r.pivots)
        if want != "()":
            assert pb.squash(solution_text(num[k], den[k])) == want, k
            solved += 1
    assert 4 <= solved < 16
    assert 100 <= (b.status == eng.ST_SOLUTION).sum().item() < len(points)
