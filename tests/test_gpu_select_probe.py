"""The functions that decide WHICH pivot is taken -- choose_column / choose_column_slow / lean_choose_column (choisir_piv),
sort_rows (tab_sort_rows), exam_rows (exam_coef) -- and the publish functions whose bitmaps, sign summaries and magnitude
classes they read, each against Python ints on small tableaux aimed at their edges.

pipamd_debug_select (piplib_amd/csrc/pip_probe.hip) stages a case's tables, summarises its rows with the SHIPPED
row_publish / lean_publish and calls the SHIPPED function; every output word of every case must equal the model
(tests/select_model.py): the return value, ref[] and fl[] afterwards, sig / rcls / cst / nzm per slot, max_row_class, and
for the lean flavours the packed image of the rows.  The lists come from tests/select_cases.py; tests/test_select_cases.py
(no GPU) checks them: tags per flavour, preconditions, fold model == brute-force model, wrap model == exact model where
nothing leaves W bits.

The last test is end to end, for the one decision the probe cannot reach without touching the kernel: the inline guard
of pip_advance_kernel that sends a pivot to the tournament or to the slow fold.
"""
import ctypes as C
import time

import numpy as np
import pytest

import select_cases as sc
import select_model as sm

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
G64 = sm.Geometry(64, 2, 1)


# ------------------------------------------------------------------------------------------------ packing
def _words(vals, EW):
    """Python ints -> uint64 words, EW per value, low word first"""
    if EW == 1:
        return np.array([v & M64 for v in vals], dtype=np.uint64)
    out = np.empty(2 * len(vals), dtype=np.uint64)
    out[0::2] = np.array([v & M64 for v in vals], dtype=np.uint64)
    out[1::2] = np.array([(v >> 64) & M64 for v in vals], dtype=np.uint64)
    return out


def pack_case(t, EW, odd):
    """the case as pipamd_debug_select reads it (`odd`: the case starts at an odd word of `in`); cached on the case"""
    key = ("in", EW, odd)
    if key not in t.extra:
        head = [t.nvar, t.ncol, t.W, t.ni, t.nligne, t.pivi, t.bigparm, sm.double_bits(t.smax)]
        head += list(t.ref) + t.urow() + t.srow() + list(t.fl) + [sm.float_bits(x) for x in t.size]
        if (len(head) + odd) & 1:
            head.append(0)
        vals = [x for r in t.rows for x in r] + list(t.den)
        t.extra[key] = np.concatenate([np.array([v & M64 for v in head], dtype=np.uint64), _words(vals, EW)])
    return t.extra[key]


def expected(t, g, ret, ref=None, fl=None):
    """every output word of the case"""
    EW = g.BITS // 64
    slots, mc = sm.publish(t, g)
    head = [1, ret & M64, mc] + list(t.ref if ref is None else ref) + list(t.fl if fl is None else fl)
    for sig, cls, cst, nz in slots:
        head += [sig, cls] + [(cst >> (64 * i)) & M64 for i in range(EW)] + nz
    out = np.array([v & M64 for v in head], dtype=np.uint64)
    if g.lean:
        img = np.zeros(EW * t.ni * t.W, dtype=np.uint64)
        for s, row in enumerate(t.rows):
            if g.lean == 32:
                a = np.array([x & 0xFFFFFFFF for x in row], dtype=np.uint64)
                img[s * t.W:s * t.W + t.W // 2] = a[0::2] | (a[1::2] << np.uint64(32))
            else:
                img[2 * s * t.W:2 * s * t.W + t.W] = np.array([x & M64 for x in row], dtype=np.uint64)
        out = np.concatenate([out, img])
    return out


class Probe:
    def __init__(self):
        import torch
        from piplib_amd import engine as eng
        self.torch = torch
        self.L = eng.lib()
        self.L.pipamd_debug_select.restype = C.c_int
        self.L.pipamd_debug_select.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        self.e = eng.Engine(0)

    def run(self, fn, g, cases, wants):
        """cases through function `fn`; returns the first case whose output differs from wants (None: all equal)"""
        t = self.torch
        EW, n = g.BITS // 64, len(cases)
        ins, oin, oout, pos, opos = [], [], [], 2 + 2 * n, 0
        for tb, w in zip(cases, wants):
            blob = pack_case(tb, EW, pos & 1)
            oin.append(pos)
            ins.append(blob)
            pos += len(blob)
            if g.lean:   # the packed image at the end of the case's output: 16-byte aligned
                opos += (opos + len(w) - EW * tb.ni * tb.W) & 1
            oout.append(opos)
            opos += len(w)
        total_out = opos + (opos & 1) + 2
        words = np.concatenate([np.array([pos, total_out] + oin + oout, dtype=np.uint64)] + ins)
        assert len(words) == pos
        din = t.from_numpy(words.view(np.int64)).cuda()
        dout = t.zeros(total_out, dtype=t.int64, device="cuda")
        assert din.data_ptr() % 16 == 0 and dout.data_ptr() % 16 == 0
        rc = self.L.pipamd_debug_select(self.e._h, fn, C.c_void_p(din.data_ptr()), C.c_void_p(dout.data_ptr()), n)
        assert rc == 0, rc
        got = dout.cpu().numpy().view(np.uint64)
        for k, (tb, w) in enumerate(zip(cases, wants)):
            gk = got[oout[k]:oout[k] + len(w)]
            if not np.array_equal(gk, w):
                d = int(np.nonzero(gk != w)[0][0])
                return "%s: case %d of %d, output word %d is %#x, the model has %#x (status %d, returned %d, model %d)" % (
                    tb.tag, k, n, d, int(gk[d]), int(w[d]), int(gk[0]), int(gk[1].view(np.int64)), int(w[1].view(np.int64)))
        return None


@pytest.fixture(scope="module")
def probe():
    return Probe()


def _timed(name, t0):
    print("%s: %.2f s" % (name, time.time() - t0))


# ------------------------------------------------------------------------------------------------ the tests
def test_choose_column_tournaments(probe):
    """choose_column<i64 / i128, NCH, SMALL> and lean_choose_column<F, SMALL>: every case the flavour admits returns the
    exact fold's column (which the CPU test holds to the brute-force lexicographic minimum)"""
    t0 = time.time()
    exact = {}
    for flavour in sc.TOURNAMENT:
        f = sc.FLAVOURS[flavour]
        cases = sc.flavour_cases(flavour)
        assert len(cases) >= 300
        for t in cases:
            if id(t) not in exact:
                exact[id(t)] = sm.fold_column(t)
        bad = probe.run(f["fn"], f["geom"], cases, [expected(t, f["geom"], exact[id(t)]) for t in cases])
        assert bad is None, "%s: %s" % (flavour, bad)
    _timed("tournament flavours", t0)


def test_choose_column_slow(probe):
    """choose_column_slow<i64 / i128>: the fold in W-bit wrap-around arithmetic, on every case -- safe or not"""
    t0 = time.time()
    for flavour in ("SLOW64", "SLOW128"):
        f = sc.FLAVOURS[flavour]
        g = f["geom"]
        cases = sc.flavour_cases(flavour)
        assert len(cases) >= 1000
        bad = probe.run(f["fn"], g, cases, [expected(t, g, sm.fold_column(t, g.BITS)) for t in cases])
        assert bad is None, "%s: %s" % (flavour, bad)
    _timed("slow fold", t0)


def test_sort_rows_both_branches(probe):
    """sort_rows<i64>: ref[] as the selection loop leaves it; a case of at most 64 rows runs again with never-picked rows
    appended to more than 64, and the other branch must leave the same first rows"""
    t0 = time.time()
    pairs = sc.sort_cases()
    cases, wants = [], []
    for t, twin in pairs:
        ref = sm.sort_ref(t)
        cases.append(t)
        wants.append(expected(t, G64, 0, ref=ref))
        if twin is not None:
            tref = sm.sort_ref(twin)
            assert tref[:t.nligne] == ref and tref[t.nligne:] == twin.ref[t.nligne:], twin.tag
            cases.append(twin)
            wants.append(expected(twin, G64, 0, ref=tref))
    bad = probe.run(sc.FN_SORT, G64, cases, wants)
    assert bad is None, bad
    _timed("sort_rows", t0)


@pytest.mark.parametrize("fn", [sc.FN_EXAM1, sc.FN_EXAM4], ids=["NW1", "NW4"])
def test_exam_rows(probe, fn):
    """exam_rows<i64, NW>: the row returned (BIG_I where exam_coef runs to the end) and every flag afterwards"""
    t0 = time.time()
    cases = sc.exam_cases(fn)
    wants = []
    for t in cases:
        i, fl = sm.exam_coef(t)
        wants.append(expected(t, G64, sm.BIG_I if i == t.nligne else i, fl=fl))
    bad = probe.run(fn, G64, cases, wants)
    assert bad is None, bad
    _timed("exam_rows", t0)


def test_probe_refuses_what_it_cannot_hold(probe):
    """a case beyond the probe's tables is reported (status 0), not run"""
    t = sc.scenario("refuse: too wide", (0, 1, 200), (1, 1, 1), [("p",), ("u", 0), ("u", 1), ("u", 2)])
    want = np.zeros(3 + t.nligne + t.ni + t.ni * (3 + G64.NM), dtype=np.uint64)
    assert probe.run(sc.FLAVOURS["C64_1"]["fn"], G64, [t], [want]) is None


def test_inline_guard_of_the_pivot_kernel():
    """pip_advance_kernel's `abits + cls_bits(mc) <= BITS - 2` picks the tournament or the slow fold: whole solves of small
    tableaux against the oracle's 64-bit wrap-around arithmetic.  A fresh tableau's first choisir_piv is decided by the unit
    rows on top, so select_cases.guard_tableaux() spends the first pivot on bringing a real row to logical row 0; the
    candidates of the SECOND pivot row and that row's entries span every pair of magnitude classes.  On the kept tableaux
    whose wrapped fold picks another column than the exact one (at least 8, tests/test_select_cases.py), only the slow
    fold gives parity: with the guard forced to admit the tournament this test fails."""
    from gpu_common import compare
    t0 = time.time()
    rows, firsts = sc.guard_tableaux()
    assert sum(1 for ex, wr, _, _ in firsts if ex != wr) >= 8
    n, piv = compare(rows, sc.GUARD_NVAR, 0, 1)
    assert n == len(rows) and piv >= n
    _timed("inline guard, %d tableaux, %d pivots" % (n, piv), t0)
