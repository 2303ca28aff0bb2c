"""-m gpu: the lean kernel's per-lane preparation of a pivot's rows and the row reductions that start from a given gcd,
against Python ints and against the entry points they replace.

The probe (piplib_amd/csrc/pip_probe.hip) runs the SHIPPED functions: pipamd_debug_arith op 128 is lean_prepare_rows
<LeanIntRows>, one row per lane, 64 rows a wave (pivot, dpiv and psmall are the wave's); pipamd_debug_row_update paths
32 ... 35 are LeanIntRows / LeanLongRows update_small / update_mid with the case's `gpre` word as the starting gcd gs
(small_reduce_from, row_reduce_rem_from, row_reduce's gpre).

A starting gcd gs is admissible when G | gs | |g0| for the row gcd G = gcd(g0, z_0, ..., z_n): then gcd(gs, z) = G (gcd is
associative), so quotients and newden = g0 / G are the same bits.  Every case runs with gs = G, gs = gcd(|g0|, |dpiv foo|)
(what lean_prepare_rows folds), a proper multiple of G that divides |g0| where there is one, gs = |g0|, and gs = 0
("nothing prepared": the old start) -- gs = 1 among them whenever G is 1.  Models: plain Python ints; no case wraps."""
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_arith_probe import mask, pack_words, signed, unpack_words

pytestmark = pytest.mark.gpu

OP_LEAN_PREP = 128
# path -> (id, W, WP, the paths that take the same words and ignore gs: the old entry points)
GS_PATHS = {
    "LI_S_GS": (32, 64, 128, (11, 4)),   # LI_S (gs = 0), S64 (update_row_small -> small_reduce)
    "LI_M_GS": (33, 64, 128, (12, 3)),   # LI_M (gs = 0), G64R (update_row<LEANREG> -> row_reduce_rem)
    "LL_S_GS": (34, 128, 256, (13,)),    # LL_S
    "LL_M_GS": (35, 128, 256, (14,)),    # LL_M
}


class Probe:
    def __init__(self):
        import torch
        from piplib_amd import engine as eng
        self.torch = torch
        self.L = eng.lib()
        for f in (self.L.pipamd_debug_arith, self.L.pipamd_debug_row_update):
            f.restype = C.c_int
        self.L.pipamd_debug_arith.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong]
        self.L.pipamd_debug_row_update.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        self.e = eng.Engine(0)

    def run(self, fn, code, words, n, nout):
        t = self.torch
        din = t.from_numpy(np.ascontiguousarray(words)).cuda()
        dout = t.zeros((n, nout), dtype=t.int64, device="cuda")
        rc = fn(self.e._h, code, C.c_void_p(din.data_ptr()), C.c_void_p(dout.data_ptr()), n)
        assert rc == 0, rc
        return dout.cpu().numpy()


@pytest.fixture(scope="module")
def probe():
    return Probe()


# ------------------------------------------------------------------------------------------------ reductions from a gcd
def row_model(c):
    """(ok, newden, z) of traiter.c:470-501 on Python ints"""
    z = [p * c["lp"] - q * c["foo"] for p, q in zip(c["p"], c["q"])]
    z[c["pivj"]] = c["dpiv"] * c["foo"]
    G = 0
    for v in [c["g0"]] + z:
        G = math.gcd(G, v)
    if G == 0:
        return 0, c["g0"], z, 0
    return 1, c["g0"] // G if c["g0"] >= 0 else -(-c["g0"] // G), [v // G if v >= 0 else -(-v // G) for v in z], G


def make_case(WP, lp, foo, dpiv, g0, pivj, entries, qentries=None, tag=""):
    p, q = [0] * WP, [0] * WP
    for j, v in entries.items():
        p[j] = v
    for j, v in (qentries or {}).items():
        q[j] = v
    return dict(lp=lp, foo=foo, dpiv=dpiv, g0=g0, pivj=pivj, p=p, q=q, tag=tag)


G0_VALUES = (1, -1, 0, 6, -6, 2 ** 20 - 1, 2 ** 20, -(2 ** 20), 2 ** 31 - 1, 2 ** 32, -(2 ** 32), 3 * 2 ** 33, 2 ** 20 * 3 * 5 * 7, 2 * 3 * 5 * 7 * 11 * 13)


def small_cases(WP):
    """LeanIntRows::update_small's domain: |p|, |q|, |lp|, |foo|, |dpiv| < 2^15 (every |z| < 2^31)"""
    out = []
    top = 2 ** 15 - 1
    for g0 in G0_VALUES:
        for lp, foo, dpiv in ((1, 0, 1), (6, 4, 9), (2 ** 10, 2 ** 5, 2 ** 10), (top, top, top), (30, -12, 6), (7, 1, 1), (210, 30, 2310)):
            # a zero row; single entries at the top; rows with a common factor; entries on both halves of a lane and in
            # the last column; the pivot row taking part
            out.append(make_case(WP, lp, foo, dpiv, g0, 3, {}, tag="zero row but pivj"))
            out.append(make_case(WP, lp, foo, dpiv, g0, 0, {1: top, 2: -top, 127: 2 ** 14}, tag="top entries"))
            out.append(make_case(WP, lp, foo, dpiv, g0, 126, {0: 6, 1: -30, 64: 210, 65: 2 ** 10, 127: 2310}, tag="common factor 2"))
            out.append(make_case(WP, lp, foo, dpiv, g0, 5, {4: 2 ** 10, 6: -(2 ** 12), 100: 2 ** 14}, tag="powers of two"))
            out.append(make_case(WP, lp, foo, dpiv, g0, 5, {4: 15, 6: 105, 7: top}, {4: 21, 6: -35, 127: top}, tag="pivot row in"))
    out.append(make_case(WP, 1, 0, 1, 0, 0, {}, tag="zero row, g0 = 0, foo = 0: the reference divides by zero"))
    out.append(make_case(WP, 5, 0, 3, 2 ** 32, 0, {}, tag="zero row under a denominator beyond 32 bits"))
    return out


def mid_cases(WP):
    """LeanIntRows::update_mid's domain: packed int rows and int multipliers (|z| < 2^63 here: nothing wraps)"""
    out = []
    top = 2 ** 31 - 1
    for g0 in G0_VALUES + (2 ** 61, -(2 ** 62) + 2 ** 31, (2 ** 31 - 1) * 2 ** 20):
        for lp, foo, dpiv in ((1, 0, 1), (6, 4, 9), (2 ** 15, 2 ** 15, 2 ** 15), (2 ** 20, 2 ** 10, 2 ** 20), (top, top, top), (top, -top, 2 ** 20),
                              (2 ** 30, 2 ** 20, 2 ** 31), (30, -12, 6)):
            out.append(make_case(WP, lp, foo, dpiv, g0, 3, {}, tag="zero row but pivj"))
            out.append(make_case(WP, lp, foo, dpiv, g0, 0, {1: 2 ** 15 - 1, 2: 2 ** 15, 3: -(2 ** 20), 127: top}, tag="entries at the class edges"))
            out.append(make_case(WP, lp, foo, dpiv, g0, 126, {0: 6 * 2 ** 20, 1: -30 * 2 ** 20, 65: 210 * 2 ** 20, 127: 2 ** 30}, tag="common factor"))
            out.append(make_case(WP, lp, foo, dpiv, g0, 5, {4: 15, 6: 105 * 2 ** 15, 7: top}, {4: 21, 6: -35 * 2 ** 15, 127: top // 2}, tag="pivot row in"))
    out.append(make_case(WP, 1, 0, 1, 0, 0, {}, tag="zero row, g0 = 0, foo = 0: the reference divides by zero"))
    return out


def starts_of(c):
    """the admissible starting gcds of a case (see the module's docstring), 0 first"""
    ok, _, _, G = row_model(c)
    a0 = abs(c["g0"])
    if a0 == 0:
        return [0]  # g0 = 0: lean_prepare_rows folds nothing, the old path decides (it may be the `false` verdict)
    gs = [0, G, a0, math.gcd(a0, abs(c["dpiv"] * c["foo"])) if c["dpiv"] * c["foo"] else a0]
    for f in (2, 3, 5, 7, 11, 2 ** 31 - 1):  # a proper multiple of G that divides |g0|
        if (a0 // G) % f == 0 and G * f != a0:
            gs.append(G * f)
            break
    return sorted(set(gs))


def words_of(cases, gss, W):
    ew = W // 64
    rows = [[c["lp"], c["foo"], c["dpiv"], c["g0"], c["pivj"], gs] + c["p"] + c["q"] for c, gs in zip(cases, gss)]
    return pack_words(rows, (ew,) * len(rows[0]))


@pytest.mark.parametrize("path", list(GS_PATHS))
def test_reduction_from_a_gcd(probe, path):
    code, W, WP, old = GS_PATHS[path]
    ew = W // 64
    base = small_cases(128) if path.endswith("_S_GS") else mid_cases(128)
    if WP == 256:  # the same rows, spread over the four column blocks of a lane
        wide = []
        for c in base:
            w = dict(c)
            w["p"] = [0] * 256
            w["q"] = [0] * 256
            for j in range(128):
                w["p"][(j * 2 + (j == 127)) % 256] = c["p"][j]
                w["q"][(j * 2 + (j == 127)) % 256] = c["q"][j]
            w["pivj"] = (c["pivj"] * 2) % 256
            wide.append(w)
        base = wide
    cases, gss = [], []
    for c in base:
        for gs in starts_of(c):
            cases.append(c)
            gss.append(gs)
    assert any(g == 1 for g in gss) and any(g > 2 ** 32 for g in gss)
    want = []
    for c in cases:
        ok, nd, z, _ = row_model(c)
        assert all(abs(v) < 2 ** 63 for v in z) and (not path.endswith("_S_GS") or all(abs(v) < 2 ** 31 for v in z)), c["tag"]
        want.append(tuple(mask(v, W) for v in [ok, nd] + z))
    words = words_of(cases, gss, W)
    nout = ew * (2 + WP)
    got = unpack_words(probe.run(probe.L.pipamd_debug_row_update, code, words, len(cases), nout), (ew,) * (2 + WP))
    bad = [i for i in range(len(cases)) if got[i] != want[i]]
    assert not bad, "%s: %d of %d cases differ from the model; first #%d [%s] lp,foo,dpiv=%s g0=%d gs=%d: ok %d/%d newden %d/%d" % (
        path, len(bad), len(cases), bad[0], cases[bad[0]]["tag"], (cases[bad[0]]["lp"], cases[bad[0]]["foo"], cases[bad[0]]["dpiv"]),
        cases[bad[0]]["g0"], gss[bad[0]], got[bad[0]][0], want[bad[0]][0], signed(got[bad[0]][1], W), signed(want[bad[0]][1], W))
    # ... and against the entry points that take no starting gcd, on the same words
    for ocode in old:
        ogot = unpack_words(probe.run(probe.L.pipamd_debug_row_update, ocode, words, len(cases), nout), (ew,) * (2 + WP))
        obad = [i for i in range(len(cases)) if ogot[i] != got[i]]
        assert not obad, "%s vs path %d: %d of %d cases differ, first #%d [%s] gs=%d" % (
            path, ocode, len(obad), len(cases), obad[0], cases[obad[0]]["tag"], gss[obad[0]])


# ------------------------------------------------------------------------------------------------ the preparation
def prep_model(pivot, dpiv, psmall, foo, den, rcls):
    lp, g0 = pivot, den
    if pivot != 1:
        d = math.gcd(pivot, abs(foo))
        lp, foo = pivot // d, (foo // d if foo >= 0 else -(-foo // d))
        g0 = signed(lp * den, 64)
    zf = signed(dpiv * foo, 64)
    gs = math.gcd(abs(g0), abs(zf)) if abs(g0) > 1 and zf != 0 else 0
    if gs >= 2 ** 32:
        gs = 0  # (the lane keeps 32 bits: beyond them nothing is folded)
    return lp, foo, g0, gs, int(bool(psmall) and rcls == 0)


def prep_cases():
    """waves of 64 lanes; pivot, dpiv and psmall are the wave's"""
    rows = []
    for pivot in (1, 2, 7919, 2 ** 15 - 1, 2 ** 31 - 1, 2 ** 4 * 3 * 5, 2 ** 30):
        foos = [0, 1, -1, pivot, -pivot, 3 * pivot if 3 * pivot < 2 ** 31 else pivot, -(5 * pivot) if 5 * pivot < 2 ** 31 else -pivot,
                pivot - 1 if pivot > 2 else 5, 2 ** 31 - 1, -(2 ** 31 - 1), 6, 2 ** 15, -(2 ** 20), 7919 * 3, 210]
        dens = [1, -1, 6, 7919, 2 ** 15 - 1, 2 ** 31, 2 ** 33 + 6, -(3 * 2 ** 32)]
        for dpiv, psmall in ((1, 1), (6, 1), (2 ** 15 - 1, 1), (2 ** 15, 0), (7919 * 6, 0), (2 ** 40, 0), (-6, 1)):
            lanes = [(pivot, dpiv, psmall, f, d, (i + k) % 2) for i, f in enumerate(foos) for k, d in enumerate(dens)]
            for s0 in range(0, len(lanes), 64):
                chunk = lanes[s0:s0 + 64]
                rows += chunk + [chunk[0]] * (64 - len(chunk))
    return rows[:-7]  # (the last wave is not full)


def test_prepared_rows(probe):
    rows = [tuple(int(x) for x in r) for r in prep_cases()]
    want = [tuple(mask(v, 64) for v in prep_model(*r)) for r in rows]
    assert any(w[3] == 1 for w in want) and any(w[3] > 1 for w in want) and any(w[4] for w in want)
    got = unpack_words(probe.run(probe.L.pipamd_debug_arith, OP_LEAN_PREP, pack_words(rows, (1,) * 6), len(rows), 5), (1,) * 5)
    bad = [i for i in range(len(rows)) if got[i] != want[i]]
    assert not bad, "%d of %d lanes differ; first #%d pivot,dpiv,psmall,foo,den,rcls=%s: got %s want %s" % (
        len(bad), len(rows), bad[0], rows[bad[0]], [signed(x, 64) for x in got[bad[0]]], [signed(x, 64) for x in want[bad[0]]])


def test_new_probe_codes_are_bounded(probe):
    t = probe.torch
    buf = t.zeros(64, dtype=t.int64, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    assert probe.L.pipamd_debug_arith(probe.e._h, 129, p, p, 1) == -1
    assert probe.L.pipamd_debug_row_update(probe.e._h, 31, p, p, 1) == -1
    assert probe.L.pipamd_debug_row_update(probe.e._h, 36, p, p, 1) == -1
