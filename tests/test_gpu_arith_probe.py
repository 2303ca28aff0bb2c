"""The pivot kernels' exact arithmetic, function by function, against Python ints at the magnitudes where it changes path.

The probe (piplib_amd/csrc/pip_probe.hip, and the probe kernel at the end of pip_quast.hip) runs the SHIPPED device
functions on operands given here: pipamd_debug_arith, one case per lane, for the scalar helpers; pipamd_debug_row_update,
one wave per case, for the row updates.  Every output word of every case must equal the model:

  * scalar helpers: math.gcd, pow(m, -1, 2**W), // and % on Python ints;
  * row updates and the determinant walk: bigint_pip.row_update / det_update -- the restatement of traiter.c:412-501 that
    test_bigint_checker_vs_oracle64 and the GMP fixtures pin -- with ONE addition (wrap_row_model below) for the cases
    whose products leave W bits on the wrap-around paths.

The case lists are built by plain functions from fixed seeds; tests/test_arith_cases.py (no GPU) checks the lists
themselves: determinism, the paths' preconditions, that every width threshold holds a case, the model's own identities.

Guarantees of the callers that narrow a case list (issue rule: the guarantee and its call site next to the entry):
  * QK::quo / QK::floordiv never see (MIN, -1) or a zero divisor: every divisor in pip_quast.hip is a gcd64 result or a
    denominator quotient (pivoter: quo(pivot, d), quo(dpiv, d), quo(dt[i], d), d = gcd64(..) >= 1; the cut and context
    normalisations: quo(vp, g), floordiv(vc, g), g = gcd64 chain >= 1 and `g > 1` tested; bezout: floordiv(u, v), v = dd =
    quo(D, delta) >= 1 at first, then a pmod result that was tested non-zero).  gcd64 returns the magnitude, never -1 (its
    one negative value is gcd64(MIN, 0) = MIN).  So the pair is outside their documented domain ("for a non-zero divisor",
    piplib.h:147-149 with a positive divisor) and is left out; test_quast_division asserts that domain on its own list.
  * cquo(i128) beyond 64 bits divides exactly (its comment): multiples only.
  * det_step takes the REDUCED pair (pivot / d, dpiv / d), d = gcd(pivot, dpiv) (pip_det_replay_kernel, pip_kernels.hip):
    ppivot and dppiv are coprime, ppivot >= 1, dppiv >= 1.
  * exact_quo(a, d): d a positive gcd that divides a (det_step is its only caller).
  * umod128 / umod_small / umod128_32: a non-zero modulus (row_reduce_rem tests g == 0 itself; gcd_mag returns on b == 0).
"""
import ctypes as C
import math
import random

import numpy as np
import pytest

import bigint_pip as bp
from replay_model import det_model  # det_step in Python ints; shared with the replay probe's model

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ word packing
def mask(x, W):
    return x & ((1 << W) - 1)


def signed(x, W):
    x &= (1 << W) - 1
    return x - (1 << W) if x >> (W - 1) else x


def uabs(x, W):
    """magnitude of a W-bit two's complement value as an unsigned number: |MIN| = 2^(W-1) (uabs64 of the kernels)"""
    return abs(signed(x, W))


def pack_words(rows, widths):
    """rows: tuples of ints, value k taking widths[k] words (low word first) -> (n, sum(widths)) int64"""
    n, nw = len(rows), sum(widths)
    out = np.empty((n, nw), dtype=np.uint64)
    col = 0
    for k, w in enumerate(widths):
        vals = [r[k] for r in rows]
        for i in range(w):
            out[:, col] = np.array([(v >> (64 * i)) & M64 for v in vals], dtype=np.uint64)
            col += 1
    return out.view(np.int64)


def unpack_words(arr, widths):
    """(n, sum(widths)) int64 -> list of tuples of UNSIGNED ints of 64 * widths[k] bits"""
    u = arr.view(np.uint64)
    cols, col = [], 0
    for w in widths:
        vals = [int(x) for x in u[:, col]]
        for i in range(1, w):
            vals = [v | (int(x) << (64 * i)) for v, x in zip(vals, u[:, col + i])]
        cols.append(vals)
        col += w
    return list(zip(*cols)) if cols else []


# ------------------------------------------------------------------------------------------------ the probe's ABI
# pipamd_debug_arith: op -> (id, words of each input value, words of each output value); pip_probe.hip probe_io()
OPS = {
    "gcd_u32": (0, (1, 1), (1,)), "gcd_u64": (1, (1, 1), (1,)), "gcd_mag64": (2, (1, 1), (1,)),
    "gcd_mag128": (3, (2, 2), (2,)), "gcd_i64": (4, (1, 1), (1,)), "gcd_i128": (5, (2, 2), (2,)),
    "inv_odd64": (6, (1,), (1,)), "inv_odd128": (7, (2,), (2,)), "invW32": (8, (1,), (1,)),
    "cquo64": (9, (1, 1), (1,)), "cquo128": (10, (2, 2), (2,)), "crem64": (11, (1, 1), (1,)),
    "crem128": (12, (2, 2), (2,)), "fmod64": (13, (1, 1), (1,)), "fmod128": (14, (2, 2), (2,)),
    "exact_quo64": (15, (1, 1), (1,)), "exact_quo128": (16, (2, 2), (2,)),
    "umod128": (17, (2, 2), (2,)), "umod128_32": (18, (2, 1), (1,)), "umod_small64": (19, (1, 1, 1), (1,)),
    "umod_small128": (20, (2, 2, 1), (2,)), "umod_tiny": (21, (1, 1), (1,)), "umod_tiny_low": (22, (1, 1), (1,)),
    "row_mod_int": (23, (1, 1, 1, 1), (1, 1)), "row_mod_long": (24, (1, 1, 1, 1, 1), (1, 1, 1, 1)),
    "log2_64": (25, (1,), (1,)), "log2_128": (26, (2,), (1,)), "bitlen64": (27, (1,), (1,)),
    "bitlen128": (28, (2,), (1,)), "ctz128": (29, (2,), (1,)), "fits64": (30, (2,), (1,)),
    "bezout64": (31, (1, 1, 1), (1,)), "bezout128": (32, (2, 2, 2), (2,)),
    "det_step64": (33, (1,) * 7, (1,) * 6), "det_step128": (34, (2, 2, 2, 2, 1, 2, 2), (2, 2, 2, 2, 1, 1)),
}
# the device tree's helpers: 64 + 2 * function + (128-bit ? 1 : 0); three entries in, the result and `bad` out
QUAST_FN = {"gcd64": 0, "quo": 1, "rem": 2, "pmod": 3, "floordiv": 4, "qudiv": 5, "qumod": 6, "qinv": 7, "blen": 8,
            "cmul": 9, "cadd": 10, "csub": 11, "bezout": 12}
for _name, _fn in QUAST_FN.items():
    for _W in (64, 128):
        _ew = _W // 64
        OPS["q_%s%d" % (_name, _W)] = (64 + 2 * _fn + (_W == 128), (_ew, _ew, _ew), (_ew, 1))

# pipamd_debug_row_update: path -> (id, W, padded width WP, family of preconditions, the paths every case ALSO runs through)
PATHS = {
    "G64_1": (0, 64, 128, "G64", ()), "G64_2": (1, 64, 256, "G64", ()), "G64_4": (2, 64, 512, "G64", ()),
    "G64R": (3, 64, 128, "G64", ("G64_1",)), "S64": (4, 64, 128, "SMALL64", ("G64_1",)),
    "G128_1": (5, 128, 64, "G128", ()), "G128_4": (6, 128, 256, "G128", ()),
    "N128_1": (7, 128, 64, "N128", ("G128_1",)), "N128_4": (8, 128, 256, "N128", ("G128_4",)),
    "NN128_1": (9, 128, 64, "NN128", ("G128_1", "N128_1")), "NN128_4": (10, 128, 256, "NN128", ("G128_4", "N128_4")),
    "LI_S": (11, 64, 128, "SMALL64", ("G64_1", "S64")), "LI_M": (12, 64, 128, "LI_M", ("G64_1",)),
    "LL_S": (13, 128, 256, "LL_S", ("G128_4", "NN128_4")), "LL_M": (14, 128, 256, "LL_M", ("G128_4",)),
}
GPRE_PATHS = ("G128_1", "G128_4", "N128_1", "N128_4", "NN128_1", "NN128_4")  # run with gpre = 0 AND the caller's gcd

# Preconditions of a family (the operands its function is defined for; "any" = wrap-around):
#   row: |v|, |prow| < 2^row   mul: |lpiv|, |foo| < 2^mul   dpiv: |dpiv| < 2^dpiv   g0: |g0| < 2^g0
#   (a bound of W means any W-bit value, MIN included)
FAMILY = {
    # update_row<i64>: any operands, wrap-around
    "G64": dict(W=64, row=64, mul=64, dpiv=64, g0=64, thresholds=(19, 20, 21, 30, 31, 32, 33, 62, 63, 64)),
    # update_row_small / LeanIntRows::update_small: rows of class 0, |lpiv|, |foo|, |dpiv| < 2^15 (pip_advance.h comment;
    # the lean loop: `psmall && S.rcls[s] == 0`), so |z| < 2^31
    "SMALL64": dict(W=64, row=15, mul=15, dpiv=15, g0=64, thresholds=(19, 20, 21, 30, 31)),
    # LeanIntRows::update_mid: packed int rows (ROW_BITS 31) and int multipliers, any denominators
    "LI_M": dict(W=64, row=31, mul=31, dpiv=64, g0=64, thresholds=(19, 20, 21, 30, 31, 32, 33, 62, 63)),
    "G128": dict(W=128, row=128, mul=128, dpiv=128, g0=128,
                 thresholds=(19, 20, 21, 30, 31, 32, 33, 62, 63, 64, 65, 126, 127, 128)),
    # narrow64: row, pivot row and multipliers fit a long long
    "N128": dict(W=128, row=63, mul=63, dpiv=128, g0=128, thresholds=(30, 31, 32, 33, 62, 63, 64, 65, 126, 127)),
    # update_row_narrow: operands below 2^31, g0 within 63 bits
    "NN128": dict(W=128, row=31, mul=31, dpiv=31, g0=63, thresholds=(19, 20, 21, 30, 31, 32, 33, 62, 63)),
    # LeanLongRows::update_small: below 2^31 and small_den (|g0| < 2^62)
    "LL_S": dict(W=128, row=31, mul=31, dpiv=31, g0=62, thresholds=(19, 20, 21, 30, 31, 32, 33, 62, 63)),
    # LeanLongRows::update_mid: packed long long rows (ROW_BITS 63) and long long multipliers, any denominators
    "LL_M": dict(W=128, row=63, mul=63, dpiv=128, g0=128, thresholds=(30, 31, 32, 33, 62, 63, 64, 65, 126, 127)),
}
ROW_CASE_CAP = 2048


class Probe:
    """ctypes wrapper of the two probe entries (exported by libpipamd.so, not part of include/piplib_amd.h)"""

    def __init__(self):
        import torch
        from piplib_amd import engine as eng
        self.torch = torch
        self.L = eng.lib()
        self.L.pipamd_debug_arith.restype = C.c_int
        self.L.pipamd_debug_arith.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong]
        self.L.pipamd_debug_row_update.restype = C.c_int
        self.L.pipamd_debug_row_update.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        self.e = eng.Engine(0)

    def _run(self, fn, code, words, n, nout):
        t = self.torch
        din = t.from_numpy(np.ascontiguousarray(words)).cuda()
        dout = t.zeros((n, nout), dtype=t.int64, device="cuda")
        rc = fn(self.e._h, code, C.c_void_p(din.data_ptr()), C.c_void_p(dout.data_ptr()), n)
        assert rc == 0, rc
        return dout.cpu().numpy()

    def arith_words(self, op, words):
        code, win, wout = OPS[op]
        assert words.shape[1] == sum(win)
        return self._run(self.L.pipamd_debug_arith, code, words, words.shape[0], sum(wout))

    def arith(self, op, rows):
        code, win, wout = OPS[op]
        return unpack_words(self.arith_words(op, pack_words(rows, win)), wout)

    def rows(self, path, words, ncases):
        code, W, WP, _, _ = PATHS[path]
        return self._run(self.L.pipamd_debug_row_update, code, words, ncases, (W // 64) * (2 + WP))

    def rc(self, which, code, inp, out, n):
        fn = self.L.pipamd_debug_arith if which == "arith" else self.L.pipamd_debug_row_update
        return fn(self.e._h, code, C.c_void_p(inp), C.c_void_p(out), n)


@pytest.fixture(scope="module")
def probe():
    return Probe()


def check(op, probe, rows, want):
    """every output word of every case equals the model"""
    got = probe.arith(op, rows)
    _, _, wout = OPS[op]
    want = [tuple(mask(x, 64 * w) for x, w in zip(r, wout)) for r in want]
    assert len(got) == len(want)
    bad = [(rows[i], got[i], want[i]) for i in range(len(got)) if got[i] != want[i]]
    assert not bad, "%s: %d of %d cases differ, first: in %s got %s want %s" % (
        op, len(bad), len(got), [hex(x) for x in bad[0][0]], [hex(x) for x in bad[0][1]], [hex(x) for x in bad[0][2]])


# ------------------------------------------------------------------------------------------------ scalar operands
def edges(W, signed_vals):
    """0, 1, -1, 2^k, 2^k +- 1 for every k up to W, MIN, MAX -- as W-bit signed values, or unsigned ones"""
    s = {0, 1, -1}
    for k in range(W + 1):
        s.update((1 << k, (1 << k) - 1, (1 << k) + 1))
    s.update((-(1 << (W - 1)), (1 << (W - 1)) - 1))
    if signed_vals:
        s |= {-x for x in s}
        return sorted({signed(x, W) for x in s})
    return sorted({mask(x, W) for x in s})


KEY_BITS = (0, 1, 2, 15, 16, 20, 30, 31, 32, 33, 62, 63, 64, 65, 96, 126, 127, 128)


def key_edges(W, signed_vals):
    """the edges at the width thresholds of the kernels only (the second operand of a pair)"""
    s = {0, 1, -1, 3, 6, 10, 255}
    for k in KEY_BITS:
        if k <= W:
            s.update((1 << k, (1 << k) - 1, (1 << k) + 1))
    s.update((-(1 << (W - 1)), (1 << (W - 1)) - 1))
    if signed_vals:
        s |= {-x for x in s}
        return sorted({signed(x, W) for x in s})
    return sorted({mask(x, W) for x in s})


def fib_pairs(W):
    out, a, b = [], 1, 1
    while b < (1 << (W - 1)):
        out.append((b, a))
        a, b = b, a + b
    return out


def rand_bits(rng, W, signed_vals, n):
    """n values of uniformly drawn bit LENGTH (so that every magnitude band is met)"""
    out = []
    for _ in range(n):
        k = int(rng.integers(0, W + (0 if signed_vals else 1)))
        x = int.from_bytes(rng.bytes(16), "little") & ((1 << k) - 1) | ((1 << k) >> 1)
        out.append(-x if signed_vals and rng.integers(0, 2) else x)
    return out


def pair_cases(W, signed_vals, seed, nrand=1500):
    """operand pairs for a two-operand function of width W: every edge against the key edges, equal operands, neighbouring
    Fibonacci numbers, one operand wide and the other around 2^32, pairs whose OR straddles 2^32 and 2^64, seeded random"""
    rng = np.random.default_rng(seed)
    E, K = edges(W, signed_vals), key_edges(W, signed_vals)
    ps = [(a, b) for a in K for b in K] + [(a, a) for a in E]
    for i, a in enumerate(E):   # every edge against six of the key edges, either way round
        for r in range(6):
            b = K[(7 * i + r) % len(K)]
            ps += [(a, b), (b, a)]
    ps += fib_pairs(W) + [(a, b) for b, a in fib_pairs(W)]
    wide = [x for x in E if abs(x) >> 33] + rand_bits(rng, W, signed_vals, 40)
    for a in wide:
        for b in ((1 << 32) - 1, 1 << 32, (1 << 32) + 1, 3 * 5 * 7 * 11 * 13, 0xfffffffb):
            ps += [(a, b), (b, a)]
    for T in (32, 64):
        if T < W:
            for lo in ((1 << T) - 1, (1 << T) - 2, 1 << (T - 1)):
                for hi in (1 << T, (1 << T) + 1, (1 << T) | 12345):
                    ps += [(lo, lo - 1), (hi, lo), (lo, hi), (hi, hi - 1), (3 * lo, 3), (hi * 6, 6 * lo)]
    ra, rb = rand_bits(rng, W, signed_vals, nrand), rand_bits(rng, W, signed_vals, nrand)
    ps += list(zip(ra, rb))
    ps += [(a * g, b * g) for a, b, g in zip(rand_bits(rng, W // 3, signed_vals, 300), rand_bits(rng, W // 3, False, 300),
                                             rand_bits(rng, W // 3, False, 300))]   # a common factor
    lim = (-(1 << (W - 1)), (1 << (W - 1)) - 1) if signed_vals else (0, (1 << W) - 1)
    return [(a, b) for a, b in ps if lim[0] <= a <= lim[1] and lim[0] <= b <= lim[1]]


def tdiv(a, b):
    """C's truncating quotient"""
    q = abs(a) // abs(b)
    return -q if (a < 0) != (b < 0) else q


def trem(a, b):
    r = abs(a) % abs(b)
    return -r if a < 0 else r


def fits(x, W):
    return -(1 << (W - 1)) <= x < (1 << (W - 1))


# ------------------------------------------------------------------------------------------------ scalar tests
def test_probe_rejects_bad_arguments(probe):
    t = probe.torch
    buf = t.zeros(64, dtype=t.int64, device="cuda")
    p = buf.data_ptr()
    assert p % 16 == 0
    for which, good in (("arith", 0), ("rows", 0)):
        assert probe.rc(which, 999, p, p, 1) == -1       # PIPAMD_E_INVALID: unknown op / path
        assert probe.rc(which, -1, p, p, 1) == -1
        assert probe.rc(which, good, 0, p, 1) == -1      # null
        assert probe.rc(which, good, p, 0, 1) == -1
        assert probe.rc(which, good, p + 8, p, 1) == -1  # misaligned
        assert probe.rc(which, good, p, p + 8, 1) == -1
    assert probe.rc("arith", 35, p, p, 1) == -1 and probe.rc("arith", 64 + 26, p, p, 1) == -1
    assert probe.rc("rows", 15, p, p, 1) == -1


def test_gcd(probe):
    """gcd_u32 / gcd_u64 / gcd_mag / gcd_i64 and the device tree's gcd64 against math.gcd (gcd_mag(u128): the umod128_32
    shortcut for an operand below 2^32 and the first path beside it; the >> 32 and >> 64 dispatches)"""
    p32 = pair_cases(32, False, 11)
    check("gcd_u32", probe, p32, [(math.gcd(a, b),) for a, b in p32])
    p64 = pair_cases(64, False, 12)
    check("gcd_u64", probe, p64, [(math.gcd(a, b),) for a, b in p64])
    check("gcd_mag64", probe, p64, [(math.gcd(a, b),) for a, b in p64])
    p128 = pair_cases(128, False, 13)
    check("gcd_mag128", probe, p128, [(math.gcd(a, b),) for a, b in p128])
    for W in (64, 128):
        ps = pair_cases(W, True, 14 + W)
        check("gcd_i%d" % W, probe, ps, [(math.gcd(a, b),) for a, b in ps])
        # QK::gcd64: the same magnitudes (gcd64(x, 0) = |x|, gcd64(0, y) by the loop)
        check("q_gcd64%d" % W, probe, [(a, b, 0) for a, b in ps], [(math.gcd(a, b), 0) for a, b in ps])


def odd_cases(W, seed):
    rng = np.random.default_rng(seed)
    return sorted({x | 1 for x in edges(W, False)} | {x | 1 for x in rand_bits(rng, W, False, 2000)})


def test_inverses(probe):
    """inv_odd64 (u64, u128), invW(unsigned), qinv (u64, u128): m * inv == 1 modulo 2^W for every odd m"""
    for op, W in (("inv_odd64", 64), ("inv_odd128", 128), ("invW32", 32)):
        ms = odd_cases(W, 20 + W)
        check(op, probe, [(m,) for m in ms], [(pow(m, -1, 1 << W),) for m in ms])
    for W in (64, 128):
        ms = odd_cases(W, 30 + W)
        check("q_qinv%d" % W, probe, [(m, 0, 0) for m in ms], [(pow(m, -1, 1 << W), 0) for m in ms])


# Finding of this probe, narrowed to the callers' domain: cquo(i128) answers (-2^63, -1) in 64 bits (its long long shortcut
# wraps: -2^63 instead of 2^63).  Every call site divides by a gcd or by a remainder, never by a negative number --
# exact_quo(a, d), d = gcd_i64(..) >= 1 (det_step; phase A / the lane preparation of pip_advance_kernel: exact_quo(pivot, d),
# exact_quo(foo, d)); the deepest cut: cquo(t, delta), cquo(D, delta), delta = gcd_i64(t, D); bezout_dev: cquo(u - r, v), v the
# positive modulus first and a non-zero fmod64 result after -- so the pair is left out; its neighbours stay in the list.
# (Answering it in 128 bits, `if (b == -1) return wneg(a)` before the shortcut, moves the register allocation of every
# 128-bit pivot kernel -- e.g. pip_advance_kernel<__int128, 4, 16>: 85 -> 125 spilled VGPRs at the same 128 VGPRs and 432
# bytes of scratch -- for a pair no caller forms.)
CQUO128_OUTSIDE = (-(1 << 63), -1)
CQUO128_NEIGHBOURS = [(-(1 << 63) + 1, -1), (-(1 << 63) - 1, -1), (-(1 << 63), 1), (1 << 63, -1), (-(1 << 127), -1)]


def division_pairs(W, seed):
    ps = pair_cases(W, True, seed) + (CQUO128_NEIGHBOURS if W == 128 else [])
    ps += [(a, b) for a in edges(W, True) for b in (0, 1, -1, 2, -2, 3, -3)]
    return ps


def test_division_total(probe):
    """cquo / crem / fmod64 (i64, i128): C's '/' and '%' made total -- divisors 0, 1 and -1 included, (MIN, -1) wraps to
    MIN; cquo(i128) with an operand beyond 64 bits on exact multiples only (it is an exact division), and without the one
    pair (-2^63, -1) that no caller forms (CQUO128_OUTSIDE above)"""
    for W in (64, 128):
        ps = division_pairs(W, 40 + W)

        def cquo(a, b):
            return 0 if b == 0 else tdiv(a, b)

        def crem(a, b):
            return 0 if b in (0, 1, -1) else trem(a, b)

        def fmod(a, b):
            return 0 if b in (0, 1, -1) else a % abs(b)
        if W == 64:
            qs = ps
        else:
            qs = [(a, b) for a, b in ps if (fits(a, 64) and fits(b, 64)) or b == 0 or (b != 0 and a % b == 0)]
            assert CQUO128_OUTSIDE in qs and all(c in qs for c in CQUO128_NEIGHBOURS)
            qs = [c for c in qs if c != CQUO128_OUTSIDE]   # the callers' domain: see CQUO128_OUTSIDE
            rng = np.random.default_rng(44)
            for q, b in zip(rand_bits(rng, 100, True, 1500), rand_bits(rng, 126, True, 1500)):
                if b and fits(q * b, 128):
                    qs.append((q * b, b))   # exact multiples, either operand beyond 64 bits
            assert sum(1 for a, b in qs if not fits(a, 64) or not fits(b, 64)) > 1500
        check("cquo%d" % W, probe, qs, [(cquo(a, b),) for a, b in qs])
        check("crem%d" % W, probe, ps, [(crem(a, b),) for a, b in ps])
        check("fmod%d" % W, probe, ps, [(fmod(a, b),) for a, b in ps])


def exact_quo_cases(W, seed):
    """(a, d): d a positive gcd dividing a -- d a power of two, odd, and mixed, quotient and divisor on both sides of the
    32-bit line of exact_quo's shortcut"""
    rng = np.random.default_rng(seed)
    ds = [1 << k for k in range(0, W - 1)] + [3, 5, 0xffffffff, 0xfffffffb, (1 << 32) + 1, (1 << 32) + 15, 3 << 31, 3 << 30, 5 << 29,
                                             0xffff0000, 0x80000000, 0x7fffffff, (1 << 61) - 1, 12 * 0x10001]
    ds += [d for d in rand_bits(rng, W - 2, False, 400) if d]
    out = []
    for d in ds:
        for q in (0, 1, -1, 2, 3, -3, (1 << 32) // d, (1 << 32) // d + 1, -((1 << 32) // d), ((1 << 32) - 1) // d,
                  ((1 << (W - 1)) - 1) // d, -((1 << (W - 1)) // d), int(rng.integers(0, 1 << 31)), -int(rng.integers(0, 1 << 20))):
            if fits(q * d, W) and fits(d, W):
                out.append((q * d, d))
    return out


def test_exact_quo(probe):
    for W in (64, 128):
        cs = exact_quo_cases(W, 50 + W)
        assert any(abs(a) | d < (1 << 32) for a, d in cs) and any((abs(a) | d) >> 32 == 1 for a, d in cs)
        check("exact_quo%d" % W, probe, cs, [(a // d,) for a, d in cs])


def test_quast_division(probe):
    """QK::quo / rem / pmod / floordiv and qudiv / qumod against // and % on Python ints.

    (MIN, -1): cannot reach quo or floordiv -- see the module docstring: every divisor at their call sites is a gcd64
    result or a quotient of denominators, at least 1.  The pair is outside their documented domain (a non-zero divisor, and
    piplib.h:147-149's floor division by a positive one) and is left out; the list below asserts that it is the only
    pair left out besides the zero divisors."""
    for W in (64, 128):
        MIN = -(1 << (W - 1))
        ps = [(a, b) for a, b in division_pairs(W, 60 + W) if b != 0]
        assert (MIN, -1) in ps and (MIN, 1) in ps and (MIN, MIN) in ps and (MIN + 1, -1) in ps
        ps = [(a, b) for a, b in ps if (a, b) != (MIN, -1)]
        tri = [(a, b, 0) for a, b in ps]
        check("q_quo%d" % W, probe, tri, [(tdiv(a, b), 0) for a, b in ps])
        check("q_rem%d" % W, probe, tri, [(trem(a, b), 0) for a, b in ps])
        check("q_pmod%d" % W, probe, tri, [(a % abs(b), 0) for a, b in ps])

        def floordiv(a, b):  # quo(csub(a, pmod(a, b)), b): the subtraction is checked (a near MIN), the quotient is exact
            x = a - a % abs(b)
            return (tdiv(signed(x, W), b), 0 if fits(x, W) else 1)
        want = [floordiv(a, b) for a, b in ps]
        assert all(q == a // b for (a, b), (q, bad) in zip(ps, want) if b > 0 and not bad)
        check("q_floordiv%d" % W, probe, tri, want)
        us = [(a, b) for a, b in pair_cases(W, False, 70 + W) if b != 0]
        tri = [(a, b, 0) for a, b in us]
        check("q_qudiv%d" % W, probe, tri, [(a // b, 0) for a, b in us])
        check("q_qumod%d" % W, probe, tri, [(a % b, 0) for a, b in us])


def test_unsigned_remainders(probe):
    """umod128, umod128_32 (a 32-bit modulus, the double estimate one off either way), umod_small in both widths"""
    rng = np.random.default_rng(80)
    us = [(a, g) for a, g in pair_cases(128, False, 81) if g != 0]
    check("umod128", probe, us, [(a % g,) for a, g in us])
    check("umod_small128", probe, [(a, g, 0) for a, g in us], [(a % g,) for a, g in us])
    s32 = [(a, g) for a, g in pair_cases(32, False, 82) if g != 0]
    check("umod_small128", probe, [(a, g, 1) for a, g in s32], [(a % g,) for a, g in s32])
    check("umod_small64", probe, [(a, g, 1) for a, g in s32], [(a % g,) for a, g in s32])
    u64 = [(a, g) for a, g in pair_cases(64, False, 83) if g != 0]
    check("umod_small64", probe, [(a, g, 0) for a, g in u64], [(a % g,) for a, g in u64])
    # umod128_32: every digit step at the edges of its estimate -- t = r * 2^32 + digit just below / at / above a multiple
    bs = sorted({1, 2, 3, 5, 0xffff, 0x10000, 0x10001, 0x7fffffff, 0x80000000, 0x80000001, 0xfffffffb, 0xfffffffe, 0xffffffff}
                | {b for b in rand_bits(rng, 32, False, 300) if b})
    cs = []
    for b in bs:
        for a in edges(128, False)[::3] + rand_bits(rng, 128, False, 12):
            cs.append((a, b))
        for q in (0xffffffff, 0xfffffffe, 1 << 31, (1 << 32) // b):
            for k in (1, 2, 3):
                m = (q * b) << (32 * k)
                cs += [(x, b) for x in (m - 1, m, m + 1, m + b - 1, m | ((1 << (32 * k)) - 1)) if 0 <= x < (1 << 128)]
        cs += [((b - 1) << 96 | (b - 1) << 64 | 0xffffffff << 32 | 0xffffffff, b), ((1 << 128) - 1, b), ((1 << 128) - b, b)]
    check("umod128_32", probe, cs, [(a % b,) for a, b in cs])


def tiny_cases(glo, seed):
    """(a, g) for every g in [glo, 2^20): a in {0, 1, g - 1, g, 2^20 - 1}, k g - 1, k g, k g + 1 for the largest k that keeps
    a < 2^20, and four seeded random a -- int64 array (n, 2)"""
    rng = np.random.default_rng(seed)
    g = np.arange(glo, 1 << 20, dtype=np.int64)
    top = (1 << 20) - 1
    k = (top - 1) // g                       # the largest k with k g + 1 < 2^20
    cols = [np.zeros_like(g), np.minimum(np.ones_like(g), top), g - 1, g, np.full_like(g, top), k * g - 1, k * g, k * g + 1]
    cols += [rng.integers(0, 1 << 20, size=g.size, dtype=np.int64) for _ in range(4)]
    a = np.clip(np.stack(cols, axis=1), 0, top)   # (k = 0 only for g = 2^20 - 1, where k g - 1 = -1 -> 0)
    return np.stack([a.ravel(), np.repeat(g, a.shape[1])], axis=1)


@pytest.mark.parametrize("op,glo", [("umod_tiny", 1), ("umod_tiny_low", 2)])
def test_float_reciprocal_remainders(probe, op, glo):
    """umod_tiny(a, g, v_rcp_f32(g)) for every g in [1, 2^20) and umod_tiny_low(a, g, rcp_low(g)) for every g in [2, 2^20),
    with the DEVICE's reciprocal (tests/test_remainder_bound.py holds the argument to a numpy model of it)"""
    cs = tiny_cases(glo, 90 + glo)
    assert cs.shape[0] > 12_000_000 and cs.min() >= 0 and cs[:, 0].max() == (1 << 20) - 1 and cs[:, 1].min() == glo
    for part in np.array_split(cs, 4):
        got = probe.arith_words(op, part)[:, 0]
        want = part[:, 0] % part[:, 1]
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "%s: %d differ, first a=%d g=%d got %d want %d" % (
            op, bad.size, part[bad[0], 0], part[bad[0], 1], got[bad[0]], want[bad[0]])


def row_mod_cases(seed):
    rng = np.random.default_rng(seed)
    ints, longs = [], []
    for D in (2, 3, (1 << 15) - 1, 1 << 15, (1 << 15) + 1, 1 << 14, 12345, (1 << 20) - 1, 1 << 20, (1 << 31) - 1, 1 << 30):
        for cls0 in (1, 0):
            lim = (1 << 15) - 1 if cls0 else (1 << 31) - 1
            vals = [0, 1, -1, D - 1, -(D - 1), D, -D, D + 1, -(D + 1), lim, -lim, (lim // D) * D, -(lim // D) * D,
                    (lim // D) * D - 1, -((lim // D) * D - 1)] + [int(x) for x in rng.integers(-lim, lim + 1, size=24)]
            vals = [v for v in vals if abs(v) <= lim]
            ints += [(a, b, D, cls0) for a, b in zip(vals, vals[1:] + vals[:1])]
    for D in (2, 3, (1 << 15) - 1, 1 << 15, (1 << 31) - 1, 1 << 31, (1 << 32) + 1, (1 << 61) - 1, 1 << 61, (1 << 62) - 1):
        lim = (1 << 63) - 1
        vals = [0, 1, -1, D - 1, -(D - 1), D, -D, D + 1, -(D + 1), lim, -lim, -(1 << 63), (lim // D) * D, -(lim // D) * D,
                (1 << 31) - 1, -(1 << 31), 1 << 32] + rand_bits(rng, 64, True, 23)
        longs += [tuple(vals[(i + k) % len(vals)] for k in range(4)) + (D,) for i in range(len(vals))]
    return ints, longs


def test_row_mod(probe):
    """LeanIntRows::row_mod (the float-reciprocal path below D = 2^15 on class-0 rows, `%` beside it) and
    LeanLongRows::row_mod: piplib_llmod of every entry -- D at 2, 2^15 - 1, 2^15; cls0 both ways; negative entries; exact
    multiples of D"""
    ints, longs = row_mod_cases(100)
    check("row_mod_int", probe, ints, [(a % D, b % D) for a, b, D, _ in ints])
    check("row_mod_long", probe, longs, [tuple(x % r[4] for x in r[:4]) for r in longs])


def test_bit_counts(probe):
    """log2_64, bitlen64, ctz128, fits64, QK::blen"""
    rng = np.random.default_rng(110)
    for W in (64, 128):
        sv = edges(W, True) + rand_bits(rng, W, True, 500)
        uv = edges(W, False) + rand_bits(rng, W, False, 500)
        check("log2_%d" % W, probe, [(x,) for x in sv], [(abs(x).bit_length() or 1,) for x in sv])
        check("bitlen%d" % W, probe, [(x,) for x in uv], [(x.bit_length(),) for x in uv])
        check("q_blen%d" % W, probe, [(x, 0, 0) for x in sv], [(abs(x).bit_length() or 1, 0) for x in sv])
    uv = [x for x in edges(128, False) + rand_bits(rng, 128, False, 500) + [1 << 64, 3 << 64, 1 << 127, 5 << 63] if x]
    check("ctz128", probe, [(x,) for x in uv], [((x & -x).bit_length() - 1,) for x in uv])
    sv = edges(128, True) + rand_bits(rng, 128, True, 500) + [-(1 << 63) - 1, -(1 << 63), (1 << 63) - 1, 1 << 63]
    check("fits64", probe, [(x,) for x in sv], [(1 if fits(x, 64) else 0,) for x in sv])


def qmulo_model(a, b, W):
    """the device tree's checked multiply flags exactly the products that leave W bits, in both widths (w128: by the bit
    lengths where they decide -- a sum of at most 127 fits, 130 and more cannot -- and by the 256-bit product in between)"""
    return 0 if fits(a * b, W) else 1


def checked_cases(W, seed):
    rng = np.random.default_rng(seed)
    ps = pair_cases(W, True, seed, nrand=600)
    # operands on both sides of each line: bit lengths summing to W - 3 .. W + 1, products just below / above 2^(W-1)
    for la in list(range(1, W, 5)) + [63, 64, 65]:
        for tot in range(W - 4, W + 2):
            lb = tot - la
            if 1 <= lb < W and la < W:
                for _ in range(2):
                    a = int.from_bytes(rng.bytes(16), "little") & ((1 << la) - 1) | (1 << (la - 1))
                    b = int.from_bytes(rng.bytes(16), "little") & ((1 << lb) - 1) | (1 << (lb - 1))
                    ps += [(a, b), (-a, b), (a, -b), (-a, -b), ((1 << la) - 1, (1 << lb) - 1), (1 << (la - 1), 1 << (lb - 1)),
                           (-(1 << (la - 1)), 1 << (lb - 1))]
    for k in range(1, W - 1):
        ps += [(1 << k, 1 << (W - 1 - k)), (-(1 << k), 1 << (W - 1 - k)), (1 << k, (1 << (W - 1 - k)) - 1)]
    return [(a, b) for a, b in ps if fits(a, W) and fits(b, W)]


def test_checked_arithmetic(probe):
    """cmul (qmulo), cadd, csub of the device tree in both widths: the result and the `bad` flag, which is set exactly when
    the true result leaves W bits.  The w128 list holds products whose operands' bit lengths sum to 128 and 129 -- where the
    lengths alone do not decide -- on both sides of 2^127, and -2^127 itself."""
    for W in (64, 128):
        ps = checked_cases(W, 120 + W)
        bad = [qmulo_model(a, b, W) for a, b in ps]
        band = [f for (a, b), f in zip(ps, bad) if abs(a).bit_length() + abs(b).bit_length() in (W, W + 1) and not (fits(a, 64) and fits(b, 64))]
        assert sum(bad) > 100 and any(a * b == -(1 << (W - 1)) for a, b in ps)
        assert W == 64 or (sum(band) > 10 and len(band) - sum(band) > 10)
        tri = [(a, b, 0) for a, b in ps]
        check("q_cmul%d" % W, probe, tri, [(a * b, f) for (a, b), f in zip(ps, bad)])
        check("q_cadd%d" % W, probe, tri, [(a + b, 0 if fits(a + b, W) else 1) for a, b in ps])
        check("q_csub%d" % W, probe, tri, [(a - b, 0 if fits(a - b, W) else 1) for a, b in ps])


def bezout_wrap(x, y, delta, W, checked):
    """integrer.c:98-150 as bezout_dev / QK::bezout run it on W-bit registers; `checked`: the device tree's overflow flag
    (cmul / csub / floordiv's subtraction), else None"""
    bad = 0

    def mul(a, b):
        nonlocal bad
        bad |= qmulo_model(a, b, W)
        return signed(a * b, W)

    def sub(a, b):
        nonlocal bad
        bad |= 0 if fits(a - b, W) else 1
        return signed(a - b, W)
    a, b, c, d, u, v = 1, 0, 0, 1, y, delta
    for _ in range(200 if checked else 4 * W):
        if v in (0, 1, -1):
            r = 0
        else:
            r = u % abs(v)
        q = 0 if v == 0 else tdiv(sub(u, r), v)
        if r == 0:
            break
        u, v = v, r
        e, f = sub(a, mul(q, c)), sub(b, mul(q, d))
        a, b, c, d = c, d, e, f
    if v != 1:
        return 0, bad
    cx = mul(c, x)
    return (0 if delta in (0, 1, -1) else cx % abs(delta)), bad


def bezout_cases(W, seed):
    rng = np.random.default_rng(seed)
    cs = []
    for a, b in fib_pairs(W)[::3]:
        cs += [(3, b, a), (a - 1, a, b), (-5, b, a)]
    for lb in (2, 5, 15, 16, 31, 32, 33, 48, 62, 63, 64, 65, 100, 126, 127):
        if lb < W:
            for _ in range(12):
                delta = int.from_bytes(rng.bytes(16), "little") & ((1 << lb) - 1) | (1 << (lb - 1))
                y = int.from_bytes(rng.bytes(16), "little") % delta
                x = int.from_bytes(rng.bytes(16), "little") % delta
                cs += [(x, y, delta), (-x, y, delta), (x, y + delta, delta) if fits(y + delta, W) else (x, y, delta), (x, 2 * y, 2 * delta)
                       if fits(2 * delta, W) else (x, y, delta), (1, y, delta), (x, 1, delta), (x, 0, delta), (0, y, delta)]
    cs += [(5, 3, 1), (0, 0, 1), (7, 7, 7), (1, 1, 2), (9, -4, 7), (9, 4, 1 << (W - 2))]
    return [c for c in cs if all(fits(v, W) for v in c) and c[2] >= 1]


def test_bezout(probe):
    """bezout_dev<i64>, bezout_dev<i128> and QK::bezout in both widths (delta >= 1, deepen()'s call): the three agree wherever
    the device tree's `bad` is clear, there (z y - x) % delta == 0 when gcd(y, delta) == 1 and z == 0 otherwise.  QK::bezout's
    `bad` is set exactly when a product or difference of the walk leaves W bits (qmulo_model: the multiply is exact in
    both widths)"""
    for W in (64, 128):
        cs = bezout_cases(W, 130 + W)
        dev = [bezout_wrap(x, y, d, W, False)[0] for x, y, d in cs]
        qk = [bezout_wrap(x, y, d, W, True) for x, y, d in cs]
        clear = 0
        for (x, y, d), zd, (zq, bad) in zip(cs, dev, qk):
            if not bad:
                clear += 1
                assert zd == zq and 0 <= zq < d
                if math.gcd(y, d) == 1:
                    assert (zq * y - x) % d == 0 and zq == (x * pow(y, -1, d)) % d
                else:
                    assert zq == 0
        assert clear > len(cs) // 2
        check("bezout%d" % W, probe, cs, [(z,) for z in dev])
        check("q_bezout%d" % W, probe, cs, qk)


def det_cases(W, seed):
    """limbs at bit lengths W - 2 and W - 1 against ppivot of 1 and 2 bits (the log2 + log2 < B line, the first-fit walk onto
    the next limb); ldet 0 .. 3, the fourth limb overflowing; dppiv sharing factors with one limb, several, none; dppiv 1.
    (ppivot, dppiv) coprime, both >= 1: the reduced pair det_step is given"""
    rng = np.random.default_rng(seed)

    def rnd(bits):
        return int.from_bytes(rng.bytes(16), "little") & ((1 << bits) - 1) | (1 << (bits - 1))
    cs = []
    junk = (rnd(W - 3), -rnd(17), rnd(40), 12345)
    for ldet in range(0, 4):
        for lb in (1, 2, 31, 32, 33, W // 2, W - 3, W - 2, W - 1):
            for pp in (1, 2, 3, rnd(31), rnd(32), rnd(33), rnd(W - 2), (1 << (W - 1)) - 1):
                for fill in (W - 1, W - 2, 5):
                    limbs = [rnd(fill) for _ in range(4)]
                    if ldet:
                        limbs[ldet - 1] = rnd(lb)
                        if lb > 2 and rng.integers(0, 2):
                            limbs[ldet - 1] = (1 << lb) - 1
                    for i in range(ldet, 4):
                        limbs[i] = junk[i]
                    cs.append((limbs, ldet, pp, 1))
        # dppiv and the limbs' factors
        for _ in range(40):
            fs = [int(x) for x in rng.choice([2, 3, 5, 7, 11, 13, 0x10001, 0xfffffffb, (1 << 31) - 1, (1 << 61) - 1], size=3)]
            limbs = [rnd(int(rng.integers(2, W - 40))) for _ in range(4)]
            kind = int(rng.integers(0, 4))
            dpp = 1
            if kind == 0 and ldet:      # all of dppiv in one limb
                i = int(rng.integers(0, ldet))
                limbs[i] = limbs[i] >> 35 or 1
                limbs[i] *= fs[0] * fs[1]
                dpp = fs[0] * fs[1]
            elif kind == 1:             # spread over the limbs in use, one factor each (some shared by two limbs)
                for i in range(ldet):
                    limbs[i] = (limbs[i] >> 70 or 1) * fs[i % 3] * (fs[(i + 1) % 3] if i == 1 else 1)
                    dpp *= fs[i % 3]
            elif kind == 2:             # a factor no limb has: overflow
                dpp = fs[0] * 1000003
                limbs = [x | 1 for x in limbs]
            if rng.integers(0, 4) == 0 and ldet:
                limbs[0] = -limbs[0]
            pp = rnd(int(rng.integers(1, W - 1)))
            while math.gcd(pp, dpp) != 1:
                pp += 1
            for i in range(ldet, 4):
                limbs[i] = junk[i]
            cs.append((limbs, ldet, pp, dpp))
    return [c for c in cs if all(fits(x, W) for x in c[0]) and fits(c[2], W) and fits(c[3], W)]


def test_det_step(probe):
    for W in (64, 128):
        cs = det_cases(W, 140 + W)
        want = [det_model(l, n, pp, dp, W) for l, n, pp, dp in cs]
        assert {w[4] for w in want} == {0, 1, 2, 3, 4} and {w[5] for w in want} == {0, 1}
        check("det_step%d" % W, probe, [tuple(l) + (n, pp, dp) for l, n, pp, dp in cs], want)


# ------------------------------------------------------------------------------------------------ the row model
def plain_row_model(c):
    """bigint_pip.row_update on the case -> (ok, newden, z, lpiv, foo, g0, products) in true integers"""
    v = np.array(c["v"], dtype=object)
    prow = np.array(c["prow"], dtype=object)
    pivj = c["pivj"]
    pivot = int(prow[pivj])
    try:
        z, newden, lpiv, foo = bp.row_update(v, c["den"], prow, pivot, c["dpiv"], pivj)
    except ZeroDivisionError:   # gcd(0, 0, ..., 0): the reference would divide by zero -- `ok` false, nothing changes
        d = math.gcd(pivot, int(v[pivj]))
        lpiv, foo = pivot // d, int(v[pivj]) // d
        return 0, lpiv * c["den"], [0] * len(v), lpiv, foo
    return 1, newden, [int(x) for x in z], lpiv, foo


def multipliers(c):
    pivot, x = c["prow"][c["pivj"]], c["v"][c["pivj"]]
    d = math.gcd(pivot, x)
    return pivot // d, x // d


def wrap_row_model(c, W):
    """The one addition to bigint_pip's model, for update_row<T> / update_mid on operands whose products leave W bits:
    each product and the difference reduced to W-bit two's complement first (wmul / wsub), magnitudes taken as unsigned
    (uabs64: |MIN| = 2^(W-1)), then the same gcd and exact division.  -> (ok, newden, z, B) with B the bit length of the
    largest |z| before the division (what row_reduce switches on)"""
    lpiv, foo = multipliers(c)
    pivj = c["pivj"]
    g0 = signed(lpiv * c["den"], W)
    z = [signed(signed(a * lpiv, W) - signed(b * foo, W), W) for a, b in zip(c["v"], c["prow"])]
    z[pivj] = signed(c["dpiv"] * foo, W)
    B = max(abs(x) for x in z).bit_length()
    g = abs(g0)
    for x in z:
        if g == 1:
            break
        g = math.gcd(g, abs(x))
    if g == 0:
        return 0, g0, z, B
    return 1, g0 // g, [x // g for x in z], B


def case_fits(c, W, but_dpiv_foo=False):
    """no product, difference or denominator product of the case leaves W bits: the plain model applies"""
    lpiv, foo = multipliers(c)
    lim = 1 << (W - 1)
    if not (abs(lpiv * c["den"]) < lim and (but_dpiv_foo or abs(c["dpiv"] * foo) < lim)):
        return False
    return all(abs(a * lpiv) < lim and abs(b * foo) < lim and abs(a * lpiv - b * foo) < lim for a, b in zip(c["v"], c["prow"]))


def row_model(c, W):
    """(ok, newden, z): the plain model wherever nothing exceeds W bits, the wrap model elsewhere"""
    if case_fits(c, W):
        ok, nd, z, _, _ = plain_row_model(c)
        return ok, nd, z
    ok, nd, z, _ = wrap_row_model(c, W)
    return ok, nd, z


def preconditions_hold(c, fam):
    f = FAMILY[fam]
    W = f["W"]
    lpiv, foo = multipliers(c)

    def below(x, bits):
        return fits(x, W) if bits == W else abs(x) < (1 << bits)
    g0 = lpiv * c["den"]
    if f["g0"] != W and not below(g0, f["g0"]):
        return False
    if f["row"] != W and not case_fits(c, W, but_dpiv_foo=fam in ("LI_M", "LL_M")):
        return False   # only the wrap-around families take products beyond W bits (the mid paths: dpiv * foo alone)
    return (all(below(x, f["row"]) for x in c["v"]) and all(below(x, f["row"]) for x in c["prow"]) and below(lpiv, f["mul"])
            and below(foo, f["mul"]) and below(c["dpiv"], f["dpiv"]) and fits(c["den"], W) and c["prow"][c["pivj"]] > 0
            and 0 <= c["pivj"] < len(c["v"]))


# ------------------------------------------------------------------------------------------------ the row cases
PRIMES = (3, 5, 7, 11, 13, 17, 19, 23)


class CaseRng:
    """the calls the case builders make, on random.Random (a row case draws several numbers per column)"""

    def __init__(self, seed):
        self.r = random.Random(seed)

    def integers(self, lo, hi):
        return self.r.randrange(lo, hi)

    def bytes(self, n):
        return self.r.getrandbits(8 * n).to_bytes(n, "little")

    def choice(self, seq):
        return seq[self.r.randrange(len(seq))]


def rnd_top(rng, bits):
    """a number of exactly `bits` bits in the top quarter of its range"""
    if bits <= 2:
        return (1 << bits) - 1
    return (3 << (bits - 2)) + (int.from_bytes(rng.bytes(16), "little") & ((1 << (bits - 2)) - 1))


def rnd_mag(rng, bits):
    if bits <= 0:
        return 0
    return int.from_bytes(rng.bytes(16), "little") & ((1 << bits) - 1)


def lane_positions(W, WP):
    """columns in lane 0, in lane 63, in every chunk and half, and in the last chunk"""
    if W == 64:   # lane (j % 128) / 2, chunk j / 128, half j & 1
        cols = [0, 1, 126, 127] + [128 * c + 2 * 17 + h for c in range(WP // 128) for h in (0, 1)] + [WP - 1, WP - 128, WP - 65]
    else:         # lane j % 64, chunk j / 64
        cols = [0, 63] + [64 * c + 21 for c in range(WP // 64)] + [WP - 1, WP - 64, WP - 30]
    return [j for j in dict.fromkeys(cols) if 0 <= j < WP]


def build_case(rng, fam, WP, B, gfac, hs, pivj, odd_pos, g0kind="M", foo_zero=False, only_pivj=False, exact_g=False, tag="",
               force=None):
    """A row update whose z (before the division) has its largest magnitude at exactly B bits, every entry a multiple of
    M = prod(gfac) * prod(hs) except one per prime of `hs` (at odd_pos: a multiple of M / h only -- one more refinement
    round each), built backwards: for coprime multipliers (lpiv, foo) any target t is v * lpiv - q * foo with
    q = -t / foo mod lpiv."""
    f = FAMILY[fam]
    W, br, bm = f["W"], min(f["row"], f["W"] - 1), min(f["mul"], f["W"] - 1)
    if B == W:   # only MIN has W bits: a power of two
        gfac, hs = [math.prod(gfac) if exact_g else 1 << int(rng.integers(0, W - 1))], []
    one = (lambda lo, hi: 1) if exact_g else rng.integers   # exact_g: the starting g = gcd(|g0|, |dpiv foo|) is M itself
    M = math.prod(gfac) * math.prod(hs)
    while M > (1 << (B - 1)) and (hs or gfac):
        if hs:
            hs = hs[:-1]
        else:
            gfac = gfac[:-1]
        M = math.prod(gfac) * math.prod(hs)
    tlo = 1 << (B - 1)
    thi = tlo if B == W else tlo + (tlo >> 2)          # targets' magnitudes stay within [.., thi]: B is exact
    both = (not foo_zero) and B - br + 2 > bm           # under operand bounds of b bits, B near 2 b: a full-size foo, and
    heavy = both and B <= br + bm                       # up to 2 b bits from q * foo alone (lpiv small), beyond from both products
    # the multipliers
    if foo_zero:
        lpiv, foo = 1, 0
    else:
        fl = list(gfac) + list(hs)
        F1 = math.prod(fl[::2])
        if both:
            if F1 >= (1 << (bm - 2)):
                F1 = 1
            foo = F1 * (rnd_top(rng, bm) // F1)        # a multiple of F1 with all of its bm bits
        else:
            if F1 >= (1 << min(bm, B - 1)) or F1 == 0:
                F1 = 1
            foo = F1 * int(one(1, 4))
            if abs(foo) >= (1 << bm) or foo * (M // F1) > thi:
                foo = F1
        if g0kind == "M" or g0kind.startswith("wide"):
            Lb = max(1, min(bm, max(1 if heavy else B - br + 2, int(rng.integers(1, 12)))))
        else:
            Lb = 1                                     # lpiv = 1: g0 is the row's own denominator, free to choose
        lpiv = rnd_top(rng, Lb) if Lb > 1 else 1
        while math.gcd(lpiv, foo) != 1:
            lpiv += 1
        if lpiv >= (1 << bm):
            lpiv = 1
        if rng.integers(0, 2):
            foo = -foo
    # the pivot row's denominator: z[pivj] = dpiv * foo, a multiple of M where the bounds allow, within the targets' range
    if foo:
        need = M // math.gcd(M, abs(foo))
        dpiv = need * int(one(1, 4))
        if abs(dpiv * foo) > thi:
            dpiv = need
        if abs(dpiv * foo) > thi or dpiv >= (1 << min(f["dpiv"], W - 1)):
            dpiv = max(1, min(thi // abs(foo), (1 << min(f["dpiv"], W - 1)) - 1) >> int(rng.integers(0, 3)))
    else:
        dpiv = M * int(rng.integers(1, 9)) if M < (1 << min(f["dpiv"], W - 1)) // 8 else 1
    # the targets
    ncol = WP if rng.integers(0, 3) else int(rng.integers(max(pivj + 1, max(odd_pos, default=0) + 1, 2), WP + 1))
    t = [0] * WP
    amax = -(-tlo // M)
    cols = [j for j in range(ncol) if j != pivj]
    if not only_pivj:
        for j in cols:
            if rng.integers(0, 4):
                a = rnd_mag(rng, int(rng.integers(0, amax.bit_length() + 1))) % (amax + (0 if B == W else 1))
                t[j] = M * (a if rng.integers(0, 2) else -a)
        holder = [j for j in cols if j not in odd_pos]
        hj = holder[int(rng.integers(0, len(holder)))]
        if B == W:
            t[hj] = -tlo
        else:
            extra = rnd_mag(rng, 8) % max(1, (thi - M * amax) // M + 1)
            t[hj] = M * (amax + extra) * (1 if rng.integers(0, 2) else -1)
        for h, j in zip(hs, odd_pos):
            if j == pivj or j == hj or j >= ncol:
                continue
            a = rnd_mag(rng, max(1, (thi // (M // h)).bit_length() - 1)) | 1
            while a % h == 0:
                a += 2
            t[j] = (M // h) * a * (1 if rng.integers(0, 2) else -1)
            if abs(t[j]) > thi:
                t[j] = M // h if (M // h) else 1
    for j, val in (force or {}).items():   # a target given by the caller (a column of `cols`, listed in odd_pos)
        t[j] = val
    # backwards: v, prow
    v, prow = [0] * WP, [0] * WP
    rlim = 1 << br
    inv = pow(foo, -1, lpiv) if (foo and lpiv > 1) else 0
    for j in cols:
        tj = t[j]
        if foo == 0:
            v[j], prow[j] = tj, (rnd_mag(rng, min(br, 20)) - (1 << min(br, 20) >> 1) if rng.integers(0, 2) else 0)
            if abs(v[j]) >= rlim:
                v[j] = t[j] = 0
            continue
        base = (-tj * inv) % lpiv if lpiv > 1 else 0
        ks = [0, -1]
        bal = [(-tj // (2 * foo) - base) // lpiv + d for d in (0, 1, -1)]   # both products carry half of the target
        bal2 = [(-tj // foo - base) // lpiv + d for d in (0, 1, -1)]        # q * foo carries the target
        if heavy:
            ks = bal2 + ks
        elif both or abs(tj) >= lpiv * (rlim >> 1):
            ks = bal + ks + bal2
        elif lpiv == 1 or f["row"] == W:
            ks = [int(rng.integers(-1 << 8, 1 << 8))] + ks + bal
        else:
            ks = ks + bal
        for k in ks:
            q = base + lpiv * k
            x = (tj + q * foo) // lpiv
            if abs(x) < rlim and abs(q) < rlim and abs(x * lpiv) < (1 << (W - 1)) and abs(q * foo) < (1 << (W - 1)):
                v[j], prow[j] = x, q
                break
        else:
            t[j] = 0   # no operands within the path's bounds give this target: a zero entry (0 * lpiv - 0 * foo)
    dmax = min((rlim - 1) // lpiv, (rlim - 1) // max(1, abs(foo)), 1 << 12)
    d = int(rng.integers(1, max(2, dmax + 1))) if dmax >= 1 else 1
    prow[pivj], v[pivj] = lpiv * d, foo * d
    # the row's denominator: g0 = lpiv * den
    glim = (1 << min(f["g0"], W - 1)) - 1
    gM = M if M * lpiv <= glim else 1
    den = {"M": gM * int(one(1, 7)), "one": 1, "minus_one": -1, "neg": -gM * int(rng.integers(1, 7)),
           "min": -(1 << (W - 1)) if f["g0"] == W else -glim, "zero": 0, "equal": gM, "divisor": gfac[0] if gfac and gfac[0] > 1 else 1,
           "multiple": gM * 2 * 3 * 1009, "wide32": (1 << 31) + rnd_mag(rng, 31), "wide33": -((1 << 33) - 1 - rnd_mag(rng, 20)),
           "wide64": (1 << 63) + rnd_mag(rng, 63), "wide65": -((1 << 65) - 1 - rnd_mag(rng, 40))}[g0kind]   # wideN: N bits
    if abs(den * lpiv) > glim + (1 if f["g0"] == W else 0):
        den = 1
    return dict(v=v, prow=prow, den=den, dpiv=dpiv, pivj=pivj, tag="%s B=%d M=%d hs=%s g0=%s" % (tag, B, M, hs, g0kind),
                wantB=None if only_pivj else B)


def random_case(rng, fam, WP, wrap):
    """a seeded random case within the family's preconditions; `wrap`: full-width operands whose products wrap around"""
    f = FAMILY[fam]
    W = f["W"]
    br, bm = min(f["row"], W - 1), min(f["mul"], W - 1)
    ncol = WP if rng.integers(0, 2) else int(rng.integers(2, WP + 1))
    pivj = int(rng.integers(0, ncol))
    if wrap:
        vb, mb = br, bm
    else:
        vb = int(rng.integers(1, br + 1))
        mb = int(rng.integers(1, min(bm, W - 1 - vb) + 1)) if W - 1 - vb >= 1 else 1
        mb = min(mb, W - 2 - vb) if W - 2 - vb >= 1 else 1
    G = [1, 1, 2, 6, 1 << int(rng.integers(0, max(1, vb - 1))), int(rng.integers(1, 1 << min(14, max(1, vb - 1))))][int(rng.integers(0, 6))]
    if G >= (1 << max(1, vb - 1)):
        G = 1
    eb = max(1, vb - G.bit_length())

    def entry():
        x = G * rnd_mag(rng, int(rng.integers(0, eb + 1)))
        return -x if rng.integers(0, 2) else x
    v = [entry() if (j < ncol and rng.integers(0, 5)) else 0 for j in range(WP)]
    prow = [entry() if (j < ncol and rng.integers(0, 5)) else 0 for j in range(WP)]
    lpiv = rnd_mag(rng, mb) | 1
    foo = rnd_mag(rng, mb) * (1 if rng.integers(0, 2) else -1)
    g = math.gcd(lpiv, foo)
    lpiv, foo = lpiv // g, foo // g
    d = int(rng.integers(1, 4))
    if lpiv * d >= (1 << br) or abs(foo * d) >= (1 << br):
        d = 1
    prow[pivj], v[pivj] = lpiv * d, foo * d
    db = min(f["dpiv"], W - 1)
    dpiv = max(1, rnd_mag(rng, int(rng.integers(1, db + 1)) if wrap or f["dpiv"] == W else int(rng.integers(1, min(db, max(1, W - 2 - mb)) + 1))))
    dpiv = dpiv * G if (dpiv * G).bit_length() <= db and not wrap else dpiv
    glim = (1 << min(f["g0"], W - 1)) - 1
    den = max(1, rnd_mag(rng, int(rng.integers(1, max(2, min(f["g0"], W - 1) - lpiv.bit_length())))))
    den = den * G if abs(den * G * lpiv) <= glim else den
    if abs(den * lpiv) > glim:
        den = 1
    if rng.integers(0, 8) == 0:
        den = -den
    return dict(v=v, prow=prow, den=den, dpiv=dpiv, pivj=pivj, tag="random%s" % (" wrap" if wrap else ""), wantB=None)


def row_cases(fam, WP, nrandom=160):
    """The case list of a family at padded width WP: the directed grid first, then seeded random cases.  Deterministic."""
    f = FAMILY[fam]
    W = f["W"]
    rng = CaseRng(1000003 * W + 1009 * WP + sum(map(ord, fam)))
    pos = lane_positions(W, WP)
    cases = []
    k = 0

    def nxt(n=1):
        nonlocal k
        out = [pos[(k + i) % len(pos)] for i in range(n)]
        k += 1
        return out
    gkinds = [("one", lambda B: [1]), ("pow2", lambda B: [1 << int(rng.integers(1, max(2, B - 2)))]), ("pow2max", lambda B: [1 << (B - 1)]),
              ("odd", lambda B: [int(rng.choice([3, 9, 21, 0x10001, 715827883])) % (1 << max(2, B - 3)) | 1]),
              ("mixed", lambda B: [1 << int(rng.integers(1, max(2, B // 2))), int(rng.choice([3, 15, 77, 65537]))]),
              # the starting g at 32 / 33 / 64 / 65 bits: two factors, one for foo and one for dpiv
              ("gbits32", lambda B: [rnd_top(rng, 16) | 1, rnd_top(rng, 16) | 1] if B < W else [1 << 31]),
              ("gbits33", lambda B: [rnd_top(rng, 17) | 1, rnd_top(rng, 16) | 1] if B < W else [1 << 32]),
              ("gbits64", lambda B: [rnd_top(rng, 32) | 1, rnd_top(rng, 32) | 1] if B < W else [1 << 63]),
              ("gbits65", lambda B: [rnd_top(rng, 33) | 1, rnd_top(rng, 32) | 1] if B < W else [1 << 64])]
    for B in f["thresholds"]:
        for gname, gf in gkinds:
            if gname.startswith("gbits") and (int(gname[5:]) >= B or (int(gname[5:]) > 33 and W == 64)):
                continue
            for rounds in (0, 1, 2, 3, 4):
                if rounds > 1 and gname not in ("one", "pow2", "mixed"):
                    continue
                hs = list(PRIMES[:rounds]) if rounds < 4 else [3, 5, 7, 11]
                pj = nxt()[0]
                odd = [j for j in nxt(rounds + 1) if j != pj][:rounds]
                cases.append(build_case(rng, fam, WP, B, gf(B), hs[:len(odd)] if not gname.startswith("gbits") else [], pj, odd,
                                        exact_g=gname.startswith("gbits"), tag="grid %s r%d" % (gname, rounds)))
        # the starting g beyond 32 (64) bits over entries below: foo = 0, so g = |g0| whatever B is
        for g0kind in ("wide32", "wide33") + (("wide64", "wide65") if W == 128 else ()):
            if f["g0"] >= int(g0kind[4:]) + 1 and B <= min(f["row"], W - 1):
                cases.append(build_case(rng, fam, WP, B, [1 << int(rng.integers(0, 3))], [], nxt()[0], [], g0kind=g0kind, foo_zero=True,
                                        tag="grid g0 wide"))
        # a denominator beyond 32 (64) bits over the entries of a full update (small_reduce's second and third branch)
        for g0kind in ("wide33",) + (("wide65",) if W == 128 else ()):
            if f["g0"] >= int(g0kind[4:]) + 1:
                cases.append(build_case(rng, fam, WP, B, [4], [], nxt()[0], [], g0kind=g0kind, tag="grid den wide"))
    # reduce_by_inverse's separation line (B <= W' - 2).  With g = m odd, the entry a = k m - 2^W' is no
    # multiple of m, yet a * m^-1 mod 2^W' = k: at |a| just below 2^(W'-2) k is still told apart by its size, one bit further
    # (B = W' - 1) it is not -- there the width W' must not be taken (TRY32 at 30 bits, the 64-in-128 sub-path at 62, the
    # remainder loop beyond W - 2).  Both sides of each line, both signs.
    for Wq in (32, 64, 128):
        for B in (Wq - 2, Wq - 1):
            if Wq > W or B > max(f["thresholds"]):
                continue
            for mb in (2, 3, 7, 13, 15):
                m = rnd_top(rng, mb) | 1
                for sign in (1, -1):
                    r = rnd_mag(rng, max(1, B - 4 - mb))
                    k = ((1 << Wq) - (1 << (B - 1)) - r) // m
                    a = sign * (k * m - (1 << Wq))
                    pj, j = nxt()[0], nxt()[0]
                    if j == pj:
                        j = nxt()[0]
                    cases.append(build_case(rng, fam, WP, B, [m], [], pj, [j], exact_g=True, force={j: a},
                                            tag="grid false quotient W'=%d" % Wq))
    # g0: 1, -1, negative, MIN, 0 over a non-zero row, equal to / a proper divisor of / a proper multiple of the row gcd
    Bs = [b for b in f["thresholds"] if b <= min(f["row"], W - 1) - 2] or [min(f["row"], W - 1) - 2]
    for g0kind in ("one", "minus_one", "neg", "min", "zero", "equal", "divisor", "multiple"):
        for B in Bs[:4]:
            for gfac in ([6], [1 << 4, 5], [1]):
                cases.append(build_case(rng, fam, WP, B, gfac, [], nxt()[0], [], g0kind=g0kind, tag="g0"))
                cases.append(build_case(rng, fam, WP, B, gfac, [], nxt()[0], [], g0kind=g0kind, foo_zero=True, tag="g0 foo=0"))
    # zero rows: under g0 = 0 (`ok` false), under denominators beyond 32 (64) bits, under a small one
    for g0kind in ("zero", "wide32", "wide33", "wide64", "wide65", "M", "minus_one", "min"):
        if g0kind.startswith("wide") and f["g0"] < int(g0kind[4:]) + 1:
            continue
        c = build_case(rng, fam, WP, 4, [1], [], nxt()[0], [], g0kind=g0kind, foo_zero=True, only_pivj=True, tag="zero row")
        c["v"] = [0] * WP
        cases.append(c)
    # rows in which z[pivj] = dpiv * foo is the only non-zero entry; pivj in column 0, the last column, every chunk and half
    for pj in pos:
        for g0kind in ("M", "neg", "multiple"):
            cases.append(build_case(rng, fam, WP, Bs[0], [12], [], pj, [], g0kind=g0kind, only_pivj=True, tag="only pivj"))
    if f["row"] == W or fam in ("LI_M", "LL_M"):
        # the wrap group: full-width operands; z = MIN through a wrapped product
        for _ in range(48):
            cases.append(random_case(rng, fam, WP, True))
        MIN = -(1 << (W - 1))
        for pj in pos[:3]:
            c = build_case(rng, fam, WP, 20, [4], [], pj, [], g0kind="one", tag="wrap dpiv*foo = MIN")
            lpiv, foo = multipliers(c)
            if foo:   # dpiv * foo == MIN modulo 2^W: dpiv = MIN / 2^k * inverse of foo's odd part
                s = (foo & -foo).bit_length() - 1
                c["dpiv"] = signed((1 << (W - 1 - s)) * pow(foo >> s, -1, 1 << W), W) % (1 << (W - 1)) or 1
                c["wantB"] = None
            cases.append(c)
    for _ in range(nrandom):
        cases.append(random_case(rng, fam, WP, False))
    cases = [c for c in cases if preconditions_hold(c, fam)]
    assert len(cases) <= ROW_CASE_CAP
    return cases


_CASES = {}


def cases_of(fam, WP):
    if (fam, WP) not in _CASES:
        _CASES[(fam, WP)] = row_cases(fam, WP)
    return _CASES[(fam, WP)]


_MODEL = {}


def models_of(fam, WP):
    """computed once per case list, shared by the paths that run it, never changed"""
    if (fam, WP) not in _MODEL:
        W = FAMILY[fam]["W"]
        _MODEL[(fam, WP)] = [row_model(c, W) for c in cases_of(fam, WP)]
    return _MODEL[(fam, WP)]


def row_words(cases, W, WP, with_gpre):
    ew = W // 64
    rows = []
    for c in cases:
        lpiv, foo = multipliers(c)
        g0 = lpiv * c["den"]
        gpre = math.gcd(uabs(g0, W), uabs(c["dpiv"] * foo, W)) if with_gpre else 0
        rows.append([lpiv, foo, c["dpiv"], g0, c["pivj"], gpre] + c["v"] + c["prow"])
    return pack_words(rows, (ew,) * (6 + 2 * WP))


@pytest.mark.parametrize("path", list(PATHS))
def test_row_update(probe, path):
    """One row path on its family's cases, and -- the equivalence ladder -- the same cases through every more general path
    of the width: all of them equal the model, word for word (ok, newden, every z)."""
    _, W, WP, fam, ladder = PATHS[path]
    cases, want = cases_of(fam, WP), models_of(fam, WP)
    ew = W // 64
    wantw = pack_words([[ok, nd] + z for ok, nd, z in want], (ew,) * (2 + WP))
    words = {}
    for p in (path,) + ladder:
        for with_gpre in ((False, True) if p in GPRE_PATHS else (False,)):
            if with_gpre not in words:
                words[with_gpre] = row_words(cases, W, WP, with_gpre)
            got = probe.rows(p, words[with_gpre], len(cases))
            bad = np.nonzero((got != wantw).any(axis=1))[0]
            if bad.size:
                i = int(bad[0])
                c = cases[i]
                g = unpack_words(got[i:i + 1], (ew,) * (2 + WP))[0]
                cols = [j for j in range(WP) if signed(g[2 + j], W) != want[i][2][j]][:4]
                raise AssertionError("%s (cases of %s, gpre %s): %d of %d cases differ; first #%d [%s] lpiv,foo=%s den=%d dpiv=%d pivj=%d: ok %d/%d "
                                     "newden %d/%d columns %s got %s want %s" % (
                                         p, path, with_gpre, bad.size, len(cases), i, c["tag"], multipliers(c), c["den"], c["dpiv"], c["pivj"],
                                         g[0], want[i][0], signed(g[1], W), want[i][1], cols, [signed(g[2 + j], W) for j in cols],
                                         [want[i][2][j] for j in cols]))
