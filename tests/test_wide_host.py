"""The host half of piplib_amd/csrc/pip_wide.h -- the width-generic integer primitives every kernel family compiles -- on
the CPU against Python ints: tests/wide_main.cpp includes that header alone, is built with the host compiler under the
address and undefined-behaviour sanitizers and run as a child process.

The operands are the scalar case lists tests/test_gpu_arith_probe.py builds for the GPU probes (same functions, same
seeds), so the text is held to the same cases where a sanitizer may run; where those lists leave out a width edge of a
function that moved into the header (the 32-bit forms, ctz of 64 bits, the division with a zero divisor, to_double, the
truncation) the edges are added here: 0 and 1 where in the domain, 2^31 +- 1, 2^32, 2^63 +- 1, 2^64, 2^127 - 1, -2^127
and their neighbours -- edges() holds 2^k and 2^k +- 1 for every k, which test_lists_hold_the_width_edges asserts.

Domains (pip_wide.h states them; a sanitizer would flag a case outside one): ctz takes no 0; the inverses take odd
numbers; the division with the native 64-bit path inside takes no zero divisor, the one without answers q = 0, r = a."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import test_gpu_arith_probe as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M128 = (1 << 128) - 1
INT_MIN = -(1 << 31)


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("wide") / "wide")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "wide_main.cpp"), "-o", exe],
                   check=True, timeout=300)

    def run(fn, rows, want):
        """rows: operand tuples (ints of any sign, taken modulo 2^128); want: result tuples -> every word equal"""
        text = "".join("%s %s\n" % (fn, " ".join("%x %x" % (x & P.M64, (x & M128) >> 64) for x in r)) for r in rows)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (fn, r.returncode, r.stderr[-2000:])
        got = []
        for ln in r.stdout.splitlines():
            w = [int(x, 16) for x in ln.split()]
            got.append(tuple(w[k] | (w[k + 1] << 64) for k in range(0, len(w), 2)))
        assert len(got) == len(rows) == len(want), (fn, len(got), len(rows))
        bad = [(rows[i], got[i], want[i]) for i in range(len(rows)) if got[i] != tuple(x & M128 for x in want[i])]
        assert not bad, "%s: %d of %d cases differ, first: in %s got %s want %s" % (
            fn, len(bad), len(rows), [hex(x) for x in bad[0][0]], [hex(x) for x in bad[0][1]], [hex(x) for x in bad[0][2]])
    return run


def bit_count_lists():
    """the operand lists of test_gpu_arith_probe.test_bit_counts, drawn in its order from its seed"""
    rng = np.random.default_rng(110)
    uv = {}
    for W in (64, 128):
        P.rand_bits(rng, W, True, 500)     # (its signed list, for log2_64 and QK::blen: not in the header)
        uv[W] = P.edges(W, False) + P.rand_bits(rng, W, False, 500)
    cz = [x for x in P.edges(128, False) + P.rand_bits(rng, 128, False, 500) + [1 << 64, 3 << 64, 1 << 127, 5 << 63] if x]
    sv = P.edges(128, True) + P.rand_bits(rng, 128, True, 500) + [-(1 << 63) - 1, -(1 << 63), (1 << 63) - 1, 1 << 63]
    return uv, cz, sv


def test_lists_hold_the_width_edges():
    for W, vals in ((32, P.edges(32, False)), (64, P.edges(64, False)), (128, P.edges(128, False))):
        need = {0, 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 1}
        if W >= 64:
            need |= {1 << 32, (1 << 32) + 1, (1 << 63) - 1, (1 << 63) + 1, 1 << 63, (1 << 64) - 1}
        if W == 128:
            need |= {1 << 64, (1 << 64) - 1, (1 << 64) + 1, (1 << 127) - 1, 1 << 127, (1 << 127) + 1, M128}
        assert need <= set(vals), (W, need - set(vals))
    sv = set(P.edges(128, True))
    assert {0, 1, -1, (1 << 63) - 1, 1 << 63, -(1 << 63), -(1 << 63) - 1, 1 << 64, -(1 << 64), (1 << 127) - 1, -(1 << 127),
            -(1 << 127) + 1} <= sv


def test_bit_counts(wide):
    """bitlen (0 at 0), ctz (no 0), fits64, uabs (|MIN| = 2^(W-1)) in every width"""
    uv, cz, sv = bit_count_lists()
    uv[32] = P.edges(32, False) + P.rand_bits(np.random.default_rng(111), 32, False, 200)
    for W in (32, 64, 128):
        assert 0 in uv[W]
        wide("bitlen%d" % W, [(x,) for x in uv[W]], [(x.bit_length(),) for x in uv[W]])
        nz = [x for x in uv[W] if x] if W < 128 else cz
        assert 0 not in nz and 1 in nz and 1 << (W - 1) in nz
        wide("ctz%d" % W, [(x,) for x in nz], [((x & -x).bit_length() - 1,) for x in nz])
        s = [P.signed(x, W) for x in uv[W]]
        assert -(1 << (W - 1)) in s and -1 in s
        wide("uabs%d" % W, [(x,) for x in s], [(abs(x),) for x in s])
    wide("fits64", [(x,) for x in sv], [(1 if P.fits(x, 64) else 0,) for x in sv])


def test_inverses(wide):
    """m * inv_odd(m) == 1 modulo 2^W for every odd m: the pivot kernels' lists and the device tree's"""
    for W in (32, 64, 128):
        ms = P.odd_cases(W, 20 + W) + (P.odd_cases(W, 30 + W) if W > 32 else [])
        assert 1 in ms and (1 << W) - 1 in ms and (1 << (W - 1)) + 1 in ms
        wide("inv%d" % W, [(m,) for m in ms], [(pow(m, -1, 1 << W),) for m in ms])


def test_division(wide):
    """udivmod against // and %: the device tree's qudiv / qumod pairs and umod128's (either instantiation), 64-bit pairs
    through the native path, and a zero divisor through the one that is defined there"""
    ps = P.pair_cases(128, False, 70 + 128) + P.pair_cases(128, False, 81)
    zero = [(a, 0) for a in P.edges(128, False)]
    nz = [(a, b) for a, b in ps if b]
    assert any(b == 0 for _, b in ps) and any(a >> 64 and b >> 64 for a, b in nz) and any(a >> 64 and not b >> 64 for a, b in nz)
    assert ((1 << 128) - 1, 1) in nz and ((1 << 128) - 1, (1 << 128) - 1) in nz and (1 << 127, (1 << 64) + 1) in nz
    wide("divmod_wide", nz + zero, [(a // b, a % b) for a, b in nz] + [(0, a) for a, _ in zero])
    n64 = [(a, b) for a, b in P.pair_cases(64, False, 70 + 64) if b]
    wide("divmod_native", nz + n64, [(a // b, a % b) for a, b in nz + n64])


def double_bits(d):
    return struct.unpack("<Q", struct.pack("<d", d))[0]


def to_double_model(x):
    """the header's formula, operation for operation, on IEEE doubles: float(int) rounds to nearest even as the C
    conversion of a 64-bit word does; times 2^64 is exact"""
    m = abs(x)
    d = float(m >> 64) * 18446744073709551616.0 + float(m & P.M64)
    return -d if x < 0 else d


def test_to_double(wide):
    """to_double: bit for bit the magnitude's hi * 2^64 + lo with the sign put back (so -x gives -to_double(x): the form
    that adds signed halves cancels on negatives); exact below 2^53; within 2^-52 of the true value everywhere -- three
    roundings (either half, the sum) of at most 2^-53 each, the halves' two never both inexact by more than the sum's ulp"""
    rng = np.random.default_rng(120)
    v128 = P.edges(128, True) + P.rand_bits(rng, 128, True, 2000)
    v64 = P.edges(64, True) + P.rand_bits(rng, 64, True, 500)
    for x in v128:
        d = to_double_model(x)
        assert to_double_model(-x) == -d or x == -(1 << 127)
        assert abs(int(d) - x) * (1 << 52) <= abs(x)
        if abs(x) < (1 << 53):
            assert int(d) == x
    wide("todouble128", [(x,) for x in v128], [(double_bits(to_double_model(x)),) for x in v128])
    wide("todouble64", [(x,) for x in v64], [(double_bits(float(x)),) for x in v64])


def trunc_model(t):
    """x86 cvttsd2si: math.trunc, and INT_MIN for a NaN, an infinity and every value whose truncation no int holds"""
    if math.isnan(t) or math.isinf(t):
        return INT_MIN
    q = math.trunc(t)
    return q if INT_MIN <= q < (1 << 31) else INT_MIN


def test_trunc_x86(wide):
    """the sort key's conversion at the edges of int, and on quotients to_double(a) / to_double(d) as tab_sort_rows forms them"""
    rng = np.random.default_rng(121)
    ts = [0.0, -0.0, 0.5, -0.5, 0.9999999999999999, 1.0, -1.0, 1.5, -1.5, 2147483646.5, 2147483647.0, 2147483647.5,
          2147483647.9999995, 2147483648.0, 2147483648.5, 4294967296.0, -2147483647.5, -2147483648.0, -2147483648.5,
          -2147483648.9999995, -2147483649.0, -2147483649.5, -4294967296.0, 9.3e18, -9.3e18, 1.8e19, 1e300, -1e300, 5e-324,
          float("inf"), float("-inf"), float("nan")]
    for a in P.key_edges(128, True) + P.rand_bits(rng, 128, True, 300):
        for d in (1, 3, 7, (1 << 31) - 1, 1 << 32, (1 << 63) + 1, (1 << 96) - 1):
            ts.append(to_double_model(a) / to_double_model(d))
    assert any(trunc_model(t) == (1 << 31) - 1 for t in ts) and any(0 < trunc_model(t) < 1000 for t in ts)
    wide("trunc", [(double_bits(t),) for t in ts], [(trunc_model(t),) for t in ts])


def test_wrap_around(wide):
    """wneg / wadd / wsub / wmul: the result modulo 2^W, MIN and MAX included (no signed overflow for the sanitizer to find)"""
    for W in (64, 128):
        ps = P.pair_cases(W, True, 130 + W, nrand=300)
        assert (-(1 << (W - 1)), -1) in ps and (-(1 << (W - 1)), -(1 << (W - 1))) in ps
        wide("wneg%d" % W, [(a,) for a, _ in ps], [(P.mask(-a, W),) for a, _ in ps])
        wide("wadd%d" % W, ps, [(P.mask(a + b, W),) for a, b in ps])
        wide("wsub%d" % W, ps, [(P.mask(a - b, W),) for a, b in ps])
        wide("wmul%d" % W, ps, [(P.mask(a * b, W),) for a, b in ps])
