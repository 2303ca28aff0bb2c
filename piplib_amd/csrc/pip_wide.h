// piplib_amd/csrc/pip_wide.h -- the width-generic integer and lane primitives under every kernel family (pivot kernels,
// batch loads, device tree, tab_Matrix2Tableau, tape evaluator) and under the host trees: one spelling per contract,
// overloaded on the width.  The first half is plain integer arithmetic for host and device alike (no HIP include
// needed: tests/wide_main.cpp compiles it with the host compiler under sanitizers); the second half, behind
// __HIPCC__, names lane and wave builtins.  Every comment states the function's domain: which arguments may be 0 and
// what comes back then.
#ifndef PIP_WIDE_H
#define PIP_WIDE_H

// (PIP_WIDE_HD, not pip_job.h's PIP_HD: that one is a bare __host__ __device__ in front of constexpr functions)
#ifdef __HIPCC__
#define PIP_WIDE_HD __host__ __device__ __forceinline__
#define PIP_WIDE_NOINLINE __host__ __device__ __noinline__
#else
#define PIP_WIDE_HD static inline
#define PIP_WIDE_NOINLINE
#endif

typedef long long i64;
typedef unsigned long long u64;
typedef __int128 i128;
typedef unsigned __int128 u128;

// ---------------------------------------------------------------- wrap-around arithmetic (piplib.h:128-169 on the
// reference's `long long`, and its 128-bit twin): total, the result modulo 2^64 / 2^128
PIP_WIDE_HD i64 wneg(i64 a) { return (i64)(0ull - (u64)a); }
PIP_WIDE_HD i64 wadd(i64 a, i64 b) { return (i64)((u64)a + (u64)b); }
PIP_WIDE_HD i64 wsub(i64 a, i64 b) { return (i64)((u64)a - (u64)b); }
PIP_WIDE_HD i64 wmul(i64 a, i64 b) { return (i64)((u64)a * (u64)b); }
PIP_WIDE_HD i128 wneg(i128 a) { return (i128)((u128)0 - (u128)a); }
PIP_WIDE_HD i128 wadd(i128 a, i128 b) { return (i128)((u128)a + (u128)b); }
PIP_WIDE_HD i128 wsub(i128 a, i128 b) { return (i128)((u128)a - (u128)b); }
PIP_WIDE_HD i128 wmul(i128 a, i128 b) { return (i128)((u128)a * (u128)b); }

// magnitude of a signed value, total: the most negative value's is 2^(W-1), which its unsigned twin holds; 0 for 0
PIP_WIDE_HD unsigned uabs(int x) { return x < 0 ? 0u - (unsigned)x : (unsigned)x; }
PIP_WIDE_HD u64 uabs(i64 x) { return x < 0 ? 0ull - (u64)x : (u64)x; }
PIP_WIDE_HD u128 uabs(i128 x) { return x < 0 ? (u128)0 - (u128)x : (u128)x; }

// the value is one a long long holds (total)
PIP_WIDE_HD bool fits64(i128 x) { return (i128)(i64)x == x; }

// bit length: the position of the highest set bit plus one; DEFINED at 0, where it is 0 (the builtin alone is not: it
// is only reached under the test for zero)
PIP_WIDE_HD int bitlen(unsigned x) { return x ? 32 - __builtin_clz(x) : 0; }
PIP_WIDE_HD int bitlen(u64 x) { return x ? 64 - __builtin_clzll(x) : 0; }
PIP_WIDE_HD int bitlen(u128 x) {
  const u64 hi = (u64)(x >> 64);
  return hi ? 128 - __builtin_clzll(hi) : bitlen((u64)x);
}

// count of trailing zeros, x != 0.  NOT defined at 0 (the builtin's result is undefined there, and the 128-bit form
// hands it the high word whenever the low one is 0): every caller keeps 0 out.  In the pivot kernels gcd_mag answers a
// zero operand before its first shift and its loop ends when b is 0; cquo answers b == 0 first; exact_quo's and
// reduce_by_inverse's argument is a gcd >= 1.  The device tree sets the top bit of a lane's idle divisor (QK::pivot_step).
// (The spelling that ORs the top bit in here, total, was not taken: every 128-bit pivot kernel comes out 117 to 175
// instructions longer with it)
PIP_WIDE_HD int ctz(unsigned x) { return __builtin_ctz(x); }
PIP_WIDE_HD int ctz(u64 x) { return __builtin_ctzll(x); }
PIP_WIDE_HD int ctz(u128 x) {
  const u64 lo = (u64)x;
  return lo ? __builtin_ctzll(lo) : 64 + __builtin_ctzll((u64)(x >> 64));
}

// a 64 / 128-bit value as the nearest double (total; a long long converts natively)
PIP_WIDE_HD double to_double(i64 x) { return (double)x; }
PIP_WIDE_HD double to_double(i128 x) {
  const u128 m = uabs(x);  // via the magnitude: hi*2^64 + lo on a negative value would cancel
  const double d = (double)(u64)(m >> 64) * 18446744073709551616.0 + (double)(u64)m;
  return x < 0 ? -d : d;
}

// inverse of an ODD number modulo 2^32 / 2^64 / 2^128 (Newton: every step doubles the correct low bits), for exact
// division.  Total as arithmetic, but the result is an inverse only for odd m (an even m, 0 included, has none)
PIP_WIDE_HD unsigned inv_odd(unsigned m) {
  unsigned x = (3u * m) ^ 2u;  // 5 correct bits
  x *= 2u - m * x;
  x *= 2u - m * x;
  x *= 2u - m * x;
  return x;
}
PIP_WIDE_HD u64 inv_odd(u64 m) {
  u64 x = m;  // 3 correct bits
  x *= 2 - m * x;
  x *= 2 - m * x;
  x *= 2 - m * x;
  x *= 2 - m * x;
  x *= 2 - m * x;
  return x;
}
PIP_WIDE_HD u128 inv_odd(u128 m) {
  // the inverse modulo 2^64 on 64-bit registers, one 128-bit step on top: a 128-bit multiplication is ten 32-bit
  // multiply-adds, a 64-bit one three
  u128 x = (u128)inv_odd((u64)m);
  x *= 2 - m * x;
  return x;
}

// x86 cvttsd2si: what the reference's (int)t yields for tab_sort_rows' key (traiter.c:583) -- total: a NaN and every
// t whose truncation no int holds give INT_MIN
PIP_WIDE_HD int trunc_x86(double t) { return (!(t > -2147483649.0 && t < 2147483648.0)) ? (int)0x80000000 : (int)t; }

// a / b and a % b, 128 by 128 bits, by shift and subtract over the difference of the bit lengths.  b == 0 gives q = 0,
// r = a.  One copy a translation unit, out of line (its callers are off the pivot path), values in registers both ways.
// NATIVE64: operands that both fit 64 bits divide natively in here -- b != 0 then (the tape evaluator, whose divisors
// are positive); without it the caller has taken those (the device tree's qudiv / qumod, which go on to 32 bits).
struct PipDivMod {
  u128 q, r;
};
template <bool NATIVE64>
PIP_WIDE_NOINLINE PipDivMod udivmod(u128 a, u128 b) {
  PipDivMod o;
  if (NATIVE64 && ((a | b) >> 64) == 0) {
    const u64 q = (u64)a / (u64)b;
    o.q = q;
    o.r = (u64)a - q * (u64)b;
    return o;
  }
  u128 q = 0;
  if (b != 0 && a >= b) {
    int sh = bitlen(a) - bitlen(b);
    u128 d = b << sh;
    for (; sh >= 0; sh--) {
      q <<= 1;
      if (a >= d) {
        a -= d;
        q |= 1;
      }
      d >>= 1;
    }
  }
  o.q = q;
  o.r = a;
  return o;
}

#ifdef __HIPCC__
// ---------------------------------------------------------------- lanes and waves (wave64)
// the value lane `src` holds, src wave-uniform and in 0..63: through the scalar unit, the result is wave-uniform
__device__ __forceinline__ int readlane(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ i64 readlane(i64 v, int src) {
  unsigned lo = __builtin_amdgcn_readlane((unsigned)(u64)v, src);
  unsigned hi = __builtin_amdgcn_readlane((unsigned)((u64)v >> 32), src);
  return (i64)(((u64)hi << 32) | lo);
}
__device__ __forceinline__ i128 readlane(i128 v, int src) {
  u64 lo = (u64)readlane((i64)(u64)(u128)v, src), hi = (u64)readlane((i64)(u64)((u128)v >> 64), src);
  return (i128)(((u128)hi << 64) | lo);
}
// wave-uniform values: pin them to scalar registers so that the gcd / division / inverse
// chains that follow run on the scalar unit instead of occupying all 64 vector lanes
__device__ __forceinline__ i64 uni(i64 v) {
  unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(u64)v);
  unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((u64)v >> 32));
  return (i64)(((u64)hi << 32) | lo);
}
__device__ __forceinline__ i128 uni(i128 v) {
  u64 lo = (u64)uni((i64)(u64)(u128)v), hi = (u64)uni((i64)(u64)((u128)v >> 64));
  return (i128)(((u128)hi << 64) | lo);
}
// the value lane `src` holds, src per lane (its low six bits count); a lane that is not active yields garbage
__device__ __forceinline__ int shfl(int v, int src) { return __shfl(v, src); }
__device__ __forceinline__ i64 shfl(i64 v, int src) { return __shfl(v, src); }
__device__ __forceinline__ i128 shfl(i128 v, int src) {
  const u64 lo = (u64)shfl((i64)(u64)(u128)v, src), hi = (u64)shfl((i64)(u64)((u128)v >> 64), src);
  return (i128)(((u128)hi << 64) | lo);
}
// sum (wrap-around), minimum and maximum over the wave's 64 lanes by a butterfly of xor-shuffles: all lanes active,
// every lane gets the result, in a vector register (a caller that wants it scalar pins it)
__device__ __forceinline__ int shfl_xor(int v, int o) { return __shfl_xor(v, o); }
__device__ __forceinline__ i64 shfl_xor(i64 v, int o) { return __shfl_xor(v, o); }
__device__ __forceinline__ i128 shfl_xor(i128 v, int o) {
  const u64 lo = (u64)shfl_xor((i64)(u64)(u128)v, o), hi = (u64)shfl_xor((i64)(u64)((u128)v >> 64), o);
  return (i128)(((u128)hi << 64) | lo);
}
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
  for (int o = 32; o; o >>= 1) v = wadd(v, shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_min(int x) {
  for (int o = 32; o; o >>= 1) {
    const int y = shfl_xor(x, o);
    x = y < x ? y : x;
  }
  return x;
}
__device__ __forceinline__ int wave_max(int x) {
  for (int o = 32; o; o >>= 1) {
    const int y = shfl_xor(x, o);
    x = x > y ? x : y;
  }
  return x;
}
#endif  // __HIPCC__
#endif  // PIP_WIDE_H
