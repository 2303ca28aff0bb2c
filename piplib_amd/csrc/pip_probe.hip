// piplib_amd/csrc/pip_probe.hip -- testing aid: the device functions of the pivot kernels (pip_advance.h, the row flavours
// of pip_lean.h) and of the device tree (pip_quast.hip) run on operands the caller gives, so that a test holds each of
// them to exact integers at the magnitudes where they change code path (tests/test_gpu_arith_probe.py).  The probe
// kernels CALL the shipped functions; nothing here restates them, and no shipped kernel calls anything here.
//
//   pipamd_debug_arith(engine, op, in, out, n)            one case per lane, n cases
//   pipamd_debug_row_update(engine, path, in, out, ncases) one wave per case (the row functions ballot and readlane)
// and the lean kernel's per-lane preparation and its reductions from a given gcd (tests/test_gpu_lean_prep_probe.py):
// pipamd_debug_arith op 128, pipamd_debug_row_update paths 32 ... 35.
//
// `in` / `out`: device pointers to int64 words, 16-byte aligned; a 128-bit value is two words, low then high (as
// det_limb).  Exported, not declared in include/piplib_amd.h (like pipamd_debug_lean): no part of the interface.
#include "pip_lean.h"
#include "pip_host.h"
#include "../../include/piplib_amd.h"

// the device tree's helpers live in pip_quast.hip's anonymous namespace: its own probe kernel, launched from here
extern "C" hipError_t pipk_launch_quast_probe(int op, const long long *in, long long *out, int n, hipStream_t stream);

namespace {

// ---- pipamd_debug_arith: words per case in and out of every op (tests/test_gpu_arith_probe.py holds the same table)
enum {
  P_GCD_U32, P_GCD_U64, P_GCD_MAG64, P_GCD_MAG128, P_GCD_I64, P_GCD_I128, P_INV64, P_INV128, P_INVW32,
  P_CQUO64, P_CQUO128, P_CREM64, P_CREM128, P_FMOD64, P_FMOD128, P_XQUO64, P_XQUO128,
  P_UMOD128, P_UMOD128_32, P_UMODS64, P_UMODS128, P_UMOD_TINY, P_UMOD_TINY_LOW, P_ROWMOD_INT, P_ROWMOD_LONG,
  P_LOG2_64, P_LOG2_128, P_BITLEN64, P_BITLEN128, P_CTZ128, P_FITS64, P_BEZOUT64, P_BEZOUT128, P_DET64, P_DET128,
  P_NOPS,
  P_QUAST0 = 64, P_QUAST_NOPS = 26,  // device tree: 64 + 2 * function + (128-bit ? 1 : 0); 3 values in, value + bad out
  P_LEAN_PREP = 128  // lean_prepare_rows<LeanIntRows>, 64 rows a wave: pivot, dpiv, psmall (those of the wave's first case hold
                     // for the wave), foo, den, rcls in; lp, foo', g0, starting gcd, small-path predicate out
};
struct ProbeIO {
  int nin, nout;
};
__host__ __device__ inline ProbeIO probe_io(int op) {
  constexpr ProbeIO io[P_NOPS] = {{2, 1}, {2, 1}, {2, 1}, {4, 2}, {2, 1}, {4, 2}, {1, 1}, {2, 2}, {1, 1},
                                  {2, 1}, {4, 2}, {2, 1}, {4, 2}, {2, 1}, {4, 2}, {2, 1}, {4, 2},
                                  {4, 2}, {3, 1}, {3, 1}, {5, 2}, {2, 1}, {2, 1}, {4, 2}, {5, 4},
                                  {1, 1}, {2, 1}, {1, 1}, {2, 1}, {2, 1}, {2, 1}, {3, 1}, {6, 2}, {7, 6}, {13, 10}};
  return io[op];
}

__device__ __forceinline__ i128 ld2(const i64 *p) { return (i128)(((u128)(u64)p[1] << 64) | (u64)p[0]); }
__device__ __forceinline__ void st2(i64 *p, i128 x) {
  p[0] = (i64)(u64)(u128)x;
  p[1] = (i64)(u64)((u128)x >> 64);
}

__global__ __launch_bounds__(64) void pip_probe_arith_kernel(int op, const i64 *in, i64 *out, long long n) {
  const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
  if (t >= n) return;
  const ProbeIO io = probe_io(op);
  const i64 *a = in + t * io.nin;
  i64 *o = out + t * io.nout;
  switch (op) {
    case P_GCD_U32: o[0] = (i64)gcd_u32((unsigned)a[0], (unsigned)a[1]); break;
    case P_GCD_U64: o[0] = (i64)gcd_u64((u64)a[0], (u64)a[1]); break;
    case P_GCD_MAG64: o[0] = (i64)gcd_mag((u64)a[0], (u64)a[1]); break;
    case P_GCD_MAG128: st2(o, (i128)gcd_mag((u128)ld2(a), (u128)ld2(a + 2))); break;
    case P_GCD_I64: o[0] = gcd_i64(a[0], a[1]); break;
    case P_GCD_I128: st2(o, gcd_i64(ld2(a), ld2(a + 2))); break;
    case P_INV64: o[0] = (i64)inv_odd64((u64)a[0]); break;
    case P_INV128: st2(o, (i128)inv_odd64((u128)ld2(a))); break;
    case P_INVW32: o[0] = (i64)invW((unsigned)a[0]); break;
    case P_CQUO64: o[0] = cquo(a[0], a[1]); break;
    case P_CQUO128: st2(o, cquo(ld2(a), ld2(a + 2))); break;
    case P_CREM64: o[0] = crem(a[0], a[1]); break;
    case P_CREM128: st2(o, crem(ld2(a), ld2(a + 2))); break;
    case P_FMOD64: o[0] = fmod64(a[0], a[1]); break;
    case P_FMOD128: st2(o, fmod64(ld2(a), ld2(a + 2))); break;
    case P_XQUO64: o[0] = exact_quo<i64>(a[0], a[1]); break;
    case P_XQUO128: st2(o, exact_quo<i128>(ld2(a), ld2(a + 2))); break;
    case P_UMOD128: st2(o, (i128)umod128((u128)ld2(a), (u128)ld2(a + 2))); break;
    case P_UMOD128_32: o[0] = (i64)umod128_32((u128)ld2(a), (unsigned)a[2]); break;
    case P_UMODS64: o[0] = (i64)umod_small((u64)a[0], (u64)a[1], a[2] != 0); break;
    case P_UMODS128: st2(o, (i128)umod_small((u128)ld2(a), (u128)ld2(a + 2), a[4] != 0)); break;
    case P_UMOD_TINY: o[0] = (i64)umod_tiny((unsigned)a[0], (unsigned)a[1], __builtin_amdgcn_rcpf((float)(unsigned)a[1])); break;
    case P_UMOD_TINY_LOW: o[0] = (i64)umod_tiny_low((unsigned)a[0], (unsigned)a[1], rcp_low((unsigned)a[1])); break;
    case P_ROWMOD_INT: {
      LeanIntRows::Row r;
      r.v[0] = (int)a[0];
      r.v[1] = (int)a[1];
      LeanIntRows::row_mod(r, (int)a[2], a[3] != 0);
      o[0] = r.v[0];
      o[1] = r.v[1];
      break;
    }
    case P_ROWMOD_LONG: {
      LeanLongRows::Row r;
      for (int c = 0; c < 4; c++) r.v[c] = a[c];
      LeanLongRows::row_mod(r, a[4], false);
      for (int c = 0; c < 4; c++) o[c] = r.v[c];
      break;
    }
    case P_LOG2_64: o[0] = log2_64(a[0]); break;
    case P_LOG2_128: o[0] = log2_64(ld2(a)); break;
    case P_BITLEN64: o[0] = bitlen64((u64)a[0]); break;
    case P_BITLEN128: o[0] = bitlen64((u128)ld2(a)); break;
    case P_CTZ128: o[0] = ctz128((u128)ld2(a)); break;
    case P_FITS64: o[0] = fits64(ld2(a)) ? 1 : 0; break;
    case P_BEZOUT64: o[0] = bezout_dev<i64>(a[0], a[1], a[2]); break;
    case P_BEZOUT128: st2(o, bezout_dev<i128>(ld2(a), ld2(a + 2), ld2(a + 4))); break;
    case P_DET64: {
      i64 d0 = a[0], d1 = a[1], d2 = a[2], d3 = a[3];
      int ldet = (int)a[4];
      const bool ok = det_step<i64>(d0, d1, d2, d3, ldet, a[5], a[6]);
      o[0] = d0, o[1] = d1, o[2] = d2, o[3] = d3, o[4] = ldet, o[5] = ok ? 1 : 0;
      break;
    }
    case P_DET128: {
      i128 d0 = ld2(a), d1 = ld2(a + 2), d2 = ld2(a + 4), d3 = ld2(a + 6);
      int ldet = (int)a[8];
      const bool ok = det_step<i128>(d0, d1, d2, d3, ldet, ld2(a + 9), ld2(a + 11));
      st2(o, d0), st2(o + 2, d1), st2(o + 4, d2), st2(o + 6, d3);
      o[8] = ldet, o[9] = ok ? 1 : 0;
      break;
    }
    default: break;
  }
}

__global__ __launch_bounds__(64) void pip_probe_lean_prep_kernel(const i64 *in, i64 *out, long long n) {
  typedef LeanIntRows F;
  __shared__ i64 den[64];
  __shared__ u8 rcls[64];
  const int lane = threadIdx.x;
  const long long t0 = (long long)blockIdx.x * 64, t = t0 + lane;
  const bool active = t < n;
  const i64 *a = in + (active ? t : t0) * 6;
  Shared<i64> S = {};
  S.den = den;
  S.rcls = rcls;
  den[lane] = a[4];
  rcls[lane] = (u8)a[5];
  __syncthreads();
  const int pivot = __builtin_amdgcn_readfirstlane((int)a[0]);
  const i64 dpiv = uni64(a[1]);
  const bool psmall = __builtin_amdgcn_readfirstlane((int)(a[2] != 0)) != 0;
  int m_lp, m_foo;
  i64 m_g0;
  F::G m_gs;
  const u64 small = lean_prepare_rows<F>(S, lane, active, (int)a[3], pivot, dpiv, psmall, m_lp, m_foo, m_g0, m_gs);
  if (active) {
    i64 *o = out + t * 5;
    o[0] = m_lp, o[1] = m_foo, o[2] = m_g0, o[3] = (i64)m_gs, o[4] = (i64)((small >> lane) & 1);
  }
}

// ---- pipamd_debug_row_update: one wave per case.  Values of a case are of the path's Entier T (one word, or two for the
// 128-bit paths): in  lpiv, foo, dpiv, g0, pivj, gpre, p[WP], q[WP];  out  ok, newden, z[WP].
enum {
  R_G64_1, R_G64_2, R_G64_4, R_G64R, R_S64, R_G128_1, R_G128_4, R_N128_1, R_N128_4, R_NN128_1, R_NN128_4,
  R_LI_S, R_LI_M, R_LL_S, R_LL_M, R_NPATHS,
  R_GS0 = 32, R_LI_S_GS = R_GS0, R_LI_M_GS, R_LL_S_GS, R_LL_M_GS, R_GS_END  // the lean flavours with `gpre` as the starting gcd gs
};
template <class T>
__device__ __forceinline__ T ldv(const i64 *p, size_t k) {
  if constexpr (sizeof(T) == 16)
    return ld2(p + 2 * k);
  else
    return p[k];
}
template <class T>
__device__ __forceinline__ void stv(i64 *p, size_t k, T x) {
  if constexpr (sizeof(T) == 16)
    st2(p + 2 * k, x);
  else
    p[k] = x;
}

// MODE 0: update_row<T, NCH, LEANREG>; 1: the same with narrow64; 2: update_row_narrow<NCH>; 3: update_row_small<1>
template <class T, int NCH, int MODE, bool LEANREG>
__global__ __launch_bounds__(64) void pip_probe_row_kernel(const i64 *in, i64 *out, int ncases) {
  constexpr int WP = NCH * 64 * ET<T>::CPL, EW = ET<T>::EW;
  const int cs = blockIdx.x, lane = threadIdx.x;
  if (cs >= ncases) return;
  const i64 *ci = in + (size_t)cs * EW * (6 + 2 * WP);
  i64 *co = out + (size_t)cs * EW * (2 + WP);
  const T lpiv = ldv<T>(ci, 0), foo = ldv<T>(ci, 1), dpiv = ldv<T>(ci, 2), g0 = ldv<T>(ci, 3);
  const int pivj = (int)ci[EW * 4];
  const typename ET<T>::U gpre = (typename ET<T>::U)ldv<T>(ci, 5);
  const T *p = reinterpret_cast<const T *>(ci + EW * 6), *q = p + WP;
  T *z = reinterpret_cast<T *>(co + EW * 2);
  RowRegs<T, NCH> r;
  row_load<T, NCH>(r, p, WP, lane);
  T nd = 0;
  bool ok;
  if constexpr (MODE == 3) {
    RowRegs32<NCH> o32;
    ok = update_row_small<NCH>(r, o32, q, pivj, (int)lpiv, (int)foo, (int)dpiv, g0, lane, nd);
    row_store32<NCH>(o32, z, WP, lane);
  } else {
    if constexpr (MODE == 2)
      ok = update_row_narrow<NCH>(r, q, pivj, (i64)lpiv, (i64)foo, (i64)dpiv, (i64)g0, lane, nd, (u64)gpre);
    else
      ok = update_row<T, NCH, LEANREG>(r, q, pivj, lpiv, foo, dpiv, g0, lane, nd, gpre, MODE == 1);
    row_store<T, NCH>(r, z, WP, lane);
  }
  if (lane == 0) {
    stv<T>(co, 0, (T)(ok ? 1 : 0));
    stv<T>(co, 1, nd);
  }
}

// the lean flavours: the probe packs the rows (int / long long) as the lean kernels hold them
template <class F, bool SMALL, bool GS = false>
__global__ __launch_bounds__(64) void pip_probe_lean_kernel(const i64 *in, i64 *out, int ncases) {
  typedef typename F::T T;
  typedef typename F::E E;
  constexpr int WP = F::WP, EW = ET<T>::EW;
  const int cs = blockIdx.x, lane = threadIdx.x;
  if (cs >= ncases) return;
  const i64 *ci = in + (size_t)cs * EW * (6 + 2 * WP);
  i64 *co = out + (size_t)cs * EW * (2 + WP);
  const T lpiv = ldv<T>(ci, 0), foo = ldv<T>(ci, 1), dpiv = ldv<T>(ci, 2), g0 = ldv<T>(ci, 3);
  const int pivj = (int)ci[EW * 4];
  const typename ET<T>::U gs = GS ? (typename ET<T>::U)ldv<T>(ci, 5) : 0;
  typename F::Row r, pr;
#pragma unroll
  for (int h = 0; h < F::NV; h++) {
    r.v[h] = (E)ldv<T>(ci, 6 + F::col(lane, h));
    pr.v[h] = (E)ldv<T>(ci, 6 + WP + F::col(lane, h));
  }
  T nd = 0;
  bool ok;
  if constexpr (SMALL) {
    ok = F::update_small(r, pr, (E)lpiv, (E)foo, dpiv, pivj, g0, gs, lane, nd);
#pragma unroll
    for (int h = 0; h < F::NV; h++) stv<T>(co, 2 + F::col(lane, h), (T)r.v[h]);
  } else {
    T zw[F::NV];
    ok = F::update_mid(zw, r, pr, (E)lpiv, (E)foo, dpiv, pivj, g0, gs, lane, nd);
#pragma unroll
    for (int h = 0; h < F::NV; h++) stv<T>(co, 2 + F::col(lane, h), zw[h]);
  }
  if (lane == 0) {
    stv<T>(co, 0, (T)(ok ? 1 : 0));
    stv<T>(co, 1, nd);
  }
}

bool probe_ptrs_ok(const void *in, const void *out) {
  return in && out && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0;
}
int probe_finish(hipError_t e) {
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    pipamd_set_error("arithmetic probe: %s", hipGetErrorString(e));
    return PIPAMD_E_HIP;
  }
  return PIPAMD_OK;
}

}  // namespace

extern "C" int pipamd_debug_arith(pipamd_engine *e, int op, const long long *in, long long *out, long long n) {
  const bool quast = op >= P_QUAST0 && op < P_QUAST0 + P_QUAST_NOPS;
  if (!e || n < 0 || n > (1ll << 30) || !probe_ptrs_ok(in, out) || !(quast || op == P_LEAN_PREP || (op >= 0 && op < P_NOPS)))
    return PIPAMD_E_INVALID;
  if (hipSetDevice(e->device) != hipSuccess) return PIPAMD_E_HIP;
  if (n == 0) return PIPAMD_OK;
  if (quast) return probe_finish(pipk_launch_quast_probe(op - P_QUAST0, in, out, (int)n, 0));
  if (op == P_LEAN_PREP) {
    hipLaunchKernelGGL(pip_probe_lean_prep_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, in, out, n);
    return probe_finish(hipGetLastError());
  }
  hipLaunchKernelGGL(pip_probe_arith_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, op, in, out, n);
  return probe_finish(hipGetLastError());
}

extern "C" int pipamd_debug_row_update(pipamd_engine *e, int path, const long long *in, long long *out, int ncases) {
  if (!e || ncases < 0 || !probe_ptrs_ok(in, out) || path < 0 || (path >= R_NPATHS && !(path >= R_GS0 && path < R_GS_END)))
    return PIPAMD_E_INVALID;
  if (hipSetDevice(e->device) != hipSuccess) return PIPAMD_E_HIP;
  if (ncases == 0) return PIPAMD_OK;
#define PIP_PROBE_ROW(...) hipLaunchKernelGGL((__VA_ARGS__), dim3(ncases), dim3(64), 0, 0, in, out, ncases)
  switch (path) {
    case R_G64_1: PIP_PROBE_ROW(pip_probe_row_kernel<i64, 1, 0, false>); break;
    case R_G64_2: PIP_PROBE_ROW(pip_probe_row_kernel<i64, 2, 0, false>); break;
    case R_G64_4: PIP_PROBE_ROW(pip_probe_row_kernel<i64, 4, 0, false>); break;
    case R_G64R: PIP_PROBE_ROW(pip_probe_row_kernel<i64, 1, 0, true>); break;
    case R_S64: PIP_PROBE_ROW(pip_probe_row_kernel<i64, 1, 3, false>); break;
    case R_G128_1: PIP_PROBE_ROW(pip_probe_row_kernel<i128, 1, 0, false>); break;
    case R_G128_4: PIP_PROBE_ROW(pip_probe_row_kernel<i128, 4, 0, false>); break;
    case R_N128_1: PIP_PROBE_ROW(pip_probe_row_kernel<i128, 1, 1, false>); break;
    case R_N128_4: PIP_PROBE_ROW(pip_probe_row_kernel<i128, 4, 1, false>); break;
    case R_NN128_1: PIP_PROBE_ROW(pip_probe_row_kernel<i128, 1, 2, false>); break;
    case R_NN128_4: PIP_PROBE_ROW(pip_probe_row_kernel<i128, 4, 2, false>); break;
    case R_LI_S: PIP_PROBE_ROW(pip_probe_lean_kernel<LeanIntRows, true>); break;
    case R_LI_M: PIP_PROBE_ROW(pip_probe_lean_kernel<LeanIntRows, false>); break;
    case R_LL_S: PIP_PROBE_ROW(pip_probe_lean_kernel<LeanLongRows, true>); break;
    case R_LL_M: PIP_PROBE_ROW(pip_probe_lean_kernel<LeanLongRows, false>); break;
    case R_LI_S_GS: PIP_PROBE_ROW(pip_probe_lean_kernel<LeanIntRows, true, true>); break;
    case R_LI_M_GS: PIP_PROBE_ROW(pip_probe_lean_kernel<LeanIntRows, false, true>); break;
    case R_LL_S_GS: PIP_PROBE_ROW(pip_probe_lean_kernel<LeanLongRows, true, true>); break;
    case R_LL_M_GS: PIP_PROBE_ROW(pip_probe_lean_kernel<LeanLongRows, false, true>); break;
  }
#undef PIP_PROBE_ROW
  return probe_finish(hipGetLastError());
}
