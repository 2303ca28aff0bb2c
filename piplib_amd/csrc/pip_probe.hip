// piplib_amd/csrc/pip_probe.hip -- testing aid: the device functions of the pivot kernels (pip_advance.h, the row flavours
// of pip_lean.h) and of the device tree (pip_quast.hip) run on operands the caller gives, so that a test holds each of
// them to exact integers at the magnitudes where they change code path (tests/test_gpu_arith_probe.py).  The probe
// kernels CALL the shipped functions; nothing here restates them, and no shipped kernel calls anything here.
//
//   pipamd_debug_arith(engine, op, in, out, n)            one case per lane, n cases
//   pipamd_debug_row_update(engine, path, in, out, ncases) one wave per case (the row functions ballot and readlane)
// and the lean kernel's per-lane preparation and its reductions from a given gcd (tests/test_gpu_lean_prep_probe.py):
// pipamd_debug_arith op 128, pipamd_debug_row_update paths 32 ... 35;
//   pipamd_debug_select(engine, fn, in, out, ncases)      one workgroup per case: the functions that decide which pivot is
//     taken -- choose_column / choose_column_slow / lean_choose_column (choisir_piv), sort_rows (tab_sort_rows), exam_rows
//     (exam_coef) -- on a small tableau, after row_publish / lean_publish have summarised its rows; the summaries are
//     reported too (tests/test_gpu_select_probe.py; the case layout stands above the kernels).
//   pipamd_debug_det_replay(engine, which, ebits, in, out, njobs, list, nlist)   the determinant replay's kernels and the
//     spare blocks' one-lane walk on job headers and logs the caller gives (tests/test_gpu_det_replay_probe.py).
//   pipamd_debug_quast_step(engine, inst, in, nin, out, nout, ncases)   one wave per case: the wave-level steps of the device
//     tree (pip_quast.hip: classify_rows, sort_rows, pivot_step, make_cut, deepen, find_quotient, build_sub, solve_plain)
//     on a tableau the caller gives (tests/test_gpu_quast_step_probe.py; the case layout stands in pip_quast.h).
//
// `in` / `out`: device pointers to int64 words, 16-byte aligned; a 128-bit value is two words, low then high (as
// det_limb).  Exported, not declared in include/piplib_amd.h (like pipamd_debug_lean): no part of the interface.
#include <string.h>

#include <vector>

#include "pip_lean.h"
#include "pip_host.h"
#include "pip_quast.h"
#include "../../include/piplib_amd.h"

// the device tree's helpers live in pip_quast.hip's anonymous namespace: its own probe kernel, launched from here
extern "C" hipError_t pipk_launch_quast_probe(int op, const long long *in, long long *out, int n, hipStream_t stream);
// the two replay kernels live in pip_kernels.hip: its launcher for a caller's jobs, list and count
extern "C" hipError_t pipk_launch_det_replay(PipJob *jobs, long long *arena, int njobs, int ebits, int wave_per_job,
                                             const int *in_list, const int *in_count, hipStream_t stream);

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
    case P_INV64: o[0] = (i64)inv_odd((u64)a[0]); break;
    case P_INV128: st2(o, (i128)inv_odd((u128)ld2(a))); break;
    case P_INVW32: o[0] = (i64)inv_odd((unsigned)a[0]); break;
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
    case P_BITLEN64: o[0] = bitlen((u64)a[0]); break;
    case P_BITLEN128: o[0] = bitlen((u128)ld2(a)); break;
    case P_CTZ128: o[0] = ctz((u128)ld2(a)); break;
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
  const i64 dpiv = uni(a[1]);
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

// ---- pipamd_debug_select: one workgroup per case, the functions that decide WHICH pivot is taken (choisir_piv,
// tab_sort_rows, exam_coef) on a small tableau the caller gives.  `in`: words 0, 1 the lengths of `in` and `out` in words,
// then the cases' offsets into `in` (ncases words) and into `out` (ncases words), then the cases.  A case, in int64 words
// (values of the flavour's Entier T: one word, or two, low then high):
//   nvar, ncol, W, ni, nligne, pivi, bigparm, smax (the bits of a double)            8 words
//   ref[nligne], urow[nvar], srow[ni], fl[ni], size[ni] (the bits of a float)        a word each
//   the ni real rows of W entries, slot by slot, then den[ni]                        values of T, at an even word offset
// out: status (1; 0 = the case does not fit the probe and nothing was run), the function's return value,
// max_row_class, ref[nligne], fl[ni], then per slot sig, rcls, cst (a value of T) and the NM words of nzm; the lean
// flavours append the packed image of the rows (ni slots of W values of T), which they read the rows back from.
// Every real row is summarised by the shipped row_publish / lean_publish before the function under test runs.
enum {
  SEL_SLOTS = 192, SEL_ROWS = 256,          // row slots and logical rows the probe's tables hold ...
  SEL_SLOTS_NW4 = 320, SEL_ROWS_NW4 = 384,  // ... and for exam_rows<i64, 4>, whose 256 threads wrap around at 257 rows
  S_C64S_1 = 0, S_C64S_2, S_C64S_4, S_C64_1, S_C64_2, S_C64_4, S_C128_1, S_C128_4, S_C128_8, S_SLOW64, S_SLOW128,
  S_LI_S, S_LI_M, S_LL_S, S_LL_M, S_SORT64, S_EXAM64_1, S_EXAM64_4, S_NFN
};
enum { SM_CHOOSE_SMALL, SM_CHOOSE, SM_SLOW, SM_SORT, SM_EXAM };

template <class T, int WP, int NM, int SLOTS, int ROWS>
struct SelectImage {
  static constexpr int NS = SLOTS, NR = ROWS;
  T den[SLOTS], prow[WP], cst[SLOTS];
  u64 nzm[SLOTS * NM];
  float size[SLOTS];
  u16 sig[SLOTS], srow[SLOTS], work[SLOTS], ref[ROWS], urow[WP];
  u8 fl[SLOTS], nf[SLOTS], rcls[SLOTS];
  Scalars sc;
  __device__ __forceinline__ Shared<T> shared() {
    Shared<T> S = {den, prow, cst, nzm, size, sig, srow, work, ref, urow, fl, nf, rcls};
    return S;
  }
};

struct SelectCase {
  int nvar, ncol, W, ni, nligne, pivi, bigparm;
  double smax;
  const i64 *ref, *urow, *srow, *fl, *size, *vals, *den;  // vals: the rows
  i64 *out;
  size_t nout;
};

// the case's header and extents, checked against the probe's tables and the two buffers; uniform over the workgroup
template <class T>
__device__ __forceinline__ bool select_case(const i64 *in, i64 *out, int cs, int ncases, int WP, int NM, int slots, int rows, bool lean,
                                            SelectCase &c) {
  constexpr size_t EW = ET<T>::EW;
  const u64 nin = (u64)in[0], nall = (u64)in[1], oi = (u64)in[2 + cs], oo = (u64)in[2 + ncases + cs];
  if (oo >= nall) return false;
  c.out = out + oo;
  c.out[0] = 0;
  if (oi < 2 + 2 * (u64)ncases || oi + 8 > nin) return false;
  const i64 *h = in + oi;
  for (int k = 0; k < 7; k++)
    if (h[k] < -1 || h[k] > 4096) return false;
  c.nvar = (int)h[0], c.ncol = (int)h[1], c.W = (int)h[2], c.ni = (int)h[3], c.nligne = (int)h[4], c.pivi = (int)h[5];
  c.bigparm = (int)h[6];
  c.smax = __longlong_as_double(h[7]);
  if (c.nvar < 1 || c.nvar > WP || c.ncol < c.nvar || c.ncol > c.W || c.W > WP || (c.W & 1) || c.ni < 0 || c.ni > slots ||
      c.nligne < 0 || c.nligne > rows)
    return false;
  size_t o = 8;
  c.ref = h + o, o += c.nligne;
  c.urow = h + o, o += c.nvar;
  c.srow = h + o, o += c.ni;
  c.fl = h + o, o += c.ni;
  c.size = h + o, o += c.ni;
  o += (oi + o) & 1;
  c.vals = h + o, o += EW * (size_t)c.ni * c.W;
  c.den = h + o, o += EW * (size_t)c.ni;
  c.nout = 3 + (size_t)c.nligne + c.ni + (size_t)c.ni * (2 + EW + NM) + (lean ? EW * (size_t)c.ni * c.W : 0);
  if (oi + o > nin || oo + c.nout > nall) return false;
  // what the functions index tables with
  for (int k = 0; k < c.nligne; k++) {
    const i64 rf = c.ref[k];
    if (rf < 0 || ((rf & UNITBIT) ? (rf & ~(i64)(UNITBIT | UNITZERO)) >= c.nvar : rf >= c.ni)) return false;
  }
  for (int k = 0; k < c.nvar; k++)
    if (c.urow[k] < 0 || c.urow[k] > 0xffff) return false;
  for (int k = 0; k < c.ni; k++)
    if (c.srow[k] < 0 || c.srow[k] > 0xffff) return false;
  if (c.pivi >= 0 && (c.pivi >= c.nligne || (c.ref[c.pivi] & UNITBIT))) return false;
  return true;
}

template <class T, class IM>
__device__ __forceinline__ void select_stage(IM &im, const SelectCase &c, int WP, int tid, int nt) {
  for (int k = tid; k < IM::NS; k += nt) {
    const bool in = k < c.ni;
    im.den[k] = in ? ldv<T>(c.den, k) : (T)0;
    im.cst[k] = 0;
    im.size[k] = in ? __uint_as_float((unsigned)c.size[k]) : 0.f;
    im.sig[k] = 0, im.work[k] = 0, im.nf[k] = 0, im.rcls[k] = 0;
    im.srow[k] = in ? (u16)c.srow[k] : (u16)NOROW;
    im.fl[k] = in ? (u8)c.fl[k] : (u8)0;
  }
  for (int k = tid; k < IM::NR; k += nt) im.ref[k] = k < c.nligne ? (u16)c.ref[k] : (u16)UNITBIT;
  for (int k = tid; k < WP; k += nt) {
    im.prow[k] = 0;
    im.urow[k] = k < c.nvar ? (u16)c.urow[k] : (u16)NOROW;
  }
}

// what every case reports: the tables the function may have written and what the publish functions left per slot
template <class T, int NM>
__device__ __forceinline__ void select_report(const Shared<T> &S, const T *cst, const SelectCase &c, int ret, int mc, int tid, int nt) {
  constexpr int EW = ET<T>::EW;
  i64 *o = c.out;
  if (tid == 0) o[0] = 1, o[1] = ret, o[2] = mc;
  o += 3;
  for (int k = tid; k < c.nligne; k += nt) o[k] = S.ref[k];
  o += c.nligne;
  for (int k = tid; k < c.ni; k += nt) o[k] = S.fl[k];
  o += c.ni;
  for (int s = tid; s < c.ni; s += nt) {
    i64 *p = o + (size_t)s * (2 + EW + NM);
    p[0] = S.sig[s], p[1] = S.rcls[s];
    stv<T>(p + 2, 0, cst[s]);
    for (int e = 0; e < NM; e++) p[2 + EW + e] = (i64)S.nzm[(size_t)s * NM + e];
  }
}

template <class T, int NCH, int NW, int MODE, int SLOTS = SEL_SLOTS, int ROWS = SEL_ROWS>
__global__ __launch_bounds__(64 * NW) void pip_probe_select_kernel(const i64 *in, i64 *out, int ncases) {
  constexpr int WP = NCH * 64 * ET<T>::CPL, NM = NCH * ET<T>::CPL, NT = 64 * NW;
  __shared__ SelectImage<T, WP, NM, SLOTS, ROWS> im;
  const int cs = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (cs >= ncases) return;
  SelectCase c;
  if (!select_case<T>(in, out, cs, ncases, WP, NM, SLOTS, ROWS, false, c)) return;
  select_stage<T>(im, c, WP, tid, NT);
  __syncthreads();
  const Shared<T> S = im.shared();
  const T *vals = reinterpret_cast<const T *>(c.vals);
  int ret = 0, mc = 0;
  RowRegs<T, NCH> pr = {};
  if (wave == 0) {
    for (int s = 0; s < c.ni; s++) {
      RowRegs<T, NCH> r;
      row_load<T, NCH>(r, vals + (size_t)s * c.W, c.W, lane);
      row_publish<T, NCH>(r, S, s, c.nvar, c.ncol, c.bigparm, -1, 0, c.ncol > c.nvar + 1, lane);
    }
    __builtin_amdgcn_wave_barrier();
    mc = max_row_class(S, c.ni, lane);
    if (c.pivi >= 0) {  // the pivot row as phase A stages it: zero beyond ncol, a copy in LDS
      row_load<T, NCH>(pr, vals + (size_t)S.ref[c.pivi] * c.W, c.W, lane);
#pragma unroll
      for (int ch = 0; ch < NCH; ch++)
#pragma unroll
        for (int h = 0; h < ET<T>::CPL; h++) {
          const int j = colof<T>(ch, lane, h);
          if (j >= c.ncol) pr.v[ch][h] = 0;
          S.prow[j] = pr.v[ch][h];
        }
    }
  }
  __syncthreads();
  if constexpr (MODE == SM_EXAM) {
    ret = exam_rows<T, NW>(S, &im.sc, c.ni);
  } else if (wave == 0) {
    if constexpr (MODE == SM_CHOOSE_SMALL || MODE == SM_CHOOSE)
      ret = choose_column<T, NCH, MODE == SM_CHOOSE_SMALL>(S, pr, vals, c.W, c.nvar, c.nligne, c.pivi, c.W, &im.sc);
    else if constexpr (MODE == SM_SLOW)
      ret = choose_column_slow<T>(S, vals, c.W, c.nvar, c.nligne);
    else
      sort_rows<T>(S, c.nvar, c.nligne, c.smax);
  }
  __syncthreads();
  if (wave == 0) select_report<T, NM>(S, S.cst, c, ret, mc, lane, 64);
}

// the lean flavours: the rows are packed into the case's output image (F::store), read back from it (F::load) and
// summarised by lean_publish, as the lean kernels hold them
template <class F, bool SMALL>
__global__ __launch_bounds__(64) void pip_probe_select_lean_kernel(const i64 *in, i64 *out, int ncases) {
  typedef typename F::T T;
  typedef typename F::E E;
  constexpr int WP = F::WP, NM = F::NM, EW = ET<T>::EW;
  __shared__ SelectImage<T, WP, NM, SEL_SLOTS, SEL_ROWS> im;
  __shared__ T cstw[SEL_SLOTS];
  const int cs = blockIdx.x, lane = threadIdx.x;
  if (cs >= ncases) return;
  SelectCase c;
  if (!select_case<T>(in, out, cs, ncases, WP, NM, SEL_SLOTS, SEL_ROWS, true, c) || c.nvar >= WP) return;
  select_stage<T>(im, c, WP, lane, 64);
  __syncthreads();
  const Shared<T> S = im.shared();
  E *cst = reinterpret_cast<E *>(im.cst);
  const i64 *rows = c.vals;
  T *vals = reinterpret_cast<T *>(c.out + (c.nout - (size_t)EW * c.ni * c.W));
  if (((uintptr_t)vals & 15) != 0) return;
  for (int s = 0; s < c.ni; s++) {
    typename F::Row r, z;
#pragma unroll
    for (int h = 0; h < F::NV; h++) {
      const int j = F::col(lane, h);
      r.v[h] = j < c.W ? (E)ldv<T>(rows, (size_t)s * c.W + j) : (E)0;
    }
    F::store(r, vals + (size_t)s * c.W, lane, c.W);
    __builtin_amdgcn_wave_barrier();
    F::load(z, vals + (size_t)s * c.W, lane, c.W);
    lean_publish<F, false>(z, S, cst, s, -1, 0, lane, c.nvar);
  }
  __syncthreads();
  const int mc = max_row_class(S, c.ni, lane);
  typename F::Row pr = {};
  if (c.pivi >= 0) F::load(pr, vals + (size_t)S.ref[c.pivi] * c.W, lane, c.W);
  const int ret = lean_choose_column<F, SMALL>(S, pr, vals, c.W, c.nvar, c.nligne, c.pivi, &im.sc);
  __syncthreads();
  for (int s = lane; s < c.ni; s += 64) cstw[s] = (T)cst[s];
  __syncthreads();
  select_report<T, NM>(S, cstw, c, ret, mc, lane, 64);
}

// ---- pipamd_debug_det_replay: the determinant replay (pip_kernels.hip, det_replay_lane of pip_advance.h) on job headers
// and logs the caller gives.  Per job RP_IN words in: the header's det[] (8 words), ldet, npiv, status, nlog, ebits, aux, two
// words of padding, then the log area as the pivot kernels fill it -- pair k at entries 2k, 2k + 1 of the job's entry
// type, room for PIPAMD_DETLOG pairs of 128-bit entries; what stands behind the job's nlog pairs is the caller's too (no
// replay may read it into a result).  RP_OUT words out: det[], ldet, npiv, status, nlog as the launch left them.
enum { RP_HDR = 16, RP_LOG = 2 * PIPAMD_DETLOG * 2, RP_IN = RP_HDR + RP_LOG, RP_OUT = 12 };

// which = 2: the lean kernel's spare blocks' instantiation of the one-lane walk (lean_spare_replay, pip_lean.h), a lane
// per job as pip_det_replay_lanes_kernel indexes them
template <class T>
__global__ __launch_bounds__(64) void pip_probe_replay_spare_kernel(PipJob *jobs, i64 *arena, int njobs, const int *in_list,
                                                                    const int *in_count) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int nq = in_count ? *in_count : njobs;
  if (t >= nq) return;
  det_replay_lane<T, PIP_LEAN_REPLAY_CH>(&jobs[in_list ? in_list[t] : t], arena);
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

extern "C" int pipamd_debug_select(pipamd_engine *e, int fn, const long long *in, long long *out, int ncases) {
  if (!e || ncases < 0 || !probe_ptrs_ok(in, out) || fn < 0 || fn >= S_NFN) return PIPAMD_E_INVALID;
  if (hipSetDevice(e->device) != hipSuccess) return PIPAMD_E_HIP;
  if (ncases == 0) return PIPAMD_OK;
#define PIP_PROBE_SEL(NW, ...) hipLaunchKernelGGL((__VA_ARGS__), dim3(ncases), dim3(64 * NW), 0, 0, in, out, ncases)
  switch (fn) {
    case S_C64S_1: PIP_PROBE_SEL(1, pip_probe_select_kernel<i64, 1, 1, SM_CHOOSE_SMALL>); break;
    case S_C64S_2: PIP_PROBE_SEL(1, pip_probe_select_kernel<i64, 2, 1, SM_CHOOSE_SMALL>); break;
    case S_C64S_4: PIP_PROBE_SEL(1, pip_probe_select_kernel<i64, 4, 1, SM_CHOOSE_SMALL>); break;
    case S_C64_1: PIP_PROBE_SEL(1, pip_probe_select_kernel<i64, 1, 1, SM_CHOOSE>); break;
    case S_C64_2: PIP_PROBE_SEL(1, pip_probe_select_kernel<i64, 2, 1, SM_CHOOSE>); break;
    case S_C64_4: PIP_PROBE_SEL(1, pip_probe_select_kernel<i64, 4, 1, SM_CHOOSE>); break;
    case S_C128_1: PIP_PROBE_SEL(1, pip_probe_select_kernel<i128, 1, 1, SM_CHOOSE>); break;
    case S_C128_4: PIP_PROBE_SEL(1, pip_probe_select_kernel<i128, 4, 1, SM_CHOOSE>); break;
    case S_C128_8: PIP_PROBE_SEL(1, pip_probe_select_kernel<i128, 8, 1, SM_CHOOSE>); break;
    case S_SLOW64: PIP_PROBE_SEL(1, pip_probe_select_kernel<i64, 4, 1, SM_SLOW>); break;
    case S_SLOW128: PIP_PROBE_SEL(1, pip_probe_select_kernel<i128, 8, 1, SM_SLOW>); break;
    case S_LI_S: PIP_PROBE_SEL(1, pip_probe_select_lean_kernel<LeanIntRows, true>); break;
    case S_LI_M: PIP_PROBE_SEL(1, pip_probe_select_lean_kernel<LeanIntRows, false>); break;
    case S_LL_S: PIP_PROBE_SEL(1, pip_probe_select_lean_kernel<LeanLongRows, true>); break;
    case S_LL_M: PIP_PROBE_SEL(1, pip_probe_select_lean_kernel<LeanLongRows, false>); break;
    case S_SORT64: PIP_PROBE_SEL(1, pip_probe_select_kernel<i64, 1, 1, SM_SORT>); break;
    case S_EXAM64_1: PIP_PROBE_SEL(1, pip_probe_select_kernel<i64, 1, 1, SM_EXAM>); break;
    case S_EXAM64_4: PIP_PROBE_SEL(4, pip_probe_select_kernel<i64, 1, 4, SM_EXAM, SEL_SLOTS_NW4, SEL_ROWS_NW4>); break;
  }
#undef PIP_PROBE_SEL
  return probe_finish(hipGetLastError());
}

// ---- pipamd_debug_quast_step: the cases of a call, checked on the host before anything is launched (layout: pip_quast.h).
// Every index a step forms from the case's own words is held within the image here -- the kernel stages and calls, it
// checks nothing -- and every case's image within the dynamic LDS a kernel gets without opting in to more.  `h`: the nin
// words of `in`.  Returns the largest image in bytes, 0 for a call that must not run.
static size_t quast_step_check(const long long *h, size_t nin, size_t nout, int inst, int ncases) {
  const int NB = 1 + (inst & 1), CMAX = 64 * NB;
  const size_t EW = inst >= 2 ? 2 : 1;
  if (nin < 2 + 2 * (size_t)ncases || (size_t)h[0] != nin || (size_t)h[1] != nout) return 0;
  size_t shm = 0, out_end = 0;
  for (int cs = 0; cs < ncases; cs++) {
    const unsigned long long oi = (unsigned long long)h[2 + cs], oo = (unsigned long long)h[2 + ncases + cs];
    if (oi < 2 + 2 * (size_t)ncases || oi > nin || nin - oi < QS_HDR || oo < out_end || oo > nout) return 0;
    const long long *c = h + oi;
    for (int k = 0; k < QS_HDR; k++)
      if (c[k] < -1 || c[k] > 4096 || (k >= 18 && c[k] != 0)) return 0;
    QStepCase g;
    qstep_read(c, &g);
    if (g.fn < 0 || g.fn >= QS_NFN || g.W < 1 || g.W > CMAX || g.S < 1 || g.S > 256 || g.R < 1 || g.R > 256 || g.CR < 0 || g.CR > 128 ||
        g.CW < 1 || g.CW > 64 || g.nvar < 1 || g.nvar >= g.ncol || g.ncol > g.W || g.nligne < 0 || g.nligne > g.R || g.ni < 0 ||
        g.ni > g.S || g.bigparm >= g.ncol || g.pivi < 0 || g.nc < 0 || g.nc > g.CR || g.nparm < 0 || g.nparm >= g.CW ||
        g.deepest < 0 || g.deepest > 1 || g.budget < 0 || g.opts < 0 || g.opts > 7 || g.ldet < 0 || g.ldet > PIPAMD_MAXDET)
      return 0;
    const size_t lds = qstep_lds_bytes(g, 8 * EW), nw = qstep_in_words(g, EW), ow = qstep_out_words(g, EW, NB);
    if (lds > QS_LDS_MAX || nin - oi < nw || nout - oo < ow) return 0;
    out_end = oo + ow;
    shm = lds > shm ? lds : shm;
    const long long *flag = c + QS_HDR, *ref = flag + g.R, *pos = ref + g.R, *den = pos + QS_POS + EW * PIPAMD_MAXDET;
    for (int k = 0; k < g.R; k++) {
      if (flag[k] < 0 || flag[k] > 63 || ref[k] < 0 || ref[k] >= ((flag[k] & 1) ? g.nvar : g.S)) return 0;
      const long long hi = den[EW * k + EW - 1];  // a denominator is at least 1: every step divides by it
      if (hi < 0 || (hi == 0 && (EW == 1 || den[EW * k] == 0))) return 0;
    }
    for (int k = 0; k < QS_POS; k++)
      if (pos[k] < 0 || pos[k] > 255) return 0;
    const bool row_step = g.fn == QS_PIVOT || g.fn == QS_MAKE_CUT || g.fn == QS_DEEPEN || g.fn == QS_CUT_CHAIN;
    if (row_step && (g.pivi >= g.nligne || (flag[g.pivi] & 1))) return 0;  // the pivot row / the row to cut is a real row
    if (g.fn == QS_SORT && g.nvar > g.nligne) return 0;
    if (g.fn >= QS_FIND_QUOTIENT && NB != 1) return 0;  // as shipped: one column block
    if (g.fn == QS_SOLVE_PLAIN && (g.ncol != g.nvar + 1 || g.nvar + g.ni != g.nligne)) return 0;
  }
  return shm;
}

// pipamd_debug_quast_step(engine, inst, in, nin, out, nout, ncases): `in` / `out` device pointers to nin / nout words.
// inst: 0 <long long, 1>, 1 <long long, 2>, 2 <__int128, 1>, 3 <__int128, 2> of QK<QI, NB> (pip_quast.hip).  A call with a
// malformed case is refused whole: nothing is launched and `out` is left alone.
extern "C" int pipamd_debug_quast_step(pipamd_engine *e, int inst, const long long *in, long long nin, long long *out, long long nout,
                                       int ncases) {
  if (!e || inst < 0 || inst > 3 || ncases < 0 || ncases > 65536 || nin < 2 || nout < 0 || nin > (1ll << 27) || nout > (1ll << 27) ||
      !probe_ptrs_ok(in, out))
    return PIPAMD_E_INVALID;
  if (hipSetDevice(e->device) != hipSuccess) return PIPAMD_E_HIP;
  if (ncases == 0) return PIPAMD_OK;
  std::vector<long long> h((size_t)nin);
  if (hipMemcpy(h.data(), in, h.size() * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) return PIPAMD_E_HIP;
  const size_t shm = quast_step_check(h.data(), (size_t)nin, (size_t)nout, inst, ncases);
  if (shm == 0) return PIPAMD_E_INVALID;
  return probe_finish(pipk_launch_quast_step(inst, in, out, ncases, shm, 0));
}

// pipamd_debug_det_replay(engine, which, ebits, in, out, njobs, list, nlist): `in` / `out` device pointers (layout above
// the probe kernel), `list` a HOST array of nlist job indices or NULL.  The job headers and their log areas are built in a
// scratch arena of the call's own; then ONE launch of the shipped code for entries of `ebits` bits -- which = 0:
// pip_det_replay_kernel (a wave per job), 1: pip_det_replay_lanes_kernel (a lane per job), 2: the spare blocks'
// det_replay_lane<T, PIP_LEAN_REPLAY_CH> -- over all njobs jobs, or, with a list, over the listed ones with the count in a
// device word and the grid still sized by njobs (the blocks and lanes beyond the count must leave every job alone).
extern "C" int pipamd_debug_det_replay(pipamd_engine *e, int which, int ebits, const long long *in, long long *out, int njobs,
                                       const int *list, int nlist) {
  if (!e || njobs < 0 || njobs > 65536 || !probe_ptrs_ok(in, out) || which < 0 || which > 2 || (ebits != 64 && ebits != 128) ||
      (list ? (nlist < 0 || nlist > njobs) : nlist != 0))
    return PIPAMD_E_INVALID;
  for (int i = 0; list && i < nlist; i++)
    if (list[i] < 0 || list[i] >= njobs) return PIPAMD_E_INVALID;
  if (hipSetDevice(e->device) != hipSuccess) return PIPAMD_E_HIP;
  if (njobs == 0) return PIPAMD_OK;
  std::vector<long long> h((size_t)njobs * RP_IN), arena_h((size_t)njobs * RP_LOG), o((size_t)njobs * RP_OUT);
  std::vector<PipJob> jobs_h(njobs);
  if (hipMemcpy(h.data(), in, h.size() * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) return PIPAMD_E_HIP;
  for (int j = 0; j < njobs; j++) {
    const long long *c = &h[(size_t)j * RP_IN];
    PipJob &J = jobs_h[j];
    memset(&J, 0, sizeof J);
    if (c[11] < 0 || c[11] > PIPAMD_DETLOG || (c[12] != 64 && c[12] != 128)) return PIPAMD_E_INVALID;  // the log holds no more
    for (int i = 0; i < 2 * PIPAMD_MAXDET; i++) J.det[i] = c[i];
    J.ldet = (int)c[8];
    J.npiv = (int)c[9];
    J.status = (int)c[10];
    J.nlog = (int)c[11];
    J.ebits = (int)c[12];
    J.aux = (int)c[13];
    J.log_off = (int64_t)j * RP_LOG;
    memcpy(&arena_h[(size_t)j * RP_LOG], c + RP_HDR, RP_LOG * sizeof(long long));
  }
  PipJob *d_jobs = nullptr;
  long long *d_arena = nullptr;
  int *d_list = nullptr;  // the list, then the count
  hipError_t he = hipMalloc((void **)&d_jobs, jobs_h.size() * sizeof(PipJob));
  if (he == hipSuccess) he = hipMalloc((void **)&d_arena, arena_h.size() * sizeof(long long));
  if (he == hipSuccess && list) he = hipMalloc((void **)&d_list, ((size_t)nlist + 1) * sizeof(int));
  if (he == hipSuccess) he = hipMemcpy(d_jobs, jobs_h.data(), jobs_h.size() * sizeof(PipJob), hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemcpy(d_arena, arena_h.data(), arena_h.size() * sizeof(long long), hipMemcpyHostToDevice);
  if (he == hipSuccess && list) {
    std::vector<int> l(list, list + nlist);
    l.push_back(nlist);
    he = hipMemcpy(d_list, l.data(), l.size() * sizeof(int), hipMemcpyHostToDevice);
  }
  if (he == hipSuccess) {
    const int *cnt = list ? d_list + nlist : nullptr;
    if (which == 2) {
      if (ebits == 128)
        hipLaunchKernelGGL(pip_probe_replay_spare_kernel<i128>, dim3((njobs + 63) / 64), dim3(64), 0, 0, d_jobs, d_arena, njobs, d_list, cnt);
      else
        hipLaunchKernelGGL(pip_probe_replay_spare_kernel<i64>, dim3((njobs + 63) / 64), dim3(64), 0, 0, d_jobs, d_arena, njobs, d_list, cnt);
      he = hipGetLastError();
    } else {
      he = pipk_launch_det_replay(d_jobs, d_arena, njobs, ebits, which == 0, d_list, cnt, 0);
    }
  }
  if (he == hipSuccess) he = hipDeviceSynchronize();
  if (he == hipSuccess) he = hipMemcpy(jobs_h.data(), d_jobs, jobs_h.size() * sizeof(PipJob), hipMemcpyDeviceToHost);
  for (int j = 0; he == hipSuccess && j < njobs; j++) {
    const PipJob &J = jobs_h[j];
    long long *c = &o[(size_t)j * RP_OUT];
    for (int i = 0; i < 2 * PIPAMD_MAXDET; i++) c[i] = J.det[i];
    c[8] = J.ldet, c[9] = J.npiv, c[10] = J.status, c[11] = J.nlog;
  }
  if (he == hipSuccess) he = hipMemcpy(out, o.data(), o.size() * sizeof(long long), hipMemcpyHostToDevice);
  hipFree(d_jobs);
  hipFree(d_arena);
  hipFree(d_list);
  if (he != hipSuccess) {
    pipamd_set_error("replay probe: %s", hipGetErrorString(he));
    return PIPAMD_E_HIP;
  }
  return PIPAMD_OK;
}
