// piplib_amd/csrc/pip_lean.h -- the lean bulk kernels: pip_advance_kernel's pivot loop specialised for the regimes the
// batches live in, written once (the text under PIP_LEAN_LOOP at the end of this file) against a "row flavour", compiled
// for the two flavours below.
//
// A lean kernel is one wave per tableau (pip_lean_kernel also four, NW: for the launch over the few hundred tableaux a first
// lean launch paused, see the entry points below), no parameters (BIG flavour of the int rows: the big parameter alone), rows skipped, plain cuts -- and EVERY entry of
// EVERY row stored at HALF the width of the flavour's Entier T (the packed element E).  Under that invariant
//   * rows live in HBM packed (the first half of the row's slot of W entries of T): half the traffic of the reference's
//     rows, half the working set, half the registers;
//   * while the rows involved are in magnitude class 0 (entries below 2^CLS0_BITS; pivot row's denominator too) every
//     product of a pivot fits E: the "small" path;
//   * a row of class 1 (an entry beyond that, still an E), or a pivot row of class 1, takes the "mid" path: the same
//     packed rows, products in T (nothing wraps), the row gcd and the division through row_reduce<T> -- the code
//     pip_advance_kernel runs on such a row, on the same values -- and choisir_piv's cross products in T.  The result
//     is a packed row again, almost always;
//   * none of the general kernel's other paths (wide tournament, parameters, deepest cuts, row tables in HBM) is
//     compiled in, the pivot row stays in registers, the LDS image is smaller (lean_image_bytes).
// A rewritten row that does NOT fit E any more is stored in the general format (W entries of T, the whole slot) and
// summarised with pip_advance_kernel's magnitude classes (2, 3); the pivot is finished -- no row is read twice in a pivot
// -- and the running maximum of the classes, checked between pivots, then ends the lean run.  A tableau that leaves --
// or anything else these kernels do not do: entries beyond E at entry, a cut under too large a denominator,
// PIPAMD_T_NOSKIP / _DEEPEST, a paused job -- is handed over in the general format (packed rows widened in place, the
// same row tables and saved summaries as a paused job of pip_advance_kernel) and stays PIPAMD_ST_RUN on the launch
// list: pipamd_batch_solve's next launches (pip_advance_kernel) take it from there.  Same algorithm, same statuses,
// same bits as pip_advance_kernel -- the reference's traiter()/pivoter()/choisir_piv()/exam_coef()/integrer()/tab_sort_rows
// (traiter.c:101-159, 297-548, 556-623, 628-791; integrer.c:305-486) -- which the parity tests check tableau by tableau.
//
// LeanIntRows, pip_lean_kernel<SC, FULL>: the regime the headline workload lives in.  64-bit Entier, int rows, at most
//   127 unknowns + constant in rows of W <= 128 columns (FULL: exactly 127 + 1, compile-time column counts),
//   compile-time row capacity SC.  A row is two 32-bit registers per lane (columns 2l, 2l + 1).  Small path (96 % of the
//   headline's pivots): 24-bit multiplies, the row gcd by float-reciprocal remainders, 32-bit summaries and cuts; mid
//   path (round 4): v_mad_i64_i32 products below 2^62.  64 VGPRs, no scratch, eight waves per SIMD.
//   Round 5 (PIP_LEAN_PREP): what a row's update needs of the row before it arrives -- gcd(pivot, foo), the multipliers,
//   the denominator product g0 and its gcd with the one entry of the new row known beforehand, dpiv * foo -- is
//   computed for all rows of a pivot at once, one row per lane (lean_prepare_rows; the rows' entries in the pivot column
//   are gathered from HBM ahead of the row queue), and the row loop takes each row's scalars out of the lanes: the
//   scalar unit no longer runs a binary gcd, two exact quotients and a 64-bit product per row, and the row gcd starts
//   from the folded value (small_reduce_from / row_reduce_rem_from) -- no remainder pass at all when that is 1.
//   (PIP_LEAN_KEEPCUT) a cut integrer() has just built stays in registers as the next pivot row.
//   (tests/test_gpu_lean_prep.py, tests/test_gpu_lean_prep_probe.py.)
//   (tests/test_gpu_parity.py: test_lean_kernel_paths, test_lean_kernel_other_widths, and every batch test of the suite.)
//   BIG, pip_lean_kernel<SC, false, true>: the same kernel for the tableaux whose ONE parameter is the big one (nparm == 1,
//   bigparm == nvar + 1, nvar + 2 <= W <= 128: what pip_solve builds for Maximize / Urs_unknowns, tab.c:292-393).  Such
//   a tableau needs no host decision -- exam_coef decides every sign from the big coefficient, then the constant
//   (traiter.c:107-157), integrer treats the big parameter as divisible by any number (integrer.c:373-377), so every
//   cut is a constant cut -- and the big column is one more column of the packed row that every pivot updates.  What
//   differs, all under `if constexpr (BIG)`: the caller's rows are nvar + 2 wide; lean_publish puts the big entry's
//   sign into the summary as row_publish does (bits 2-3 and 4-5), so that a job paused here resumes in
//   pip_advance_kernel and the other way round; exam_rows instead of the prepared exam flags; the cut's big column is
//   0; solution() emits two numerators per unknown, the big one gathered from the packed row.  PREP and KEEPCUT stay
//   on: 64 VGPRs, no scratch, eight waves per SIMD like the plain flavour, whose instantiations compile to what they
//   compiled to before.  OPT-IN (pipamd_engine_set_lean_big): 13-35 % ahead of pip_advance_kernel's launches except on a
//   lone Urs_unknowns batch, 3 % behind.  (tests/test_gpu_lean_bigparm.py, tests/test_gpu_batch_shift.py.)
// LeanLongRows, pip_lean64_kernel: the same one width up.  128-bit Entier, long long rows, 129 ... 256 columns, run-time
//   row capacity; lane l holds columns l, 64 + l, 128 + l, 192 + l (the geometry of pip_advance_kernel<__int128, 4>, so
//   that the saved summaries of a paused job mean the same to both kernels).  The overflow-safe flavour (piplib.h:42-88)
//   exists for the tableaux on which 64-bit arithmetic overflows -- but what outgrows 64 bits there are the determinant
//   limbs and the products of a row update, seldom the rows themselves: of the 1,000 tableaux of BASELINE's configs[4]
//   (the batch pinned by tests/golden/gmp/wide128.json) the reference's GMP build forms a value beyond 2^63 on 587, yet on
//   two in three every STORED entry stays below 2^63 from the first pivot to the last (657 of the 1,000 finish in this
//   kernel, 325 leave on a row beyond 2^63).  Small path: 64-bit arithmetic; mid path: 64 x 64 -> 128-bit products (four
//   32-bit multiply-adds each, not ten), reduce_by_inverse picks the narrowest width that holds them.  The per-lane
//   preparation of a pivot's rows (below) is NOT taken: with it the kernel needs 168 VGPRs and 12 bytes of scratch, so
//   PREP is false here and the row loop computes each row's multipliers itself, as before.  OPT-IN
//   (pipamd_engine_set_lean64): measured on that batch it is no faster than the four-wave pip_advance_kernel<__int128>
//   (16 registers a row, 128 VGPRs, 400 bytes of scratch per lane, three waves in four waiting during choisir_piv),
//   DESIGN.md section 3.  (tests/test_gpu_parity.py: test_lean64_kernel_paths, test_full_size_int128_config, against the
//   128-bit oracle and the reference's GMP build.)
#if !defined(PIP_LEAN_LOOP) && !defined(PIP_LEAN_H)
#define PIP_LEAN_H
#include "pip_advance.h"

#ifndef PIP_LEAN_PF
#define PIP_LEAN_PF 2  // int rows of a pivot's work list in flight
#endif
#ifndef PIP_LEAN_MID_INV
#define PIP_LEAN_MID_INV 0  // (A/B switch) the int mid path's row gcd and division by inverse multiplication (12 bytes of scratch per lane)
#endif
#ifndef PIP_LEAN_PREP
#define PIP_LEAN_PREP 1  // (A/B switch) int rows: multipliers and first gcd fold of a pivot's rows prepared one row per lane (lean_prepare_rows)
#endif
#ifndef PIP_LEAN_KEEPCUT
#define PIP_LEAN_KEEPCUT 1  // (A/B switch) a cut that integrer() has just built stays in registers as the pivot row
#endif
#ifndef PIP_LEAN_REPLAY_CH
#define PIP_LEAN_REPLAY_CH 4  // log entries a lane of a spare block loads at a time (lean_spare_replay; within the 64 VGPRs)
#endif
#ifndef PIP_LEAN_WAVES
#define PIP_LEAN_WAVES 8  // waves per SIMD pip_lean_kernel is bounded to (64 VGPRs)
#endif
#ifndef PIP_LEAN64_WAVES
#define PIP_LEAN64_WAVES 3  // waves per SIMD pip_lean64_kernel is bounded to (168 VGPRs)
#endif

// a packed row in registers: lane l's NV values (which columns: the flavour's col())
template <class E, int NV>
struct LeanRow {
  E v[NV];
};

// ---- the row flavours: what the two kernels disagree on.  T the Entier (general entry, product type), E the packed
// element, NV values per lane = NM bitmap words per row, NCH pip_advance_kernel's column blocks of the same width (the
// state_nch of a paused job), WP the padded row width; entries of class 0 are below 2^CLS0_BITS, a packed row's below
// 2^ROW_BITS, a cut is taken under a denominator below 2^CUT_BITS.
struct LeanIntRows {
  typedef i64 T;
  typedef int E;
  typedef LeanRow<int, 2> Row;
  typedef unsigned G;  // a prepared row's starting gcd as its lane keeps it (0: nothing folded, or beyond G)
  static constexpr int NV = 2, NM = 2, NCH = 1, WP = 128, CLS0_BITS = 15, ROW_BITS = 31, CUT_BITS = 31;
  static constexpr int ENTRY_PF = 4, PF = PIP_LEAN_PF, UNPACK_GROUP = 4;  // rows in flight: entry pass, work list, rows_unpack
  static constexpr bool FRESH = true;  // the entry pass may read the caller's rows (PIPAMD_T_FRESHROWS)
  static constexpr bool PREP = PIP_LEAN_PREP != 0;  // a pivot's rows are prepared one row per lane (lean_prepare_rows)
  static __device__ __forceinline__ int col(int lane, int h) { return 2 * lane + h; }
  static __device__ __forceinline__ int lane_of(int j) { return j >> 1; }
  static __device__ __forceinline__ int val_of(int j) { return j & 1; }
  static __device__ __forceinline__ bool shape(const PipJob *J, int nvar, int W) {  // the jobs this flavour takes
    return J->nvar == nvar && nvar < 128 && J->nparm == 0 && J->bigparm < 0 && J->W == W && W <= 128 && !(W & 1) && J->ebits != 128;
  }
  // ... and the BIG flavour: one parameter, the big one, behind the constant (unknowns | constant | big)
  static __device__ __forceinline__ bool shape_big(const PipJob *J, int nvar, int W) {
    return J->nvar == nvar && J->nparm == 1 && J->bigparm == nvar + 1 && J->W == W && nvar + 2 <= W && W <= 128 && !(W & 1) &&
           J->ebits != 128;
  }
  static __device__ __forceinline__ unsigned mag(int v) { return (unsigned)(v < 0 ? -v : v); }
  static __device__ __forceinline__ bool fits(i64 x) { return x > -((i64)1 << 31) && x < ((i64)1 << 31); }
  static __device__ __forceinline__ unsigned gcd(int a, int b) { return gcd_u32((unsigned)a, mag(b)); }
  // lane l holds columns 2l, 2l + 1, 8 bytes per lane (W even; lanes beyond the row hold zeros)
  static __device__ __forceinline__ void load(Row &r, const i64 *slot, int lane, int W) {
    int2 t = {0, 0};
    if (2 * lane < W) t = *reinterpret_cast<const int2 *>(reinterpret_cast<const int *>(slot) + 2 * lane);
    r.v[0] = t.x;
    r.v[1] = t.y;
  }
  // column j of a packed row, from any lane
  static __device__ __forceinline__ int gather(const i64 *slot, int j) { return reinterpret_cast<const int *>(slot)[j]; }
  static __device__ __forceinline__ void store(const Row &r, i64 *slot, int lane, int W) {
    int2 t;
    t.x = r.v[0];
    t.y = r.v[1];
    if (2 * lane < W) *reinterpret_cast<int2 *>(reinterpret_cast<int *>(slot) + 2 * lane) = t;
  }
  static __device__ __forceinline__ void store_wide(const i64 (&z)[2], i64 *slot, int lane, int W) {
    longlong2 t;
    t.x = z[0];
    t.y = z[1];
    if (2 * lane < W) *reinterpret_cast<longlong2 *>(slot + 2 * lane) = t;
  }
  // choisir_piv's cross product ab * n - nb * a: 24-bit multiplies while every row is in class 0, else below 2^62
  template <bool SMALL>
  static __device__ __forceinline__ void cross(int ab, int n, int nb, int a, bool &xneg, bool &xzero) {
    if constexpr (SMALL) {
      const int x = __mul24(ab, n) - __mul24(nb, a);
      xneg = x < 0;
      xzero = x == 0;
    } else {
      const i64 x = (i64)ab * (i64)n - (i64)nb * (i64)a;
      xneg = x < 0;
      xzero = x == 0;
    }
  }
  // piplib_llmod (integrer.c:69-74): r's entries -> their remainders in [0, D); through a float reciprocal when the row is
  // in class 0 and D < 2^15
  static __device__ __forceinline__ void row_mod(Row &r, int D, bool cls0) {
    const bool tinyD = D < (1 << 15) && cls0;
    const float rD = __builtin_amdgcn_rcpf((float)D);
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int v = r.v[h];
      if (tinyD) {
        const unsigned m = umod_tiny(mag(v), (unsigned)D, rD);
        r.v[h] = v < 0 ? (m ? D - (int)m : 0) : (int)m;
      } else {
        const int m = v % D;
        r.v[h] = m < 0 ? m + D : m;
      }
    }
  }
  static __device__ __forceinline__ bool small_den(i64) { return true; }
  // small path: every operand below 2^15, every product below 2^30.  r <- (lp r - foo pr) / gcd, nd the new denominator;
  // gs: where the row gcd starts (gcd(|g0|, |dpiv foo|) from lean_prepare_rows; 0: nothing prepared, from |g0|)
  static __device__ __forceinline__ bool update_small(Row &r, const Row &pr, int lp, int foo, i64 dpiv, int pivj, i64 g0, u64 gs,
                                                      int lane, i64 &nd) {
    int z[1][2];
    unsigned mx = 0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      int v = __mul24(r.v[h], lp) - __mul24(pr.v[h], foo);
      if (2 * lane + h == pivj) v = __mul24((int)dpiv, foo);
      z[0][h] = v;
      mx |= mag(v);
    }
    const bool ok = small_reduce_from<1>(z, mx, g0, gs ? gs : uabs(g0), lane, nd);
    r.v[0] = z[0][0];
    r.v[1] = z[0][1];
    return ok;
  }
  // mid path: int operands, products below 2^62 in long longs -- pip_advance_kernel's update_row on the same values (its
  // wrap-around arithmetic has nothing to wrap here, except dpiv * foo under a denominator beyond ints, which wraps the
  // same way)
  static __device__ __forceinline__ bool update_mid(i64 (&zw)[2], const Row &r, const Row &pr, int lp, int foo, i64 dpiv, int pivj,
                                                    i64 g0, u64 gs, int lane, i64 &nd) {
    u64 mx = 0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      i64 v = (i64)r.v[h] * (i64)lp - (i64)pr.v[h] * (i64)foo;
      if (2 * lane + h == pivj) v = wmul(dpiv, (i64)foo);
      zw[h] = v;
      mx |= uabs(v);
    }
#if PIP_LEAN_MID_INV
    return row_reduce<i64, 2, false>(zw, mx, g0, lane, nd, wmul(dpiv, (i64)foo), gs);
#else
    return row_reduce_rem_from<i64, 2>(zw, mx, g0, gs ? gs : uabs(g0), lane, nd);  // (the remainder loop: reduce_by_inverse costs this kernel 12 bytes of scratch)
#endif
  }
};

struct LeanLongRows {
  typedef i128 T;
  typedef i64 E;
  typedef LeanRow<i64, 4> Row;
  typedef u64 G;
  static constexpr int NV = 4, NM = 4, NCH = 4, WP = 256, CLS0_BITS = 31, ROW_BITS = 63, CUT_BITS = 62;
  static constexpr int ENTRY_PF = 1, PF = 2, UNPACK_GROUP = 2;
  static constexpr bool FRESH = false;
  static constexpr bool PREP = false;  // (128-bit gcds one per lane: 12 bytes of scratch under the 168-register bound, see the header comment)
  static __device__ __forceinline__ int col(int lane, int c) { return 64 * c + lane; }
  static __device__ __forceinline__ int lane_of(int j) { return j & 63; }
  static __device__ __forceinline__ int val_of(int j) { return j >> 6; }
  static __device__ __forceinline__ bool shape(const PipJob *J, int nvar, int W) {
    return nvar < 256 && nvar >= 1 && J->nparm == 0 && J->bigparm < 0 && W > 128 && W <= 256 && J->ebits == 128;
  }
  static __device__ __forceinline__ bool shape_big(const PipJob *, int, int) { return false; }  // (no BIG flavour of long long rows)
  static __device__ __forceinline__ u64 mag(i64 v) { return uabs(v); }
  static __device__ __forceinline__ bool fits(i128 x) { return fits64(x); }
  static __device__ __forceinline__ u64 gcd(i64 a, i64 b) { return gcd_mag((u64)a, uabs(b)); }
  static __device__ __forceinline__ void load(Row &r, const i128 *slot, int lane, int W) {
    const i64 *p = reinterpret_cast<const i64 *>(slot);
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int j = 64 * c + lane;
      r.v[c] = j < W ? p[j] : 0;
    }
  }
  static __device__ __forceinline__ i64 gather(const i128 *slot, int j) { return reinterpret_cast<const i64 *>(slot)[j]; }
  static __device__ __forceinline__ void store(const Row &r, i128 *slot, int lane, int W) {
    i64 *p = reinterpret_cast<i64 *>(slot);
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int j = 64 * c + lane;
      if (j < W) p[j] = r.v[c];
    }
  }
  static __device__ __forceinline__ void store_wide(const i128 (&z)[4], i128 *slot, int lane, int W) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int j = 64 * c + lane;
      if (j < W) {
        longlong2 t;
        t.x = (i64)(u64)(u128)z[c];
        t.y = (i64)(u64)((u128)z[c] >> 64);
        *reinterpret_cast<longlong2 *>(slot + j) = t;
      }
    }
  }
  // 64-bit while every row is in class 0 (entries below 2^31), else below 2^126
  template <bool SMALL>
  static __device__ __forceinline__ void cross(i64 ab, i64 n, i64 nb, i64 a, bool &xneg, bool &xzero) {
    if constexpr (SMALL) {
      const i64 x = ab * n - nb * a;
      xneg = x < 0;
      xzero = x == 0;
    } else {
      const i128 x = (i128)ab * (i128)n - (i128)nb * (i128)a;
      xneg = x < 0;
      xzero = x == 0;
    }
  }
  static __device__ __forceinline__ void row_mod(Row &r, i64 D, bool) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const i64 m = crem(r.v[c], D);
      r.v[c] = m < 0 ? m + D : m;
    }
  }
  static __device__ __forceinline__ bool small_den(i128 g0) { return g0 < ((i128)1 << 62) && g0 > -((i128)1 << 62); }
  // small path: every operand below 2^31, every product below 2^62; the denominator product a long long (small_den)
  static __device__ __forceinline__ bool update_small(Row &r, const Row &pr, i64 lp, i64 foo, i128 dpiv, int pivj, i128 g0, u128 gs,
                                                      int lane, i128 &nd) {
    u64 mx = 0;
    const i64 zf = (i64)dpiv * foo;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      i64 v = r.v[c] * lp - pr.v[c] * foo;
      if (64 * c + lane == pivj) v = zf;
      r.v[c] = v;
      mx |= uabs(v);
    }
    i64 nd64;
    const bool ok = row_reduce<i64, 4>(r.v, mx, (i64)g0, lane, nd64, zf, (u64)gs);  // (small_den: gs <= |g0| < 2^62)
    nd = (i128)nd64;
    return ok;
  }
  // mid path: long long operands, products below 2^126 -- pip_advance_kernel's update_row on the same values (its
  // wrap-around arithmetic has nothing to wrap here, except the products with denominators beyond long longs, which wrap
  // the same way)
  static __device__ __forceinline__ bool update_mid(i128 (&zw)[4], const Row &r, const Row &pr, i64 lp, i64 foo, i128 dpiv, int pivj,
                                                    i128 g0, u128 gs, int lane, i128 &nd) {
    u128 mx = 0;
    const i128 zf = wmul(dpiv, (i128)foo);
#pragma unroll
    for (int c = 0; c < 4; c++) {
      i128 v = (i128)r.v[c] * (i128)lp - (i128)pr.v[c] * (i128)foo;
      if (64 * c + lane == pivj) v = zf;
      zw[c] = v;
      mx |= uabs(v);
    }
    return row_reduce<i128, 4>(zw, mx, g0, lane, nd, zf, gs);
  }
};

// bytes of a lean kernel's LDS image for S row slots and L logical rows (smaller than pip_advance_kernel's: no pivot
// row, constant terms as packed elements)
template <class F>
__host__ __device__ constexpr size_t lean_image_bytes(int S, int L) {
  return ((sizeof(typename F::T) + sizeof(typename F::E) + 8 * F::NM + 9) * (size_t)S + 2 * (size_t)L + 2 * F::WP + 15) & ~(size_t)15;
}
__host__ __device__ constexpr size_t lean_lds_bytes(int SC) { return lean_image_bytes<LeanIntRows>(SC, SC + 128); }
__host__ __device__ constexpr size_t lean64_lds_bytes(int S, int L) { return lean_image_bytes<LeanLongRows>(S, L); }

// value k (uniform) of a row, read from lane src
template <class F, class X>
__device__ __forceinline__ X lean_entry(const X (&v)[F::NV], int k, int src) {
  X mine = 0;
#pragma unroll
  for (int h = 0; h < F::NV; h++)
    if (h == k) mine = v[h];
  if constexpr (sizeof(X) == 4)
    return __builtin_amdgcn_readlane(mine, src);
  else
    return readlane(mine, src);
}

// lane k's copy of a value (k uniform)
template <class X>
__device__ __forceinline__ X lean_lane(X v, int k) {
  if constexpr (sizeof(X) == 4)
    return (X)__builtin_amdgcn_readlane((int)v, k);
  else if constexpr (sizeof(X) == 8)
    return (X)readlane((i64)v, k);
  else
    return (X)readlane((i128)v, k);
}

// The part of a row's update that needs no more of the row than its entry `foo` in the pivot column (traiter.c:470-476):
// the multipliers lp = pivot / d and foo / d, d = gcd(pivot, foo); the denominator product g0 = lp * den; and the first
// fold of the row gcd, gs = gcd(|g0|, |dpiv * foo|) -- dpiv * foo is the new row's entry in the pivot column, the one
// entry known before the row arrives.  gs = 0: nothing folded (that entry is 0, or g0 is 0 or +-1), the row gcd starts
// from |g0|.  Plain per-lane code: pip_lean's row loop used to run it once per row on the scalar unit, lean_prepare_rows
// runs it for 64 rows at once, one per lane.
template <class F>
__device__ __forceinline__ void lean_prep_lane(typename F::E pivot, typename F::T dpiv, typename F::T den, typename F::E &foo,
                                               typename F::E &lp, typename F::T &g0, typename ET<typename F::T>::U &gs) {
  typedef typename F::T T;
  typedef typename F::E E;
  lp = pivot;
  g0 = den;
  if (pivot != 1) {
    const auto d = F::gcd(pivot, foo);
    if (d != 1) {  // (d == 0 cannot be: pivot > 0)
      lp = (E)exact_quo<i64>((i64)pivot, (i64)d);
      foo = (E)exact_quo<i64>((i64)foo, (i64)d);
    }
    g0 = wmul((T)lp, den);
  }
  gs = 0;
  const auto ag = uabs(g0);
  const T zf = wmul(dpiv, (T)foo);
  if (ag > 1 && zf != 0) gs = gcd_mag(ag, uabs(zf));
}

// Lane k prepares the row of S.work[w0 + k] (k < nwork - w0; the recycled pivot slot is skipped): `fk` is the row's entry
// in the pivot column, gathered by the caller (F::gather, issued ahead of the row queue's loads); the denominator and the
// magnitude class come from LDS.  Out, per lane: the multipliers, g0, the starting gcd (as F::G); returns the mask of
// the lanes whose row takes the small path.
template <class F>
__device__ __forceinline__ u64 lean_prepare_rows(const Shared<typename F::T> &S, int sk, bool active, typename F::E fk, typename F::E pivot,
                                                 typename F::T dpiv, bool psmall, typename F::E &m_lp, typename F::E &m_foo,
                                                 typename F::T &m_g0, typename F::G &m_gs) {
  typedef typename F::T T;
  bool small = false;
  m_lp = pivot;
  m_foo = 0;
  m_g0 = 1;
  m_gs = 0;
  if (active) {
    typename ET<T>::U gs;
    m_foo = fk;
    lean_prep_lane<F>(pivot, dpiv, S.den[sk], m_foo, m_lp, m_g0, gs);
    m_gs = (typename F::G)gs == gs ? (typename F::G)gs : 0;
    small = psmall && S.rcls[sk] == 0 && F::small_den(m_g0);
  }
  return ballot64(small);
}

// rows [0, n) of a block, packed -> the general format, each within its own slot (the loads of a group of rows are back
// before their slots are overwritten); rows of class 2 or 3 (rcls, LDS) are in the general format already.
// (first, step: the calling wave's share of the rows -- first, first + step, ... -- where several waves hold a tableau)
template <class F>
__device__ __forceinline__ void rows_unpack(typename F::T *vals, int n, int lane, int W, const u8 *rcls, int first = 0, int step = 1) {
  constexpr int G = F::UNPACK_GROUP;
  for (int s0 = 0; first + step * s0 < n; s0 += G) {
    typename F::Row rr[G];
    bool packed[G];
#pragma unroll
    for (int qq = 0; qq < G; qq++) {
      const int s = first + step * (s0 + qq);
      packed[qq] = s < n && rcls[s] < 2;
      if (packed[qq]) F::load(rr[qq], vals + (size_t)s * W, lane, W);
    }
#pragma unroll
    for (int qq = 0; qq < G; qq++)
      if (packed[qq]) {
        typename F::T z[F::NV];
#pragma unroll
        for (int h = 0; h < F::NV; h++) z[h] = (typename F::T)rr[qq].v[h];
        F::store_wide(z, vals + (size_t)(first + step * (s0 + qq)) * W, lane, W);
      }
  }
}

// sign summary, non-zero bitmap and magnitude class (0: every entry below 2^CLS0_BITS, 1: a packed row) of a packed
// row of nvar unknowns + constant; lane 0 publishes them for slot s (row_publish32 for this image: constant terms kept
// as packed elements).  Returns the class.  BIG: column nvar + 1 is the big parameter's; its sign goes into the summary as
// row_publish writes it for a tableau whose one parameter is the big one (bits 2-3 and 4-5).
template <class F, bool BIG = false>
__device__ __forceinline__ int lean_publish(const typename F::Row &z, const Shared<typename F::T> &S, typename F::E *cst, int s, int pivj,
                                            int extra_sig, int lane, int nvar) {
  typedef typename F::E E;
  const E cz = lean_entry<F>(z.v, F::val_of(nvar), F::lane_of(nvar));  // the constant term, column nvar
  int sig = extra_sig | (cz > 0 ? 1 : (cz < 0 ? 2 : 0));
  if (pivj >= 0) {
    const E pz = lean_entry<F>(z.v, F::val_of(pivj), F::lane_of(pivj));
    sig |= (pz > 0 ? 1 : (pz < 0 ? 2 : 0)) << 6;
  }
  if constexpr (BIG) {
    const E bz = lean_entry<F>(z.v, F::val_of(nvar + 1), F::lane_of(nvar + 1));
    sig |= bz > 0 ? (4 | 16) : (bz < 0 ? (8 | 32) : 0);
  }
  decltype(F::mag(cz)) mx = 0;
  u64 nz[F::NV];
#pragma unroll
  for (int h = 0; h < F::NV; h++) {
    mx |= F::mag(z.v[h]);
    nz[h] = ballot64(z.v[h] != 0);
  }
  const int cls = ballot64((mx >> F::CLS0_BITS) != 0) ? 1 : 0;
  if (lane == 0) {
    S.sig[s] = (u16)sig;
    S.rcls[s] = (u8)cls;
    cst[s] = cz;
#pragma unroll
    for (int h = 0; h < F::NV; h++) S.nzm[(size_t)s * F::NM + h] = nz[h];
  }
  return cls;
}

// the same for a row that left the packed elements (z: lane l's values as T): pip_advance_kernel's classes (2, 3); the
// constant term kept here is truncated -- the lean run ends before anything reads it
template <class F, bool BIG = false>
__device__ __forceinline__ int lean_publish_wide(const typename F::T (&z)[F::NV], const Shared<typename F::T> &S, typename F::E *cst,
                                                 int s, int pivj, int extra_sig, int lane, int nvar) {
  typedef typename F::T T;
  const T cz = lean_entry<F>(z, F::val_of(nvar), F::lane_of(nvar));
  int sig = extra_sig | sign_code(cz);
  if (pivj >= 0) sig |= sign_code(lean_entry<F>(z, F::val_of(pivj), F::lane_of(pivj))) << 6;
  if constexpr (BIG) {
    const int bs = sign_code(lean_entry<F>(z, F::val_of(nvar + 1), F::lane_of(nvar + 1)));
    sig |= bs == 1 ? (4 | 16) : (bs == 2 ? (8 | 32) : 0);
  }
  typename ET<T>::U mx = 0;
  u64 nz[F::NV];
#pragma unroll
  for (int h = 0; h < F::NV; h++) {
    mx |= uabs(z[h]);
    nz[h] = ballot64(z[h] != 0);
  }
  int cls = cls_of<T>(mx);
  if (cls < 2) cls = 2;  // (it does not fit E: at least 2^ROW_BITS)
  if (lane == 0) {
    S.sig[s] = (u16)sig;
    S.rcls[s] = (u8)cls;
    cst[s] = (typename F::E)cz;
#pragma unroll
    for (int h = 0; h < F::NV; h++) S.nzm[(size_t)s * F::NM + h] = nz[h];
  }
  return cls;
}

// choisir_piv (traiter.c:297-341) as choose_column<T, NCH, SMALL> does it, on packed rows.  SMALL: every row of the
// tableau is in class 0 (F::cross).
template <class F, bool SMALL>
__device__ __forceinline__ int lean_choose_column(const Shared<typename F::T> &S, const typename F::Row &prow, const typename F::T *vals,
                                                  int W, int nvar, int nligne, int pivi, Scalars *sc) {
  typedef typename F::E E;
  constexpr int NV = F::NV, NM = F::NM;
  const int lane = threadIdx.x & 63;
  E a[NV];
  int u[NV];
  bool cand[NV];
  u64 cm[NM];
  int count = 0;
#pragma unroll
  for (int h = 0; h < NV; h++) {
    const int j = F::col(lane, h);
    a[h] = j < nvar ? prow.v[h] : 0;
    cand[h] = a[h] > 0;
    u[h] = cand[h] ? (int)S.urow[j] : -1;
    cm[h] = ballot64(cand[h]);
    count += __popcll(cm[h]);
  }
  if (count == 0) return -1;
  // does the row of slot rf have a non-zero entry in a candidate column?
  auto touches = [&](int rf) {
    const u64 *m = S.nzm + (size_t)rf * NM;
    u64 t = 0;
#pragma unroll
    for (int h = 0; h < NM; h++) t |= m[h] & cm[h];
    return t != 0;
  };
  for (int k0 = 0; k0 < nligne && count > 1; k0 += 64) {
    const int k = k0 + lane;
    bool rel = false;
    if (k < nligne && k != pivi) {
      const int rf = S.ref[k];
      if (!(rf & UNITBIT)) rel = touches(rf);
    }
    u64 relmask = ballot64(rel);
    while (relmask && count > 1) {
      const int kk = k0 + __ffsll((long long)relmask) - 1;
      relmask &= relmask - 1;
      const int sl = S.ref[kk];
      // unit rows above kk knock out their own column
      int nel = 0;
#pragma unroll
      for (int h = 0; h < NV; h++) nel += __popcll(ballot64(cand[h] && u[h] < kk));
      if (nel == count) goto last_unit_wins;
      if (nel) {
#pragma unroll
        for (int h = 0; h < NV; h++) {
          if (u[h] < kk) cand[h] = false;
          cm[h] = ballot64(cand[h]);
        }
        count -= nel;
        if (count == 1) break;
      }
      if (!touches(sl)) continue;  // cannot separate them
      // real row kk: keep the minimal ratios
      typename F::Row n;
      F::load(n, vals + (size_t)sl * W, lane, W);
      for (;;) {
        // reference column b = first remaining candidate
        int cb = NV - 1;
#pragma unroll
        for (int h = NV - 2; h >= 0; h--)
          if (cm[h]) cb = h;
        const int src = __ffsll((long long)cm[cb]) - 1;
        const E ab = lean_entry<F>(a, cb, src), nb = lean_entry<F>(n.v, cb, src);
        bool neg[NV];
        int nneg = 0, nzero = 0;
#pragma unroll
        for (int h = 0; h < NV; h++) {
          bool xneg, xzero;
          F::template cross<SMALL>(ab, n.v[h], nb, a[h], xneg, xzero);
          neg[h] = cand[h] && xneg;
          const bool zero = cand[h] && xzero;
          nneg += __popcll(ballot64(neg[h]));
          nzero += __popcll(ballot64(zero));
          if (!neg[h] && !zero) cand[h] = false;  // strictly larger: out
        }
        if (nneg == 0) {
          count = nzero;
        } else {
#pragma unroll
          for (int h = 0; h < NV; h++) cand[h] = neg[h];
          count = nneg;
        }
#pragma unroll
        for (int h = 0; h < NV; h++) cm[h] = ballot64(cand[h]);
        if (nneg == 0 || count == 1) break;
      }
    }
  }
  if (count == 1) {
#pragma unroll
    for (int h = 0; h < NV; h++)
      if (cm[h]) return F::col(__ffsll((long long)cm[h]) - 1, h);
  }
last_unit_wins:
  // only unit rows left to look at: the column whose unit row comes last survives
  if (lane == 0) sc->tmp2 = -1;
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int h = 0; h < NV; h++)
    if (cand[h]) atomicMax(&sc->tmp2, (u[h] << 10) | F::col(lane, h));
  __builtin_amdgcn_wave_barrier();
  return sc->tmp2 & 1023;
}

// ---- the determinant replay in a lean launch's spare workgroups.  pipamd_batch_solve's second lean launch has a block
// per tableau of the batch and a list of the few the first launch paused: block nq + r (r = 0 .. ceil(njobs / 64) - 1) takes
// the jobs 64 r .. 64 r + 63, a lane each, and replays the logs of those that are finished (PIPAMD_ST_SOLUTION, _NIL)
// with the one-lane walk of pip_det_replay_lanes_kernel -- beside the launch's own jobs, not behind them on the queue.
// The jobs on the launch's list belong to its list blocks, which may finish them at any moment: the block reads the
// whole list first (it does not change during the launch) and leaves every listed job alone, whatever its status says
// by now.  So no job has two writers.  What the spare blocks do not reach (a list longer than the batch minus the
// blocks needed) is left to the replay behind the launches, for which an empty log is a no-op.
// `lds`: 8 bytes of the block's LDS image, which a spare block does not use otherwise.
template <class T>
__device__ __forceinline__ void lean_spare_replay(PipJob *jobs, i64 *arena, int njobs, const int *in_list, int nq, int r,
                                                  unsigned char *lds) {
  if (r >= (njobs + 63) / 64) return;
  const int lane = threadIdx.x;
  u64 *listed = (u64 *)lds;
  if (lane == 0) *listed = 0;
  __builtin_amdgcn_wave_barrier();
  for (int i = lane; i < nq; i += 64) {
    const int v = in_list[i];
    if ((v >> 6) == r) atomicOr((unsigned long long *)listed, 1ull << (v & 63));
  }
  __builtin_amdgcn_wave_barrier();
  const int j = 64 * r + lane;
  if (j >= njobs || ((*listed >> lane) & 1)) return;
  PipJob *J = &jobs[j];
  const int st = J->status;
  if (st != PIPAMD_ST_SOLUTION && st != PIPAMD_ST_NIL) return;
  det_replay_lane<T, PIP_LEAN_REPLAY_CH>(J, arena);
}

#ifdef PIP_PROFILE
#define PIP_LEAN_PROF_PARAM , u64 *prof
#else
#define PIP_LEAN_PROF_PARAM
#endif

// ---- the entry points.  The loop below is the body of both kernels, as text: a kernel names its flavour F, its row
// capacity Smax / Lmax and FULL, then includes this header once more with PIP_LEAN_LOOP defined.  (A __forceinline__
// function template would read better and costs pip_lean_kernel its register budget: the same text inlined through a
// call spills three VGPRs to scratch with this compiler)  pip_lean_kernel<SC, FULL> is here, one
// instantiation per row-capacity class (pip_adv_e.hip); pip_lean64_kernel, not a template, is in the translation unit
// that launches it (pip_kernels.hip).
// FULL: 127 unknowns + constant, a row fills the wave's 128 columns (the launcher's promise, as for pip_advance_kernel);
// else any number of unknowns up to 127 without parameters, rows of W <= 128 columns (W even).
// BIG (FULL == false only): one parameter, the big one, in column nvar + 1; up to 126 unknowns.
// NW: waves per tableau.  1: the kernel of the bulk launches (64 VGPRs, eight waves per SIMD).  4: for a launch over a few
// hundred paused tableaux (pipamd_batch_solve's second lean launch), where a wave has its SIMD to itself whatever the
// kernel needs and the launch lasts as long as one tableau's dependent chain: the row-parallel parts of that chain --
// the entry pass, the row loop of phase B, phase C, the widening of the epilogue -- are spread over the waves the way
// pip_advance_kernel spreads them (wave v: rows v, v + NW, ...; barriers as there), choisir_piv and the cut stay on
// wave 0, and every wave holds the pivot row in its own registers.  What decides an exit from the loop is wave-uniform
// at every point where it is tested: read from LDS behind a barrier (LeanWaves, Scalars) or counted alike by every wave.
// Same bits as one wave: a row's new value does not depend on which wave computes it.
struct LeanWaves {
  int mcw;      // largest magnitude class any wave has published (atomicMax; never lowered)
  int wide;     // entry pass: some wave met a row beyond the packed elements
  int verdict;  // integrer(): what wave 0 decided about the cut
};
template <int SC, bool FULL, bool BIG = false, int NW = 1>
__global__ __launch_bounds__(64 * NW, NW == 1 ? PIP_LEAN_WAVES : 2) void pip_lean_kernel(PipJob *jobs, i64 *arena, int njobs,
                                                                                         int iter_limit,
                                                                                         PipQueue q PIP_LEAN_PROF_PARAM) {
  static_assert(NW == 1 || (NW == 4 && !BIG), "four waves per tableau: the plain flavour only");
  typedef LeanIntRows F;
  constexpr int Smax = SC, Lmax = SC + 128;
#define PIP_LEAN_LOOP
#include "pip_lean.h"
#undef PIP_LEAN_LOOP
}
template <int SC, bool FULL, bool BIG = false, int NW = 1>
hipError_t launch_lean(const AdvanceLaunch &a) {
  const int grid = a.grid > 0 && a.grid < a.njobs ? a.grid : a.njobs;
  const size_t shm = lean_lds_bytes(SC);
#ifdef PIP_PROFILE
  hipLaunchKernelGGL((pip_lean_kernel<SC, FULL, BIG, NW>), dim3(grid), dim3(64 * NW), shm, a.stream, a.jobs, a.arena, a.njobs,
                     a.iter_limit, a.q, (u64 *)a.prof);
#else
  hipLaunchKernelGGL((pip_lean_kernel<SC, FULL, BIG, NW>), dim3(grid), dim3(64 * NW), shm, a.stream, a.jobs, a.arena, a.njobs,
                     a.iter_limit, a.q);
#endif
  return hipGetLastError();
}
// the classes that also come with four waves per tableau (pipk_lean_waves_class, pip_kernels.hip)
#define PIP_LEAN4_CLASSES(X) X(128, true) X(160, true) X(128, false) X(160, false)
#define PIP_LEAN4_DEFINE(SC, FULL) template hipError_t launch_lean<SC, FULL, false, 4>(const AdvanceLaunch &);
// the row-capacity classes of launch_static (pip_kernels.hip)
#define PIP_LEAN_CLASSES(X) \
  X(64, true) X(96, true) X(112, true) X(128, true) X(160, true) X(64, false) X(96, false) X(112, false) X(128, false) X(160, false)
#define PIP_LEAN_DEFINE(SC, FULL) template hipError_t launch_lean<SC, FULL>(const AdvanceLaunch &);
// ... and of the BIG flavour (run-time column counts only)
#define PIP_LEAN_BIG_CLASSES(X) X(64) X(96) X(112) X(128) X(160)
#define PIP_LEAN_BIG_DEFINE(SC) template hipError_t launch_lean<SC, false, true>(const AdvanceLaunch &);

#elif defined(PIP_LEAN_LOOP)
// ---- The lean pivot loop: the body of a kernel (jobs, arena, njobs, iter_limit, q[, prof]) that has named F (the row
// flavour), Smax / Lmax (the row capacity of its LDS image, compile-time or not) and FULL.
// (diagnostic build only, tools/dbg_prof_lean.py and dbg_prof_lean64.py: cycle stamps per piece of the loop -- 0
// exam/integrer, 1 pivot row load, 2 choisir_piv, 3 work list, 4 queue + recycled slot, and the barrier after the
// last row, 5 wait for a work row, 6 multipliers, 7 products + row gcd + division, 8 store + summary, 9 phase C,
// 10 entry, 11 epilogue)
  typedef typename F::T T;
  typedef typename F::E E;
  typedef typename F::Row Row;
  PROF_DECL;
  constexpr int WP = F::WP, NM = F::NM, NV = F::NV;
  constexpr int NT = 64 * NW;  // (NW: waves per tableau, named by the kernel like F; every wave-index term below folds away at 1)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ Scalars sc;
  [[maybe_unused]] __shared__ LeanWaves lw;  // (NW > 1 only)
  const int nq = q.in_count ? *q.in_count : njobs;
  if ((int)blockIdx.x >= nq) {
    // a launch sized by the batch over a shorter list: the first blocks beyond the list do the determinant bookkeeping
    // of the jobs the earlier launch finished, beside this launch's own jobs (PipQueue.replay_spare).  (64 jobs a block,
    // a lane each, whatever the block size: the first wave does it.)
    if constexpr (sizeof(T) == 8)
      if ((NW == 1 || threadIdx.x < 64) && q.replay_spare && q.in_list)
        lean_spare_replay<T>(jobs, arena, njobs, q.in_list, nq, (int)blockIdx.x - nq, smem);
    return;
  }
  const int jb = q.in_list ? q.in_list[blockIdx.x] : (int)blockIdx.x;
  PipJob *J = &jobs[jb];
  const int tid = threadIdx.x;
  const int lane = NW > 1 ? (tid & 63) : tid;
  const int wave = NW > 1 ? __builtin_amdgcn_readfirstlane(tid >> 6) : 0;
  if (J->status != PIPAMD_ST_RUN) {
    if (J->status == PIPAMD_ST_CAPACITY && q.out_count && tid == 0) {
      q.out_list[atomicAdd(q.out_count, 1)] = jb;
      atomicMax(q.out_maxni, PIPAMD_Q_CAPFLAG | J->ni);
      atomicAdd(q.out_maxni + 1, 1);  // (the list's third control word: tableaux out of rows)
    }
    return;
  }
  int tflags = J->tflags;
  int ni = J->ni;
  const int nvar = FULL ? 127 : J->nvar, W = FULL ? 128 : J->W;
  int nligne = nvar + ni;
  // what this kernel does not do stays with pip_advance_kernel: the job goes on the launch list untouched
  const bool mine = (BIG ? F::shape_big(J, nvar, W) : F::shape(J, nvar, W)) && !(tflags & (PIPAMD_T_NOSKIP | PIPAMD_T_DEEPEST)) && ni <= Smax && nligne <= Lmax &&
                    (!(tflags & PIPAMD_T_STATE) || J->state_nch == F::NCH);
  if (!mine) {
    if (tid == 0 && q.out_count) {
      q.out_list[atomicAdd(q.out_count, 1)] = jb;
      atomicMax(q.out_maxni, ni);
    }
    return;
  }
  T *vals = (T *)(arena + uni((i64)J->vals_off));
  // (what only the prologue and the epilogue need -- the row tables in HBM, the saved summaries, the counters -- is
  // derived from the job header where it is used, so that it holds no scalar registers across the pivot loop)
  const int ncut0 = J->ncut - ni;  // cuts so far = ncut0 + ni (every row this kernel appends is a cut)
  // (wave-uniform, but loaded through vector memory: pinned to scalar registers, the pivot loop needs the vector ones)
  const int cap_ni = __builtin_amdgcn_readfirstlane(min(J->S, J->L - nvar));  // rows the job's block holds
  int npiv = J->npiv, nupd = J->nupd;
  T *g_log = (T *)(arena + uni((i64)J->log_off));
  constexpr int LOGCAP = PIPAMD_DETLOG;
  int nlog = J->nlog;

  Shared<T> S;  // the tables of pip_advance_kernel's image this kernel uses
  E *cst;       // [S] constant terms (packed elements here); the entry-time sort keys share their storage
  {
    unsigned char *p = smem;
    S.den = (T *)p;      p += sizeof(T) * Smax;
    S.nzm = (u64 *)p;    p += sizeof(u64) * (size_t)Smax * NM;
    cst = (E *)p;
    S.size = (float *)p; p += sizeof(E) * Smax;
    S.prow = nullptr;
    S.cst = nullptr;
    S.sig = (u16 *)p;    p += sizeof(u16) * Smax;
    S.srow = (u16 *)p;   p += sizeof(u16) * Smax;
    S.work = (u16 *)p;   p += sizeof(u16) * Smax;
    S.ref = (u16 *)p;    p += sizeof(u16) * Lmax;
    S.urow = (u16 *)p;   p += sizeof(u16) * WP;
    S.fl = (u8 *)p;      p += Smax;
    S.nf = (u8 *)p;      p += Smax;
    S.rcls = (u8 *)p;    p += Smax;
  }

  // ---- the row tables (the sort keys share storage with the constant terms here: not zeroed)
  for (int j = tid; j < WP; j += NT) S.urow[j] = NOROW;
  if (tid == 0) {
    reset_scalars(sc);
    if constexpr (NW > 1) lw = LeanWaves{0, 0, 0};
  }
  bsync<NW>();
  stage_row_tables<T, NT, false>(S, pip_row_tables<const T>(arena + J->rows_off, J->L), nligne, tid);
  bsync<NW>();

  // ---- one pass over the tableau: the rows become packed (int rows of a job loaded with PIPAMD_T_ROWS_STAY come from
  // the caller's array), summaries, sort keys.  A row with an entry of 2^ROW_BITS or more: not a job for this kernel.
  int mcw = 0;  // largest magnitude class published so far: 0 small path everywhere, 1 packed rows, beyond: the lean run ends
  {
    constexpr int PF0 = F::ENTRY_PF, CPL = ET<T>::CPL;
    // a job that paused in an earlier launch (this kernel's or pip_advance_kernel's, rows in the general format): what the
    // entry pass cannot see in the rows -- "gcd(row, denominator) is known to be 1" -- comes from the saved summaries
    const u16 *g_sig = (tflags & PIPAMD_T_STATE) ? saved_summaries(arena + J->state_off, J->S, NM).sig : nullptr;
    const bool fresh = F::FRESH && (tflags & PIPAMD_T_FRESHROWS) != 0;
    const T *src = fresh ? (const T *)(uintptr_t)J->src_rows : vals;
    constexpr int NCOL1 = BIG ? 2 : 1;  // columns behind the unknowns: the constant (BIG: and the big parameter's)
    const int pitch = fresh ? nvar + NCOL1 : W;  // the caller's rows are that wide (an even number: pipamd_batch_load), the block's W
    int npacked = 0;
    bool wide = false;
    // (wave v of NW: rows v, v + NW, ...)
    for (int s0 = 0; wave + NW * s0 < ni && !wide; s0 += PF0) {
      RowRegs<T, F::NCH> rr[PF0];
#pragma unroll
      for (int qq = 0; qq < PF0; qq++)
        if (wave + NW * (s0 + qq) < ni)
          row_load<T, F::NCH>(rr[qq], src + (size_t)(wave + NW * (s0 + qq)) * pitch, (nvar + NCOL1 - 1 + CPL) & ~(CPL - 1), lane);
#pragma unroll
      for (int qq = 0; qq < PF0; qq++) {
        const int s = wave + NW * (s0 + qq);
        if (s >= ni || wide) break;
        typename ET<T>::U mx = 0;
        Row z;
#pragma unroll
        for (int h = 0; h < NV; h++) {
          const T v = rr[qq].v[h / CPL][h % CPL];
          mx |= uabs(v);
          z.v[h] = (E)v;
        }
        if (ballot64((mx >> F::ROW_BITS) != 0)) {  // not below 2^ROW_BITS in magnitude
          wide = true;
          break;
        }
        F::store(z, vals + (size_t)s * W, lane, W);
        npacked = s + 1;
        const bool den1 = S.den[s] == 1;
        const int red = g_sig ? (g_sig[s] & SIG_RED) : (den1 ? SIG_RED : 0);
        mcw = max(mcw, lean_publish<F, BIG>(z, S, cst, s, -1, red, lane, nvar));
        if (tflags & PIPAMD_T_SORT) {
          // traiter.c:576-589: size = max_j |(int)(v_j / den)| over the unknowns (as pip_advance_kernel computes it)
          int sz = 0;
          const double d = to_double(S.den[s]);
#pragma unroll
          for (int h = 0; h < NV; h++) {
            const E v = z.v[h];
            const int q2 = !den1 ? trunc_x86((double)v / d) : (v == (E)(int)v ? (int)v : (int)0x80000000);
            const int aq = q2 < 0 ? (int)(0u - (unsigned)q2) : q2;
            if (F::col(lane, h) < nvar) sz = sz > aq ? sz : aq;
          }
          const unsigned szw = wave_minmax_u32<true>((unsigned)sz);
          if (lane == 0) {
            S.size[s] = (float)szw;
            if ((int)S.srow[s] >= nvar) atomicMax(&sc.smaxbits, (u64)szw);
          }
        }
      }
    }
    if constexpr (NW > 1) {
      // what the waves found, each in its own rows: known to all of them behind the barrier
      if (lane == 0) {
        if (wide) lw.wide = 1;
        if (mcw) atomicMax(&lw.mcw, mcw);
      }
      __syncthreads();
      wide = lw.wide != 0;
      mcw = lw.mcw;
    }
    if (wide) {
      // an entry beyond E: not a job for this kernel.  Its header is untouched (FRESHROWS and SORT still stand); rows
      // that came from the block itself and were already packed are widened again (by the wave that packed them).
      if (!fresh) rows_unpack<F>(vals, npacked, lane, W, S.rcls, wave, NW);
      if (tid == 0 && q.out_count) {
        q.out_list[atomicAdd(q.out_count, 1)] = jb;
        atomicMax(q.out_maxni, ni);
      }
      return;
    }
  }
  if constexpr (F::FRESH) tflags &= ~PIPAMD_T_FRESHROWS;
  if constexpr (NW == 1) __builtin_amdgcn_wave_barrier();  // (NW > 1: the barrier above)
  if (tflags & PIPAMD_T_SORT) {
    if (NW == 1 || wave == 0)
      [[clang::always_inline]] sort_rows(S, nvar, nligne, (double)sc.smaxbits);  // (left to the inliner, sort_rows<__int128> stays a call: scratch)
    bsync<NW>();
    for (int i = tid; i < nligne; i += NT)
      if (!(S.ref[i] & UNITBIT)) S.srow[S.ref[i]] = (u16)i;
    tflags &= ~PIPAMD_T_SORT;
    // the sort keys overwrote the constant terms: back from the rows (column nvar)
    __threadfence_block();
    for (int s = tid; s < ni; s += NT) cst[s] = reinterpret_cast<const E *>(vals + (size_t)s * W)[nvar];
    bsync<NW>();
  }
  first_chercher<T, NT>(S, &sc, ni, BIG ? nvar + 1 : -1, tid);
  bsync<NW>();

  PROF(10);
  int status = PIPAMD_ST_RUN;
  int why = 0;  // why a job left this kernel unfinished (PipJob.pad_, read by tools/lean_split.py): 1 pivot budget,
                // 2 a row beyond E, 3 a cut's denominator, 5 no room in the LDS image
  for (int iter = 0;; iter++) {
    why = 1;
    if (iter >= iter_limit) break;  // status stays RUN: the next launch resumes the job
    if (nlog >= LOGCAP) break;
    why = 2;
    if (mcw > 1) break;  // a row left E (it is stored in the general format): the general kernel goes on
    why = 0;
    int pivi = sc.pivi;
    Row pr;                // the pivot row
    bool have_pr = false;  // ... is in registers already: the cut integrer() has just built and stored
    if (pivi == BIG_I) {
      // -------------- exam_coef (its flags were prepared by phase C), then integrer if nothing is negative
      if constexpr (BIG) {
        // exam_coef with a big parameter (traiter.c:107-157), as pip_advance_kernel runs it: the first Unknown row whose big
        // coefficient is negative, else the constants
        [[clang::always_inline]] pivi = exam_rows<T, 1>(S, &sc, ni);
      } else {
        pivi = sc.pivi2;
        apply_exam_flags<T, NT>(S, ni, pivi, tid);
        bsync<NW>();
      }
      if (pivi == BIG_I) {
        // (BIG: the one parameter is the big one, so exam_rows has decided every row -- a negative big coefficient, else a
        // positive one, else the constant -- and pip_advance_kernel's test for rows left Unknown, PIPAMD_ST_NEED_COMPA, has
        // nothing to find: it is not repeated here)
        if (!(tflags & PIPAMD_T_INT)) {
          status = PIPAMD_ST_SOLUTION;
          break;
        }
        // ------------- integrer(): first non-integral row among the unknowns (integrer.c:305-486, constant cuts)
        if (tid == 0) sc.tmp = BIG_I;
        bsync<NW>();
        for (int i = tid; i < nvar; i += NT) {
          const int rf = S.ref[i];
          if (rf & UNITBIT) continue;
          const T D = S.den[rf];
          if (D == 1) continue;
          if (wneg(fmod64(wneg((T)cst[rf]), D)) != 0) atomicMin(&sc.tmp, i);
        }
        bsync<NW>();
        const int ci = sc.tmp;
        if (ci == BIG_I) {
          status = PIPAMD_ST_SOLUTION;
          break;
        }
        const int cslot = S.ref[ci];
        const T DT = uni(S.den[cslot]);
        why = 3;
        if (DT <= 0 || DT >= ((T)1 << F::CUT_BITS)) break;  // the cut's entries (below D) might not fit E: the general kernel goes on
        const E D = (E)DT;
        int verdict = PIPAMD_ST_RUN;
        if (NW == 1 || wave == 0) {  // (several waves: the first builds and appends the cut)
          Row &r = pr;  // (PIP_LEAN_KEEPCUT: the cut is the next pivot row)
          F::load(r, vals + (size_t)cslot * W, lane, W);
          F::row_mod(r, D, S.rcls[cslot] == 0);
          bool okv = false;
#pragma unroll
          for (int h = 0; h < NV; h++) {
            const E pos = r.v[h];
            if (F::col(lane, h) < nvar)
              okv |= pos > 0;
            else
              r.v[h] = pos ? pos - D : 0;  // -((-v) mod D) == (v mod D) - D unless D divides v
            if constexpr (BIG)
              if (F::col(lane, h) == nvar + 1) r.v[h] = 0;  // the big parameter is divisible by any number (integrer.c:373-377)
          }
          const bool any_v = ballot64(okv) != 0;
          if (!any_v)
            verdict = PIPAMD_ST_NIL;  // integrer.c:482-485 case (b)
          else if (ni >= cap_ni)
            verdict = PIPAMD_ST_CAPACITY;
          else if (ni >= Smax || nligne >= Lmax)
            verdict = -1;  // no room in this launch's LDS image: pause
          else {
            verdict = PIPAMD_ST_RUN;
            F::store(r, vals + (size_t)ni * W, lane, W);
            mcw = max(mcw, lean_publish<F, BIG>(r, S, cst, ni, -1, 0, lane, nvar));
            if (lane == 0) {
              S.fl[ni] = PIPAMD_F_MINUS;
              S.nf[ni] = 0;
              S.den[ni] = DT;
              S.ref[nligne] = (u16)ni;
              S.srow[ni] = (u16)nligne;
            }
          }
          if (lane == 0) {
            sc.aux = ci;
            if constexpr (NW > 1) lw.verdict = verdict;
          }
        }
        bsync<NW>();  // (several waves: the cut's row is stored and its tables are written before another wave looks)
        if constexpr (NW > 1) verdict = lw.verdict;
        why = 5;
        if (verdict != PIPAMD_ST_RUN) {
          status = verdict < 0 ? PIPAMD_ST_RUN : verdict;
          break;
        }
        pivi = nligne;
        ni++;
        nligne++;
        have_pr = PIP_LEAN_KEEPCUT != 0 && (NW == 1 || wave == 0);
      }
    }
    PROF(0);
    // ---------------- A: pivot row, choisir_piv, work list
    const int pslot = S.ref[pivi];
    const T dpiv = uni(S.den[pslot]);
    // small path for a row: the row and the pivot row in class 0 and the pivot row's denominator below 2^CLS0_BITS (then
    // the multipliers are below it as well and every product fits E)
    const bool psmall = S.rcls[pslot] == 0 && dpiv > -((T)1 << F::CLS0_BITS) && dpiv < ((T)1 << F::CLS0_BITS);
    npiv++;
    if (!have_pr) F::load(pr, vals + (size_t)pslot * W, lane, W);
    const int psig_v = S.sig[pslot];
#ifdef PIP_PROFILE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    PROF(1);
    int pj = -1;
    if (NW == 1 || wave == 0)
      pj = mcw == 0 ? lean_choose_column<F, true>(S, pr, vals, W, nvar, nligne, pivi, &sc)
                    : lean_choose_column<F, false>(S, pr, vals, W, nvar, nligne, pivi, &sc);
    if constexpr (NW > 1) {
      // the first wave chose the column and lists the rows; the others have asked for the pivot row meanwhile (its slot
      // is rewritten only behind this barrier, their loads are issued ahead of it: the order __syncthreads() keeps
      // within a workgroup)
      if (wave == 0) {
        int nw0 = 0;
        if (pj != -1) nw0 = pivot_work_list<T, NM>(S, ni, pslot, F::val_of(pj), F::lane_of(pj), false, lane);
        if (lane == 0) {
          sc.pivj = pj;
          sc.nwork = nw0;
        }
      }
      __syncthreads();
      pj = sc.pivj;
    }
    if (pj == -1) {  // traiter.c:782-785
      status = PIPAMD_ST_NIL;
      break;
    }
    PROF(2);
    const int pe = F::val_of(pj), pl = F::lane_of(pj);
    int nwork;
    if constexpr (NW > 1) {
      nwork = sc.nwork;
    } else {
      nwork = pivot_work_list<T, NM>(S, ni, pslot, pe, pl, false, lane);
      __builtin_amdgcn_wave_barrier();
    }
    if (tid == 0) {  // phase C refills them
      sc.pivi = BIG_I;
      sc.pivi2 = BIG_I;
    }
    const int pivj = pj;
    const E pivot = lean_entry<F>(pr.v, pe, pl);
    if (tid == 0) {
      g_log[2 * nlog] = (T)pivot;
      g_log[2 * nlog + 1] = dpiv;
    }
    nlog++;
    const int ku = S.urow[pivj];  // unit row of the entering column
    const int pred = psig_v & SIG_RED;
    PROF(3);
    // ---------------- B: eliminate the pivot column
    nupd += nwork - 1;  // (counted alike by every wave)
    // wave v of NW takes entries v, v + NW, ... of the work list: entry w of its share is entry wave + NW * w of the list
    const int nmine = NW == 1 ? nwork : (nwork - wave + NW - 1) / NW;
    {
      // a queue of PF rows on their way from HBM / L2: the row at its head is updated while the loads behind it are in
      // flight
      constexpr int PF = F::PF;
      Row rq[PF];
      int sq[PF];
      // (F::PREP) the wave-uniform part of every row's update, for the first 64 rows of the work list, one row per lane
      // (lean_prepare_rows): the gather of the pivot column goes out ahead of the queue's loads
      E m_lp = 0, m_foo = 0;
      T m_g0 = 0;
      typename F::G m_gs = 0;
      u64 m_small = 0;
      int pk = 0;
      bool pact = false;
      E pf = 0;
      if constexpr (F::PREP) {
        pk = S.work[lane < nmine ? wave + NW * lane : 0];
        pact = lane < nmine && pk != pslot;
        if (pact) pf = F::gather(vals + (size_t)pk * W, pivj);
      }
#pragma unroll
      for (int q2 = 0; q2 < PF; q2++) {
        sq[q2] = S.work[q2 < nmine ? wave + NW * q2 : 0];
        if (q2 < nmine && sq[q2] != pslot) F::load(rq[q2], vals + (size_t)sq[q2] * W, lane, W);
      }
      // while the first rows are on their way: the pivot slot is recycled for the row replacing ku's unit row
      // (traiter.c:461-465,503-513) -- it needs no load, the pivot row is in registers (several waves: the first does it)
      if (NW > 1 && wave != 0) {
        // (the first wave's)
      } else if (F::fits(dpiv)) {
        Row r;
#pragma unroll
        for (int h = 0; h < NV; h++) r.v[h] = (F::col(lane, h) == pivj) ? (E)dpiv : (E)wneg((i64)pr.v[h]);
        F::store(r, vals + (size_t)pslot * W, lane, W);
        mcw = max(mcw, lean_publish<F, BIG>(r, S, cst, pslot, pivj, pred, lane, nvar));
      } else {  // the denominator does not fit E: that row does not either
        T zw[NV];
#pragma unroll
        for (int h = 0; h < NV; h++) zw[h] = (F::col(lane, h) == pivj) ? dpiv : -(T)pr.v[h];
        F::store_wide(zw, vals + (size_t)pslot * W, lane, W);
        mcw = max(mcw, lean_publish_wide<F, BIG>(zw, S, cst, pslot, pivj, pred, lane, nvar));
      }
      PROF(4);
      for (int w = 0; w < nmine; w++) {
        if constexpr (F::PREP) {
          if ((w & 63) == 0) {
            if (w) {  // (more than 64 work rows: the next 64)
              pk = S.work[w + lane < nmine ? wave + NW * (w + lane) : 0];
              pact = w + lane < nmine && pk != pslot;
              if (pact) pf = F::gather(vals + (size_t)pk * W, pivj);
            }
            m_small = lean_prepare_rows<F>(S, pk, pact, pf, pivot, dpiv, psmall, m_lp, m_foo, m_g0, m_gs);
          }
        }
        const int s = sq[0];
        Row r = rq[0];
#pragma unroll
        for (int q2 = 0; q2 + 1 < PF; q2++) {
          rq[q2] = rq[q2 + 1];
          sq[q2] = sq[q2 + 1];
        }
        if (w + PF < nmine) {
          sq[PF - 1] = S.work[wave + NW * (w + PF)];
          if (sq[PF - 1] != pslot) F::load(rq[PF - 1], vals + (size_t)sq[PF - 1] * W, lane, W);
        }
        T *row = vals + (size_t)s * W;
        if (s == pslot) continue;
#ifdef PIP_PROFILE
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PF - 1) : "memory");
#endif
        PROF(5);
        // multipliers from the row's own pivot-column entry (traiter.c:470-476); packed elements
        E foo, lp;
        T g0;
        typename ET<T>::U gs = 0;  // where the row gcd starts (0: from |g0|)
        bool small;
        if constexpr (F::PREP) {  // prepared by the row's lane
          const int k = w & 63;
          foo = lean_lane(m_foo, k);
          lp = lean_lane(m_lp, k);
          g0 = lean_lane(m_g0, k);
          gs = lean_lane(m_gs, k);
          small = (m_small >> k) & 1;
        } else {
          foo = lean_entry<F>(r.v, pe, pl);
          const T den_s = uni(S.den[s]);
          lp = pivot;
          g0 = den_s;
          if (pivot != 1) {
            const auto d = F::gcd(pivot, foo);
            if (d != 1) {  // (d == 0 cannot be: pivot > 0)
              lp = (E)exact_quo<i64>((i64)pivot, (i64)d);
              foo = (E)exact_quo<i64>((i64)foo, (i64)d);
            }
            g0 = wmul((T)lp, den_s);
          }
          small = psmall && S.rcls[s] == 0 && F::small_den(g0);
        }
        T nd;
        PROF(6);
        if (small) {
          if (!F::update_small(r, pr, lp, foo, dpiv, pivj, g0, gs, lane, nd)) {
            if (lane == 0) sc.bad = 1;
          }
          PROF(7);
          F::store(r, row, lane, W);
          mcw = max(mcw, lean_publish<F, BIG>(r, S, cst, s, pivj, SIG_RED, lane, nvar));
        } else {
          T zw[NV];
          if (!F::update_mid(zw, r, pr, lp, foo, dpiv, pivj, g0, gs, lane, nd)) {
            if (lane == 0) sc.bad = 1;
          }
          typename ET<T>::U mx = 0;
#pragma unroll
          for (int h = 0; h < NV; h++) mx |= uabs(zw[h]);
          PROF(7);
          if (ballot64((mx >> F::ROW_BITS) != 0) == 0) {
#pragma unroll
            for (int h = 0; h < NV; h++) r.v[h] = (E)zw[h];
            F::store(r, row, lane, W);
            mcw = max(mcw, lean_publish<F, BIG>(r, S, cst, s, pivj, SIG_RED, lane, nvar));
          } else {  // not a packed row any more: general format, the lean run ends after this pivot
            F::store_wide(zw, row, lane, W);
            mcw = max(mcw, lean_publish_wide<F, BIG>(zw, S, cst, s, pivj, SIG_RED, lane, nvar));
          }
        }
        if (lane == 0) S.den[s] = nd;
        PROF(8);
      }
    }
    // (several waves: every row of this pivot is stored and summarised behind this barrier -- the ordering of
    // pip_advance_kernel's row loop -- and the largest class any wave published is every wave's from here on)
    if constexpr (NW > 1)
      if (lane == 0 && mcw) atomicMax(&lw.mcw, mcw);
    bsync<NW>();
    if constexpr (NW > 1) mcw = lw.mcw;
    PROF(4);
    if (sc.bad) {
      status = PIPAMD_ST_OVERFLOW;
      break;
    }
    // ---------------- C: swap roles, refresh the sign hints, next chercher (traiter.c:503-529)
    pivot_swap_roles<T, NT>(S, &sc, ni, pivi, pivj, pslot, ku, (T)pivot, BIG ? nvar + 1 : -1, tid);
    bsync<NW>();
    PROF(9);
  }

  // ---- epilogue: the row tables, the header and (if any) the solution
  bsync<NW>();
  publish_row_tables<T, NT>(S, pip_row_tables<T>(arena + J->rows_off, J->L), nligne, tid);
  tflags &= ~PIPAMD_T_STATE;
  if (status == PIPAMD_ST_RUN) {
    save_summaries<T, NT>(S, saved_summaries(arena + J->state_off, J->S, NM), ni, NM, tid);
    tflags |= PIPAMD_T_STATE;
  }
  if (status == PIPAMD_ST_SOLUTION) {
    // solution(), traiter.c:255-271: the constant column of rows 0..nvar-1
    // (BIG: two numerators per unknown, the big parameter's coefficient -- from the packed row in HBM -- then the constant)
    constexpr int NN = BIG ? 2 : 1;
    T *sol_num = (T *)(arena + J->sol_off);
    T *sol_den = sol_num + NN * nvar;
    if constexpr (BIG) __threadfence_block();
    for (int i = tid; i < nvar; i += NT) {
      const int rf = S.ref[i];
      T v = 0, d = 1;
      [[maybe_unused]] T bv = 0;
      if (!(rf & UNITBIT)) {
        v = (T)cst[rf];  // (the constant terms are kept current in LDS by lean_publish)
        d = S.den[rf];
        if constexpr (BIG) bv = (T)F::gather(vals + (size_t)rf * W, nvar + 1);  // (every row is a packed row here: mcw <= 1)
      }
      if constexpr (BIG) sol_num[NN * i] = bv;
      sol_num[NN * i + NN - 1] = v;
      sol_den[i] = d;
    }
  }
  if (status == PIPAMD_ST_RUN || status == PIPAMD_ST_CAPACITY) {
    // the job goes on elsewhere (pip_advance_kernel, pip_rehouse_kernel): its rows in the general format again
    rows_unpack<F>(vals, ni, lane, W, S.rcls, wave, NW);
  }
  const int mc = max_row_class(S, ni, lane);
  if constexpr (NW > 1) __syncthreads();  // (no wave reads the header any more: one lane rewrites it and lists the job)
  if (tid == 0) {
    // (the header still holds the counts the launch began with: a pivot it counted and did not log is the call of pivoter
    // that found no column and ended the job -- det_unlogged, pip_advance.h)
    const bool nocolumn = status == PIPAMD_ST_NIL && npiv - nlog != J->npiv - J->nlog;
    J->ni = ni;
    J->npiv = npiv;
    J->ncut = ncut0 + ni;
    J->nupd = nupd;
    J->nlog = nlog;
    J->pad_ = why;
    J->tflags = tflags;
    J->state_nch = F::NCH;
    J->maxabs = (u64)mc;
    J->aux = nocolumn ? PIPAMD_AUX_NOCOLUMN : sc.aux;
    J->status = status;
    if (status == PIPAMD_ST_RUN && q.out_count) {
      q.out_list[atomicAdd(q.out_count, 1)] = jb;
      atomicMax(q.out_maxni, ni);
    }
    if (status == PIPAMD_ST_CAPACITY && q.out_count) {
      q.out_list[atomicAdd(q.out_count, 1)] = jb;
      atomicMax(q.out_maxni, PIPAMD_Q_CAPFLAG | ni);
      atomicAdd(q.out_maxni + 1, 1);  // (the list's third control word: tableaux out of rows)
    }
  }
  PROF(11);
#ifdef PIP_PROFILE
  PROF_FLUSH(prof);
#endif
#endif  // PIP_LEAN_H / PIP_LEAN_LOOP
