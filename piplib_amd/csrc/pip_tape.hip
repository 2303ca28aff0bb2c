// piplib_amd/csrc/pip_tape.hip -- pipamd_tape_eval: a compiled solution tape (pip_tape.h) walked at many parameter
// points, one lane per point.
//
// A workgroup is TAPE_BLOCK lanes.  The parameters in scope of a lane -- its point's, then the new ones it computes
// (integrer.c:171-180) -- live in LDS, the slot the slow index and the lane the fast one: slot j of lane t is word
// j * TAPE_BLOCK + t (128-bit values: the low words of a slot in one row, the high words in the next), so the 8-byte
// accesses of neighbouring lanes fall on neighbouring banks and no lane holds an array it indexes at run time.  The
// program is staged behind the slots when both fit TAPE_LDS_BYTES (STAGED) and read from global memory otherwise.
//
// Lanes of a wave end up at different nodes.  A position only grows (pip_tape.h), so a wave serves, in every step, the
// LOWEST position any of its lanes is at: the lanes there execute the node, the others wait.  The node's words are then
// the same address for every lane -- a broadcast LDS read, or a scalar load --, a wave executes each node at most once,
// and lanes that took different branches meet again at the first node they share.  pip_tape_set_eval_kernel walks the
// programs of a set of tapes the same way, a tape per point, through the same walk (tape_walk).
//
// Arithmetic.  int64 cells: sum c_j theta_j + c is formed exactly -- a product of two int64 values is below 2^126; its
// signed high and unsigned low halves are summed apart (at most TAPE_MAX_SLOTS terms, nothing wraps) and joined at the
// end, as inst_constant does in pip_kernels.hip.  A condition needs the sign alone; a new parameter, and a numerator in
// lowest terms, must fit int64 (PIPAMD_ST_RANGE otherwise).  128-bit cells: every product and every running sum is
// checked against 128 bits in cell order, exactly, and the first that leaves them ends the point.
#include <hip/hip_runtime.h>

#include "../../include/piplib_amd.h"
#include "pip_tape.h"
#include "pip_wide.h"

namespace {
enum { END = 0x7fffffff };

// a / b and a % b, b > 0: the shared division with the native 64-bit path inside (one copy, out of line)
__device__ __forceinline__ PipDivMod tape_divmod(u128 a, u128 b) { return udivmod<true>(a, b); }
__device__ __forceinline__ u128 ugcd(u128 x, u128 y) {  // gcd(0, y) = y
  while (y) {
    const u128 r = tape_divmod(x, y).r;
    x = y;
    y = r;
  }
  return x;
}
// a * b in 128 bits; true where the product leaves them (exact: the magnitudes' halves)
__device__ __forceinline__ bool mul_leaves128(i128 a, i128 b, i128 *r) {
  if (fits64(a) && fits64(b)) {
    *r = a * b;
    return false;
  }
  const u128 ua = uabs(a), ub = uabs(b);
  const u64 ah = (u64)(ua >> 64), al = (u64)ua, bh = (u64)(ub >> 64), bl = (u64)ub;
  *r = 0;
  if (ah && bh) return true;
  const u128 cross = ah ? (u128)ah * bl : (u128)bh * al;
  if (cross >> 64) return true;
  const u128 low = (u128)al * bl, m = low + (cross << 64);
  if (m < low) return true;
  if ((a < 0) != (b < 0)) {
    if (m > ((u128)1 << 127)) return true;
    *r = (i128)((u128)0 - m);
  } else {
    if (m >> 127) return true;
    *r = (i128)m;
  }
  return false;
}

template <class T>
struct Width;
template <>
struct Width<i64> {
  enum { EW = 1 };
  static __device__ __forceinline__ i64 slot(const i64 *S, int j, int tid) { return S[j * TAPE_BLOCK + tid]; }
  static __device__ __forceinline__ void set_slot(i64 *S, int j, int tid, i64 v) { S[j * TAPE_BLOCK + tid] = v; }
  static __device__ __forceinline__ i64 word(const i64 *p, int k) { return p[k]; }
  static __device__ __forceinline__ void out(void *a, i64 at, i64 v) { ((i64 *)a)[at] = v; }
  static __device__ __forceinline__ bool fits(u128 mag, bool neg) { return neg ? mag <= ((u128)1 << 63) : (mag >> 63) == 0; }
};
template <>
struct Width<i128> {
  enum { EW = 2 };
  static __device__ __forceinline__ i128 slot(const i64 *S, int j, int tid) {
    return (i128)(((u128)(u64)S[(2 * j + 1) * TAPE_BLOCK + tid] << 64) | (u64)S[2 * j * TAPE_BLOCK + tid]);
  }
  static __device__ __forceinline__ void set_slot(i64 *S, int j, int tid, i128 v) {
    S[2 * j * TAPE_BLOCK + tid] = (i64)(u64)(u128)v;
    S[(2 * j + 1) * TAPE_BLOCK + tid] = (i64)(u64)((u128)v >> 64);
  }
  static __device__ __forceinline__ i128 word(const i64 *p, int k) { return (i128)(((u128)(u64)p[2 * k + 1] << 64) | (u64)p[2 * k]); }
  static __device__ __forceinline__ void out(void *a, i64 at, i128 v) {
    ((i64 *)a)[2 * at] = (i64)(u64)(u128)v;
    ((i64 *)a)[2 * at + 1] = (i64)(u64)((u128)v >> 64);
  }
  static __device__ __forceinline__ bool fits(u128 mag, bool neg) { return neg ? mag <= ((u128)1 << 127) : (mag >> 127) == 0; }
};

// sum n_j slot_j + n_P of the P + 1 values at `f`.  ok: the value is `v` (int64 cells: it fits 128 bits; 128-bit cells:
// no product and no running sum left them); neg: its sign (int64 cells: exact even where !ok)
struct FormValue {
  i128 v;
  bool ok, neg;
};
__device__ __forceinline__ FormValue form_value(const i64 *f, int P, const i64 *S, int tid, i64 *) {
  i128 hi = 0;
  u128 lo = 0;
  for (int j = 0; j < P; j++) {
    const i128 p = (i128)f[j] * (i128)S[j * TAPE_BLOCK + tid];
    hi += (i128)(i64)(p >> 64);
    lo += (u128)(u64)(u128)p;
  }
  const i64 c = f[P];
  hi += (i128)(c >> 63);
  lo += (u128)(u64)c;
  hi += (i128)(u64)(lo >> 64);
  FormValue r;
  r.ok = fits64(hi);
  r.neg = hi < 0;
  r.v = (i128)(((u128)hi << 64) | (u64)lo);
  return r;
}
__device__ __forceinline__ FormValue form_value(const i64 *f, int P, const i64 *S, int tid, i128 *) {
  i128 acc = 0;
  bool bad = false;
  for (int j = 0; j < P; j++) {
    i128 p;
    bad = bad || mul_leaves128(Width<i128>::word(f, j), Width<i128>::slot(S, j, tid), &p);
    bad = bad || __builtin_add_overflow(acc, p, &acc);
  }
  bad = bad || __builtin_add_overflow(acc, Width<i128>::word(f, P), &acc);
  FormValue r;
  r.ok = !bad;
  r.neg = acc < 0;
  r.v = acc;
  return r;
}

// floor(v / D), D > 0; false where it does not fit T
template <class T>
__device__ __forceinline__ bool floor_div(i128 v, T D, T *q) {
  const PipDivMod d = tape_divmod(uabs(v), (u128)D);
  const bool neg = v < 0;
  const u128 uq = d.q + (neg && d.r ? 1 : 0);
  if (!Width<T>::fits(uq, neg)) return false;
  *q = neg ? (T)((u128)0 - uq) : (T)uq;
  return true;
}
// N / D in lowest terms -- N negated first where `flip` --, D > 0 ((0, 1) for N == 0); false where the numerator does
// not fit T.  (The magnitude of the most negative i128 is itself; flipping it leaves 128 bits, and no T holds it.)
template <class T>
__device__ __forceinline__ bool lowest_terms(i128 N, bool flip, T D, T *num, T *den) {
  const u128 mag = uabs(N), g = ugcd(mag, (u128)D);
  const u128 qn = tape_divmod(mag, g).q, qd = tape_divmod((u128)D, g).q;
  const bool neg = flip ? N > 0 : N < 0;
  if (flip && mag == ((u128)1 << 127)) return false;
  if (!Width<T>::fits(qn, neg)) return false;
  *num = neg ? (T)((u128)0 - qn) : (T)qn;
  *den = (T)qd;
  return true;
}

// The results of a launch, and where a point's go: unknown i of point pt is value pt * xs + i, dual value i is
// pt * ds + i (one tape: its own nvar and ndual; a set: the set's maxima)
struct TapeOut {
  int *status, *leaf;
  void *x_num, *x_den, *dual_num, *dual_den;
  int xs, ds;
};

// The walk of a lane that starts at word `pc` of `prog` (END: it has nothing to walk), together with its wave: in
// every step the lanes at the lowest position execute the node there, the others wait.  At the end st and leaf are set
// and a solution's values written.  nvar and ndual are the lane's tape's.  MARKS: the program may hold the two marks of
// pip_solve's result edits (pip_tape.h); a program without them is walked by code that does not look for them.
// STOP (pip_tape_compare_kernel): a lane stops AT its leaf -- st PIPAMD_ST_SOLUTION, `leaf` the LEAF's word position --
// and nothing is evaluated or written there; the caller does that.
template <class T, bool MARKS, bool STOP = false>
__device__ __forceinline__ void tape_walk(const i64 *prog, int pc, i64 *S, int tid, int nvar, int ndual, i64 pt,
                                          const TapeOut &o, int &st, int &leaf) {
  typedef Width<T> W;
  constexpr int EW = W::EW;
  for (;;) {
    const int cur = __builtin_amdgcn_readfirstlane(wave_min(pc));
    if (cur == END) break;
    const i64 hdr = prog[cur];
    const int op = (int)(hdr & 0xff), P = (int)((hdr >> 8) & 0xffff), aux = (int)(hdr >> 32);
    const i64 *body = prog + cur + 1;
    if (pc != cur) {
      // (this lane is further on: it waits for the wave to get there)
    } else if (op == TAPE_NEW) {
      const FormValue f = form_value(body + EW, P, S, tid, (T *)nullptr);
      T q = 0;
      if (f.ok && floor_div<T>(f.v, W::word(body, 0), &q)) {
        W::set_slot(S, P, tid, q);
        pc = cur + 1 + EW * (P + 2);
      } else {
        st = PIPAMD_ST_RANGE;
        pc = END;
      }
    } else if (op == TAPE_IF) {
      const FormValue f = form_value(body, P, S, tid, (T *)nullptr);
      if (EW == 2 && !f.ok) {
        st = PIPAMD_ST_RANGE;
        pc = END;
      } else {
        pc = f.neg ? aux : cur + 1 + EW * (P + 1);
      }
    } else if (STOP && op == TAPE_LEAF) {
      st = PIPAMD_ST_SOLUTION;
      leaf = cur;
      pc = END;
    } else if (op == TAPE_LEAF) {
      const bool flip = MARKS && (hdr & TAPE_LEAF_NEGATE) != 0;
      bool good = true;
      for (int i = 0; i < nvar; i++) {
        const i64 *u = body + (size_t)i * EW * (P + 2);
        const FormValue f = form_value(u + EW, P, S, tid, (T *)nullptr);
        // (a negative D_i marks an unbounded unknown, pip_tape.h: the reduction is by -D_i, the denominator handed out 0)
        const T D = W::word(u, 0);
        T num = 0, den = 0;
        const bool unbounded = MARKS && D < 0;
        good = good && f.ok && lowest_terms<T>(f.v, flip, unbounded ? -D : D, &num, &den);
        if (!good) break;
        if (unbounded) den = 0;
        if (o.x_num) W::out(o.x_num, pt * o.xs + i, num);
        if (o.x_den) W::out(o.x_den, pt * o.xs + i, den);
      }
      if (good) {
        const i64 *d = body + (size_t)nvar * EW * (P + 2);
        for (int i = 0; i < ndual; i++) {
          if (o.dual_num) W::out(o.dual_num, pt * o.ds + i, W::word(d, 2 * i));
          if (o.dual_den) W::out(o.dual_den, pt * o.ds + i, W::word(d, 2 * i + 1));
        }
        st = PIPAMD_ST_SOLUTION;
        leaf = aux;
      } else {
        st = PIPAMD_ST_RANGE;
      }
      pc = END;
    } else {  // TAPE_NIL
      st = PIPAMD_ST_NIL;
      leaf = aux;
      pc = END;
    }
  }
}

// status and leaf of a point, and (0, 0) in the values from `xfrom` / `dfrom` on: everything for a point without a
// solution (also where a leaf's later unknown left the range), a set's padding behind a tape's own counts otherwise
template <class T>
__device__ __forceinline__ void tape_finish(const TapeOut &o, i64 pt, int st, int leaf, int xfrom, int dfrom) {
  typedef Width<T> W;
  if (o.status) o.status[pt] = st;
  if (o.leaf) o.leaf[pt] = leaf;
  for (int i = xfrom; i < o.xs; i++) {
    if (o.x_num) W::out(o.x_num, pt * o.xs + i, (T)0);
    if (o.x_den) W::out(o.x_den, pt * o.xs + i, (T)0);
  }
  for (int i = dfrom; i < o.ds; i++) {
    if (o.dual_num) W::out(o.dual_num, pt * o.ds + i, (T)0);
    if (o.dual_den) W::out(o.dual_den, pt * o.ds + i, (T)0);
  }
}

template <class T, bool STAGED, bool MARKS>
__global__ __launch_bounds__(TAPE_BLOCK) void pip_tape_eval_kernel(TapeLaunch a) {
  typedef Width<T> W;
  constexpr int EW = W::EW;
  extern __shared__ __attribute__((aligned(16))) i64 tape_lds[];
  i64 *S = tape_lds;  // (slots - 1) * EW rows of TAPE_BLOCK words
  const int tid = threadIdx.x, nvar = a.nvar, ndual = a.ndual;
  const i64 pt = (i64)blockIdx.x * TAPE_BLOCK + tid;
  const bool live = pt < a.n_points;
  const int words = (int)a.words;
  const i64 *prog = a.prog;
  if (STAGED) {
    i64 *L = tape_lds + (size_t)(a.slots - 1) * EW * TAPE_BLOCK;
    for (int i = tid; i < words; i += TAPE_BLOCK) L[i] = a.prog[i];
    prog = L;
  }
  if (live)
    for (int j = 0; j < a.nparm; j++) W::set_slot(S, j, tid, (T)a.points[pt * a.nparm + j]);
  if (STAGED) __syncthreads();
  TapeOut o;
  o.status = a.status, o.leaf = a.leaf;
  o.x_num = a.x_num, o.x_den = a.x_den, o.dual_num = a.dual_num, o.dual_den = a.dual_den;
  o.xs = nvar, o.ds = ndual;

  int pc = live && words ? 0 : END;
  int st = PIPAMD_ST_NIL, leaf = -1;
  tape_walk<T, MARKS>(prog, pc, S, tid, nvar, ndual, pt, o, st, leaf);
  if (!live) return;
  if (st != PIPAMD_ST_SOLUTION) {
    tape_finish<T>(o, pt, st, leaf, 0, 0);  // (0, 0) throughout
  } else {
    if (a.status) a.status[pt] = st;
    if (a.leaf) a.leaf[pt] = leaf;
  }
}

// A set of tapes: point pt is of tape a.tape[pt], and its lane starts at that tape's first word.  Positions only grow
// within a tape and tapes do not overlap in the buffer, so serving the lowest position of the wave still executes every
// node at most once a wave: a wave of one tape walks as above, a wave of 64 tapes serves them one after the other.  The
// programs are read from global memory, at a wave-uniform address.
template <class T>
__global__ __launch_bounds__(TAPE_BLOCK) void pip_tape_set_eval_kernel(TapeSetLaunch a) {
  typedef Width<T> W;
  extern __shared__ __attribute__((aligned(16))) i64 tape_lds[];
  i64 *S = tape_lds;  // (a.slots - 1) * W::EW rows of TAPE_BLOCK words
  const int tid = threadIdx.x;
  const i64 pt = (i64)blockIdx.x * TAPE_BLOCK + tid;
  const bool live = pt < a.n_points;  // (the other lanes stay for the wave's shuffles, at END)
  TapeOut o;
  o.status = a.status, o.leaf = a.leaf;
  o.x_num = a.x_num, o.x_den = a.x_den, o.dual_num = a.dual_num, o.dual_den = a.dual_den;
  o.xs = a.nvar, o.ds = a.ndual;

  const int k = live ? a.tape[pt] : -1;
  int pc = END, st = PIPAMD_ST_BADINPUT, leaf = -1, nvar = 0, ndual = 0;
  if (k >= 0 && k < a.n) {  // (nothing is read through an index outside the table)
    const TapeSetEntry e = a.table[k];
    nvar = e.nvar, ndual = e.ndual;
    for (int j = 0; j < e.point_cols; j++) W::set_slot(S, j, tid, (T)a.points[pt * a.point_cols + j]);
    st = PIPAMD_ST_NIL;
    if (e.words) pc = e.start;
  }
  tape_walk<T, true>(a.prog, pc, S, tid, nvar, ndual, pt, o, st, leaf);
  if (!live) return;
  const bool sol = st == PIPAMD_ST_SOLUTION;
  tape_finish<T>(o, pt, st, leaf, sol ? nvar : 0, sol ? ndual : 0);
}

// ------------------------------------------------------------------ pipamd_tape_sweep
// The points of a box, made here (TapeSweepLaunch, pip_tape.h).  gridDim.x persistent workgroups take the chunks of
// TAPE_BLOCK consecutive k in turn; a staged program is copied to LDS once per workgroup.  Per chunk: the first k is
// decoded into its mixed-radix digits from the last column -- wave-uniform divisions, in 32 bits where both operands
// fit, none once the quotient is 0 --, and in the same pass lane t carries its offset t through them (a carry is at most 127: behind an extent of 2^16
// and more it is 0 or 1, a compare; behind a smaller one a 32-bit division).  The raw int64 point goes to slot rows
// 0 .. cols-1 as int64 cells have them; the context's rows are tested on those by the int64 form_value (exact sign,
// exactly zero iff ok && v == 0), read at a wave-uniform address; then 128-bit cells widen the rows in place, from the
// last (row j moves to rows 2j, 2j+1 >= j, and a lane touches its own column alone).  A lane outside leaves the walk at
// END with PIPAMD_ST_OUTSIDE; its wave still takes part in wave_min.
// Summary: the four status counts and firsts are wave-uniform accumulators over all chunks of a wave (a ballot and a
// popcount per status and chunk; the lowest set lane holds the smallest k, k growing with the lane).  Per leaf a wave
// aggregates likewise -- the leaf of its first pending lane, the ballot of the lanes that share it -- and each group's
// lowest lane adds (count, its k) to the workgroup's LDS bins (binned) or to the summary in global memory, all groups in
// one atomic instruction pair.  At the end the bins -- with the waves' status figures added -- are flushed, one 64-bit
// atomicAdd and one unsigned atomicMin per non-empty bin; -1, all ones, is the minimum's identity.  Without
// bins a wave flushes its status figures itself.
// OUT / SUM: per-point arrays / a summary are asked for; what is not costs no instruction in the loop.
__device__ __forceinline__ int sweep_class(int st) {
  return st == PIPAMD_ST_SOLUTION ? PIPAMD_SWEEP_SOLUTION
                                  : (st == PIPAMD_ST_NIL ? PIPAMD_SWEEP_NIL : (st == PIPAMD_ST_OUTSIDE ? PIPAMD_SWEEP_OUTSIDE : PIPAMD_SWEEP_RANGE));
}
__device__ __forceinline__ bool sweep_zero_word(i64 i, i64 L) { return i < PIPAMD_SWEEP_FIRST || (i >= 8 && i < 8 + L); }

// Point k0 + tid of the box (lo, ext), as raw int64 values in slot rows 0 .. cols-1 of S: the decode described above
// (pip_tape_compare_kernel calls these two; pip_tape_sweep_kernel has the same steps written out, see there)
__device__ __forceinline__ void box_point(const i64 *lo, const u64 *exts, int cols, i64 k0, int tid, i64 *S) {
  u64 rem = (u64)k0;
  unsigned carry = (unsigned)tid;
  for (int c = cols - 1; c >= 0; c--) {
    const u64 ext = exts[c];
    u64 s = carry;
    if (rem) {  // (wave-uniform; operands of 32 bits, every box below 2^32 points, divide in 32)
      const u64 q = ((rem | ext) >> 32) ? rem / ext : (u64)((unsigned)rem / (unsigned)ext);
      s += rem - q * ext;
      rem = q;
    }
    if (ext >> 16) {
      carry = s >= ext;
      s -= carry ? ext : 0;
    } else {
      const unsigned q = (unsigned)s / (unsigned)ext;
      s = (unsigned)s - q * (unsigned)ext;
      carry = q;
    }
    S[c * TAPE_BLOCK + tid] = (i64)((u64)lo[c] + s);
  }
}
// `inside`, and the raw int64 point of lane tid meets every row of the context, exactly
__device__ __forceinline__ bool box_inside(bool inside, const i64 *ctx, int n_ctx, int cols, const i64 *S, int tid) {
  for (int r = 0; r < n_ctx; r++) {
    const i64 *row = ctx + (size_t)r * (cols + 2);
    const FormValue f = form_value(row + 1, cols, S, tid, (i64 *)nullptr);
    inside = inside && (row[0] == 0 ? f.ok && f.v == 0 : !f.neg);
  }
  return inside;
}

__global__ void pip_tape_sweep_fill_kernel(i64 *sum, i64 L) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < PIPAMD_SWEEP_WORDS(L)) sum[i] = sweep_zero_word(i, L) ? 0 : -1;
}

template <class T, bool STAGED, bool MARKS, bool OUT, bool SUM>
__global__ __launch_bounds__(TAPE_BLOCK) void pip_tape_sweep_kernel(TapeSweepLaunch a) {
  typedef Width<T> W;
  constexpr int EW = W::EW;
  extern __shared__ __attribute__((aligned(16))) i64 tape_lds[];
  i64 *S = tape_lds;  // (slots - 1) * EW rows of TAPE_BLOCK words
  const int tid = threadIdx.x, lane = tid & 63, nvar = a.t.nvar, ndual = a.t.ndual, cols = a.t.nparm;
  const int words = (int)a.t.words;
  const i64 n = a.t.n_points, L = a.leaves;
  const i64 *prog = a.t.prog;
  i64 *behind = tape_lds + (size_t)(a.t.slots - 1) * EW * TAPE_BLOCK;
  if (STAGED) {
    for (int i = tid; i < words; i += TAPE_BLOCK) behind[i] = a.t.prog[i];
    prog = behind;
    behind += words;
  }
  u64 *bins = (u64 *)behind;  // binned: the summary's PIPAMD_SWEEP_WORDS(L) words, for this workgroup
  u64 *sum = (u64 *)a.summary;
  const bool binned = SUM && a.binned;
  if (binned)
    for (i64 i = tid; i < PIPAMD_SWEEP_WORDS(L); i += TAPE_BLOCK) bins[i] = sweep_zero_word(i, L) ? 0 : ~(u64)0;
  if (STAGED || SUM) __syncthreads();
  TapeOut o;
  o.status = OUT ? a.t.status : nullptr, o.leaf = OUT ? a.t.leaf : nullptr;
  o.x_num = OUT ? a.t.x_num : nullptr, o.x_den = OUT ? a.t.x_den : nullptr;
  o.dual_num = OUT ? a.t.dual_num : nullptr, o.dual_den = OUT ? a.t.dual_den : nullptr;
  o.xs = nvar, o.ds = ndual;
  u64 cnt[4] = {0, 0, 0, 0}, first[4] = {~(u64)0, ~(u64)0, ~(u64)0, ~(u64)0};

  for (i64 k0 = (i64)blockIdx.x * TAPE_BLOCK; k0 < n; k0 += (i64)gridDim.x * TAPE_BLOCK) {
    const i64 pt = k0 + tid;
    const bool live = pt < n;
    // (box_point and box_inside, written out: through the calls the compiler allocates this kernel's scalar registers
    // differently, and its instantiations are held to their recorded figures)
    u64 rem = (u64)k0;
    unsigned carry = (unsigned)tid;
    for (int c = cols - 1; c >= 0; c--) {
      const u64 ext = a.ext[c];
      u64 s = carry;
      if (rem) {  // (wave-uniform; operands of 32 bits, every box below 2^32 points, divide in 32)
        const u64 q = ((rem | ext) >> 32) ? rem / ext : (u64)((unsigned)rem / (unsigned)ext);
        s += rem - q * ext;
        rem = q;
      }
      if (ext >> 16) {
        carry = s >= ext;
        s -= carry ? ext : 0;
      } else {
        const unsigned q = (unsigned)s / (unsigned)ext;
        s = (unsigned)s - q * (unsigned)ext;
        carry = q;
      }
      S[c * TAPE_BLOCK + tid] = (i64)((u64)a.lo[c] + s);
    }
    bool inside = live;
    for (int r = 0; r < a.n_ctx; r++) {
      const i64 *row = a.ctx + (size_t)r * (cols + 2);
      const FormValue f = form_value(row + 1, cols, S, tid, (i64 *)nullptr);
      inside = inside && (row[0] == 0 ? f.ok && f.v == 0 : !f.neg);
    }
    if (EW == 2)
      for (int j = cols - 1; j >= 0; j--) W::set_slot(S, j, tid, (T)S[j * TAPE_BLOCK + tid]);

    int st = live && !inside ? PIPAMD_ST_OUTSIDE : PIPAMD_ST_NIL, leaf = -1;
    tape_walk<T, MARKS>(prog, inside && words ? 0 : END, S, tid, nvar, ndual, pt, o, st, leaf);
    if (OUT && live) {
      if (st != PIPAMD_ST_SOLUTION) {
        tape_finish<T>(o, pt, st, leaf, 0, 0);  // (0, 0) throughout
      } else {
        if (o.status) o.status[pt] = st;
        if (o.leaf) o.leaf[pt] = leaf;
      }
    }
    if (SUM) {
      const int cls = sweep_class(st);
      const u64 wave_k = (u64)(k0 + (tid & ~63));
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const u64 m = __ballot(live && cls == i);
        if (m) {
          const u64 k = wave_k + (u64)(__ffsll((unsigned long long)m) - 1);
          cnt[i] += (u64)__popcll(m);
          first[i] = k < first[i] ? k : first[i];
        }
      }
      // per leaf: every lane learns its group's size and whether it is the group's lowest lane; the leaders then add
      // (size, their k) in one atomic instruction pair for the whole wave -- no memory operation inside the loop
      u64 pend = __ballot(live && leaf >= 0);
      int group = 0;
      bool leader = false;
      while (pend) {
        const int src = __ffsll((unsigned long long)pend) - 1;
        const int l = __builtin_amdgcn_readlane(leaf, src);
        const u64 m = __ballot(live && leaf == l);
        if (live && leaf == l) {
          group = __popcll(m);
          leader = lane == src;
        }
        pend &= ~m;
      }
      if (leader && (u64)leaf < (u64)L) {  // (a compiled program's ordinals are below L; nothing is written beyond)
        u64 *to = binned ? bins : sum;
        atomicAdd(&to[PIPAMD_SWEEP_LEAF_COUNT(L) + leaf], (u64)group);
        atomicMin(&to[PIPAMD_SWEEP_LEAF_FIRST(L) + leaf], (u64)pt);
      }
    }
  }

  if (SUM) {
    if (lane == 0)
      for (int i = 0; i < 4; i++)
        if (cnt[i]) {
          u64 *to = binned ? bins : sum;
          atomicAdd(&to[PIPAMD_SWEEP_COUNT + i], cnt[i]);
          atomicMin(&to[PIPAMD_SWEEP_FIRST + i], first[i]);
        }
    if (binned) {
      __syncthreads();
      for (i64 i = tid; i < 4 + L; i += TAPE_BLOCK) {
        const i64 ci = i < 4 ? PIPAMD_SWEEP_COUNT + i : PIPAMD_SWEEP_LEAF_COUNT(L) + (i - 4);
        const i64 fi = i < 4 ? PIPAMD_SWEEP_FIRST + i : PIPAMD_SWEEP_LEAF_FIRST(L) + (i - 4);
        const u64 c = bins[ci];
        if (c) {
          atomicAdd(&sum[ci], c);
          atomicMin(&sum[fi], bins[fi]);
        }
      }
    }
  }
}

template <class T, bool MARKS, bool OUT, bool SUM>
hipError_t launch_sweep_as(const TapeSweepLaunch &s, hipStream_t stream) {
  size_t lds = tape_slot_bytes(s.t.slots, s.t.bits) + (s.t.staged ? (size_t)s.t.words * 8 : 0);
  if (SUM && s.binned) lds += tape_sweep_bin_bytes(s.leaves);
  void (*kernel)(TapeSweepLaunch) = s.t.staged ? pip_tape_sweep_kernel<T, true, MARKS, OUT, SUM> : pip_tape_sweep_kernel<T, false, MARKS, OUT, SUM>;
  // the grid: as many workgroups as the device holds at once with this kernel's registers and this launch's LDS (a
  // workgroup that waited for room would start its share of the chunks late), no more than there are chunks
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, TAPE_BLOCK, lds) != hipSuccess || per_cu < 1) per_cu = 1;
  // (with a summary every workgroup ends with an atomic add on the few words all share, and they end together: fewer,
  // longer-lived workgroups keep that queue short -- measured)
  const int bound = SUM ? TAPE_SWEEP_WG_PER_CU_SUM : TAPE_SWEEP_WG_PER_CU;
  if (per_cu > bound) per_cu = bound;
  const long long chunks = (s.t.n_points + TAPE_BLOCK - 1) / TAPE_BLOCK;
  long long blocks = (long long)(s.cus > 0 ? s.cus : 1) * per_cu;
  if (s.max_blocks > 0 && s.max_blocks < blocks) blocks = s.max_blocks;
  if (chunks < blocks) blocks = chunks;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(TAPE_BLOCK), lds, stream, s);
  return hipGetLastError();
}
template <class T, bool MARKS>
hipError_t launch_sweep(const TapeSweepLaunch &s, hipStream_t stream) {
  const bool out = s.t.status || s.t.leaf || s.t.x_num || s.t.x_den || s.t.dual_num || s.t.dual_den;
  if (s.summary) return out ? launch_sweep_as<T, MARKS, true, true>(s, stream) : launch_sweep_as<T, MARKS, false, true>(s, stream);
  return launch_sweep_as<T, MARKS, true, false>(s, stream);  // (nothing asked for: the walk with nothing to write)
}

// ------------------------------------------------------------------ pipamd_tape_compare / pipamd_tape_compare_sweep
// Two programs per lane (TapeCompareLaunch, pip_tape.h), `a` of TA cells and `b` of TB cells, each with slot rows of
// its own.  Per chunk the point is decoded (BOX: as the sweep does, and tested against the context) or loaded once as
// raw int64 rows of a's area, copied to b's area in b's width, then widened in place where a is 128-bit.  Tape a is
// walked to its end node, then tape b, both with STOP: a lane is then at a (leaf of a, leaf of b) pair of word
// positions, -1 for a side that did not end in a LEAF.  The wave serves its pairs one at a time -- the pair of its
// first pending lane, read by readlane, and the ballot of the lanes that share it (cheaper than a minimum over the
// combined key, and the order plays no part) --, so the leaves' words stay one address per wave.  The lanes of a pair
// evaluate unknown i of both leaves as tape_walk does -- form_value, lowest_terms, negate and unbounded marks -- and
// compare the pairs handed out in 128 bits; they keep `range` per side and `where`.  Every unknown of both leaves is
// evaluated, so a side's status is pipamd_tape_eval's whatever the other side does.  The dual pairs are words of the
// programs, the same for all lanes of a pair.
// Summary: five counts and five firsts as wave-uniform accumulators, a ballot and a popcount per class and chunk;
// each wave flushes what it counted, a 64-bit atomicAdd and an unsigned atomicMin per class it met.
__global__ void pip_tape_compare_fill_kernel(i64 *sum) {
  const int i = threadIdx.x;
  if (i < PIPAMD_CMP_WORDS) sum[i] = i < PIPAMD_CMP_WORDS / 2 ? 0 : -1;
}

// unknown i of the LEAF at word `at` of prog, at lane tid's point: the pair handed out, widened.  false: it leaves T
template <class T>
__device__ __forceinline__ bool leaf_pair(const i64 *prog, int at, int i, const i64 *S, int tid, i128 *num, i128 *den) {
  typedef Width<T> W;
  constexpr int EW = W::EW;
  const i64 hdr = prog[at];
  const int P = (int)((hdr >> 8) & 0xffff);
  const i64 *u = prog + at + 1 + (size_t)i * EW * (P + 2);
  const FormValue f = form_value(u + EW, P, S, tid, (T *)nullptr);
  const T D = W::word(u, 0);
  const bool unbounded = D < 0;
  T n = 0, d = 0;
  const bool good = f.ok && lowest_terms<T>(f.v, (hdr & TAPE_LEAF_NEGATE) != 0, unbounded ? -D : D, &n, &d);
  *num = (i128)n;
  *den = unbounded ? (i128)0 : (i128)d;
  return good;
}

template <class TA, class TB, bool STAGED, bool BOX>
__global__ __launch_bounds__(TAPE_BLOCK) void pip_tape_compare_kernel(TapeCompareLaunch a) {
  typedef Width<TA> WA;
  typedef Width<TB> WB;
  constexpr int EA = WA::EW, EB = WB::EW;
  extern __shared__ __attribute__((aligned(16))) i64 tape_lds[];
  i64 *SA = tape_lds;                                       // (slots_a - 1) * EA rows of TAPE_BLOCK words
  i64 *SB = SA + (size_t)(a.slots_a - 1) * EA * TAPE_BLOCK;  // (slots_b - 1) * EB rows
  const int tid = threadIdx.x, lane = tid & 63, nvar = a.nvar, ndual = a.ndual, cols = a.nparm;
  const int words_a = (int)a.words_a, words_b = (int)a.words_b;
  const i64 n = a.n_points;
  const i64 *pa = a.prog_a, *pb = a.prog_b;
  if (STAGED) {
    i64 *LA = SB + (size_t)(a.slots_b - 1) * EB * TAPE_BLOCK, *LB = LA + words_a;
    for (int i = tid; i < words_a; i += TAPE_BLOCK) LA[i] = a.prog_a[i];
    for (int i = tid; i < words_b; i += TAPE_BLOCK) LB[i] = a.prog_b[i];
    pa = LA, pb = LB;
    __syncthreads();
  }
  u64 *sum = (u64 *)a.summary;
  TapeOut none;  // (STOP: the walk writes nothing)
  none.status = none.leaf = nullptr;
  none.x_num = none.x_den = none.dual_num = none.dual_den = nullptr;
  none.xs = none.ds = 0;
  u64 cnt[5] = {0, 0, 0, 0, 0}, first[5] = {~(u64)0, ~(u64)0, ~(u64)0, ~(u64)0, ~(u64)0};

  for (i64 k0 = (i64)blockIdx.x * TAPE_BLOCK; k0 < n; k0 += (i64)gridDim.x * TAPE_BLOCK) {
    const i64 pt = k0 + tid;
    const bool live = pt < n;
    bool inside = live;
    if (BOX) {
      box_point(a.lo, a.ext, cols, k0, tid, SA);
      inside = box_inside(live, a.ctx, a.n_ctx, cols, SA, tid);
    } else if (live) {
      for (int j = 0; j < cols; j++) SA[j * TAPE_BLOCK + tid] = a.points[pt * cols + j];
    }
    // (a lane touches its own column alone; a lane that is not live holds whatever was there and walks nothing)
    for (int j = 0; j < cols; j++) WB::set_slot(SB, j, tid, (TB)SA[j * TAPE_BLOCK + tid]);
    if (EA == 2)
      for (int j = cols - 1; j >= 0; j--) WA::set_slot(SA, j, tid, (TA)SA[j * TAPE_BLOCK + tid]);

    int sa = live && !inside ? PIPAMD_ST_OUTSIDE : PIPAMD_ST_NIL, sb = sa, la = -1, lb = -1;
    tape_walk<TA, true, true>(pa, inside && words_a ? 0 : END, SA, tid, nvar, 0, pt, none, sa, la);
    tape_walk<TB, true, true>(pb, inside && words_b ? 0 : END, SB, tid, nvar, 0, pt, none, sb, lb);
    la = sa == PIPAMD_ST_SOLUTION ? la : -1;
    lb = sb == PIPAMD_ST_SOLUTION ? lb : -1;

    bool range_a = false, range_b = false;
    int where = -1;
    u64 pend = __ballot(la >= 0 || lb >= 0);
    while (pend) {
      const int src = __ffsll((unsigned long long)pend) - 1;
      const int ua = __builtin_amdgcn_readlane(la, src), ub = __builtin_amdgcn_readlane(lb, src);
      const bool mine = la == ua && lb == ub;  // (not both -1: lane src is pending)
      if (mine) {
        for (int i = 0; i < nvar; i++) {
          i128 na = 0, da = 0, nb = 0, db = 0;
          if (ua >= 0) range_a = !leaf_pair<TA>(pa, ua, i, SA, tid, &na, &da) || range_a;
          if (ub >= 0) range_b = !leaf_pair<TB>(pb, ub, i, SB, tid, &nb, &db) || range_b;
          if (where < 0 && (na != nb || da != db)) where = i;
        }
        if (ndual && ua >= 0 && ub >= 0 && where < 0) {
          const i64 *qa = pa + ua + 1 + (size_t)nvar * EA * ((int)((pa[ua] >> 8) & 0xffff) + 2);
          const i64 *qb = pb + ub + 1 + (size_t)nvar * EB * ((int)((pb[ub] >> 8) & 0xffff) + 2);
          for (int i = 0; i < ndual && where < 0; i++)
            if ((i128)WA::word(qa, 2 * i) != (i128)WB::word(qb, 2 * i) || (i128)WA::word(qa, 2 * i + 1) != (i128)WB::word(qb, 2 * i + 1))
              where = nvar + i;
        }
      }
      pend &= ~__ballot(mine);
    }
    if (range_a) sa = PIPAMD_ST_RANGE;
    if (range_b) sb = PIPAMD_ST_RANGE;
    int cls = PIPAMD_CMP_SAME;
    if (live && !inside) cls = PIPAMD_CMP_OUTSIDE;
    else if (sa == PIPAMD_ST_RANGE || sb == PIPAMD_ST_RANGE) cls = PIPAMD_CMP_RANGE;
    else if (sa != sb) cls = PIPAMD_CMP_STATUS;
    else if (sa == PIPAMD_ST_SOLUTION && where >= 0) cls = PIPAMD_CMP_VALUE;
    if (live) {
      if (a.cls) a.cls[pt] = cls;
      if (a.where) a.where[pt] = cls == PIPAMD_CMP_VALUE ? where : -1;
      if (a.status_a) a.status_a[pt] = sa;
      if (a.status_b) a.status_b[pt] = sb;
    }
    if (sum) {
      const u64 wave_k = (u64)(k0 + (tid & ~63));
#pragma unroll
      for (int i = 0; i < 5; i++) {
        const u64 m = __ballot(live && cls == i);
        if (m) {
          const u64 k = wave_k + (u64)(__ffsll((unsigned long long)m) - 1);
          cnt[i] += (u64)__popcll(m);
          first[i] = k < first[i] ? k : first[i];
        }
      }
    }
  }
  if (sum && lane == 0)
    for (int i = 0; i < 5; i++)
      if (cnt[i]) {
        atomicAdd(&sum[i], cnt[i]);
        atomicMin(&sum[PIPAMD_CMP_WORDS / 2 + i], first[i]);
      }
}

template <class TA, class TB>
hipError_t launch_compare(const TapeCompareLaunch &c, hipStream_t stream) {
  size_t lds = tape_slot_bytes(c.slots_a, c.bits_a) + tape_slot_bytes(c.slots_b, c.bits_b);
  if (c.staged) lds += (size_t)(c.words_a + c.words_b) * 8;
  void (*kernel)(TapeCompareLaunch) =
      c.box ? (c.staged ? pip_tape_compare_kernel<TA, TB, true, true> : pip_tape_compare_kernel<TA, TB, false, true>)
            : (c.staged ? pip_tape_compare_kernel<TA, TB, true, false> : pip_tape_compare_kernel<TA, TB, false, false>);
  const long long chunks = (c.n_points + TAPE_BLOCK - 1) / TAPE_BLOCK;
  long long blocks = chunks;
  if (c.box) {  // the sweep's bounded persistent grid (launch_sweep_as)
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, TAPE_BLOCK, lds) != hipSuccess || per_cu < 1) per_cu = 1;
    const int bound = c.summary ? TAPE_SWEEP_WG_PER_CU_SUM : TAPE_SWEEP_WG_PER_CU;
    if (per_cu > bound) per_cu = bound;
    blocks = (long long)(c.cus > 0 ? c.cus : 1) * per_cu;
    if (c.max_blocks > 0 && c.max_blocks < blocks) blocks = c.max_blocks;
    if (chunks < blocks) blocks = chunks;
  } else if (blocks > (1ll << 24)) {
    blocks = 1ll << 24;  // (a workgroup per chunk up to 2^31 points; beyond, the kernel's loop takes the rest in turn)
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(TAPE_BLOCK), lds, stream, c);
  return hipGetLastError();
}

template <class T, bool MARKS>
hipError_t launch(const TapeLaunch &t, hipStream_t stream) {
  const long long blocks = (t.n_points + TAPE_BLOCK - 1) / TAPE_BLOCK;
  const size_t slot_bytes = tape_slot_bytes(t.slots, t.bits);
  if (t.staged)
    hipLaunchKernelGGL((pip_tape_eval_kernel<T, true, MARKS>), dim3((unsigned)blocks), dim3(TAPE_BLOCK),
                       slot_bytes + (size_t)t.words * 8, stream, t);
  else
    hipLaunchKernelGGL((pip_tape_eval_kernel<T, false, MARKS>), dim3((unsigned)blocks), dim3(TAPE_BLOCK), slot_bytes, stream, t);
  return hipGetLastError();
}
template <class T>
hipError_t launch_set(const TapeSetLaunch &t, hipStream_t stream) {
  const long long blocks = (t.n_points + TAPE_BLOCK - 1) / TAPE_BLOCK;
  hipLaunchKernelGGL((pip_tape_set_eval_kernel<T>), dim3((unsigned)blocks), dim3(TAPE_BLOCK),
                     tape_slot_bytes(t.slots, t.bits), stream, t);
  return hipGetLastError();
}
}  // namespace

extern "C" hipError_t pipk_launch_tape_eval(const TapeLaunch *t, hipStream_t stream) {
  if (t->n_points <= 0) return hipSuccess;
  // (the caller checked: slots <= TAPE_MAX_SLOTS, and a staged program fits TAPE_LDS_BYTES beside the slots)
  if (t->marks) return t->bits == 128 ? launch<i128, true>(*t, stream) : launch<i64, true>(*t, stream);
  return t->bits == 128 ? launch<i128, false>(*t, stream) : launch<i64, false>(*t, stream);
}

extern "C" hipError_t pipk_launch_tape_sweep(const TapeSweepLaunch *s, hipStream_t stream) {
  // (the caller checked: 1 <= n_points < 2^38, every extent's product within it, slots <= TAPE_MAX_SLOTS, the LDS the
  // plan counted within TAPE_LDS_BYTES)
  if (s->summary) {
    const long long w = PIPAMD_SWEEP_WORDS(s->leaves);
    hipLaunchKernelGGL(pip_tape_sweep_fill_kernel, dim3((unsigned)((w + 255) / 256)), dim3(256), 0, stream, s->summary, s->leaves);
    const hipError_t he = hipGetLastError();
    if (he != hipSuccess) return he;
  }
  if (s->t.marks) return s->t.bits == 128 ? launch_sweep<i128, true>(*s, stream) : launch_sweep<i64, true>(*s, stream);
  return s->t.bits == 128 ? launch_sweep<i128, false>(*s, stream) : launch_sweep<i64, false>(*s, stream);
}

extern "C" hipError_t pipk_launch_tape_compare(const TapeCompareLaunch *c, hipStream_t stream) {
  // (the caller checked: 0 <= n_points < 2^38, both slot counts <= TAPE_MAX_SLOTS, the two slot areas -- and the two
  // programs where staged -- within TAPE_LDS_BYTES)
  if (c->summary) {
    hipLaunchKernelGGL(pip_tape_compare_fill_kernel, dim3(1), dim3(64), 0, stream, c->summary);
    const hipError_t he = hipGetLastError();
    if (he != hipSuccess) return he;
  }
  if (c->n_points <= 0) return hipSuccess;
  if (c->bits_a == 128) return c->bits_b == 128 ? launch_compare<i128, i128>(*c, stream) : launch_compare<i128, i64>(*c, stream);
  return c->bits_b == 128 ? launch_compare<i64, i128>(*c, stream) : launch_compare<i64, i64>(*c, stream);
}

extern "C" hipError_t pipk_launch_tape_set_eval(const TapeSetLaunch *t, hipStream_t stream) {
  if (t->n_points <= 0) return hipSuccess;
  // (pipamd_tape_set_create checked: slots <= TAPE_MAX_SLOTS, every jump inside its own tape's words)
  return t->bits == 128 ? launch_set<i128>(*t, stream) : launch_set<i64>(*t, stream);
}
