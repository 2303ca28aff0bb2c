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

// ------------------------------------------------------------------ pipamd_tape_sweep_values
// Per unknown the counts, the minimum and the maximum with the smallest k that attains them, and the exact sum of the
// integer values a box's SOLUTION points hand out (TapeValuesLaunch, pip_tape.h; the record: piplib_amd.h).  The sweep's
// grid, decode, context test and walk -- with STOP, so a lane is at its leaf's word position.  Then, unknown by unknown
// in a wave-uniform loop: the wave serves its distinct leaves one at a time as the compare kernel does -- the leaf of
// the first pending lane by readlane, the ballot of the lanes that share it -- and those lanes evaluate the unknown with
// leaf_pair; once every lane has its pair, ONE wave reduction per unknown and chunk: the three counts are popcounts of
// ballots; the minimum and the maximum are butterflies over the values alone, the lane of the smallest k then the
// lowest set bit of the ballot `value == minimum` (k grows with the lane); the sum is a butterfly over pieces whose 64
// terms cannot carry out of a register pair.  Lane i of the wave merges unknown i's figures into the ValuesAcc it keeps
// in registers -- no lane indexes an array --, in the (value, lowest k) order, which is order-independent.
// RANGE is known only after a point's last unknown, and such a point takes part in nothing.  A chunk is accumulated
// into a copy of the accumulators with every SOLUTION lane taking part; when the ballot shows a RANGE lane the copy is
// dropped and the chunk done again without those lanes (a second time is the last: RANGE is a property of the lane).
// The alternative -- a first pass over the unknowns for RANGE alone, a second that accumulates -- evaluates every leaf
// twice at every point and measured slower.
// The head words are the sweep's: wave-uniform counts and firsts, flushed by the sweep's atomics.  The records are not
// touched by an atomic: every wave stores its 64 accumulators -- the identity where it met nothing -- as row
// 2 * blockIdx.x + wave of `work` with plain stores, and pip_tape_values_fold_kernel, a workgroup per unknown, merges
// the rows in the same order-independent way and writes the record.
struct Sum192 {
  u64 w0, w1, w2;  // two's complement, little-endian limbs
};
__device__ __forceinline__ Sum192 add192(Sum192 a, Sum192 b) {
  Sum192 r;
  u128 t = (u128)a.w0 + b.w0;
  r.w0 = (u64)t;
  t = (u128)a.w1 + b.w1 + (u64)(t >> 64);
  r.w1 = (u64)t;
  r.w2 = a.w2 + b.w2 + (u64)(t >> 64);
  return r;
}
struct ValuesAcc {
  u64 n_int, n_frac, n_unb;
  i128 mn, mx;    // meaningful with n_int > 0
  i64 k_mn, k_mx;
  Sum192 sum;
};
__device__ __forceinline__ ValuesAcc values_identity() {
  ValuesAcc a;
  a.n_int = a.n_frac = a.n_unb = 0;
  a.mn = a.mx = 0;
  a.k_mn = a.k_mx = -1;
  a.sum.w0 = a.sum.w1 = a.sum.w2 = 0;
  return a;
}
// a and b merged into a: commutative and associative, a minimum's and a maximum's k the smallest that attains it
__device__ __forceinline__ void values_merge(ValuesAcc &a, const ValuesAcc &b) {
  if (b.n_int) {
    if (!a.n_int || b.mn < a.mn || (b.mn == a.mn && b.k_mn < a.k_mn)) a.mn = b.mn, a.k_mn = b.k_mn;
    if (!a.n_int || b.mx > a.mx || (b.mx == a.mx && b.k_mx < a.k_mx)) a.mx = b.mx, a.k_mx = b.k_mx;
  }
  a.n_int += b.n_int, a.n_frac += b.n_frac, a.n_unb += b.n_unb;
  a.sum = add192(a.sum, b.sum);
}
template <class V>
__device__ __forceinline__ V wave_min_of(V x) {
  for (int o = 32; o; o >>= 1) {
    const V y = shfl_xor(x, o);
    x = y < x ? y : x;
  }
  return x;
}
template <class V>
__device__ __forceinline__ V wave_max_of(V x) {
  for (int o = 32; o; o >>= 1) {
    const V y = shfl_xor(x, o);
    x = y > x ? y : x;
  }
  return x;
}
__device__ __forceinline__ i64 wave_add64(i64 x) {
  for (int o = 32; o; o >>= 1) x = (i64)((u64)x + (u64)shfl_xor(x, o));
  return x;
}
// the exact sum of the wave's 64 values.  int64: the low and the signed high 32 bits summed apart, each below 2^38
__device__ __forceinline__ Sum192 wave_sum192(i64 v) {
  const i64 lo = wave_add64((i64)(u64)(unsigned)(u64)v), hi = wave_add64(v >> 32);
  const i128 s = (i128)lo + (i128)hi * ((i128)1 << 32);
  Sum192 r;
  r.w0 = (u64)(u128)s, r.w1 = (u64)((u128)s >> 64), r.w2 = (u64)(i64)(s >> 127);
  return r;
}
// 128 bits: pieces of 43, 43 and 42 (signed) bits, each sum below 2^49; joined in 192 bits
__device__ __forceinline__ Sum192 wave_sum192(i128 v) {
  const u64 mask = ((u64)1 << 43) - 1;
  const i64 s0 = wave_add64((i64)((u64)(u128)v & mask)), s1 = wave_add64((i64)((u64)((u128)v >> 43) & mask));
  const i64 s2 = wave_add64((i64)(v >> 86));
  const i128 low = (i128)s0 + ((i128)s1 << 43), high = (i128)s2 * ((i128)1 << 22);  // high counts 2^64
  Sum192 a, b;
  a.w0 = (u64)(u128)low, a.w1 = (u64)((u128)low >> 64), a.w2 = 0;  // (0 <= low < 2^93)
  b.w0 = 0, b.w1 = (u64)(u128)high, b.w2 = (u64)((u128)high >> 64);
  return add192(a, b);
}
template <class T>
struct ValueLimits;
template <>
struct ValueLimits<i64> {
  static __device__ __forceinline__ i64 max() { return (i64)(~(u64)0 >> 1); }
};
template <>
struct ValueLimits<i128> {
  static __device__ __forceinline__ i128 max() { return (i128)(~(u128)0 >> 1); }
};

// the wave's figures for one unknown: lanes with `isint` hand out v over 1, `isfrac` over more, `isunb` over 0; lane l
// is point wave_k + l.  Every lane gets the same ValuesAcc.
template <class T>
__device__ __forceinline__ ValuesAcc values_reduce(bool isint, bool isfrac, bool isunb, T v, u64 wave_k) {
  ValuesAcc r = values_identity();
  const u64 mi = __ballot(isint);
  r.n_int = (u64)__popcll(mi);
  r.n_frac = (u64)__popcll(__ballot(isfrac));
  r.n_unb = (u64)__popcll(__ballot(isunb));
  if (mi) {  // (wave-uniform)
    const T top = ValueLimits<T>::max(), bottom = -top - 1;
    const T lo = wave_min_of<T>(isint ? v : top), hi = wave_max_of<T>(isint ? v : bottom);
    r.mn = (i128)lo, r.mx = (i128)hi;
    r.k_mn = (i64)(wave_k + (u64)(__ffsll((unsigned long long)__ballot(isint && v == lo)) - 1));
    r.k_mx = (i64)(wave_k + (u64)(__ffsll((unsigned long long)__ballot(isint && v == hi)) - 1));
    r.sum = wave_sum192(isint ? v : (T)0);
  }
  return r;
}

// One pass of a wave over the unknowns of its lanes' leaves: the lanes with `take` are at the LEAF at word `leaf`.
// Lane i merges unknown i into acc.  Returns whether the lane's point is RANGE (only a lane with `take` can be).
template <class T>
__device__ __forceinline__ bool values_pass(const i64 *prog, const i64 *S, int tid, int nvar, bool take, int leaf, u64 wave_k,
                                            ValuesAcc &acc) {
  const int lane = tid & 63;
  bool range = false;
  for (int i = 0; i < nvar; i++) {
    i128 num = 0, den = 0;
    bool ok = true;
    u64 pend = __ballot(take);
    while (pend) {
      const int src = __ffsll((unsigned long long)pend) - 1;
      const int l = __builtin_amdgcn_readlane(leaf, src);
      const bool mine = take && leaf == l;
      if (mine) ok = leaf_pair<T>(prog, l, i, S, tid, &num, &den);
      pend &= ~__ballot(mine);
    }
    range = range || !ok;
    const bool good = take && ok;
    const ValuesAcc r = values_reduce<T>(good && den == 1, good && den > 1, good && den == 0, (T)num, wave_k);
    if (lane == i) values_merge(acc, r);
  }
  return range;
}

// the partial row of a wave and what the fold reads: TAPE_VALUES_PART words an unknown
__device__ __forceinline__ void values_store(i64 *p, const ValuesAcc &a) {
  p[0] = (i64)a.n_int, p[1] = (i64)a.n_frac, p[2] = (i64)a.n_unb;
  p[3] = (i64)(u64)(u128)a.mn, p[4] = (i64)(u64)((u128)a.mn >> 64), p[5] = a.k_mn;
  p[6] = (i64)(u64)(u128)a.mx, p[7] = (i64)(u64)((u128)a.mx >> 64), p[8] = a.k_mx;
  p[9] = (i64)a.sum.w0, p[10] = (i64)a.sum.w1, p[11] = (i64)a.sum.w2;
}
__device__ __forceinline__ ValuesAcc values_load(const i64 *p) {
  ValuesAcc a;
  a.n_int = (u64)p[0], a.n_frac = (u64)p[1], a.n_unb = (u64)p[2];
  a.mn = (i128)(((u128)(u64)p[4] << 64) | (u64)p[3]), a.k_mn = p[5];
  a.mx = (i128)(((u128)(u64)p[7] << 64) | (u64)p[6]), a.k_mx = p[8];
  a.sum.w0 = (u64)p[9], a.sum.w1 = (u64)p[10], a.sum.w2 = (u64)p[11];
  return a;
}

template <class T, bool STAGED, bool MARKS>
__global__ __launch_bounds__(TAPE_BLOCK) void pip_tape_values_kernel(TapeValuesLaunch a) {
  typedef Width<T> W;
  constexpr int EW = W::EW;
  extern __shared__ __attribute__((aligned(16))) i64 tape_lds[];
  i64 *S = tape_lds;  // (slots - 1) * EW rows of TAPE_BLOCK words
  const int tid = threadIdx.x, lane = tid & 63, nvar = a.t.nvar, cols = a.t.nparm;
  const int words = (int)a.t.words;
  const i64 n = a.t.n_points;
  const i64 *prog = a.t.prog;
  if (STAGED) {
    i64 *L = tape_lds + (size_t)(a.t.slots - 1) * EW * TAPE_BLOCK;
    for (int i = tid; i < words; i += TAPE_BLOCK) L[i] = a.t.prog[i];
    prog = L;
    __syncthreads();
  }
  u64 *sum = (u64 *)a.summary;
  TapeOut none;  // (STOP: the walk writes nothing)
  none.status = none.leaf = nullptr;
  none.x_num = none.x_den = none.dual_num = none.dual_den = nullptr;
  none.xs = none.ds = 0;
  u64 cnt[4] = {0, 0, 0, 0}, first[4] = {~(u64)0, ~(u64)0, ~(u64)0, ~(u64)0};
  ValuesAcc acc = values_identity();  // lane i: unknown i

  for (i64 k0 = (i64)blockIdx.x * TAPE_BLOCK; k0 < n; k0 += (i64)gridDim.x * TAPE_BLOCK) {
    const i64 pt = k0 + tid;
    const bool live = pt < n;
    box_point(a.lo, a.ext, cols, k0, tid, S);
    const bool inside = box_inside(live, a.ctx, a.n_ctx, cols, S, tid);
    if (EW == 2)
      for (int j = cols - 1; j >= 0; j--) W::set_slot(S, j, tid, (T)S[j * TAPE_BLOCK + tid]);

    int st = live && !inside ? PIPAMD_ST_OUTSIDE : PIPAMD_ST_NIL, leaf = -1;
    tape_walk<T, MARKS, true>(prog, inside && words ? 0 : END, S, tid, nvar, 0, pt, none, st, leaf);
    const bool sol = st == PIPAMD_ST_SOLUTION;  // (only a live lane inside the context walks)
    const u64 wave_k = (u64)(k0 + (tid & ~63));
    bool range = false;
    for (;;) {  // (twice at most: a chunk without a RANGE lane is done)
      ValuesAcc trial = acc;
      const bool r = values_pass<T>(prog, S, tid, nvar, sol && !range, leaf, wave_k, trial);
      if (!__ballot(r)) {
        acc = trial;
        break;
      }
      range = range || r;
    }
    if (range) st = PIPAMD_ST_RANGE;
    const int cls = sweep_class(st);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const u64 m = __ballot(live && cls == i);
      if (m) {
        const u64 k = wave_k + (u64)(__ffsll((unsigned long long)m) - 1);
        cnt[i] += (u64)__popcll(m);
        first[i] = k < first[i] ? k : first[i];
      }
    }
  }

  if (lane == 0)
    for (int i = 0; i < 4; i++)
      if (cnt[i]) {
        atomicAdd(&sum[PIPAMD_SWEEP_COUNT + i], cnt[i]);
        atomicMin(&sum[PIPAMD_SWEEP_FIRST + i], first[i]);
      }
  // (row 2 * blockIdx.x + wave < 2 * gridDim.x, the rows the host counted in work_bytes)
  if (lane < nvar) values_store(a.work + (((size_t)blockIdx.x * (TAPE_BLOCK / 64) + (tid >> 6)) * nvar + lane) * TAPE_VALUES_PART, acc);
}

// Unknown blockIdx.x: the lanes stride over the `rows` partial rows, a wave merges by butterfly, the waves through LDS,
// and thread 0 writes the record.  blockDim.x is a multiple of 64, at most TAPE_VALUES_FOLD_BLOCK.
__global__ __launch_bounds__(TAPE_VALUES_FOLD_BLOCK) void pip_tape_values_fold_kernel(const i64 *work, int rows, int nvar, i64 *summary) {
  __shared__ i64 part[TAPE_VALUES_FOLD_BLOCK / 64][TAPE_VALUES_PART];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  ValuesAcc acc = values_identity();
  for (int r = tid; r < rows; r += blockDim.x) values_merge(acc, values_load(work + ((size_t)r * nvar + i) * TAPE_VALUES_PART));
  for (int o = 32; o; o >>= 1) {
    ValuesAcc b;
    b.n_int = (u64)shfl_xor((i64)acc.n_int, o), b.n_frac = (u64)shfl_xor((i64)acc.n_frac, o), b.n_unb = (u64)shfl_xor((i64)acc.n_unb, o);
    b.mn = shfl_xor(acc.mn, o), b.mx = shfl_xor(acc.mx, o);
    b.k_mn = shfl_xor(acc.k_mn, o), b.k_mx = shfl_xor(acc.k_mx, o);
    b.sum.w0 = (u64)shfl_xor((i64)acc.sum.w0, o), b.sum.w1 = (u64)shfl_xor((i64)acc.sum.w1, o), b.sum.w2 = (u64)shfl_xor((i64)acc.sum.w2, o);
    values_merge(acc, b);
  }
  if (lane == 0) values_store(part[wave], acc);
  __syncthreads();
  if (tid) return;
  for (int w = 1; w < (int)(blockDim.x >> 6); w++) values_merge(acc, values_load(part[w]));
  i64 *rec = summary + PIPAMD_VALUES_HEAD + (size_t)PIPAMD_VALUES_REC * i;
  const bool any = acc.n_int != 0;
  rec[0] = (i64)acc.n_int, rec[1] = (i64)acc.n_frac, rec[2] = (i64)acc.n_unb, rec[3] = 0;
  rec[4] = any ? (i64)(u64)(u128)acc.mn : 0, rec[5] = any ? (i64)(u64)((u128)acc.mn >> 64) : 0, rec[6] = any ? acc.k_mn : -1;
  rec[7] = any ? (i64)(u64)(u128)acc.mx : 0, rec[8] = any ? (i64)(u64)((u128)acc.mx >> 64) : 0, rec[9] = any ? acc.k_mx : -1;
  rec[10] = (i64)acc.sum.w0, rec[11] = (i64)acc.sum.w1, rec[12] = (i64)acc.sum.w2;
  rec[13] = rec[14] = rec[15] = 0;
}

template <class T, bool MARKS>
hipError_t launch_values(const TapeValuesLaunch &v, hipStream_t stream) {
  const size_t lds = tape_slot_bytes(v.t.slots, v.t.bits) + (v.t.staged ? (size_t)v.t.words * 8 : 0);
  void (*kernel)(TapeValuesLaunch) = v.t.staged ? pip_tape_values_kernel<T, true, MARKS> : pip_tape_values_kernel<T, false, MARKS>;
  // the sweep's bounded persistent grid with a summary (launch_sweep_as), and no more workgroups than `work` has rows for
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, TAPE_BLOCK, lds) != hipSuccess || per_cu < 1) per_cu = 1;
  if (per_cu > TAPE_SWEEP_WG_PER_CU_SUM) per_cu = TAPE_SWEEP_WG_PER_CU_SUM;
  long long blocks = (long long)(v.cus > 0 ? v.cus : 1) * per_cu;
  if (v.max_blocks > 0 && v.max_blocks < blocks) blocks = v.max_blocks;
  blocks = tape_values_blocks(v.t.n_points, blocks);
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(TAPE_BLOCK), lds, stream, v);
  hipError_t he = hipGetLastError();
  if (he != hipSuccess || v.t.nvar == 0) return he;
  const int rows = (int)blocks * (TAPE_BLOCK / 64);
  const int threads = rows >= TAPE_VALUES_FOLD_BLOCK ? TAPE_VALUES_FOLD_BLOCK : (rows + 63) / 64 * 64;
  hipLaunchKernelGGL(pip_tape_values_fold_kernel, dim3((unsigned)v.t.nvar), dim3(threads), 0, stream, v.work, rows, v.t.nvar, v.summary);
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

// ------------------------------------------------------------------ pipamd_tape_set_sweep_run
// The jobs of a set swept in one launch (TapeSetSweepLaunch, pip_tape.h).  gridDim.x persistent workgroups take the
// chunks of ALL jobs in grid stride.  The job of a chunk is found by bisection of chunk_off: a workgroup's chunk indices
// only grow, and by gridDim.x a step, so -- every job being a chunk at least -- its job lies between the previous one
// and gridDim.x jobs further on: at most 12 steps, none while it stays in a job of many chunks.  The index goes through
// readfirstlane, so the job's record, the tape's table entry, lo, the extents and the context rows are all read at
// wave-uniform addresses, from the buffer and not from the arguments.
// Both waves of a workgroup are on one tape: the chunk is decoded, tested and walked as pip_tape_sweep_kernel does it
// on the global-memory path, the walk starting at the tape's first word as in pip_tape_set_eval_kernel.  A lane touches
// its own column of the slot rows alone and a tape reads no slot it has not written, so nothing is cleared between jobs.
// Summary: no LDS bins.  The per-leaf figures go to the job's words by the wave-aggregated atomics of the sweep's
// unbinned path.  The status figures stay wave-uniform accumulators while the workgroup stays in a job and are flushed
// -- lanes 0 .. 3, one atomic instruction pair -- when it moves to another and at the end.
__global__ void pip_tape_set_sweep_fill_kernel(i64 *sum, const i64 *summary_off, const TapeSetSweepJob *jobs, int n_jobs, i64 words) {
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (i64)gridDim.x * blockDim.x) {
    int lo = 0, hi = n_jobs - 1;  // the job with summary_off[lo] <= i < summary_off[lo + 1]
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (summary_off[mid] <= i) lo = mid;
      else hi = mid - 1;
    }
    sum[i] = sweep_zero_word(i - summary_off[lo], jobs[lo].leaves) ? 0 : -1;
  }
}

// (the figures by value: selected through pointers they would be an indexed array, which lives in scratch)
__device__ __forceinline__ void sweep_flush_status(u64 *to, u64 c0, u64 c1, u64 c2, u64 c3, u64 f0, u64 f1, u64 f2, u64 f3, int lane) {
  if (lane < 4) {
    const u64 c = lane == 0 ? c0 : (lane == 1 ? c1 : (lane == 2 ? c2 : c3));
    const u64 f = lane == 0 ? f0 : (lane == 1 ? f1 : (lane == 2 ? f2 : f3));
    if (c) {
      atomicAdd(&to[PIPAMD_SWEEP_COUNT + lane], c);
      atomicMin(&to[PIPAMD_SWEEP_FIRST + lane], f);
    }
  }
}

template <class T>
__global__ __launch_bounds__(TAPE_BLOCK) void pip_tape_set_sweep_kernel(TapeSetSweepLaunch a) {
  typedef Width<T> W;
  constexpr int EW = W::EW;
  extern __shared__ __attribute__((aligned(16))) i64 tape_lds[];
  i64 *S = tape_lds;  // (a.slots - 1) * EW rows of TAPE_BLOCK words
  const int tid = threadIdx.x, lane = tid & 63;
  const i64 *chunk_off = a.buf;
  const TapeSetSweepJob *jobs = (const TapeSetSweepJob *)(a.buf + 2 * ((i64)a.n_jobs + 1));
  u64 *sum = (u64 *)a.summary;
  TapeOut none;  // (a summary alone: the walk writes nothing)
  none.status = none.leaf = nullptr;
  none.x_num = none.x_den = none.dual_num = none.dual_den = nullptr;
  none.xs = none.ds = 0;
  u64 cnt[4] = {0, 0, 0, 0}, first[4] = {~(u64)0, ~(u64)0, ~(u64)0, ~(u64)0};
  int j = 0;        // the workgroup's job
  i64 counted = -1;  // the summary offset of the job cnt and first are of; -1: they are of none

  for (i64 c = blockIdx.x; c < a.chunks; c += gridDim.x) {
    int lo = j, hi = (int)((i64)j + gridDim.x < (i64)a.n_jobs - 1 ? (i64)j + gridDim.x : (i64)a.n_jobs - 1);
    if (c < chunk_off[j + 1]) hi = j;  // (still in the job it was in)
    while (lo < hi) {
      const int mid = (int)(((i64)lo + hi + 1) >> 1);
      if (chunk_off[mid] <= c) lo = mid;
      else hi = mid - 1;
    }
    j = __builtin_amdgcn_readfirstlane(lo);
    const TapeSetSweepJob *J = jobs + j;
    const TapeSetEntry *e = a.table + J->tape;
    const i64 off = J->summary_off;
    if (counted != off) {  // (wave-uniform) another job: what the wave counted belongs to the one it leaves
      if (counted >= 0) sweep_flush_status(sum + counted, cnt[0], cnt[1], cnt[2], cnt[3], first[0], first[1], first[2], first[3], lane);
#pragma unroll
      for (int i = 0; i < 4; i++) cnt[i] = 0, first[i] = ~(u64)0;
      counted = off;
    }
    const int cols = e->point_cols;
    const i64 *box = a.buf + J->box;
    const i64 n = J->n_points, L = J->leaves, k0 = (c - J->chunk_off) * TAPE_BLOCK, pt = k0 + tid;
    const bool live = pt < n;
    box_point(box, (const u64 *)(box + cols), cols, k0, tid, S);
    const bool inside = box_inside(live, a.buf + J->ctx, J->n_ctx, cols, S, tid);
    if (EW == 2)
      for (int q = cols - 1; q >= 0; q--) W::set_slot(S, q, tid, (T)S[q * TAPE_BLOCK + tid]);

    int st = live && !inside ? PIPAMD_ST_OUTSIDE : PIPAMD_ST_NIL, leaf = -1;
    tape_walk<T, true>(a.prog, inside && e->words ? e->start : END, S, tid, e->nvar, e->ndual, pt, none, st, leaf);

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
    // per leaf, as pip_tape_sweep_kernel without bins: the lowest lane of every group adds (size, its k)
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
      u64 *to = sum + off;
      atomicAdd(&to[PIPAMD_SWEEP_LEAF_COUNT(L) + leaf], (u64)group);
      atomicMin(&to[PIPAMD_SWEEP_LEAF_FIRST(L) + leaf], (u64)pt);
    }
  }
  if (counted >= 0) sweep_flush_status(sum + counted, cnt[0], cnt[1], cnt[2], cnt[3], first[0], first[1], first[2], first[3], lane);
}

template <class T>
int set_sweep_blocks(int bits, int slots, int cus) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pip_tape_set_sweep_kernel<T>, TAPE_BLOCK, tape_slot_bytes(slots, bits)) != hipSuccess || per_cu < 1)
    per_cu = 1;
  if (per_cu > TAPE_SWEEP_WG_PER_CU_SUM) per_cu = TAPE_SWEEP_WG_PER_CU_SUM;
  return (cus > 0 ? cus : 1) * per_cu;
}
template <class T>
hipError_t launch_set_sweep(const TapeSetSweepLaunch &s, hipStream_t stream) {
  long long blocks = s.blocks > 0 ? s.blocks : 1;
  if (s.max_blocks > 0 && s.max_blocks < blocks) blocks = s.max_blocks;
  if (s.chunks < blocks) blocks = s.chunks;
  hipLaunchKernelGGL((pip_tape_set_sweep_kernel<T>), dim3((unsigned)blocks), dim3(TAPE_BLOCK), tape_slot_bytes(s.slots, s.bits), stream, s);
  return hipGetLastError();
}
}  // namespace

extern "C" int pipk_tape_set_sweep_blocks(int bits, int slots, int cus) {
  return bits == 128 ? set_sweep_blocks<i128>(bits, slots, cus) : set_sweep_blocks<i64>(bits, slots, cus);
}

extern "C" hipError_t pipk_launch_tape_set_sweep(const TapeSetSweepLaunch *s, hipStream_t stream) {
  // (pipamd_tape_set_sweep_create checked: 1 <= n_jobs <= 2^20, every tape index inside the set's table, every box of
  // 1 .. 2^38 - 1 points and all together below 2^38, every offset inside the buffer)
  if (s->n_jobs <= 0 || s->chunks <= 0) return hipSuccess;
  long long fill = (s->words + 255) / 256;
  if (fill > 65536) fill = 65536;
  hipLaunchKernelGGL(pip_tape_set_sweep_fill_kernel, dim3((unsigned)fill), dim3(256), 0, stream, s->summary, s->buf + s->n_jobs + 1,
                     (const TapeSetSweepJob *)(s->buf + 2 * ((long long)s->n_jobs + 1)), s->n_jobs, s->words);
  const hipError_t he = hipGetLastError();
  if (he != hipSuccess) return he;
  return s->bits == 128 ? launch_set_sweep<i128>(*s, stream) : launch_set_sweep<i64>(*s, stream);
}

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

extern "C" hipError_t pipk_launch_tape_values(const TapeValuesLaunch *v, hipStream_t stream) {
  // (the caller checked: 1 <= n_points < 2^38, nvar <= PIPAMD_VALUES_MAX_NVAR, slots <= TAPE_MAX_SLOTS, a staged program
  // within TAPE_LDS_BYTES beside the slots, `work` of tape_values_work_bytes)
  hipLaunchKernelGGL(pip_tape_sweep_fill_kernel, dim3(1), dim3(256), 0, stream, v->summary, 0);  // the eight head words
  const hipError_t he = hipGetLastError();
  if (he != hipSuccess) return he;
  if (v->t.marks) return v->t.bits == 128 ? launch_values<i128, true>(*v, stream) : launch_values<i64, true>(*v, stream);
  return v->t.bits == 128 ? launch_values<i128, false>(*v, stream) : launch_values<i64, false>(*v, stream);
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
