// piplib_amd/csrc/pip_kernels.hip -- hand-written HIP kernels for gfx950 (MI355X).
//
// The pivot kernel itself (pip_advance_kernel: traiter() / pivoter() / choisir_piv() / exam_coef() / integrer() /
// tab_sort_rows of the reference) lives in pip_advance.h and is instantiated by the pip_adv_*.hip files; this file
// holds the determinant replay, the batch load / results / counters kernels (pip_batch_load_system_kernel: the load from
// pip_solve's plain system), Compute_dual for the batch layer (pip_batch_dual_kernel),
// expanser for the batch layer, the helpers of the lock-step scheduler and every launcher.
#include "pip_lean.h"
#include "pip_host.h"

// the instantiations of the pivot kernel's launcher live in pip_adv_*.hip
#define PIP_ADV_EXTERN(...) extern template hipError_t launch_advance_t<__VA_ARGS__>(const AdvanceLaunch &);
PIP_ADV_GROUP_A(PIP_ADV_EXTERN)
PIP_ADV_GROUP_B(PIP_ADV_EXTERN)
PIP_ADV_GROUP_C(PIP_ADV_EXTERN)
PIP_ADV_GROUP_D(PIP_ADV_EXTERN)
PIP_ADV_GROUP_F(PIP_ADV_EXTERN)
#undef PIP_ADV_EXTERN
#define PIP_LEAN_EXTERN(SC, FULL) extern template hipError_t launch_lean<SC, FULL>(const AdvanceLaunch &);
PIP_LEAN_CLASSES(PIP_LEAN_EXTERN)
#undef PIP_LEAN_EXTERN
#define PIP_LEAN_BIG_EXTERN(SC) extern template hipError_t launch_lean<SC, false, true>(const AdvanceLaunch &);
PIP_LEAN_BIG_CLASSES(PIP_LEAN_BIG_EXTERN)
#undef PIP_LEAN_BIG_EXTERN
#define PIP_LEAN4_EXTERN(SC, FULL) extern template hipError_t launch_lean<SC, FULL, false, 4>(const AdvanceLaunch &);
PIP_LEAN4_CLASSES(PIP_LEAN4_EXTERN)
#undef PIP_LEAN4_EXTERN

// ------------------------------------------------------------- determinant replay
// traiter.c:394-446 for the pivots a launch logged: d = gcd(pivot, dpiv); the limbs lose the
// factors of dpiv / d (if some factor is left: "Integer overflow"); the first limb with room takes
// pivot / d (a fourth limb: "Integer overflow").  The bookkeeping never feeds back into the pivot
// loop, so it can trail it; an overflow found here overrides whatever the job's status became
// and sets the pivot count to the pivot that overflowed.  In the pivot loop itself this was
// wave-uniform scalar work: ~12 % of all instructions with 64-bit entries, ~18 % of the run time
// with 128-bit ones.
// One WAVE per job: gcd(pivot, dpiv) and the two quotients do not depend on the limbs, so the
// lanes compute them for 64 pivots at once; only the walk over the limbs is sequential, on the
// scalar unit.  Shortest latency: used where few jobs ran and someone waits for them.
template <class T>
__global__ __launch_bounds__(64) void pip_det_replay_kernel(PipJob *jobs, i64 *arena, int njobs, PipQueue q) {
  const int t = blockIdx.x, lane = threadIdx.x;
  const int nq = q.in_count ? *q.in_count : njobs;
  if (t >= nq) return;
  PipJob *J = &jobs[q.in_list ? q.in_list[t] : t];
  const int nlog = J->nlog;
  if (nlog <= 0 || (J->ebits == 128) != (sizeof(T) == 16)) return;
  const T *lg = (const T *)(arena + J->log_off);
  T det0 = uni(det_limb<T>(J, 0)), det1 = uni(det_limb<T>(J, 1)), det2 = uni(det_limb<T>(J, 2)),
    det3 = uni(det_limb<T>(J, 3));
  int ldet = __builtin_amdgcn_readfirstlane(J->ldet);
  int bad = -1;
  for (int base = 0; base < nlog && bad < 0; base += 64) {
    const int k = base + lane;
    T pp = 1, dp = 1;
    if (k < nlog) {
      pp = lg[2 * k];
      dp = lg[2 * k + 1];
      if (dp != 1) {
        const T d = gcd_i64(pp, dp);
        if (d != 1) {
          pp = exact_quo(pp, d);
          dp = exact_quo(dp, d);
        }
      }
    }
    const int n = nlog - base < 64 ? nlog - base : 64;
    for (int j = 0; j < n; j++) {
      if (!det_step<T>(det0, det1, det2, det3, ldet, readlane(pp, j), readlane(dp, j))) {
        bad = base + j;  // traiter.c:424,442: the reference exits inside this call of pivoter
        break;
      }
    }
  }
  if (lane == 0) {
    if (bad >= 0) {
      J->npiv = J->npiv - det_unlogged(J) - nlog + bad + 1;
      J->status = PIPAMD_ST_OVERFLOW;
    }
    det_limb_store<T>(J, 0, det0);
    det_limb_store<T>(J, 1, det1);
    det_limb_store<T>(J, 2, det2);
    det_limb_store<T>(J, 3, det3);
    J->ldet = ldet;
    J->nlog = 0;
  }
}

// One LANE per job (64 jobs per wave): far fewer instructions issued in all -- what counts behind
// a bulk launch, when the GPU is kept busy by other batches -- at the price of a longer latency
// per job (a lane walks its log alone).
template <class T>
__global__ __launch_bounds__(64) void pip_det_replay_lanes_kernel(PipJob *jobs, i64 *arena, int njobs, PipQueue q) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int nq = q.in_count ? *q.in_count : njobs;
  if (t >= nq) return;
  PipJob *J = &jobs[q.in_list ? q.in_list[t] : t];
  det_replay_lane<T, sizeof(T) == 16 ? 4 : 8>(J, arena);  // (a chunk: the log entries of a 128-byte line)
}

// ---------------------------------------------------------------- batch load
// tab_alloc + tab_get (tab.c:158-248) for a uniform batch: nvar unit rows, then
// ni Unknown rows with denominator 1; spare slots and columns zeroed.  Input rows are int64
// whatever the entry type of the tableau.  The three pieces below are what every load kernel does around its own way
// of writing the ni input rows.

// the row tables of a block: unit rows, unknown rows, empty slots
template <class T>
__device__ __forceinline__ void load_row_tables(i64 *blk, const PipBatchLayout &lay, int ni, int tid) {
  const auto [g_den, g_flag, g_ref] = pip_row_tables<T>(blk, lay.blk.L);
  for (int i = tid; i < lay.blk.L; i += blockDim.x) {
    if (i < lay.nvar) {
      g_flag[i] = PIPAMD_F_UNIT;
      g_ref[i] = i;
      g_den[i] = 1;
    } else if (i < lay.nvar + ni) {
      g_flag[i] = PIPAMD_F_UNKNOWN;
      g_ref[i] = i - lay.nvar;
      g_den[i] = 1;
    } else {
      g_flag[i] = 0;
      g_ref[i] = 0;
      g_den[i] = 0;
    }
  }
}

// spare slots (the rows from first_pad_row on) only need their columns beyond ncol cleared: a cut row writes its
// first ncol columns itself, a parametric cut relies on the new column being 0 elsewhere
template <class T>
__device__ __forceinline__ void load_clear_spare(T *vals, const PipBatchLayout &lay, int first_pad_row, int tid) {
  const int ncol = lay.nvar + lay.nparm + 1, pad = lay.W - ncol;
  for (int e = tid; e < (lay.S - first_pad_row) * pad; e += blockDim.x) {
    int s = first_pad_row + e / pad, j = ncol + e % pad;
    vals[(size_t)s * lay.W + j] = 0;
  }
}

// the job header (one thread) of a tableau of `ni` rows that starts with `status`.  defer (PIPAMD_T_ROWS_STAY): the first
// pivot launch fetches the rows from `src` itself
template <class T>
__device__ __forceinline__ void load_job_header(PipJob *J, int64_t base, const PipBatchLayout &lay, int ni, int status, bool defer,
                                                const i64 *src) {
  pip_job_place(J, base, lay.blk);
  J->nlog = 0;
  J->nvar = lay.nvar;
  J->nparm = lay.nparm;
  J->ni = ni;
  J->bigparm = lay.bigparm;
  J->tflags = lay.tflags | PIPAMD_T_SORT | (defer ? PIPAMD_T_FRESHROWS : 0);
  J->src_rows = defer ? (int64_t)(uintptr_t)src : 0;
  J->home_sol_off = 0;
  J->S = lay.S;
  J->W = lay.W;
  J->status = status;
  J->aux = 0;
  J->npiv = 0;
  J->ncut = 0;
  J->nupd = 0;
  J->ldet = 1;
  for (int i = 0; i < 2 * PIPAMD_MAXDET; i++) J->det[i] = 0;
  J->det[0] = 1;
  J->maxabs = 0;
  J->state_nch = 0;
  J->ebits = ET<T>::BITS;
}

// pipamd_batch_load: `rows` holds the tableau rows themselves, nvar + nparm + 1 columns a row
template <class T>
__global__ void pip_batch_load_kernel(PipJob *jobs, i64 *arena, const i64 *rows, PipBatchLayout lay, int first) {
  constexpr int EW = ET<T>::EW;
  const int b = first + blockIdx.x;  // `rows` holds the tableaux first, first + 1, ... of the batch
  const int tid = threadIdx.x;
  const int ncol = lay.nvar + lay.nparm + 1;
  const int64_t base = lay.arena_off + (int64_t)b * lay.blk.words;
  T *vals = (T *)(arena + base + lay.blk.vals);
  load_row_tables<T>(arena + base, lay, lay.ni, tid);
  const i64 *src = rows + (size_t)blockIdx.x * lay.ni * ncol;
  const bool defer = lay.pad != 0 && EW == 1;  // PIPAMD_T_ROWS_STAY: the first pivot launch fetches the rows itself
  if (!defer) {
    // (row, column) advance with the thread stride: no division per element
    const int ds = (int)blockDim.x / lay.W, dj = (int)blockDim.x % lay.W;
    int s = tid / lay.W, j = tid % lay.W;
    for (int e = tid; e < lay.ni * lay.W; e += blockDim.x) {
      vals[e] = j < ncol ? (T)src[(size_t)s * ncol + j] : (T)0;
      s += ds;
      j += dj;
      if (j >= lay.W) {
        j -= lay.W;
        s++;
      }
    }
  }
  load_clear_spare(vals, lay, defer ? 0 : lay.ni, tid);
  if (tid == 0) load_job_header<T>(&jobs[b], base, lay, lay.ni, PIPAMD_ST_RUN, defer, src);
}

// ---------------------------------------------------------------- batch load from a plain system
// pipamd_batch_load_system: tab_Matrix2Tableau (tab.c:328-389) and, for integer problems, tab_simplify (tab.c:396-427)
// for a uniform batch.  `rows` holds the caller's system, nrows x (nvar + 1) int64 a tableau; input row r becomes
// tableau row r + (equalities before r): a_j | c without a shift; under a new big parameter (tab.c:342-377; the layout
// has nparm == 1, bigparm == nvar + 1) -a_j | c | +sum a_j for shift > 0 (Maximize) and a_j | c | -sum a_j for
// shift < 0 (Urs_unknowns), the sum in the entry type (64-bit entries: it wraps as the reference's long long build
// does); an equality is followed by its negation in every column.  One WAVE per input row, a lane per column (CPL
// columns a lane): the row's sum and the gcd of its columns are reductions over the lanes that hold it.
// pipamd_batch_load_shifted is the launch with no equality, simplify == 0 and nrows == ni.
// (pip_wide.h's wave_sum, spelled with the lane the kernel already holds: through xor-shuffles the load kernels are 21 to
// 25 instructions longer each)
template <class T>
__device__ __forceinline__ T sys_wave_sum(T v, int lane) {
  for (int o = 32; o; o >>= 1) v = wadd(v, shfl(v, lane ^ o));
  return v;
}
// gcd of the lanes' magnitudes (gcd(0, x) = x); any bit pattern ends the binary gcd
__device__ __forceinline__ u64 sys_wave_gcd(u64 g, int lane) {
  for (int o = 32; o; o >>= 1) g = gcd_mag(g, (u64)shfl((i64)g, lane ^ o));
  return (u64)uni((i64)g);
}
// x / g for a g > 1 that divides x; g is a magnitude of up to 64 bits (2^63 for a row of INT64_MINs)
__device__ __forceinline__ i64 sys_exact(i64 x, u64 g) {
  const u64 q = uabs(x) / g;
  return x < 0 ? wneg((i64)q) : (i64)q;
}
__device__ __forceinline__ i128 sys_exact(i128 x, u64 g) { return cquo(x, (i128)g); }
// floor(c / g), g > 1, for a constant of at most 2^63 in magnitude (an input value or its negation)
template <class T>
__device__ __forceinline__ T sys_floor(T c, u64 g) {
  const u64 uc = (u64)uabs(c);
  return c < 0 ? wneg((T)(i64)((uc + (g - 1)) / g)) : (T)(i64)(uc / g);
}

// Which rows are equalities, and how many rows a system has, is the kernel's EQ policy (pip_batch_dual_kernel below has
// the same ones):
//   PipEqMask: one mask and one row count for the batch, both from the launch (pipamd_batch_load_system, _shifted).
//   PipEqMarkers (pipamd_batch_load_matrices): every system has max_rows rows of room, nvar + 2 words a row with the
//     PolyLib marker first (0: an equality), and a row count of its own on the device.  The block builds the system's
//     mask words in LDS from the marker column, a ballot per 64 rows, and its tableau has ni_b = rows + equalities rows
//     of the lay.ni the layout has room for.  A system whose count is below 1 or above max_rows, or whose tableau does
//     not fit, is finished here: no row of it is read, its tableau is empty and its status PIPAMD_ST_BADINPUT.
//   PipNoEq (the dual kernel only): no equalities, nothing travels with the launch.
struct PipNoEq {};
__device__ __forceinline__ u64 eq_word(const PipEqMask &eq, const u64 *, int w) { return eq.w[w]; }
__device__ __forceinline__ u64 eq_word(const PipEqMarkers &, const u64 *words, int w) { return words[w]; }
__device__ __forceinline__ u64 eq_word(const PipNoEq &, const u64 *, int) { return 0; }

// PipEqMarkers, by the NWAVE waves of a block: the mask words of system `sys` of the launch, whose rows start at `src`
// (`srcrow` words a row), into `words` (LDS; room for the words of min(max_rows, room) rows).  Returns the system's row
// count and, in ni_b, its tableau's; both 0 for a bad system.  Every thread of the block gets the same answer.
template <int NWAVE>
__device__ __forceinline__ int eq_from_markers(const PipEqMarkers &mk, int sys, const i64 *src, int srcrow, int room, u64 *words,
                                               int &ni_b) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int n = __builtin_amdgcn_readfirstlane(mk.nrows ? mk.nrows[sys] : mk.max_rows);
  if (n < 1 || n > mk.max_rows || n > room) n = 0;
  const int nw = (n + 63) >> 6;
  for (int q = wave; q < nw; q += NWAVE) {
    const int r = 64 * q + lane;
    const u64 word = ballot64(r < n && src[(size_t)r * srcrow] == 0);
    if (lane == 0) words[q] = word;
  }
  __syncthreads();
  int neq = 0;
  for (int q = 0; q < nw; q++) neq += __popcll(words[q]);
  if (n + neq > room) n = 0;
  ni_b = n ? n + neq : 0;
  return n;
}

// Where a lane's input value comes from is the kernel's SRC policy (pip_batch_dual_kernel has the same ones):
//   PipDenseRows: `rows`, nvar + 1 (+ marker) int64 a row; the lane reads its columns.  Nothing travels with the launch.
//   PipCsrRows (pipamd_batch_load_sparse; with PipEqMask): a row's stored entries, column and value, strictly
//     increasing columns, the constant as column nvar.  The wave reads them 64 at a time, an entry per lane, and a
//     readlane loop over the entries hands each value to the lane that owns its column: a sparse row has a few
//     entries, the loop costs as many steps, and neither LDS nor a register is added to the dense instantiations.
//     Before anything is stored the block checks the system (csr_system_ok); a bad one is finished here as the
//     markers policy finishes its bad systems: an empty tableau, PIPAMD_ST_BADINPUT.
//   PipInstanceRows (pipamd_batch_load_instances; with PipEqMask): ONE matrix for the launch, unknowns | parameters |
//     constant, and a point per system.  The block reads its point once into LDS; a lane reads its unknown columns from
//     the shared matrix (every block reads the same lines: they stay in L2) and the constant's lane gets c_r +
//     sum_k p_rk * theta_k, summed exactly across the wave (inst_constant).  All constants are formed, and the system
//     declared bad if one does not fit the entry type, before anything is stored; the main loop takes them from LDS.
struct PipDenseRows {};
// words of a source row between its unknowns and its constant
__device__ __forceinline__ int src_parms(const PipDenseRows &) { return 0; }
__device__ __forceinline__ int src_parms(const PipCsrRows &) { return 0; }
__device__ __forceinline__ int src_parms(const PipInstanceRows &is) { return is.nparm; }

// PipCsrRows, by all waves of a block: may system `sys` of the launch (`nrows` rows) be read?  First its nrows + 1
// pointers: within [0, nnz], not decreasing, at most nvar + 1 entries a row; then, only if they hold, its entries: every
// column strictly above its predecessor in the row (above -1 for the first: none is negative) and at most nvar.
// Nothing of cols is read outside [0, nnz) and nothing of vals at all.  Every thread gets the same answer.
__device__ __forceinline__ bool csr_system_ok(const PipCsrRows &cs, int sys, int nrows, int nvar) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwave = (int)blockDim.x >> 6;
  const i64 *rp = (const i64 *)cs.row_ptr + (size_t)sys * nrows;
  bool ok = true;
  for (int r = tid; r < nrows; r += blockDim.x) {
    const i64 p0 = rp[r], p1 = rp[r + 1];
    ok = ok && p0 >= 0 && p1 >= p0 && p1 <= cs.nnz && p1 - p0 <= nvar + 1;
  }
  if (!__syncthreads_and(ok)) return false;
  for (int r = wave; r < nrows; r += nwave) {
    const i64 p0 = rp[r], p1 = rp[r + 1];
    for (i64 e = p0 + lane; e < p1; e += 64) {
      const int c = cs.cols[e], prev = e > p0 ? cs.cols[e - 1] : -1;
      ok = ok && c > prev && c <= nvar;
    }
  }
  return __syncthreads_and(ok);
}

// PipCsrRows: the values of the row whose entries are p0 .. p1 - 1 (checked), to the lanes that own their columns:
// a[c] of lane l is column l + 64 * c, zero where nothing is stored
template <int CPL>
__device__ __forceinline__ void csr_row_to_lanes(const PipCsrRows &cs, i64 p0, i64 p1, int lane, i64 (&a)[CPL]) {
#pragma unroll
  for (int c = 0; c < CPL; c++) a[c] = 0;
  for (i64 e0 = p0; e0 < p1; e0 += 64) {
    const int n = p1 - e0 < 64 ? (int)(p1 - e0) : 64;
    const int col = lane < n ? cs.cols[e0 + lane] : 0;
    const i64 val = lane < n ? cs.vals[e0 + lane] : 0;
    for (int i = 0; i < n; i++) {
      const int ci = __builtin_amdgcn_readlane(col, i);
      const i64 vi = readlane(val, i);
      if (lane == (ci & 63)) {
#pragma unroll
        for (int c = 0; c < CPL; c++)
          if (c == (ci >> 6)) a[c] = vi;
      }
    }
  }
}

// PipInstanceRows, by one wave: the constant of a matrix row at the block's point.  `row` points at the row's parameter
// columns (nparm of them, then c), `theta` at the point in LDS: c + sum_k p_k * theta_k, exactly.  A product of two int64
// values is below 2^126 in magnitude; its signed high and its unsigned low 64-bit half go to 128-bit accumulators of
// their own, the constant as one more term -- at most 512 terms, so either sum stays below 2^73 and nothing wraps --,
// first within a lane, then over the lanes that hold a term (a butterfly from `top` down; inst_top below).  Only the
// totals are joined, value = hi * 2^64 + low word with 0 <= low word < 2^64, and held against the entry type.  Returns
// whether the value fits T; every lane gets the same answer and, if it fits, the value in `out`.
__device__ __forceinline__ int inst_top(int nparm) {
  int top = 1;
  while (top < 64 && top < nparm + 1) top <<= 1;
  return top >> 1;
}
template <class T>
__device__ __forceinline__ bool inst_constant(const i64 *row, const i64 *theta, int nparm, int top, int lane, T &out) {
  i128 hi = 0;
  u128 lo = 0;
  for (int k = lane; k < nparm; k += 64) {
    const i128 p = (i128)row[k] * (i128)theta[k];
    hi += (i128)(i64)(p >> 64);
    lo += (u128)(u64)(u128)p;
  }
  if (lane == (nparm < 64 ? nparm : 0)) {
    const i64 c = row[nparm];
    hi += (i128)(c >> 63);
    lo += (u128)(u64)c;
  }
  for (int o = top; o; o >>= 1) {
    hi = wadd(hi, shfl(hi, lane ^ o));
    lo = (u128)wadd((i128)lo, shfl((i128)lo, lane ^ o));
  }
  hi = uni(hi);  // lane 0 has the totals
  lo = (u128)uni((i128)lo);
  hi += (i128)(u64)(lo >> 64);
  const u64 l0 = (u64)lo;
  if constexpr (sizeof(T) == 8) {
    out = (T)(i64)l0;
    return hi == (i128)((i64)l0 >> 63);
  } else {
    out = (T)(((u128)hi << 64) | l0);
    return fits64(hi);
  }
}
// floor(c / g), g > 1, for a constant of PipInstanceRows: any value of the entry type.  Within 2^63 it is sys_floor.
__device__ __forceinline__ i64 inst_floor(i64 c, u64 g) { return sys_floor(c, g); }
__device__ __forceinline__ i128 inst_floor(i128 c, u64 g) {
  const u128 uc = uabs(c);  // (2^127 for the smallest value)
  if ((uc >> 63) == 0) return sys_floor(c, g);
  const u128 rem = umod128(uc, (u128)g);
  const int s = __builtin_ctzll(g);
  u128 q = ((uc - rem) >> s) * inv_odd((u128)(g >> s));  // exact, and below 2^127: g >= 2
  if (c < 0 && rem) q += 1;
  return c < 0 ? wneg((i128)q) : (i128)q;
}
#define PIP_INST_KEEP 512 /* rows of a system whose constants the load kernel keeps in LDS; later rows are formed twice */

template <class T, int CPL, class EQ, class SRC>
__global__ __launch_bounds__(256) void pip_batch_load_system_kernel(PipJob *jobs, i64 *arena, const i64 *rows, PipBatchLayout lay,
                                                                    int first, int shift, int simplify, int nrows, EQ eq,
                                                                    SRC rs) {
  typedef typename ET<T>::U U;
  constexpr bool MARKED = std::is_same<EQ, PipEqMarkers>::value;
  constexpr bool CSR = std::is_same<SRC, PipCsrRows>::value;
  constexpr bool INST = std::is_same<SRC, PipInstanceRows>::value;
  static_assert(!(MARKED && CSR), "sparse rows come with the launch's equality mask");
  static_assert(!(MARKED && INST), "instances of one system come with the launch's equality mask");
  constexpr int MK = MARKED ? 1 : 0;  // words of a source row before its unknowns
  const int b = first + blockIdx.x;  // `rows` holds the systems first, first + 1, ... of the batch
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nvar = lay.nvar, srccol = nvar + 1, srcrow = srccol + MK + src_parms(rs), W = lay.W;
  const int64_t base = lay.arena_off + (int64_t)b * lay.blk.words;
  T *vals = (T *)(arena + base + lay.blk.vals);
  int ni = lay.ni;  // rows of this tableau
  const i64 *src;
  const u64 *eqw = nullptr;
  if constexpr (MARKED) {
    __shared__ u64 words[(PIPAMD_SMAX + 63) / 64];
    src = rows + (size_t)blockIdx.x * eq.max_rows * srcrow;
    nrows = eq_from_markers<4>(eq, blockIdx.x, src, srcrow, lay.ni, words, ni);
    eqw = words;
  }
  bool bad = false;  // (PipCsrRows, PipInstanceRows)
  if constexpr (CSR) {
    bad = !csr_system_ok(rs, blockIdx.x, nrows, nvar);
    if (bad) nrows = ni = 0;
  }
  const i64 *theta = nullptr;  // (PipInstanceRows) the block's point and its rows' constants, in LDS
  const T *konst = nullptr;
  int top = 0;
  if constexpr (INST) {
    __shared__ i64 point[PIPAMD_MAXCOL];
    __shared__ T kept[PIP_INST_KEEP];
    const int np = rs.nparm;
    for (int k = tid; k < np; k += 256) point[k] = (i64)rs.points[(size_t)blockIdx.x * np + k];
    __syncthreads();
    top = inst_top(np);
    bool ok = true;
    for (int r = wave; r < nrows; r += 4) {
      T c;
      ok = inst_constant<T>((const i64 *)rs.matrix + (size_t)r * srcrow + nvar, point, np, top, lane, c) && ok;
      if (lane == 0 && r < PIP_INST_KEEP) kept[r] = c;
    }
    bad = !__syncthreads_and(ok);
    if (bad) nrows = ni = 0;
    theta = point;
    konst = kept;
  }
  load_row_tables<T>(arena + base, lay, ni, tid);
  if constexpr (INST)
    src = (const i64 *)rs.matrix;
  else if constexpr (!MARKED && !CSR)
    src = rows + (size_t)blockIdx.x * nrows * srccol;
  int wcur = 0, before = 0;  // equalities among the rows below 64 * wcur
  for (int r = wave; r < nrows; r += 4) {
    for (; wcur < (r >> 6); wcur++) before += __popcll(eq_word(eq, eqw, wcur));
    const u64 word = eq_word(eq, eqw, r >> 6);
    const int k = r + before + __popcll(word & ((1ull << (r & 63)) - 1));
    const bool twin = (word >> (r & 63)) & 1;
    if (k + (int)twin >= ni) break;  // (the host has held the list against ni; the markers' count gave ni)
    const i64 *in = CSR ? nullptr : src + (size_t)r * srcrow + MK;
    i64 sp[CSR ? CPL : 1];  // PipCsrRows: the row's values, each in the lane of its column
    if constexpr (CSR) {
      const i64 *rp = (const i64 *)rs.row_ptr + (size_t)blockIdx.x * nrows + r;
      csr_row_to_lanes<CPL>(rs, uni(rp[0]), uni(rp[1]), lane, sp);
    }
    T cst = 0;  // PipInstanceRows: the row's constant at the block's point
    if constexpr (INST) {
      if (r < PIP_INST_KEEP)
        cst = konst[r];
      else
        inst_constant<T>(in + nvar, theta, rs.nparm, top, lane, cst);
    }
    T v[CPL], sum = 0;
    u64 g = 0;
#pragma unroll
    for (int c = 0; c < CPL; c++) {
      const int j = lane + 64 * c;
      i64 a;
      if constexpr (CSR)
        a = sp[c];
      else if constexpr (INST)
        a = j < nvar ? in[j] : 0;
      else
        a = j < srccol ? in[j] : 0;
      v[c] = (T)a;  // the constant as it is, zero beyond it
      if constexpr (INST)
        if (j == nvar) v[c] = cst;
      if (j < nvar) {
        sum = wadd(sum, (T)a);
        if (simplify) g = gcd_mag(g, uabs(a));
        if (shift > 0) v[c] = wneg((T)a);
      }
    }
    T big = 0;
    if (shift) {  // the new column, tab.c:368-377
      sum = sys_wave_sum(sum, lane);
      big = shift > 0 ? sum : wneg(sum);
#pragma unroll
      for (int c = 0; c < CPL; c++)
        if (lane + 64 * c == nvar + 1) v[c] = big;
    }
    // tab_simplify: the gcd of every column but the constant, the new one included; a row with 0 or 1 stays.  It is below
    // 2^64 in the 128-bit flavour too: it divides an input value, or every one of them is zero and so is their exact sum
    if (simplify) {
      g = sys_wave_gcd(g, lane);
      if (shift) g = (u64)gcd_mag((U)g, (U)uni((T)uabs(big)));
    }
    T *out = vals + (size_t)k * W;
#pragma unroll
    for (int c = 0; c < CPL; c++) {
      const int j = lane + 64 * c;
      if (j >= W) continue;
      T x = v[c], y = wneg(x);
      if (g > 1) {
        if (j == nvar) {
          x = INST ? inst_floor(x, g) : sys_floor(x, g);
          y = INST ? inst_floor(y, g) : sys_floor(y, g);
        } else {
          x = sys_exact(x, g);
          y = wneg(x);
        }
      }
      out[j] = x;
      if (twin) out[W + j] = y;
    }
  }
  load_clear_spare(vals, lay, ni, tid);
  if (tid == 0)
    load_job_header<T>(&jobs[b], base, lay, ni, (MARKED && nrows == 0) || bad ? PIPAMD_ST_BADINPUT : PIPAMD_ST_RUN, false,
                       nullptr);
}

// sol_vector_edit (sol.c:435-512) with SOL_REMOVE and SOL_MAX / SOL_SHIFT for a batch solved under a big parameter
// (nparm == 1; the job's solution block holds big coefficient then constant per unknown, then the denominators): the
// value of unknown i is constant / denominator in lowest terms, negated for Maximize (shift > 0); its denominator is 0
// -- the reference's mark for "unbounded" -- unless the big coefficient equals the denominator (the shift cancels).
// A tableau that is not PIPAMD_ST_SOLUTION gets (0, 0) throughout.
template <class T>
__global__ void pip_batch_results_shifted_kernel(const PipJob *jobs, const i64 *arena, int njobs, int nvar, int shift, int *status,
                                                 int *pivots, int *cuts, T *x_num, T *x_den) {
  const int b = blockIdx.x;
  if (b >= njobs) return;
  const PipJob *J = &jobs[b];
  if (threadIdx.x == 0) {
    if (status) status[b] = J->status;
    if (pivots) pivots[b] = J->npiv;
    if (cuts) cuts[b] = J->ncut;
  }
  const T *sn = (const T *)(arena + J->sol_off);
  const bool ok = J->status == PIPAMD_ST_SOLUTION;
  for (int i = threadIdx.x; i < nvar; i += blockDim.x) {
    T xn = 0, xd = 0;
    if (ok) {
      const T B = sn[2 * i], N = sn[2 * i + 1], D = sn[2 * nvar + i];
      T g = gcd_i64(N, D);  // (gcd(0, D) = |D|)
      if (g == 0) g = 1;
      xn = cquo(N, g);
      if (shift > 0) xn = wneg(xn);
      xd = B != D ? (T)0 : cquo(D, g);
    }
    if (x_num) x_num[(size_t)b * nvar + i] = xn;
    if (x_den) x_den[(size_t)b * nvar + i] = xd;
  }
}

template <class T>
__global__ void pip_batch_results_kernel(const PipJob *jobs, const i64 *arena, int njobs, int nvar, int nparm,
                                         int *status, int *pivots, int *cuts, T *sol_num, T *sol_den) {
  const int b = blockIdx.x;
  const PipJob *J = &jobs[b];
  if (threadIdx.x == 0) {
    if (status) status[b] = J->status;
    if (pivots) pivots[b] = J->npiv;
    if (cuts) cuts[b] = J->ncut;
  }
  const int nn = nvar * (nparm + 1);
  const T *sn = (const T *)(arena + J->sol_off);
  const bool ok = J->status == PIPAMD_ST_SOLUTION;
  if (sol_num)
    for (int e = threadIdx.x; e < nn; e += blockDim.x) sol_num[(size_t)b * nn + e] = ok ? sn[e] : (T)0;
  if (sol_den)
    for (int i = threadIdx.x; i < nvar; i += blockDim.x) sol_den[(size_t)b * nvar + i] = ok ? sn[nn + i] : (T)0;
}

// totals over a batch: [0] pivots [1] cuts [2] rows rewritten [3] jobs finished (solution or nil)
__global__ void pip_batch_counters_kernel(const PipJob *jobs, int njobs, unsigned long long *out) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= njobs) return;
  const PipJob *J = &jobs[b];
  atomicAdd(&out[0], (unsigned long long)J->npiv);
  atomicAdd(&out[1], (unsigned long long)J->ncut);
  atomicAdd(&out[2], (unsigned long long)J->nupd);
  if (J->status == PIPAMD_ST_SOLUTION || J->status == PIPAMD_ST_NIL) atomicAdd(&out[3], 1ull);
}

// ---------------------------------------------------------------- Compute_dual for the batch layer
// solution_dual (traiter.c:273-294) for the tableaux of a uniform batch without parameters, after their rational solve:
// one wave per tableau.  Nothing of tab_sort_rows' `pos` table survives the solve, so it is recomputed from the input
// rows -- the keys of traiter.c:576-589 as pip_advance_kernel's entry pass forms them for denominator 1, then the
// selection sort of traiter.c:591-614 on (key, inequality) pairs -- and the values are read from the job's final row
// tables in HBM (den | flag | ref by LOGICAL row, as publish_row_tables leaves them) and its logical row 0 in the general
// row format.  Every loop bound comes from the launch's layout; what is read from the tables is range-checked.
#define PIP_DUAL_MAXNI 8192 /* inequalities per tableau: 6 bytes of LDS each, 48 KB */
extern "C" int pipk_batch_dual_max_ni(void) { return PIP_DUAL_MAXNI; }
extern "C" size_t pipk_batch_dual_lds_bytes(int ni) { return (6 * (size_t)(ni > 0 ? ni : 1) + 15) & ~(size_t)15; }

// |(int)a| of traiter.c:583 for an entry under denominator 1: an entry that does not fit an int gives INT_MIN (x86
// cvttsd2si), and abs(INT_MIN) stays negative, so neither it nor -2^31 itself ever wins the row's maximum
__device__ __forceinline__ int dual_key_term(i64 v) {
  const int q = (v == (i64)(int)v) ? (int)v : (int)0x80000000;
  return q < 0 ? (int)(0u - (unsigned)q) : q;
}

// The selection sort of traiter.c:591-614 on the pairs (key[r], ineq[r]), r < n, in LDS; one wave.  It chooses and
// swaps exactly as sort_rows (pip_advance.h) does in both of its forms: for r = 0, 1, ... the first pair at or after r
// with the smallest key strictly below smax goes to r (pairs whose key is not below smax are never picked, and nothing
// is swapped when none is left); the pair that sat at r takes its place (not stable).
__device__ void dual_sort_pairs(float *key, u16 *ineq, int n, double smax, int lane) {
  if (n <= 64) {
    // a pair per lane, in registers; keys are non-negative floats, so their bit patterns order like the values
    unsigned k = 0xFFFFFFFFu, id = (unsigned)lane;
    if (lane < n) {
      const float sj = key[lane];
      if ((double)sj < smax) k = __float_as_uint(sj);
    }
    for (int i = 0; i < n; i++) {
      const unsigned m = wave_minmax_u32<false>(lane >= i ? k : 0xFFFFFFFFu);
      if (m == 0xFFFFFFFFu) break;  // nothing below smax is left: this pair and all behind it stay
      const int pv = __builtin_ctzll(ballot64(lane >= i && k == m));
      if (pv != i) {
        const unsigned ki = __builtin_amdgcn_readlane(k, i), di = __builtin_amdgcn_readlane(id, i);
        const unsigned dp = __builtin_amdgcn_readlane(id, pv);
        if (lane == pv) {
          k = ki;
          id = di;
        }
        if (lane == i) {
          k = m;
          id = dp;
        }
      }
    }
    if (lane < n) ineq[lane] = (u16)id;
    __syncthreads();
    return;
  }
  for (int i = 0; i < n; i++) {
    float best = 0;
    int bj = BIG_I;
    for (int j = i + lane; j < n; j += 64) {
      const float sj = key[j];
      if (!((double)sj < smax)) continue;
      if (bj == BIG_I || sj < best) {
        best = sj;
        bj = j;
      }
    }
    for (int o = 32; o; o >>= 1) {  // the smallest key, the lowest index among equals
      const float ob = __shfl(best, lane ^ o);
      const int oj = __shfl(bj, lane ^ o);
      if (oj != BIG_I && (bj == BIG_I || ob < best || (ob == best && oj < bj))) {
        best = ob;
        bj = oj;
      }
    }
    if (bj == BIG_I) break;  // (keys do not change: no later i finds one either)
    if (bj != i && lane == 0) {
      const float tk = key[bj];
      key[bj] = key[i];
      key[i] = tk;
      const u16 td = ineq[bj];
      ineq[bj] = ineq[i];
      ineq[i] = td;
    }
    __syncthreads();
  }
  __syncthreads();
}

// `rows` holds the int64 rows the tableaux first, first + 1, ... were loaded from, nrows x (nvar + 1) a tableau, of
// which `eq` marks the equalities: the tableau has ni = nrows + equalities rows.  tab_sort_rows saw the expanded rows: a
// row's key is taken over the unknown columns alone (traiter.c:581), where a shift and the negation change signs only,
// so an equality's two rows have the key of the input row.  dual_num / dual_den: [batch][nrows] values of the entry
// type, one pair per INPUT row.  A tableau that is not PIPAMD_ST_SOLUTION, or whose header or tables are not what a
// finished solve of this layout leaves, gets (0, 0) throughout.
//   EQ == PipNoEq (pipamd_batch_dual: rows loaded by pipamd_batch_load, so no equalities and nrows == ni; no mask
//     travels with the launch): the pair solution_dual hands to sol_val, not reduced.
//   EQ == PipEqMask (pipamd_batch_dual_system, with or without a big parameter): the pair as pip_solve hands it out,
//     reduced as sol_vector_edit with flags 0 reduces it (sol.c:475-500), and for an equality with the values u (its
//     row) and v (the negated row) u if u != 0, else -v (piplib.c:670-688).
//   EQ == PipEqMarkers (pipamd_batch_dual_matrices): the same pair, for systems of max_rows rows of room that carry
//     their markers and a row count each (eq_from_markers above: the mask the load built, rebuilt from the same rows).
//     The tableau at hand has ni_b = rows + equalities rows, which its header must agree with, and ni_b pairs are
//     sorted; the LDS tables keep the room of lay.ni.  [batch][max_rows] pairs are written, (0, 0) from the system's
//     row count on, and throughout for a bad system.
//   SRC == PipCsrRows (pipamd_batch_dual_sparse, with PipEqMask): the rows are the CSR arrays the batch was loaded
//     from.  A row's key is the maximum over its stored entries with a column below nvar -- an absent entry is a zero
//     and adds nothing.  A system csr_system_ok refuses was bad for the load: (0, 0) throughout.
//   SRC == PipInstanceRows (pipamd_batch_dual_instances, with PipEqMask): the rows are those of the launch's shared
//     matrix; a key is taken over the unknown columns alone, which the point does not touch, so neither the point nor
//     the parameter columns are read.  A system that was bad for the load has status PIPAMD_ST_BADINPUT and an empty
//     tableau: (0, 0) throughout by the header check below.
template <class T, class EQ, class SRC>
__global__ __launch_bounds__(64) void pip_batch_dual_kernel(const PipJob *jobs, const i64 *arena, const i64 *rows,
                                                            PipBatchLayout lay, int first, int nrows, EQ eq, T *dual_num,
                                                            T *dual_den, SRC rs) {
  constexpr bool SYSTEM = !std::is_same<EQ, PipNoEq>::value;
  constexpr bool MARKED = std::is_same<EQ, PipEqMarkers>::value;
  constexpr bool CSR = std::is_same<SRC, PipCsrRows>::value;
  constexpr bool INST = std::is_same<SRC, PipInstanceRows>::value;
  static_assert(!CSR || std::is_same<EQ, PipEqMask>::value, "sparse rows come with the launch's equality mask");
  static_assert(!INST || std::is_same<EQ, PipEqMask>::value, "instances of one system come with the launch's equality mask");
  constexpr int MK = MARKED ? 1 : 0;  // words of a source row before its unknowns
  extern __shared__ __align__(16) unsigned char dual_lds[];
  const int lane = threadIdx.x;
  const int b = first + blockIdx.x;
  const int nvar = lay.nvar, srccol = lay.nvar + 1, srcrow = srccol + MK + src_parms(rs);
  const int nout = nrows;  // pairs written per system
  int ni = lay.ni;         // rows of this tableau
  if (ni <= 0 || ni > PIP_DUAL_MAXNI || nrows <= 0 || (!MARKED && nrows > ni)) return;
  float *key = (float *)dual_lds;          // [ni]; after the sort its room holds pos
  u16 *ineq = (u16 *)(dual_lds + 4 * (size_t)ni);  // [ni]
  u16 *pos = (u16 *)dual_lds;              // [ni]: logical row of each tableau row after the sort

  // 1. keys: a lane per column pair, four input rows in flight; an equality's key goes to both of its rows
  const i64 *src;
  const u64 *eqw = nullptr;
  if constexpr (MARKED) {
    __shared__ u64 words[PIP_DUAL_MAXNI / 64];
    src = rows + (size_t)blockIdx.x * eq.max_rows * srcrow;
    nrows = eq_from_markers<1>(eq, blockIdx.x, src, srcrow, lay.ni, words, ni);
    eqw = words;
  } else if constexpr (CSR) {
    src = nullptr;
    if (!csr_system_ok(rs, blockIdx.x, nrows, nvar)) nrows = 0;  // no key, k stays 0: not ok below
  } else if constexpr (INST) {
    src = (const i64 *)rs.matrix;  // (a system that was bad for the load is not PIPAMD_ST_SOLUTION: nothing to decide here)
  } else {
    src = rows + (size_t)blockIdx.x * nrows * srccol;
  }
  unsigned smaxw = 0;
  int k = 0;  // tableau row of the input row at hand
  for (int i0 = 0; i0 < nrows; i0 += 4) {
    int sz[4] = {0, 0, 0, 0};
    if constexpr (CSR) {  // a lane per stored entry
      const i64 *rp = (const i64 *)rs.row_ptr + (size_t)blockIdx.x * nrows + i0;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        if (i0 + q >= nrows) break;
        for (i64 e = rp[q] + lane; e < rp[q + 1]; e += 64) {
          const int a = rs.cols[e] < nvar ? dual_key_term(rs.vals[e]) : 0;
          sz[q] = sz[q] > a ? sz[q] : a;
        }
      }
    }
    for (int j = 2 * lane; !CSR && j < nvar; j += 128) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        if (i0 + q >= nrows) break;
        const i64 *r = src + (size_t)(i0 + q) * srcrow + MK;
        const int a0 = dual_key_term(r[j]);
        const int a1 = j + 1 < nvar ? dual_key_term(r[j + 1]) : 0;
        const int a = a0 > a1 ? a0 : a1;
        sz[q] = sz[q] > a ? sz[q] : a;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if (i0 + q >= nrows) break;
      const unsigned szw = wave_minmax_u32<true>((unsigned)sz[q]);
      const int twin = (int)((eq_word(eq, eqw, (i0 + q) >> 6) >> ((i0 + q) & 63)) & 1);
      if (lane <= twin && k + lane < ni) {
        key[k + lane] = (float)szw;
        ineq[k + lane] = (u16)(k + lane);
      }
      k += 1 + twin;
      smaxw = smaxw > szw ? smaxw : szw;
    }
  }
  __syncthreads();
  bool ok = k == ni;  // (the host has held the list against ni; the markers' count gave ni)
  if constexpr (MARKED) ok = ok && nrows > 0;

  // 2. the sort, then pos[ineq[r]] = nvar + r (all ni rows are real at load time)
  if (ok) dual_sort_pairs(key, ineq, ni, (double)smaxw, lane);
  for (int r = lane; ok && r < ni; r += 64) {
    const int i = ineq[r];
    if (i < ni) pos[i] = (u16)(nvar + r);
  }
  __syncthreads();

  // 3. the values, as emit_dual (pip_tree.cpp) reads them from a snapshot of the job's block
  const PipJob *J = &jobs[b];
  const i64 base = lay.arena_off + (i64)b * lay.blk.words;
  const int L = lay.blk.L, S = lay.S, W = lay.W, nligne = nvar + ni;
  ok = ok && J->status == PIPAMD_ST_SOLUTION && J->rows_off == base && J->vals_off == base + lay.blk.vals && J->L == L &&
       J->W == W && J->nvar == nvar && J->ni == ni && J->nparm == lay.nparm && nligne <= L;
  const PipRowTables<const T> tb = pip_row_tables<const T>(arena + base, L);
  const T *vals = (const T *)(arena + base + lay.blk.vals);
  int f0 = 0, r0 = 0;
  T d0 = 0;
  if (ok) {
    f0 = tb.flag[0];
    r0 = tb.ref[0];
    d0 = tb.den[0];
    if (!(f0 & PIPAMD_F_UNIT) && (r0 < 0 || r0 >= S)) ok = false;
  }
  // tableau row t: (valeur(tp, 0, its unit column), Denom(tp, 0)) if it has become a unit row, otherwise (0, 1)
  auto value = [&](int t, T &num, T &den) {
    num = 0;
    den = 0;
    const int p = pos[t];
    if (p < nvar || p >= nligne) return;
    if (tb.flag[p] & PIPAMD_F_UNIT) {
      const int u = tb.ref[p];
      if (u >= 0 && u < nvar) {
        num = (f0 & PIPAMD_F_UNIT) ? (r0 == u ? d0 : (T)0) : vals[(size_t)r0 * W + u];
        den = d0;
      }
    } else
      den = 1;
  };
  int before = 0;  // equalities among the input rows below r0w
  for (int r0w = 0; r0w < nout; r0w += 64) {
    const u64 word = (!MARKED || r0w < nrows) ? eq_word(eq, eqw, r0w >> 6) : 0;
    const int r = r0w + lane;
    if (r < nout) {
      T num = 0, den = 0;
      if (ok && (!MARKED || r < nrows)) {
        const int t = r + before + __popcll(word & ((1ull << lane) - 1));
        const bool twin = (word >> lane) & 1;
        if (t + (int)twin < ni) {
          value(t, num, den);
          if constexpr (SYSTEM) {
            if (twin && num == 0) {
              value(t + 1, num, den);
              num = wneg(num);
            }
            T g = gcd_i64(num, den);
            if (g == 0) g = 1;
            num = cquo(num, g);
            den = cquo(den, g);
          }
        }
      }
      dual_num[(size_t)b * nout + r] = num;
      dual_den[(size_t)b * nout + r] = den;
    }
    before += __popcll(word);
  }
}

// The launches from a PipBatchSource (pip_job.h).  visit_source is the one step from the source's kind to the kernels'
// (EQ, SRC): f(eq, rs) gets the members of the kind.  TABLEAU is the dual's alone and is left out of the load's visit at
// compile time (no PipNoEq load kernel is instantiated); the kinds are visited in the kernels' order in this file.
template <bool DUAL, class F>
static hipError_t visit_source(const PipBatchSource &s, F &&f) {
  switch (s.kind) {
    case PIP_SRC_INSTANCES: return f(s.mask, s.inst);
    case PIP_SRC_CSR: return f(s.mask, s.csr);
    case PIP_SRC_MATRICES: return f(s.markers, PipDenseRows{});
    case PIP_SRC_DENSE: return f(s.mask, PipDenseRows{});
    case PIP_SRC_TABLEAU:
      if constexpr (DUAL) return f(PipNoEq{}, PipDenseRows{});
  }
  return hipErrorInvalidValue;
}

// What the kernels rely on, per kind, and the entries of pip_host.cpp have checked (with a message) before they come here:
// the row count within the tableau's inequalities -- the layout's own for tableau rows, max_rows of room, within the
// engine's limit, for matrices --, the layout's parameters against the shift (tableau rows: none), and a matrix row of
// instances within the PIPAMD_MAXCOL values the load keeps of a point in LDS.
static bool source_ok(const PipBatchSource &s, const PipBatchLayout &lay, int *nrows) {
  const bool tableau = s.kind == PIP_SRC_TABLEAU, marked = s.kind == PIP_SRC_MATRICES;
  *nrows = tableau ? lay.ni : marked ? s.markers.max_rows : s.nrows;
  if (*nrows < 0 || *nrows > (marked ? PIPAMD_SMAX : lay.ni)) return false;
  if (tableau) return lay.nparm == 0;
  if (s.shift < -1 || s.shift > 1 || lay.nparm != (s.shift ? 1 : 0) || (s.shift && lay.bigparm != lay.nvar + 1)) return false;
  if (s.kind != PIP_SRC_INSTANCES) return true;
  return s.inst.matrix && s.inst.nparm >= 0 && (s.inst.nparm == 0 || s.inst.points) && lay.nvar + s.inst.nparm + 1 <= PIPAMD_MAXCOL;
}

extern "C" hipError_t pipk_launch_batch_dual_source(const PipJob *jobs, const i64 *arena, PipBatchLayout lay,
                                                    const PipBatchSource *s, int first, int count, void *dual_num,
                                                    void *dual_den, hipStream_t stream) {
  int nrows;
  if (count <= 0) return hipSuccess;
  if (!source_ok(*s, lay, &nrows) || lay.ni > PIP_DUAL_MAXNI) return hipErrorInvalidValue;
  if (lay.ni <= 0 || nrows <= 0) return hipSuccess;
  const size_t shm = pipk_batch_dual_lds_bytes(lay.ni);
  const auto launch = [&](auto t) {
    using T = decltype(t);
    return visit_source<true>(*s, [&](const auto &eq, const auto &rs) {
      hipLaunchKernelGGL((pip_batch_dual_kernel<T, std::decay_t<decltype(eq)>, std::decay_t<decltype(rs)>>), dim3(count),
                         dim3(64), shm, stream, jobs, arena, (const i64 *)s->rows, lay, first, nrows, eq, (T *)dual_num,
                         (T *)dual_den, rs);
      return hipGetLastError();
    });
  };
  return lay.ebits == 128 ? launch(i128{}) : launch(i64{});
}

// ---------------------------------------------------------------- expanser for the batch layer
// traiter.c:55-88 / integrer.c:410-415: a tableau whose spare rows are spent is copied into a larger one.  One
// workgroup per entry of the launch list: a job still PIPAMD_ST_RUN is passed on as it is; a job at
// PIPAMD_ST_CAPACITY gets block number atomicAdd(side_count) of the side arena (layout `nl`: same columns, more
// rows; nl.arena_off = the arena-relative offset of the side arena's first block), its row tables and rows are
// copied, the new spare rows zeroed, and it is passed on as PIPAMD_ST_RUN (summaries are rebuilt by the next
// launch, as after the host tree's grow()).  Its determinant log is empty at this point (replayed after every
// launch) and the limbs live in the PipJob.
__global__ __launch_bounds__(256) void pip_rehouse_kernel(PipJob *jobs, i64 *arena, PipQueue q, PipBatchLayout nl,
                                                          int *side_count, int side_cap) {
  const int nq = *q.in_count;
  if ((int)blockIdx.x >= nq) return;
  const int jb = q.in_list[blockIdx.x], tid = threadIdx.x;
  PipJob *J = &jobs[jb];
  const int st = J->status;
  if (st == PIPAMD_ST_RUN) {
    if (tid == 0) {
      q.out_list[atomicAdd(q.out_count, 1)] = jb;
      atomicMax(q.out_maxni, J->ni);
    }
    return;
  }
  if (st != PIPAMD_ST_CAPACITY || nl.S <= J->S || nl.W != J->W) return;  // cannot grow: the status stands
  __shared__ int s_idx;
  if (tid == 0) s_idx = atomicAdd(side_count, 1);
  __syncthreads();
  if (s_idx >= side_cap) return;
  const int EW = J->ebits == 128 ? 2 : 1;
  const int oL = J->L, oS = J->S, W = J->W, nligne = J->nvar + J->ni;
  const i64 base = nl.arena_off + (i64)s_idx * nl.blk.words;
  // (entries move as int64 words, whatever their width)
  const auto [oden, oflag, oref] = pip_row_words(arena + J->rows_off, oL, EW);
  const auto [nden, nflag, nref] = pip_row_words(arena + base, nl.blk.L, EW);
  for (int e = tid; e < nl.blk.L * EW; e += blockDim.x) nden[e] = e < nligne * EW ? oden[e] : 0;
  for (int k = tid; k < nl.blk.L; k += blockDim.x) {
    nflag[k] = k < nligne ? oflag[k] : 0;
    nref[k] = k < nligne ? oref[k] : 0;
  }
  const i64 *ovals = arena + J->vals_off;
  i64 *nvals = arena + base + nl.blk.vals;
  const i64 ow = (i64)oS * W * EW, nw = (i64)nl.S * W * EW;
  for (i64 e = tid; e < nw; e += blockDim.x) nvals[e] = e < ow ? ovals[e] : 0;
  __syncthreads();
  if (tid == 0) {
    if (J->home_sol_off == 0) J->home_sol_off = J->sol_off;
    pip_job_place(J, base, nl.blk);
    J->S = nl.S;
    J->tflags &= ~PIPAMD_T_STATE;
    J->status = PIPAMD_ST_RUN;
    q.out_list[atomicAdd(q.out_count, 1)] = jb;
    atomicMax(q.out_maxni, J->ni);
  }
}
// when the solve ends: the solution of a re-housed job goes back into its own block of the caller's workspace
// (the side arena belongs to the engine and serves the next solve)
__global__ void pip_rehouse_finish_kernel(PipJob *jobs, i64 *arena, int njobs, int sol_words) {
  const int b = blockIdx.x;
  if (b >= njobs) return;
  PipJob *J = &jobs[b];
  const i64 home = J->home_sol_off;
  if (home == 0) return;
  const i64 *src = arena + J->sol_off;
  i64 *dst = arena + home;
  for (int e = threadIdx.x; e < sol_words; e += blockDim.x) dst[e] = src[e];
  __syncthreads();
  if (threadIdx.x == 0) {
    J->sol_off = home;
    J->home_sol_off = 0;
  }
}
extern "C" hipError_t pipk_launch_rehouse(PipJob *jobs, i64 *arena, void *const *q5, int grid, PipBatchLayout nl,
                                          int *side_count, int side_cap, hipStream_t stream) {
  if (grid <= 0) return hipSuccess;
  const PipQueue q{(const int *)q5[0], (const int *)q5[1], (int *)q5[2], (int *)q5[3], (int *)q5[4]};
  hipLaunchKernelGGL(pip_rehouse_kernel, dim3(grid), dim3(256), 0, stream, jobs, arena, q, nl, side_count, side_cap);
  return hipGetLastError();
}
extern "C" hipError_t pipk_launch_rehouse_finish(PipJob *jobs, i64 *arena, int njobs, int sol_words, hipStream_t stream) {
  if (njobs <= 0) return hipSuccess;
  hipLaunchKernelGGL(pip_rehouse_finish_kernel, dim3(njobs), dim3(64), 0, stream, jobs, arena, njobs, sol_words);
  return hipGetLastError();
}

// ---------------------------------------------------------------- forest helpers
// Batched host<->device traffic of the lock-step decision-tree scheduler (pip_forest.cpp):
// one clone pass, one patch pass, one advance launch and one gather pass per step serve every
// problem of the batch.
// clone: list of (src word, dst word, n words) int64 triples -- expanser for a tree split
__global__ void pip_clone_kernel(i64 *arena, const i64 *list, int n) {
  const int b = blockIdx.x;
  if (b >= n) return;
  const i64 *src = arena + list[3 * b];
  i64 *dst = arena + list[3 * b + 1];
  const i64 nw = list[3 * b + 2];
  for (i64 i = threadIdx.x; i < nw; i += blockDim.x) dst[i] = src[i];
}
// patch: patch p = { dst (32-bit word index into the arena), n, payload[n] } at buf[index[p]]
__global__ void pip_patch_kernel(int *arena32, const int *buf, const i64 *index, int n) {
  const int b = blockIdx.x;
  if (b >= n) return;
  const int *p = buf + index[b];
  const i64 dst = ((i64)(unsigned)p[0]) | ((i64)p[1] << 32);
  const int nw = p[2];
  for (int i = threadIdx.x; i < nw; i += blockDim.x) arena32[dst + i] = p[3 + i];
}
// fresh: build new tableaux (tab_alloc + tab_get, tab.c:158-248) from their rows alone.
// Record r at buf[index[r]] (int64 words): rows_off, nvar, ni, ncol, L, S, W, vals_off, then ni*ncol values of the entry type T
// (the offsets are the job's, in int64 words; a 128-bit value is two words, low first).
template <class T>
__global__ void pip_fresh_kernel(i64 *arena, const i64 *buf, const i64 *index, int n) {
  const int b = blockIdx.x;
  if (b >= n) return;
  const i64 *p = buf + index[b];
  const i64 rows_off = p[0];
  const int nvar = (int)p[1], ni = (int)p[2], ncol = (int)p[3], L = (int)p[4], S = (int)p[5], W = (int)p[6];
  const T *src = (const T *)(p + 8);
  const auto [g_den, g_flag, g_ref] = pip_row_tables<T>(arena + rows_off, L);
  T *vals = (T *)(arena + p[7]);
  for (int i = threadIdx.x; i < nvar + ni; i += blockDim.x) {
    g_den[i] = 1;
    g_flag[i] = i < nvar ? PIPAMD_F_UNIT : PIPAMD_F_UNKNOWN;
    g_ref[i] = i < nvar ? i : i - nvar;
  }
  for (int e = threadIdx.x; e < ni * W; e += blockDim.x) {
    const int s = e / W, j = e % W;
    vals[e] = j < ncol ? src[(size_t)s * ncol + j] : (T)0;
  }
  const int pad = W - ncol;
  for (int e = threadIdx.x; e < (S - ni) * pad; e += blockDim.x) {
    const int s = ni + e / pad, j = ncol + e % pad;
    vals[(size_t)s * W + j] = 0;
  }
}

// gather: what the host needs from each job of the last launch, by status, into out + off[b] (off in int64 words; every
// item is a value of the entry type T):
//   NEED_COMPA  : n, then per undecided row (ascending): row, critic, constant, nparm parameter coefs
//   NEED_PARMCUT: row (aux), denominator, ncol entries
//   SOLUTION    : the solution block (nvar*(nparm+1) numerators, nvar denominators)
template <class T>
__global__ void pip_gather_kernel(const PipJob *jobs, const i64 *arena, int njobs, i64 *out, const i64 *off) {
  const int b = blockIdx.x;
  if (b >= njobs) return;
  const PipJob *J = &jobs[b];
  if (off[b + 1] == off[b]) return;  // the host does not want anything from this job
  T *o = (T *)(out + off[b]);
  const int nvar = J->nvar, nparm = J->nparm, L = J->L, W = J->W, ncol = nvar + nparm + 1;
  const auto [g_den, g_flag, g_ref] = pip_row_tables<const T>(arena + J->rows_off, L);
  const T *vals = (const T *)(arena + J->vals_off);
  const int lane = threadIdx.x;  // one wave
  if (J->status == PIPAMD_ST_NEED_COMPA) {
    const int nligne = nvar + J->ni;
    const int rec = 3 + nparm;
    int base = 0;
    for (int k0 = 0; k0 < nligne; k0 += 64) {
      const int k = k0 + lane;
      const bool und = k < nligne && (g_flag[k] & (PIPAMD_F_CRITIC | PIPAMD_F_UNKNOWN));
      const u64 m = __ballot(und);
      if (und) {
        const T *r = vals + (size_t)g_ref[k] * W;
        T *q = o + 1 + (size_t)(base + __popcll(m & ((1ull << lane) - 1))) * rec;
        int critic = 1;
        for (int j = 0; j < nvar; j++)
          if (r[j] > 0) {
            critic = 0;
            break;
          }
        q[0] = k;
        q[1] = critic;
        q[2] = r[nvar];
        for (int j = 0; j < nparm; j++) q[3 + j] = r[nvar + 1 + j];
      }
      base += __popcll(m);
    }
    if (lane == 0) o[0] = base;
  } else if (J->status == PIPAMD_ST_NEED_PARMCUT) {
    const int ci = J->aux;
    const T *r = vals + (size_t)g_ref[ci] * W;
    if (lane == 0) {
      o[0] = ci;
      o[1] = g_den[ci];
    }
    for (int j = lane; j < ncol; j += 64) o[2 + j] = r[j];
  } else if (J->status == PIPAMD_ST_SOLUTION) {
    const T *sn = (const T *)(arena + J->sol_off);
    const int n = nvar * (nparm + 1) + nvar;
    for (int e = lane; e < n; e += 64) o[e] = sn[e];
  }
}

extern "C" hipError_t pipk_launch_clone(i64 *arena, const i64 *list, int n, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(pip_clone_kernel, dim3(n), dim3(256), 0, stream, arena, list, n);
  return hipGetLastError();
}
extern "C" hipError_t pipk_launch_patch(i64 *arena, const int *buf, const i64 *index, int n, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(pip_patch_kernel, dim3(n), dim3(128), 0, stream, (int *)arena, buf, index, n);
  return hipGetLastError();
}
extern "C" hipError_t pipk_launch_fresh(i64 *arena, const i64 *buf, const i64 *index, int n, int ebits, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  if (ebits == 128)
    hipLaunchKernelGGL(pip_fresh_kernel<i128>, dim3(n), dim3(128), 0, stream, arena, buf, index, n);
  else
    hipLaunchKernelGGL(pip_fresh_kernel<i64>, dim3(n), dim3(128), 0, stream, arena, buf, index, n);
  return hipGetLastError();
}
extern "C" hipError_t pipk_launch_gather(const PipJob *jobs, const i64 *arena, int njobs, i64 *out, const i64 *off, int ebits,
                                         hipStream_t stream) {
  if (njobs <= 0) return hipSuccess;
  if (ebits == 128)
    hipLaunchKernelGGL(pip_gather_kernel<i128>, dim3(njobs), dim3(64), 0, stream, jobs, arena, njobs, out, off);
  else
    hipLaunchKernelGGL(pip_gather_kernel<i64>, dim3(njobs), dim3(64), 0, stream, jobs, arena, njobs, out, off);
  return hipGetLastError();
}

// ------------------------------------------------------------------ launchers
// columns a wave's registers cover (row chunks x 16 B per lane), by entry width
static int wp_of(int Wmax, int ebits) {
  if (ebits == 128) return Wmax <= 64 ? 64 : (Wmax <= 128 ? 128 : (Wmax <= 256 ? 256 : 512));
  return Wmax <= 128 ? 128 : (Wmax <= 256 ? 256 : 512);
}

extern "C" size_t pipk_advance_lds_bytes(int Lmax, int Smax, int Wmax, int ebits) {
  const size_t WP = (size_t)wp_of(Wmax, ebits);
  const size_t NM = WP / 64, EB = ebits == 128 ? 16 : 8;
  size_t shm = EB * 2 * (size_t)Smax + prow_bytes(EB * WP, Smax) + sizeof(u64) * (size_t)Smax * NM +
               sizeof(u16) * (3 * (size_t)Smax + (size_t)Lmax + WP) + 3 * (size_t)Smax;
  return (shm + 15) & ~(size_t)15;
}

extern "C" hipError_t pipk_launch_batch_counters(const PipJob *jobs, int njobs, unsigned long long *out,
                                                 hipStream_t stream) {
  hipError_t e = hipMemsetAsync(out, 0, 4 * sizeof(unsigned long long), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pip_batch_counters_kernel, dim3((njobs + 255) / 256), dim3(256), 0, stream, jobs, njobs, out);
  return hipGetLastError();
}

// the one-wave kernel of <= 128 int64 columns with a compile-time row capacity (see SC above)
template <int SC>
static hipError_t launch_static(AdvanceLaunch a, int ebits) {
  a.Smax = SC;
  a.Lmax = SC + 128;
  a.shm = pipk_advance_lds_bytes(a.Lmax, a.Smax, 128, ebits);
  return a.full ? launch_advance_t<i64, 1, 1, false, SC, true>(a) : launch_advance_t<i64, 1, 1, false, SC, false>(a);
}
// the row-capacity classes of the one-wave kernels, of the lean kernel, and of its four-wave flavour (pip_plan.h)
extern "C" int pipk_static_class(int smax) { return pip_static_class(smax); }
extern "C" int pipk_lean_class(int smax) { return pip_lean_class(smax); }
extern "C" int pipk_lean_waves_class(int smax) { return pip_lean_waves_class(smax); }
// the lean kernel of the 128-bit flavour: pip_lean.h's loop on long long rows, row capacity at run time
__global__ __launch_bounds__(64, PIP_LEAN64_WAVES) void pip_lean64_kernel(PipJob *jobs, i64 *arena, int njobs, int Smax, int Lmax,
                                                                          int iter_limit, PipQueue q PIP_LEAN_PROF_PARAM) {
  typedef LeanLongRows F;
  constexpr bool FULL = false, BIG = false;
  constexpr int NW = 1;  // (one wave per tableau)
#define PIP_LEAN_LOOP
#include "pip_lean.h"
#undef PIP_LEAN_LOOP
}
// the launch of pip_lean64_kernel: a.Smax / a.Lmax = the row capacity of the LDS image (the caller sizes it with
// lean64_lds_bytes); an image above 48 KB needs the dynamic-LDS limit raised, once per device
static hipError_t launch_lean64(const AdvanceLaunch &a) {
  const int grid = a.grid > 0 && a.grid < a.njobs ? a.grid : a.njobs;
  const size_t shm = lean64_lds_bytes(a.Smax, a.Lmax);
  const void *fn = (const void *)pip_lean64_kernel;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  if (shm > 48 * 1024) {
    static std::atomic<unsigned long long> raised{0};
    if (!((raised.load(std::memory_order_acquire) >> dev) & 1)) {
      e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, PIPAMD_LDS_BUDGET);
      if (e != hipSuccess) return e;
      raised.fetch_or(1ull << dev, std::memory_order_release);
    }
  }
#ifdef PIP_PROFILE
  hipLaunchKernelGGL(pip_lean64_kernel, dim3(grid), dim3(64), shm, a.stream, a.jobs, a.arena, a.njobs, a.Smax, a.Lmax, a.iter_limit,
                     a.q, (u64 *)a.prof);
#else
  hipLaunchKernelGGL(pip_lean64_kernel, dim3(grid), dim3(64), shm, a.stream, a.jobs, a.arena, a.njobs, a.Smax, a.Lmax, a.iter_limit,
                     a.q);
#endif
  return hipGetLastError();
}
extern "C" size_t pipk_lean64_lds_bytes(int Smax, int Lmax) { return lean64_lds_bytes((Smax + 3) & ~3, (Lmax + 3) & ~3); }
// the lean bulk kernel over a launch list; the caller has checked pipk_lean_class(a.Smax) != 0
// (big: every job has one parameter, the big one, in column nvar + 1 -- the BIG flavour, run-time column counts)
static hipError_t launch_lean_class(AdvanceLaunch a, bool big) {
  const int sc = pipk_lean_class(a.Smax);
  a.Smax = sc;
  a.Lmax = sc + 128;
  a.shm = pipk_advance_lds_bytes(a.Lmax, a.Smax, 128, 64);
  if (big) {
    switch (sc) {
      case 64: return launch_lean<64, false, true>(a);
      case 96: return launch_lean<96, false, true>(a);
      case 112: return launch_lean<112, false, true>(a);
      case 128: return launch_lean<128, false, true>(a);
      case 160: return launch_lean<160, false, true>(a);
    }
    return hipErrorInvalidValue;
  }
  if (a.waves == 4) {  // (the caller has checked pipk_lean_waves_class)
    switch (sc) {
      case 128: return a.full ? launch_lean<128, true, false, 4>(a) : launch_lean<128, false, false, 4>(a);
      case 160: return a.full ? launch_lean<160, true, false, 4>(a) : launch_lean<160, false, false, 4>(a);
    }
    return hipErrorInvalidValue;
  }
  switch (sc) {
    case 64: return a.full ? launch_lean<64, true>(a) : launch_lean<64, false>(a);
    case 96: return a.full ? launch_lean<96, true>(a) : launch_lean<96, false>(a);
    case 112: return a.full ? launch_lean<112, true>(a) : launch_lean<112, false>(a);
    case 128: return a.full ? launch_lean<128, true>(a) : launch_lean<128, false>(a);
    case 160: return a.full ? launch_lean<160, true>(a) : launch_lean<160, false>(a);
  }
  return hipErrorInvalidValue;
}
template <class T, int NCH>
static hipError_t launch_advance_w(bool one, const AdvanceLaunch &a) {
  if constexpr (sizeof(T) == 8) {
    if (a.gimg) return launch_advance_t<T, NCH, 4, true, 0, false>(a);  // tables in HBM: four waves per job
#if !defined(PIP_NO_STATIC_IMAGE)
    if constexpr (NCH == 1) {
      // row-capacity classes; a launch goes to the smallest class that holds it if that costs at most
      // an eighth more LDS than its exact size (occupancy is LDS-bound at 24 tableaux per CU)
      if (one && a.Lmax - a.Smax <= 128) {
        switch (pipk_static_class(a.Smax)) {
          case 64: return launch_static<64>(a, 64);
          case 96: return launch_static<96>(a, 64);
          case 112: return launch_static<112>(a, 64);
          case 128: return launch_static<128>(a, 64);
          case 160: return launch_static<160>(a, 64);
        }
      }
    }
#endif
  }
  if constexpr (sizeof(T) == 8 && NCH == 1) {
    // eight waves per job: the rows of a late pivot of a long tableau (15-25 of them change) are
    // spread over twice the waves -- for the few tableaux of a tail launch
    if (a.waves == 8) return launch_advance_t<T, NCH, 8, false, 0, false>(a);
  }
  if constexpr (sizeof(T) == 16 && NCH <= 4) {
    // sixteen waves per job, a whole CU: the hundreds of rows a late pivot of a long 128-bit tableau rewrites, spread over
    // four times the waves -- for a tail launch over a few such tableaux (fewer than the GPU has CUs)
    if (a.waves == 16) return launch_advance_t<T, NCH, 16, false, 0, false>(a);
  }
  return one ? launch_advance_t<T, NCH, 1, false, 0, false>(a) : launch_advance_t<T, NCH, 4, false, 0, false>(a);
}

// The determinant logs of at most `nrep` jobs replayed (the bound of the list in `q`; without a list: njobs), in either
// entry width.  A lane per job (jobs with an empty log cost a load): fewest instructions, what counts behind a bulk
// launch and when other batches keep the device busy.  A wave per job: shortest latency (a lane walks its up to 200 log
// entries alone for half a millisecond), where few jobs ran and someone is waiting for them.
static hipError_t launch_det_replay(PipJob *jobs, i64 *arena, int njobs, const PipQueue &q, int nrep, bool wave_per_job, int ebits,
                                    hipStream_t stream) {
  const dim3 grid(wave_per_job ? nrep : (nrep + 63) / 64);
  if (wave_per_job) {
    if (ebits == 128)
      hipLaunchKernelGGL(pip_det_replay_kernel<i128>, grid, dim3(64), 0, stream, jobs, arena, njobs, q);
    else
      hipLaunchKernelGGL(pip_det_replay_kernel<i64>, grid, dim3(64), 0, stream, jobs, arena, njobs, q);
  } else if (ebits == 128)
    hipLaunchKernelGGL(pip_det_replay_lanes_kernel<i128>, grid, dim3(64), 0, stream, jobs, arena, njobs, q);
  else
    hipLaunchKernelGGL(pip_det_replay_lanes_kernel<i64>, grid, dim3(64), 0, stream, jobs, arena, njobs, q);
  return hipGetLastError();
}

// waves_per_job: 1 = one wave64 per tableau (latency-bound sparse batches: more tableaux in
// flight per CU), 4 = four waves share a tableau's rows (few, large tableaux).
// ebits: 64 or 128 -- every job of the launch must have that entry width.
static hipError_t launch_by_shape(const AdvanceLaunch &a, bool one, int wp, int ebits);

// q5: NULL = job b is workgroup b's; else five device pointers {in_list, in_count, out_list,
// out_count, out_maxni} (see PipQueue; the in_ pair and the out_ triple may each be NULL) and
// `grid` = an upper bound on *in_count (0: njobs).
// big: NULL, or {void **buffer, size_t *bytes} of the caller -- a device buffer this function
// (re)allocates when the row tables of the launch do not fit LDS (64-bit entries only): the launch
// then keeps them there, `grid` blocks of the image size.  Without it such a launch is refused.
// hints: PIPK_HINT_* bits (pip_host.h).
extern "C" hipError_t pipk_launch_advance_q(PipJob *jobs, i64 *arena, int njobs, int Lmax, int Smax, int Wmax,
                                            int iter_limit, int waves_per_job, int ebits, void *const *q5, int grid,
                                            void **big, int hints, unsigned long long *prof, hipStream_t stream) {
  if (njobs <= 0) return hipSuccess;
  // LDS arrays are carved at 16/8/4/2/1-byte granularity in that order: keep Lmax, Smax multiples of 4
  Lmax = (Lmax + 3) & ~3;
  Smax = (Smax + 3) & ~3;
  if (Wmax > 512) return hipErrorInvalidValue;
  AdvanceLaunch a;
  a.jobs = jobs;
  a.arena = arena;
  a.njobs = njobs;
  a.Lmax = Lmax;
  a.Smax = Smax;
  a.Wmax = Wmax;
  a.iter_limit = iter_limit;
  a.q = PipQueue{nullptr, nullptr, nullptr, nullptr, nullptr};
  a.grid = njobs;
  if (q5) {
    a.q = PipQueue{(const int *)q5[0], (const int *)q5[1], (int *)q5[2], (int *)q5[3], (int *)q5[4]};
    a.grid = grid;
    a.q.replay_spare = (hints & PIPK_HINT_LEAN) && (hints & PIPK_HINT_SPARE_REPLAY) ? 1 : 0;
  }
  a.prof = prof;
  a.waves = waves_per_job;
  a.full = (hints & PIPK_HINT_FULL) != 0;
  a.shm = pipk_advance_lds_bytes(Lmax, Smax, Wmax, ebits);
  a.gimg = nullptr;
  a.gslots = 0;
  if (a.shm > PIPAMD_LDS_BUDGET) {  // the row tables of this job mix do not fit a CU's LDS
    if (ebits != 64 || !big) return hipErrorInvalidConfiguration;
    void **buf = (void **)big[0];
    size_t *cap = (size_t *)big[1];
    // A pool of image blocks, not one per workgroup: a launch over a 10k-tableau list of which a handful are
    // unfinished would otherwise pin (and possibly fail to get) gigabytes.  Workgroup b uses block b % slots
    // behind a lock word; 1,024 blocks cover the workgroups a GPU keeps resident (256 CUs x at most 4 of these
    // 256-thread, ~100-register workgroups), so a workgroup seldom waits.
    const int wgs = a.grid > 0 && a.grid < njobs ? a.grid : njobs;
    a.gslots = wgs < 1024 ? wgs : 1024;
    const size_t locks = ((size_t)a.gslots * sizeof(int) + 255) & ~(size_t)255;
    const size_t need = locks + (size_t)a.gslots * a.shm;
    if (*cap < need) {
      if (*buf) {
        hipError_t fe = hipFree(*buf);  // waits for the launches that may still use it
        if (fe != hipSuccess) return fe;
      }
      *buf = nullptr;
      *cap = 0;
      hipError_t me = hipMalloc(buf, need);
      if (me != hipSuccess) return me;
      *cap = need;
      me = hipMemsetAsync(*buf, 0, need, stream);  // every lock free; re-zeroed below for a smaller pool
      if (me != hipSuccess) return me;
    }
    a.gimg = (unsigned char *)*buf;
    // the lock words sit at the head of the buffer whatever the pool size: all are free between launches
    // (every workgroup releases its block before it ends), so nothing needs zeroing per launch
  }
  a.stream = stream;
  // (the lean kernel with four waves per tableau is a bulk launch like the one-wave kernels: same replay behind it)
  const bool lean4 = (hints & PIPK_HINT_LEAN) && !(hints & PIPK_HINT_BIG) && waves_per_job == 4 && pipk_lean_waves_class(a.Smax);
  const bool one = waves_per_job == 1 || lean4;
  const int wp = wp_of(Wmax, ebits);
  hipError_t le;
  if (hints & PIPK_HINT_LEAN) {
    if (!one || ebits != 64 || wp != 128 || a.gimg || !pipk_lean_class(a.Smax)) return hipErrorInvalidValue;
    le = launch_lean_class(a, (hints & PIPK_HINT_BIG) != 0);
  } else if (hints & PIPK_HINT_LEAN64) {
    if (!one || ebits != 128 || wp != 256 || pipk_lean64_lds_bytes(a.Smax, a.Lmax) > PIPAMD_LDS_BUDGET) return hipErrorInvalidValue;
    le = launch_lean64(a);
  } else {
    le = launch_by_shape(a, one, wp, ebits);
  }
  if (le != hipSuccess) return le;
  // the determinant bookkeeping of the pivots just logged (PIPK_HINT_NO_REPLAY: the caller replays later --
  // pipk_launch_replay_all): a lane per job behind a bulk launch, a wave per job behind the few jobs of a tail launch
  if (hints & PIPK_HINT_NO_REPLAY) return hipGetLastError();
  return launch_det_replay(jobs, arena, njobs, a.q, a.grid > 0 && a.grid < njobs ? a.grid : njobs, !one, ebits, stream);
}

// The determinant logs of ALL jobs 0..njobs-1 replayed: behind a sequence of launches that ran with
// PIPK_HINT_NO_REPLAY, a lane (wave_per_job = 0) or a wave per job (launch_det_replay: the second for a caller that runs
// one batch at a time).  The log holds PIPAMD_DETLOG pivots and the pivot
// kernels pause a job whose log is full, so a sequence may log at most that many pivots per job between replays.
extern "C" hipError_t pipk_launch_replay_all(PipJob *jobs, i64 *arena, int njobs, int ebits, int wave_per_job, hipStream_t stream) {
  if (njobs <= 0) return hipSuccess;
  return launch_det_replay(jobs, arena, njobs, PipQueue{nullptr, nullptr, nullptr, nullptr, nullptr}, njobs, wave_per_job != 0, ebits,
                           stream);
}

// One of the two replay kernels over a caller's jobs, a block (wave_per_job) or a lane per job of `njobs`, with or
// without an input list and its device-side count: for the replay probe (pip_probe.hip, pipamd_debug_det_replay), which
// cannot name the kernels of this file.  Nothing else calls it.
extern "C" hipError_t pipk_launch_det_replay(PipJob *jobs, i64 *arena, int njobs, int ebits, int wave_per_job, const int *in_list,
                                             const int *in_count, hipStream_t stream) {
  if (njobs <= 0) return hipSuccess;
  return launch_det_replay(jobs, arena, njobs, PipQueue{in_list, in_count, nullptr, nullptr, nullptr}, njobs, wave_per_job != 0, ebits,
                           stream);
}

static hipError_t launch_by_shape(const AdvanceLaunch &a, bool one, int wp, int ebits) {
#ifdef PIP_ONLY_MAIN  // diagnostic builds (tools/isa_lines.sh): only the 64-bit, <= 128-column, one-wave kernel
  return (ebits == 64 && wp == 128 && one && !a.gimg) ? launch_advance_w<i64, 1>(true, a) : hipErrorInvalidValue;
#else
  if (ebits == 128) {
    switch (wp) {
      case 64: return launch_advance_w<i128, 1>(one, a);
      case 128: return launch_advance_w<i128, 2>(one, a);
      case 256: return launch_advance_w<i128, 4>(one, a);
      default: return launch_advance_w<i128, 8>(one, a);
    }
  }
  switch (wp) {
    case 128: return launch_advance_w<i64, 1>(one, a);
    case 256: return launch_advance_w<i64, 2>(one, a);
    default: return launch_advance_w<i64, 4>(one, a);
  }
#endif
}

extern "C" hipError_t pipk_launch_advance(PipJob *jobs, i64 *arena, int njobs, int Lmax, int Smax, int Wmax,
                                          int iter_limit, int waves_per_job, int ebits, unsigned long long *prof,
                                          hipStream_t stream) {
  return pipk_launch_advance_q(jobs, arena, njobs, Lmax, Smax, Wmax, iter_limit, waves_per_job, ebits, nullptr, 0, nullptr,
                               0, prof, stream);
}

extern "C" hipError_t pipk_launch_batch_load(PipJob *jobs, i64 *arena, const i64 *rows, PipBatchLayout lay, int first,
                                             int count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (lay.ebits == 128)
    hipLaunchKernelGGL(pip_batch_load_kernel<i128>, dim3(count), dim3(256), 0, stream, jobs, arena, rows, lay, first);
  else
    hipLaunchKernelGGL(pip_batch_load_kernel<i64>, dim3(count), dim3(256), 0, stream, jobs, arena, rows, lay, first);
  return hipGetLastError();
}

// the load from the caller's system: equalities expanded, shift 0 / +1 / -1, tab_simplify
extern "C" hipError_t pipk_launch_batch_load_source(PipJob *jobs, i64 *arena, PipBatchLayout lay, const PipBatchSource *s,
                                                    int first, int count, hipStream_t stream) {
  int nrows;
  if (count <= 0) return hipSuccess;
  if (!source_ok(*s, lay, &nrows) || lay.W < lay.nvar + lay.nparm + 1 || lay.W > 512) return hipErrorInvalidValue;
  lay.pad = 0;
  const auto launch = [&](auto t, auto cpl) {
    return visit_source<false>(*s, [&](const auto &eq, const auto &rs) {
      hipLaunchKernelGGL((pip_batch_load_system_kernel<decltype(t), decltype(cpl)::value, std::decay_t<decltype(eq)>,
                                                       std::decay_t<decltype(rs)>>),
                         dim3(count), dim3(256), 0, stream, jobs, arena, (const i64 *)s->rows, lay, first, s->shift, s->simplify,
                         nrows, eq, rs);
      return hipGetLastError();
    });
  };
  const std::integral_constant<int, 2> narrow;  // columns per lane: the tableau's columns over the 64 lanes
  const std::integral_constant<int, 8> wide;
  if (lay.ebits == 128) return lay.W <= 128 ? launch(i128{}, narrow) : launch(i128{}, wide);
  return lay.W <= 128 ? launch(i64{}, narrow) : launch(i64{}, wide);
}

extern "C" hipError_t pipk_launch_batch_results_shifted(const PipJob *jobs, const i64 *arena, int njobs, int nvar, int ebits,
                                                        int shift, int *status, int *pivots, int *cuts, void *x_num, void *x_den,
                                                        hipStream_t stream) {
  if (njobs <= 0) return hipSuccess;
  if (ebits == 128)
    hipLaunchKernelGGL(pip_batch_results_shifted_kernel<i128>, dim3(njobs), dim3(128), 0, stream, jobs, arena, njobs, nvar, shift,
                       status, pivots, cuts, (i128 *)x_num, (i128 *)x_den);
  else
    hipLaunchKernelGGL(pip_batch_results_shifted_kernel<i64>, dim3(njobs), dim3(128), 0, stream, jobs, arena, njobs, nvar, shift,
                       status, pivots, cuts, (i64 *)x_num, (i64 *)x_den);
  return hipGetLastError();
}

extern "C" hipError_t pipk_launch_batch_results(const PipJob *jobs, const i64 *arena, int njobs, int nvar, int nparm,
                                                int ebits, int *status, int *pivots, int *cuts, void *sol_num,
                                                void *sol_den, hipStream_t stream) {
  if (ebits == 128)
    hipLaunchKernelGGL(pip_batch_results_kernel<i128>, dim3(njobs), dim3(256), 0, stream, jobs, arena, njobs, nvar, nparm,
                       status, pivots, cuts, (i128 *)sol_num, (i128 *)sol_den);
  else
    hipLaunchKernelGGL(pip_batch_results_kernel<i64>, dim3(njobs), dim3(256), 0, stream, jobs, arena, njobs, nvar, nparm,
                       status, pivots, cuts, (i64 *)sol_num, (i64 *)sol_den);
  return hipGetLastError();
}
