// piplib_amd/csrc/pip_job.h -- structures shared by the HIP kernels and the host side.
#ifndef PIP_JOB_H
#define PIP_JOB_H
#include <stdint.h>

#include "../../include/piplib_amd.h"

#define PIPAMD_MAXDET 4   /* reference tab.h:67 MAX_DETERMINANT */
#define PIPAMD_MAXCOL 512 /* reference type.h:44 */
#define PIPAMD_MAXPARM 50 /* reference type.h:45 */
/* Row tables are indexed with 16-bit codes (slot < 0x4000, logical row < 0xffff).  A job whose row
 * tables fit a workgroup's LDS (about 3,400 rows of <= 128 int64 columns) is staged there; a larger
 * 64-bit job runs with the same tables in HBM (the kernel's GM instantiation), so that a tableau
 * can grow as with the reference's expanser (traiter.c:55-88) up to these limits. */
#define PIPAMD_SMAX 16000 /* real rows (slots) per job */
#define PIPAMD_LMAX (PIPAMD_SMAX + PIPAMD_MAXCOL) /* logical rows */
#define PIPAMD_LDS_BUDGET (160 * 1024 - 1024) /* dynamic LDS a workgroup can get */
/* The pivot kernel does not run the determinant bookkeeping of traiter.c:412-446 itself
 * (wave-uniform scalar work, ~12 % of its instructions with 64-bit entries); it logs (pivot,
 * denominator of the pivot row) per pivot -- at most this many per launch -- and pip_det_replay_kernel replays
 * the log right after the launch, one wave per job: the gcds of 64 pivots at a time on the lanes,
 * only the walk over the limbs sequentially. */
#define PIPAMD_DETLOG 512
/* PipJob.aux of a job that ended PIPAMD_ST_NIL in a call of pivoter that found no pivot column (traiter.c:782-785): that
 * call is counted in npiv and has no log entry, which the replay's pivot count of an overflow has to know (a cut's row
 * index, the other use of aux, is never negative) */
#define PIPAMD_AUX_NOCOLUMN (-1)

/* One problem ("job") in the device arena: a PipJob header and a block of int64 words.  Every offset is in int64
 * units and even (rows are 16-byte aligned); an entry is `ew` words (1: 64-bit entries, 2: 128-bit entries).  A block
 * of L logical rows, S real rows (slots) and W columns, in this order (pip_block_layout below is the one place that
 * computes it):
 *   rows  : den[L] (entries) | flag[L] (int32) | ref[L] (int32)         -- pip_row_tables
 *   vals  : S slots of W entries (zero beyond the live columns)
 *   sol   : nvar*(nparm+1) numerators | nvar denominators (entries; room for the columns a job may grow)
 *   state : summaries of a paused job: nzm[S][NM] (u64) | sig[S] (u16) | rcls[S] (u8), NM bitmap words per slot
 *   log   : 2 * PIPAMD_DETLOG entries, the determinant log of the last launch
 * Mirrors the reference's struct T / struct L (tab.h:36-85) without pointers. */
/* internal tflags bit: the job's rows still sit in the caller's array (src_rows); the first pivot launch
 * reads them from there while it builds its summaries and writes them into the block (PIPAMD_T_ROWS_STAY) */
#define PIPAMD_T_FRESHROWS 4096

typedef struct PipJob {
  int64_t vals_off, rows_off, sol_off, state_off;
  int64_t log_off; /* 2 * PIPAMD_DETLOG entries: the determinant log of the last launch */
  int32_t nvar, nparm, ni, bigparm;
  int32_t tflags;
  int32_t L, S, W;
  int32_t status, aux, npiv, ncut;
  int32_t ldet, nupd; /* nupd: rows rewritten by pivots so far (excludes skipped zero-multiplier rows) */
  int64_t det[2 * PIPAMD_MAXDET]; /* multi-limb determinant, tab.h:76-81: det[i] (64-bit entries) or
                                     det[2i] | det[2i+1] << 64 (128-bit entries) */
  uint64_t maxabs;
  int32_t nlog, pad_; /* entries of the determinant log not replayed yet */
  int32_t state_nch, ebits; /* ebits: 64 or 128 (0 = 64) */ /* row-chunk count (NCH) of the launch that saved the state block */
  int64_t src_rows; /* PIPAMD_T_FRESHROWS: device address of the caller's ni x ncol input rows (not yet in the block) */
  int64_t home_sol_off; /* != 0: the job was re-housed in a larger block outside its batch's workspace (expanser,
                           pip_rehouse_kernel); its solution is copied back to this offset when the solve ends */
} PipJob;

/* pipamd_batch_solve's launch lists: a job that ran out of spare rows (PIPAMD_ST_CAPACITY) stays on the list, and
 * the list's `maxni` word carries this bit, until the host has re-housed it in a larger block; the word behind `maxni`
 * counts these jobs (the host sizes the larger blocks' arena by it) */
#define PIPAMD_Q_CAPFLAG (1 << 30)

/* Which rows of a caller's plain system are equalities (pipamd_system.eq_rows): bit r % 64 of w[r / 64], zero beyond
 * the system's rows.  The host builds it from the caller's list and hands it to the kernels by value, as 2,000 bytes of
 * kernel arguments: nothing of the caller's list has to outlive the call. */
typedef struct PipEqMask {
  uint64_t w[(PIPAMD_SMAX + 63) / 64];
} PipEqMask;

/* The same question answered on the device (pipamd_matrices): every system has max_rows rows of room, each row led by
 * its PolyLib marker (0: an equality), and a row count of its own in `nrows` (a DEVICE array, one per system of the
 * launch; NULL: max_rows each).  The kernels build a system's mask words in LDS from its marker column. */
typedef struct PipEqMarkers {
  const int32_t *nrows;
  int32_t max_rows;
} PipEqMarkers;

/* Where a system's input rows come from when they are not dense (pipamd_sparse): CSR over the systems of the launch, all
 * three arrays on the DEVICE.  Row r of system s (nrows rows each) owns the entries row_ptr[s * nrows + r] ..
 * row_ptr[s * nrows + r + 1] - 1 of cols / vals; a column is 0 .. nvar - 1 for an unknown and nvar for the constant.
 * The kernels check a system's pointers against [0, nnz] before they read an entry through them. */
typedef struct PipCsrRows {
  const int64_t *row_ptr;
  const int32_t *cols;
  const int64_t *vals;
  int64_t nnz;
} PipCsrRows;

/* The same for the instances of ONE parametric system (pipamd_instances): `matrix` is nrows x (nvar + nparm + 1), unknowns |
 * parameters | constant, shared by every system of the launch; `points` holds the launch's systems' parameter values,
 * nparm each (not looked at when nparm == 0).  Both on the DEVICE.  The kernels substitute a system's point into the
 * parameter columns: its row r is a_r0 .. a_r(nvar-1) | c_r + sum_k p_rk * theta_k, the sum exact. */
typedef struct PipInstanceRows {
  const int64_t *matrix;
  const int64_t *points;
  int32_t nparm;
} PipInstanceRows;

/* What a batch is loaded from, and what its dual is read against: ONE source, of one kind.  The host's check of an entry
 * fills it in place (the mask is built where the launch reads it), pipk_launch_batch_load_source / _dual_source turn the
 * kind into the kernels' (EQ, SRC) and hand those members over by value.  Only the members of the kind mean anything:
 *   kind      | equalities (EQ) | rows (SRC)            | nrows
 *   TABLEAU   | none            | `rows`, as loaded     | the layout's ni      (dual only: pipamd_batch_dual)
 *   DENSE     | `mask`          | `rows`                | the system's         (pipamd_system; the shifted load: empty mask)
 *   MATRICES  | `markers`       | `rows`, marker first  | markers.max_rows     (pipamd_matrices)
 *   CSR       | `mask`          | `csr`                 | the system's         (pipamd_sparse)
 *   INSTANCES | `mask`          | `inst`                | the system's         (pipamd_instances) */
enum PipSourceKind { PIP_SRC_TABLEAU, PIP_SRC_DENSE, PIP_SRC_MATRICES, PIP_SRC_CSR, PIP_SRC_INSTANCES };
typedef struct PipBatchSource {
  int32_t kind;
  int32_t shift, simplify, nrows; /* (the dual looks at nrows alone) */
  const int64_t *rows;
  PipEqMask mask;
  PipEqMarkers markers;
  PipCsrRows csr;
  PipInstanceRows inst;
} PipBatchSource;

#ifdef __HIPCC__
#define PIP_HD __host__ __device__
#else
#define PIP_HD
#endif

/* Where the parts of a block start (int64 words from the block's first word) and how long it is. */
typedef struct PipBlockLayout {
  int32_t L, pad; /* logical rows: nvar + S, rounded up to even */
  int64_t vals, sol, state, log, words;
} PipBlockLayout;

/* sol_entries: entries of the solution part; nm: bitmap words per slot the saved summaries have room for */
PIP_HD constexpr PipBlockLayout pip_block_layout(int nvar, int S, int W, int ew, int64_t sol_entries, int nm) {
  PipBlockLayout b{};
  b.L = (nvar + S + 1) & ~1;
  b.vals = (int64_t)b.L * ew + b.L;
  b.sol = b.vals + (int64_t)S * W * ew;
  b.state = b.sol + ((sol_entries * ew + 1) & ~(int64_t)1);
  b.log = b.state + (((int64_t)S * nm + (3 * b.L + 7) / 8 + 1) & ~(int64_t)1);
  b.words = b.log + 2 * PIPAMD_DETLOG * ew;
  return b;
}
/* a job's header takes a block of layout `b` at arena word `base` */
PIP_HD inline void pip_job_place(PipJob *J, int64_t base, const PipBlockLayout &b) {
  J->rows_off = base;
  J->vals_off = base + b.vals;
  J->sol_off = base + b.sol;
  J->state_off = base + b.state;
  J->log_off = base + b.log;
  J->L = b.L;
}
/* the row tables at the head of a block of L logical rows with entries of type T (pointer arithmetic only: the
 * pointers are as const, and as dereferenceable, as `rows` is); the flag table in 32-bit words from the block's start */
PIP_HD constexpr int64_t pip_flag_off32(int L, int ew) { return (int64_t)2 * L * ew; }
template <class T>
struct PipRowTables {
  T *den;
  int *flag, *ref;
};
/* (den as int64 words, ew per entry: for code that learns the entry width at run time) */
PIP_HD inline PipRowTables<int64_t> pip_row_words(const void *rows, int L, int ew) {
  int *flag = (int *)rows + pip_flag_off32(L, ew);
  return {(int64_t *)rows, flag, flag + L};
}
template <class T>
PIP_HD inline PipRowTables<T> pip_row_tables(const void *rows, int L) {
  const PipRowTables<int64_t> w = pip_row_words(rows, L, sizeof(T) / 8);
  return {(T *)w.den, w.flag, w.ref};
}

typedef struct PipBatchLayout {
  int64_t arena_off;  /* first job's block, int64 units */
  PipBlockLayout blk; /* every job's block (blk.words apart) */
  int32_t batch, nvar, nparm, ni, bigparm, tflags;
  int32_t S, W;
  int32_t ebits, pad;
} PipBatchLayout;

#endif
