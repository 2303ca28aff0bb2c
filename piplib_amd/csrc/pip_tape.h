// piplib_amd/csrc/pip_tape.h -- a solution tape evaluated at many parameter points (pip_tape.hip): the compiled program
// and the launch interface.
//
// pipamd_tape_compile (pip_host.cpp) turns a checked tape into a flat program of 8-byte words, nodes in tape order.  A
// value takes EW words, 1 for int64 cells and 2 (low, high) for 128-bit cells.  A node is a header word
//     bits 0-7 the TAPE_* operation | bits 8-23 P, the parameters in scope | bits 32-62 aux
// followed by its values:
//     TAPE_NEW   aux 0              D, c_0 .. c_P            slot P = floor((sum c_j slot_j + c_P) / D); the next node follows
//     TAPE_IF    aux the else node  n_0 .. n_P               sum n_j slot_j + n_P >= 0: the next node, otherwise word aux
//     TAPE_LEAF  aux its ordinal    nvar x (D_i, n_0 .. n_P), then ndual x (numerator, denominator) in lowest terms
//     TAPE_NIL   aux its ordinal
// The host writes aux of an IF only behind the node's own words and within the program, and every other node either
// ends the walk or is followed by the next one: a point's position only grows, so the kernel ends after at most as many
// steps as the program has nodes and reads nothing outside it, whatever the points are.
//
// pip_solve's result edits (pipamd_tape_compile_pip, sol.c:435-512) are applied by the compiler where they can be: P
// counts the KEPT parameters in scope, the values of dropped columns are not emitted, and a shifted coefficient is
// emitted shifted.  Two marks remain for the kernel, both absent from a program compiled without an edit:
//     TAPE_LEAF_NEGATE, bit 24 of a LEAF's header (bits 24-31 are 0 in every other header): SOL_NEGATE, every unknown's
//                       exact value N is negated before the range check and the reduction
//     D_i < 0 in a LEAF: the unknown is unbounded (its shifted coefficient of the big parameter is not 0); the
//                       denominator is -D_i for the reduction and 0 in what is handed out.  D_i is never 0.
// The compile says whether a program holds either mark (TapeLaunch.marks); one that holds none is walked by an
// instantiation of the kernel that does not look for them, so a tape compiled without an edit costs what it did.
//
// A set of tapes (pipamd_tape_set_create) is their programs one behind the other in one buffer, every else target moved
// by its tape's start word, and a table of TapeSetEntry: a lane starts at its tape's first word, positions still only
// grow, and no jump leaves its tape's words.
#ifndef PIP_TAPE_H
#define PIP_TAPE_H
#include <hip/hip_runtime.h>
#include <stddef.h>

enum { TAPE_NIL = 1, TAPE_IF = 2, TAPE_LEAF = 3, TAPE_NEW = 5 };
enum {
  TAPE_BLOCK = 128,       // points per workgroup, a lane each
  TAPE_MAX_SLOTS = 32,    // PIPAMD_TAPE_MAX_SLOTS: the largest P + 1 served
  TAPE_LDS_BYTES = 65536  // PIPAMD_TAPE_LDS_BYTES: parameters in scope, and the program when it fits beside them
};
// bytes of LDS the parameters in scope take: a row of TAPE_BLOCK values per parameter, slots - 1 of them
static inline size_t tape_slot_bytes(int slots, int bits) { return (size_t)(slots - 1) * TAPE_BLOCK * (bits / 8); }
static inline long long tape_header(int op, int P, long long aux) { return (long long)op | ((long long)P << 8) | (aux << 32); }
static const long long TAPE_LEAF_NEGATE = 1ll << 24;

struct TapeLaunch {
  const long long *prog;  // device; `words` words
  long long words;        // 0: the empty tape
  int bits;               // 64 or 128
  int staged;             // 1: the program is copied to LDS first; 0: read from global memory
  int marks;              // 1: the program holds a TAPE_LEAF_NEGATE bit or a negative D_i; 0: it holds neither
  int nvar, nparm, ndual;  // nparm: the values of a point (pipamd_tape_point_cols)
  int slots;              // pipamd_tape_info.slots
  long long n_points;
  const long long *points;
  int *status, *leaf;
  void *x_num, *x_den, *dual_num, *dual_den;
};

struct TapeSetEntry {
  int start, words;  // first word in the set's buffer; 0 words: the empty tape
  int point_cols, nvar, ndual;
  int pad[3];
};  // 32 bytes

struct TapeSetLaunch {
  const long long *prog;      // device; all programs, else targets relocated
  const TapeSetEntry *table;  // device; n entries
  int n, bits;
  int point_cols, nvar, ndual, slots;  // the maxima: the strides of points, x_* and dual_*, and the LDS rows
  long long n_points;
  const int *tape;  // device; a tape index per point
  const long long *points;
  int *status, *leaf;
  void *x_num, *x_den, *dual_num, *dual_den;
};

// pipamd_tape_sweep: the points are those of a box, made by the kernel.  Point k, 0 <= k < n_points, is the box in
// row-major order, the last column fastest: column c is lo[c] + digit_c(k), the digits of k in the mixed radix ext[].
// A bounded grid of persistent workgroups takes the chunks of TAPE_BLOCK consecutive k in turn: as many as the device
// holds at once (the occupancy of the instantiation with the launch's LDS, at most TAPE_SWEEP_WG_PER_CU a compute
// unit, TAPE_SWEEP_WG_PER_CU_SUM with a summary).  The summary (piplib_amd.h, PIPAMD_SWEEP_*): the status figures are gathered per wave in registers; with `binned` they and a count and a minimum
// per leaf are gathered per workgroup in LDS behind the slots and the staged program and flushed once; without `binned`
// a wave's aggregates go to global atomics directly.
enum {
  TAPE_SWEEP_WG_PER_CU = 16,    // the grid's bound: workgroups per compute unit (8 waves per SIMD)
  TAPE_SWEEP_WG_PER_CU_SUM = 8  // the same when a summary is asked for
};
static inline size_t tape_sweep_bin_bytes(long long leaves) { return 16 * ((size_t)leaves + 4); }
struct TapeSweepLaunch {
  TapeLaunch t;           // the program and the outputs; t.points is not read; t.n_points = prod ext[c]
  int n_ctx;              // rows of the context
  int binned;             // pipamd_tape_sweep_plan.binned
  int cus;                // compute units of the device
  int max_blocks;         // testing aid: at most this many workgroups (0: the bound above)
  const long long *ctx;   // device; n_ctx x (t.nparm + 2): marker, coefficients, constant
  long long *summary;     // device; 8 + 2 * leaves words, initialised by the launch; or NULL
  long long leaves;
  long long lo[TAPE_MAX_SLOTS - 1];
  unsigned long long ext[TAPE_MAX_SLOTS - 1];  // hi[c] - lo[c] + 1, each below 2^38
};

// pipamd_tape_compare / pipamd_tape_compare_sweep: two programs, possibly of different cell widths, walked per lane at
// the same point, their leaves compared without writing them out (piplib_amd.h, PIPAMD_CMP_*).  LDS: the slot rows of
// `a`, those of `b`, then -- staged -- the words of `a` and of `b`.  box: the points are those of lo / ext as in
// TapeSweepLaunch, tested against ctx, taken by the sweep's bounded persistent grid; otherwise they are read from
// `points`, a workgroup per chunk of TAPE_BLOCK.
struct TapeCompareLaunch {
  const long long *prog_a, *prog_b;  // device
  long long words_a, words_b;        // 0: the empty tape
  int bits_a, bits_b;                // 64 or 128
  int slots_a, slots_b;              // pipamd_tape_info.slots of either
  int staged;                        // 1: both programs are copied to LDS first; 0: both are read from global memory
  int box;
  int nvar, nparm;                   // the same for both; nparm: the values of a point
  int ndual;                         // dual pairs compared behind the unknowns (0: none, or PIPAMD_CMP_DUAL not set)
  int n_ctx, cus, max_blocks;        // as in TapeSweepLaunch
  long long n_points;
  const long long *points;           // device; the list form
  const long long *ctx;              // device; n_ctx x (nparm + 2)
  long long *summary;                // device; PIPAMD_CMP_WORDS words, initialised by the launch; or NULL
  int *cls, *where, *status_a, *status_b;  // device; each may be NULL
  long long lo[TAPE_MAX_SLOTS - 1];
  unsigned long long ext[TAPE_MAX_SLOTS - 1];
};

// pipamd_tape_sweep_values: the sweep's box, context, grid and head words; per unknown a record of counts, minimum,
// maximum (each with the smallest k that attains it) and exact sum (piplib_amd.h, PIPAMD_VALUES_*).  Two stages: every
// wave of the main kernel stores its accumulators as a partial row of `work` -- row 2 * workgroup + wave,
// nvar x TAPE_VALUES_PART words: n_int, n_frac, n_unbounded, min (low, high), k_min, max (low, high), k_max, sum (three
// limbs) --, and the fold kernel, a workgroup per unknown, merges the rows into the summary.  LDS: the slot rows and,
// staged, the program; the reduction itself lives in registers and takes none.
enum {
  TAPE_VALUES_PART = 12,           // words of a partial record
  TAPE_VALUES_MAX_BLOCKS = 2048,   // the grid's cap: 2 rows x 64 unknowns x 96 bytes each is 24 MiB of work at most
  TAPE_VALUES_FOLD_BLOCK = 1024    // lanes of the fold kernel's workgroup, at most
};
// workgroups of the main kernel: no more than chunks of TAPE_BLOCK points, than the cap, and than `bound` (> 0)
static inline long long tape_values_blocks(long long n_points, long long bound) {
  long long b = (n_points + TAPE_BLOCK - 1) / TAPE_BLOCK;
  if (b > TAPE_VALUES_MAX_BLOCKS) b = TAPE_VALUES_MAX_BLOCKS;
  return b < bound ? b : bound;
}
// bytes of `work` a call needs, whatever the device: the rows of tape_values_blocks(n_points, no bound)
static inline size_t tape_values_work_bytes(long long n_points, int nvar) {
  return (size_t)tape_values_blocks(n_points, TAPE_VALUES_MAX_BLOCKS) * (TAPE_BLOCK / 64) * (size_t)nvar * TAPE_VALUES_PART * 8;
}
struct TapeValuesLaunch {
  TapeLaunch t;           // the program; t.points and the outputs are not used; t.n_points = prod ext[c]
  int n_ctx;              // rows of the context
  int cus;                // compute units of the device
  int max_blocks;         // testing aid, as in TapeSweepLaunch
  int pad;
  const long long *ctx;   // device; n_ctx x (t.nparm + 2)
  long long *summary;     // device; PIPAMD_VALUES_WORDS(t.nvar) words, written by the launch
  long long *work;        // device; tape_values_work_bytes(t.n_points, t.nvar) bytes, need not be initialised
  long long lo[TAPE_MAX_SLOTS - 1];
  unsigned long long ext[TAPE_MAX_SLOTS - 1];
};

// pipamd_tape_set_sweep_run: every job -- a tape of a set, a box, a context -- swept in one launch, a summary per job.
// Everything a job needs lies in ONE device buffer of 8-byte words that pipamd_tape_set_sweep_create fills once:
//     chunk_off[n_jobs + 1]    the chunks of TAPE_BLOCK consecutive k before job j; the last word is all chunks
//     summary_off[n_jobs + 1]  the summary words before job j; the last word is all words
//     n_jobs x TapeSetSweepJob
//     per job: lo[cols], ext[cols], then its n_ctx context rows of cols + 2 words (cols: the tape's point_cols) -- ragged
// Offsets inside the buffer count words from its start.  A chunk never spans jobs: chunk c belongs to the job j with
// chunk_off[j] <= c < chunk_off[j + 1] and holds the k from (c - chunk_off[j]) * TAPE_BLOCK on, inside job j's own box.
// The sweep's bounded persistent grid (TAPE_SWEEP_WG_PER_CU_SUM) takes the chunks 0 .. chunk_off[n_jobs] - 1 in grid
// stride; the programs are read from the set's buffer in global memory as pip_tape_set_eval_kernel reads them.
struct TapeSetSweepJob {
  int tape, n_ctx;       // index into the set's table; rows of the context
  long long box;         // word of lo[0]; ext[0] is `cols` words behind
  long long ctx;         // word of the first context row
  long long n_points;    // prod ext[c], 1 .. 2^38 - 1
  long long summary_off; // first word of the job's PIPAMD_SWEEP_WORDS(leaves) in the summary
  long long leaves;
  long long chunk_off;   // chunk_off[j]
  long long pad;
};  // 64 bytes
struct TapeSetSweepLaunch {
  const long long *prog;      // device; the set's programs
  const TapeSetEntry *table;  // device; the set's table
  const long long *buf;       // device; the buffer above
  int n_jobs, bits, slots;    // slots: the set's, the LDS rows
  int blocks;                 // pipk_tape_set_sweep_blocks of the set: what the device holds at once
  int max_blocks;             // testing aid, as in TapeSweepLaunch
  int pad;
  long long chunks, words;    // chunk_off[n_jobs], summary_off[n_jobs]
  long long *summary;         // device; `words` words, initialised by the launch
};

extern "C" {
// workgroups the device holds at once of pip_tape_set_sweep_kernel for a set of `slots` slots: the occupancy with that
// LDS, at most TAPE_SWEEP_WG_PER_CU_SUM a compute unit
int pipk_tape_set_sweep_blocks(int bits, int slots, int cus);
hipError_t pipk_launch_tape_set_sweep(const TapeSetSweepLaunch *t, hipStream_t stream);
hipError_t pipk_launch_tape_values(const TapeValuesLaunch *t, hipStream_t stream);
hipError_t pipk_launch_tape_compare(const TapeCompareLaunch *t, hipStream_t stream);
hipError_t pipk_launch_tape_sweep(const TapeSweepLaunch *t, hipStream_t stream);
hipError_t pipk_launch_tape_eval(const TapeLaunch *t, hipStream_t stream);
hipError_t pipk_launch_tape_set_eval(const TapeSetLaunch *t, hipStream_t stream);
}
#endif
