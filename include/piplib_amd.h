/* include/piplib_amd.h -- C ABI of the MI355X-native PipLib hot path.
 *
 * Plain C, plain pointers and sizes: this is what a PipLib maintainer binds to
 *  in place of the CPU implementations of
 *
 *   traiter()/pivoter()/choisir_piv()/exam_coef()   reference source/traiter.c:101-159,297-548,628-791
 *   integrer() (Gomory cut rows)                    reference source/integrer.c:305-534
 *   tab_alloc()/tab_get()/expanser() row store      reference source/tab.c:158-248, traiter.c:55-88
 *
 * Two public layers, lowest first:
 *   1. pipamd_batch_*   : a *uniform* batch of tableaux that lives in HBM; one
 *                         workgroup per tableau runs the whole pivot loop on the GPU.
 *   3. pipamd_traiter, pipamd_solve_*
 *                       : traiter() itself (traiter.c:628) -- the quast decision tree on the
 *                         host, every pivot on the GPU -- filling the reference's solution tape,
 *                         so that piplib.c / maind.c / sol.c stay the reference's own.
 * (Layer 2 -- heterogeneous jobs of any shape in one arena, advanced until each is finished or
 *  needs a host decision -- is internal: it is what layer 3's quast builder drives.)
 *
 * All device pointers are ordinary HIP device pointers (e.g. torch
 * `tensor.data_ptr()`); `stream` is a hipStream_t passed as void*.
 * Every function returns 0 on success or a negative PIPAMD_E_* code; nothing
 * here falls back to a CPU implementation.
 */
#ifndef PIPLIB_AMD_H
#define PIPLIB_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this interface, also returned by pipamd_version() of the library that was loaded: a binding checks
 * the two against each other before it calls anything else (entry points were added and changed between versions
 * without the symbols changing).  100: round 1.  200: round 2 -- pipamd_traiter / pipamd_solve_tableau* hand out
 * tape cells (`cells, n_cells`) instead of text; the transliterated pip_solve front end (pipamd_pip_solve,
 * pipamd_quast_*) is gone: pip_solve stays the reference's piplib.c over bindings/piplib_traiter_hook.c.
 * 300: round 3 -- pipamd_batch_solve_async / _wait / _poll, pipamd_batch_load_part, unbounded row growth in the
 * batch layer (no PIPAMD_ST_CAPACITY short of the engine's 16,000-row limit), pipamd_solve_tableaux128,
 * pipamd_engine_set_max_rows.  400: round 4 -- pipamd_solve_tableaux_lockstep128, pipamd_engine_set_lean64; the 128-bit
 * entries try the device-resident traiter() first (pipamd_last_device_tree answers for them too); nothing removed.
 * 500: the device-resident traiter() takes problems of 65 ... 128 columns too (two column blocks per wave);
 * pipamd_device_tree_fits tells whether a shape is in its box; nothing removed.  Added since, the version unchanged (a
 * binding looks them up in the library): pipamd_traiter_many / pipamd_traiter_many128 -- traiter() for many problems,
 * flags per problem --, and the device-resident traiter() computes the dual (PIPAMD_T_DUAL) for every shape of its box,
 * not only up to 64 inequalities; pipamd_batch_dual / pipamd_batch_dual_part -- the dual values of a rational batch of
 * layer 1; pipamd_batch_load_system / pipamd_batch_dual_system and their _part forms -- layer 1 from the plain system
 * pip_solve takes (equalities, tab_simplify, the dual under Maximize / Urs_unknowns and of equalities);
 * pipamd_batch_load_matrices / pipamd_batch_dual_matrices and their _part forms -- the same from PolyLib matrices, each
 * system with its own row count and its equalities where its marker column has them (PIPAMD_ST_BADINPUT);
 * pipamd_batch_load_sparse / pipamd_batch_dual_sparse and their _part forms -- the plain system as sparse rows (CSR on
 * the device), the tableaux built from them as from the dense expansion; pipamd_batch_load_instances /
 * pipamd_batch_dual_instances and their _part forms -- one parametric system at many parameter points, substituted
 * exactly on the device (a constant that does not fit the entry type: PIPAMD_ST_BADINPUT); pipamd_tape_check /
 * pipamd_tape_compile / pipamd_tape_eval / pipamd_tape_free and the 128-bit forms of the first two (and
 * pipamd_tape_check_pip / pipamd_tape_compile_pip with pip_solve's result edits, pipamd_tape_point_cols,
 * pipamd_tape_set_create / _eval / _free for many tapes in one launch) -- a tape evaluated at
 * many parameter points, a lane per point; pipamd_tape_sweep_plan / pipamd_tape_sweep -- a tape swept over a box of
 * points the kernel makes itself, under a context (PIPAMD_ST_OUTSIDE), with a summary reduced on the device;
 * pipamd_tape_compare_plan / pipamd_tape_compare / pipamd_tape_compare_sweep -- two tapes, of either cell width each,
 * compared by value at the points of a list or a box (PIPAMD_CMP_*); pipamd_tape_sweep_values_plan /
 * pipamd_tape_sweep_values -- per unknown the minimum, the maximum, where they are attained and the exact sum over a
 * box (PIPAMD_VALUES_*). */
#define PIPAMD_VERSION 500

/* ---- error codes (return values) ---- */
#define PIPAMD_OK 0
#define PIPAMD_E_INVALID -1   /* bad argument / shape */
#define PIPAMD_E_HIP -2       /* a HIP runtime call failed (no GPU, OOM, ...) */
#define PIPAMD_E_TOOLARGE -3  /* shape exceeds the engine's compiled limits */
#define PIPAMD_E_NOMEM -4
#define PIPAMD_E_SOLVER -5    /* per-problem failure, see the status array */

/* ---- traiter flags (reference funcall.h:32-33) ---- */
#define PIPAMD_T_INT 1
#define PIPAMD_T_DUAL 2
/* engine-only flags */
#define PIPAMD_T_SORT 256    /* rows not yet sorted (tab_sort_rows, traiter.c:556) */
#define PIPAMD_T_DEEPEST 512 /* deepest-cut option (integrer.c:417-438) */
#define PIPAMD_T_NOSKIP 2048 /* measurement aid: rewrite every real row on every pivot, as the
                               reference's loop does (traiter.c:467-502); results are identical */
#define PIPAMD_T_ROWS_STAY 8192 /* pipamd_batch_desc.tflags: the caller keeps the `rows` array of pipamd_batch_load alive
                                  and unchanged until the batch's next pipamd_batch_solve has returned.  The load then
                                  only builds the row tables; the first pivot launch reads the rows from the caller's
                                  array in the pass that builds its summaries anyway (64-bit entries, an even number
                                  of columns, a 16-byte aligned array; otherwise the rows are copied as usual). */
#define PIPAMD_T_STATE 1024  /* a paused job's LDS summaries are saved in its state block */

/* ---- per-problem status written by the engine ---- */
#define PIPAMD_ST_RUN 0          /* not finished (iteration limit reached: relaunch) */
#define PIPAMD_ST_SOLUTION 1     /* all rows non-negative (and integral if T_INT): solution rows valid */
#define PIPAMD_ST_NIL 2          /* no solution (traiter.c:782-785, integrer.c:482-485) */
#define PIPAMD_ST_NEED_COMPA 3   /* parametric signs undecided: host runs compa_test (traiter.c:682) */
#define PIPAMD_ST_NEED_PARMCUT 4 /* parametric Gomory cut on row `aux`: host runs find/add_parm */
#define PIPAMD_ST_OVERFLOW 5     /* the reference's "Integer overflow" exit (traiter.c:424,442) */
#define PIPAMD_ST_CAPACITY 6     /* spare columns (cap_newparm) exhausted, or the engine's row limit (16,000 rows; 128-bit
                                    entries: what fits a workgroup's LDS) reached; pipamd_batch_solve itself grows rows */
#define PIPAMD_ST_RANGE 7        /* entries too large for the exact fast pivot-column choice */
#define PIPAMD_ST_INTERNAL 8
#define PIPAMD_ST_MAXCOL 9       /* "Too many variables" (integrer.c:324) */
#define PIPAMD_ST_BADINPUT 10    /* a system the load could not take (see pipamd_batch_load_matrices, _sparse, _instances) */
#define PIPAMD_ST_OUTSIDE 11     /* pipamd_tape_sweep alone: the point violates a row of the context */

/* ---- row flags (reference tab.h:55-62) ---- */
#define PIPAMD_F_UNIT 1
#define PIPAMD_F_PLUS 2
#define PIPAMD_F_MINUS 4
#define PIPAMD_F_ZERO 8
#define PIPAMD_F_CRITIC 16
#define PIPAMD_F_UNKNOWN 32

typedef struct pipamd_engine pipamd_engine;

/* Engine = device + limits.  `device` is a HIP ordinal (after HIP_VISIBLE_DEVICES). */
int pipamd_engine_create(pipamd_engine **out, int device);
void pipamd_engine_destroy(pipamd_engine *e);
const char *pipamd_last_error(void);
/* Upper bound on pivots per problem per launch (a problem still PIPAMD_ST_RUN afterwards is resumed by the next
 * launch of the same pipamd_batch_solve).  At most 512 (the default; larger values are clamped): a launch logs
 * (pivot, denominator) per pivot for the determinant bookkeeping of traiter.c:412-446, which a replay kernel runs
 * after the launch, and a job's log holds 512 entries.  pipamd_batch_solve gives up on a batch (PIPAMD_E_SOLVER)
 * after 512 launches, i.e. a tableau may take 262,144 pivots. */
int pipamd_engine_set_iter_limit(pipamd_engine *e, int pivots_per_launch);
/* Waves (64 lanes each) that share one tableau: 1 keeps more tableaux in flight per CU (best for
 * large batches of sparse problems), 4 spreads a tableau's rows over four waves (few or dense
 * tableaux), 8 likewise (64-bit entries of <= 128 columns); 0 (default) = 1 when the batch has >= 2048
 * tableaux, else 4. */
int pipamd_engine_set_waves_per_job(pipamd_engine *e, int waves);
/* Waves per tableau of the tail launch of pipamd_batch_solve (4, the default, or 8).  Eight spread
 * the 15-25 rows a late pivot of a long tableau rewrites over twice the waves: a caller that runs
 * one batch at a time gains ~8 %; with many batches in flight the extra waves of a tail crowd out
 * other batches' bulk launches (-3 %).  64-bit entries of <= 128 columns; 4 otherwise.
 * A tail launch of a 128-bit batch over at most 256 tableaux gives each a whole CU (sixteen waves): the hundreds of rows a
 * late pivot of a long tableau rewrites spread over four times the waves (built in; this call or
 * pipamd_engine_set_waves_per_job switch it off). */
int pipamd_engine_set_tail_waves(pipamd_engine *e, int waves);
/* One batch at a time (1) or many in flight on other engines (0, the default).  A bulk-sized batch of 127 unknowns in
 * 64 bits starts with the lean one-wave launch (entries below 2^15); the tableaux that launch leaves go through the
 * general one-wave launch and then the tail launches.  That middle launch keeps the device full when other batches'
 * launches run beside it; for a lone batch it is a long, nearly empty launch, and the tableaux go straight to the
 * tail launches instead (a lone 10k batch: 4.7 ms instead of 6.3 ms; 14 batches in flight: 10 % fewer pivots/s). */
int pipamd_engine_set_lone_batches(pipamd_engine *e, int on);
/* The second lean launch of a bulk batch has a block per tableau over a list of the few hundred the first one paused.
 * 1 (default): its blocks beyond the list replay the determinant logs of the tableaux the first launch finished, beside
 * the launch's own tableaux, and the replay behind the launches, which then finds most logs empty, goes out a wave per
 * tableau.  0: that replay does all the work, a lane per tableau (the sequence of rounds 3 to 5).  Same statuses, pivot
 * counts and solutions either way; the switch is for measurements. */
int pipamd_engine_set_spare_replay(pipamd_engine *e, int on);
/* Waves per tableau in that second lean launch: 4 (default) -- the launch lasts as long as its longest tableau's chain of
 * pivots, so the rows a pivot rewrites are spread over four waves (csrc/pip_lean.h, NW = 4), where the launch's row
 * capacity has such a kernel (113 ... 160 row slots, no big parameter), else one wave as before -- or 1, the sequence of
 * round 6.  Same statuses, pivot counts and solutions either way; the switch is for measurements. */
int pipamd_engine_set_lean2_waves(pipamd_engine *e, int waves);
/* 128-bit batches without parameters of 129 ... 256 columns (at least 128 tableaux): 1 = the first launch of
 * pipamd_batch_solve is pip_lean64_kernel (csrc/pip_lean.h, long long rows) -- one wave per tableau, rows held as long longs while every
 * entry fits 63 bits (half the traffic and registers), tableaux with a wider entry handed over to the 128-bit kernel.
 * Default 0: on BASELINE's configs[4] it is no faster than the four-waves-per-tableau 128-bit kernel. */
int pipamd_engine_set_lean64(pipamd_engine *e, int on);
/* Bulk batches whose one parameter is the big one (nparm == 1, bigparm == nvar + 1, at most 126 unknowns, 64-bit entries:
 * what pipamd_batch_load_shifted builds for lexicographic maxima and unknowns of either sign): 1 = their one-wave launches
 * are the lean kernel's big-parameter flavour (csrc/pip_lean.h), as for batches without parameters.  Same statuses, pivot
 * counts and solutions.  Default 0, the launches such a batch always took: measured on 10,000 tableaux of 126 unknowns x 64
 * inequalities the flavour is 13-35 % ahead with eight batches in flight and for a lone Maximize batch, but 3 % behind for a
 * lone Urs_unknowns batch.  A caller that keeps batches in flight switches it on. */
int pipamd_engine_set_lean_big(pipamd_engine *e, int on);
/* How pipamd_batch_solve waits for the device at its end: 0 (default) polls the stream, which is the
 * quickest for a few host threads; 1 naps 40 us between looks at the stream.  With more batches in flight
 * than the host has CPUs the spinning threads take turns on the cores: 48 batches of 1,250 tableaux on 16 CPUs ran
 * at 157 M pivots/s polling and 240 M sleeping. */
int pipamd_engine_set_blocking_wait(pipamd_engine *e, int on);
int pipamd_version(void);

/* ------------------------------------------------------------------ layer 1 */
typedef struct pipamd_batch_desc {
  int32_t batch;       /* number of tableaux */
  int32_t nvar;        /* unknowns */
  int32_t nparm;       /* parameters (0 => whole solve stays on the GPU) */
  int32_t ni;          /* inequality rows per tableau */
  int32_t bigparm;     /* column index of the big parameter or -1 */
  int32_t tflags;      /* PIPAMD_T_INT ... */
  int32_t cap_cuts;    /* spare rows per tableau for Gomory cuts */
  int32_t cap_newparm; /* spare columns per tableau (parametric cuts) */
  int32_t entier_bits; /* 0 or 64: int64 entries (the reference's long long build);
                          128: __int128 entries, same algorithm, overflow-safe variant */
} pipamd_batch_desc;

/* bytes of device workspace the batch needs (tableaux + row tables + job table + results) */
size_t pipamd_batch_workspace_bytes(const pipamd_batch_desc *d);

/* tab_get() for a whole batch: rows[b][i][0..ncol) (ncol = nvar+nparm+1, PIP column
 * order unknowns|constant|parameters) become Unknown rows with denominator 1 under nvar
 * unit rows.  `d_rows` is device memory, int64. */
int pipamd_batch_load(pipamd_engine *e, void *d_workspace, const pipamd_batch_desc *d,
                      const int64_t *d_rows, void *stream);

/* The same for the tableaux first .. first + count - 1 of the batch only; `d_rows` holds those `count` tableaux.  A
 * batch can thus be assembled from several row arrays -- e.g. one GPU's shards of the K batches a caller has in
 * flight, fused into one workspace so that ONE launch sequence serves them all instead of K small ones (what
 * bench.py's strong-scaling mode does; piplib_amd/dist.py).  Every tableau of the batch must have been loaded by
 * some call before pipamd_batch_solve. */
int pipamd_batch_load_part(pipamd_engine *e, void *d_workspace, const pipamd_batch_desc *d, const int64_t *d_rows,
                           int first, int count, void *stream);

/* traiter() on every tableau of the batch.  Launches on `stream` and returns when every
 * tableau has a final status (it synchronises the stream between rounds).  A tableau that spends its cap_cuts
 * spare rows is moved to a block of twice the row capacity (the reference's expanser, traiter.c:55-88, as integrer
 * calls it on a full tableau, integrer.c:410-415) as often as it takes, up to the engine's 16,000 rows: cap_cuts
 * is a size hint, not a limit. */
int pipamd_batch_solve(pipamd_engine *e, void *d_workspace, const pipamd_batch_desc *d, void *stream);

/* The same in two halves, so that ONE host thread keeps many batches in flight: pipamd_batch_solve_async enqueues
 * the launch sequence (bulk launch, tail launch, a copy of the tail's control words) on `stream` and returns without
 * waiting.  pipamd_batch_poll never blocks: 0 while the launches enqueued so far run; once they have ended it looks at
 * what they left -- if tableaux remain (beyond the per-launch pivot limit, or out of spare rows: those are re-housed)
 * it enqueues the next launches and returns 0 again; 1 when every tableau has its final status (or nothing is in
 * flight); < 0 on error.  pipamd_batch_wait does the same blocking and returns PIPAMD_OK when the batch is done.
 * One solve in flight per engine -- an engine is a small host object: a caller keeps K of them, each with its own
 * stream and workspace, starts a batch on each and polls them in turn, starting the next batch on whichever is done:
 * a lone batch leaves most of the GPU idle in its latency-bound tail, K batches in different phases fill it
 * (bench.py: one host thread, K = 14).  Results may be fetched once poll has returned 1 / wait has returned. */
int pipamd_batch_solve_async(pipamd_engine *e, void *d_workspace, const pipamd_batch_desc *d, void *stream);
/* Row budget of the growth above: a tableau is re-housed only while its row capacity stays within `rows` (at least
 * ni + cap_cuts; 0 = the default, only the engine's own limit) and ends PIPAMD_ST_CAPACITY beyond it.  The reference
 * grows without bound and so does the default; on inputs where Gomory cuts converge slowly (thousands of cut rows,
 * every pivot then rewriting thousands of rows) a caller bounds the memory and time of a batch with it. */
int pipamd_engine_set_max_rows(pipamd_engine *e, int rows);
int pipamd_batch_wait(pipamd_engine *e);
int pipamd_batch_poll(pipamd_engine *e);

/* Copy out, device to device: status[b], pivots[b], cuts[b] (int32 each, may be NULL),
 * sol_num[b][i][0..nparm] (parameter coefficients then constant, as solution() emits them,
 * traiter.c:255-271) and sol_den[b][i], i < nvar: int64 each, or little-endian pairs of
 * int64 (low, high) per value when entier_bits == 128. */
int pipamd_batch_results(pipamd_engine *e, const void *d_workspace, const pipamd_batch_desc *d,
                         int32_t *d_status, int32_t *d_pivots, int32_t *d_cuts, int64_t *d_sol_num,
                         int64_t *d_sol_den, void *stream);

/* Lexicographic maxima and unknowns of either sign: pip_solve with Maximize or Urs_unknowns (piplib.c:777-797, 846-858)
 * for a whole batch.  The reference rewrites every inequality under a new "big parameter" Bg (tab_Matrix2Tableau,
 * tab.c:292-393), solves with traiter(..., bigparm = Bg, ...) and undoes the shift in the answer (sol_vector_edit,
 * sol.c:435-512).  Such a tableau needs no host decision -- exam_coef decides every sign from the big coefficient, then
 * the constant (traiter.c:107-157), and integrer cuts on the constant alone (integrer.c:373-377) -- so layer 1 finishes
 * the batch on its own, through the launch sequence of a batch without parameters (with pipamd_engine_set_lean_big, bulk
 * batches of at most 126 unknowns start with the lean kernel's big-parameter flavour, csrc/pip_lean.h).
 * The descriptor `d` describes the tableau AS IT IS SOLVED, for these entries and for pipamd_batch_workspace_bytes /
 * pipamd_batch_solve alike: nparm == 1, bigparm == nvar + 1 (column order unknowns | constant | big).
 * pipamd_batch_load_shifted: `d_rows` holds the caller's PLAIN system, batch x ni x (nvar + 1) int64 (unknowns then
 * constant); the load kernel writes per row what tab.c:342-377 writes for a new big parameter:
 *     PIPAMD_SHIFT_MAX:  -a_j | c | +sum a_j          PIPAMD_SHIFT_URS:  a_j | c | -sum a_j
 * The sum wraps in 64 bits as the reference's long long build does; with entier_bits == 128 it is exact.
 * PIPAMD_T_ROWS_STAY in tflags is ignored by these two entries (the caller's array is not the tableau; it may be
 * released once the load's work on `stream` is done).  _part: tableaux first .. first + count - 1, as
 * pipamd_batch_load_part.
 * pipamd_batch_results_shifted: sol_vector_edit with SOL_REMOVE and SOL_MAX / SOL_SHIFT.  For unknown i with big
 * numerator B, constant numerator N and denominator D (what pipamd_batch_results hands out as sol_num[b][i][0..1],
 * sol_den[b][i]): g = gcd(N, D) >= 0 (gcd(0, D) = D), d_x_num[b][i] = N / g, negated for PIPAMD_SHIFT_MAX;
 * d_x_den[b][i] = D / g, or 0 if B != D -- the reference's mark for an unbounded unknown (it prints "/0"), the numerator
 * kept.  A tableau whose status is not PIPAMD_ST_SOLUTION gets (0, 0) in every entry.  int64 each, or (low, high) pairs
 * for entier_bits == 128; status, pivots and cuts as in pipamd_batch_results; each of the five arrays may be NULL.
 * PIPAMD_E_INVALID, before any HIP call: a null engine, workspace, descriptor or rows pointer; shift other than +-1;
 * nparm != 1 or bigparm != nvar + 1; first / count outside the batch.
 * pipamd_batch_dual still refuses batches with a big parameter. */
#define PIPAMD_SHIFT_MAX 1    /* Maximize:     lexicographic maximum, unknowns >= 0      */
#define PIPAMD_SHIFT_URS (-1) /* Urs_unknowns: lexicographic minimum, unknowns of any sign */
int pipamd_batch_load_shifted(pipamd_engine *e, void *d_workspace, const pipamd_batch_desc *d, const int64_t *d_rows,
                              int shift, void *stream);
int pipamd_batch_load_shifted_part(pipamd_engine *e, void *d_workspace, const pipamd_batch_desc *d, const int64_t *d_rows,
                                   int shift, int first, int count, void *stream);
int pipamd_batch_results_shifted(pipamd_engine *e, const void *d_workspace, const pipamd_batch_desc *d, int shift,
                                 int32_t *d_status, int32_t *d_pivots, int32_t *d_cuts, int64_t *d_x_num, int64_t *d_x_den,
                                 void *stream);

/* Compute_dual (the reference's TRAITER_DUAL, traiter.c:273-294, 567-620) for a batch solved with PIPAMD_T_DUAL in
 * tflags: the list of dual values solution_dual emits behind a rational solution, one per input inequality.  Callable
 * once pipamd_batch_solve / _wait has returned or _poll has returned 1; launches one kernel on `stream` and does not
 * synchronise, like pipamd_batch_results.  `d_rows` is the array the tableaux were loaded from (pipamd_batch_load),
 * unchanged: the reference's `pos` table -- where each inequality sits after tab_sort_rows -- does not survive the
 * solve and is recomputed from the input rows; the caller keeps the array until the call's work on `stream` is done.
 * d_dual_num[b][i], d_dual_den[b][i], i < ni: what solution_dual hands to sol_val, not reduced -- if inequality i's row
 * has become a unit row, (valeur(tp, 0, its unit column), Denom(tp, 0)), otherwise (0, 1); int64 each, or little-endian
 * (low, high) int64 pairs when entier_bits == 128.  A tableau whose status is not PIPAMD_ST_SOLUTION gets (0, 0) in
 * every entry (a real dual never has denominator 0).
 * PIPAMD_E_INVALID, before any HIP call: a null pointer, a descriptor without PIPAMD_T_DUAL or with PIPAMD_T_INT (the
 * dual needs a rational solve, as in pipamd_traiter), nparm != 0 or bigparm >= 0 (layer 1 finishes only batches without
 * parameters on its own), first / count outside the batch.  PIPAMD_E_TOOLARGE: more than 8,192 inequalities per tableau
 * (the kernel sorts them in 48 KB of LDS).
 * The price of PIPAMD_T_DUAL is paid in the solve: such a batch does not start with the lean launches (pip_lean_kernel
 * / pip_lean64_kernel) but with the general one-wave bulk launch, so that every finished tableau has its rows in the
 * general format -- a tableau the lean kernels finish keeps them packed, and teaching them to unpack would cost
 * registers pip_lean_kernel does not have (64 VGPRs, no slack).  Dual batches of 2,048 tableaux and more are therefore
 * slower than plain ones; statuses, pivot counts and solutions are the same, and batches without the flag take exactly
 * the launches they took before. */
int pipamd_batch_dual(pipamd_engine *e, const void *d_workspace, const pipamd_batch_desc *d, const int64_t *d_rows,
                      int64_t *d_dual_num, int64_t *d_dual_den, void *stream);
/* The same for the tableaux first .. first + count - 1 only: `d_rows` holds those `count` tableaux (what
 * pipamd_batch_load_part was given), d_dual_num / d_dual_den are the arrays of the whole batch. */
int pipamd_batch_dual_part(pipamd_engine *e, const void *d_workspace, const pipamd_batch_desc *d, const int64_t *d_rows,
                           int first, int count, int64_t *d_dual_num, int64_t *d_dual_den, void *stream);

/* The system pip_solve(inequnk, NULL, -1, options) takes, for a whole batch: what tab_Matrix2Tableau (tab.c:292-393) and
 * tab_simplify (tab.c:396-427) do to it on the way to traiter(), and what pip_solve does to the dual on the way back
 * (sol_vector_edit with flags 0, sol.c:475-500; pip_quast_equalities_dual, piplib.c:651-690).  `d_rows` holds the caller's
 * PLAIN systems, batch x nrows x (nvar + 1) int64 (unknowns then constant: a PolyLib row without its marker column).  The
 * rows whose marker is 0 -- the equalities -- are named by ONE host list for the batch (same-shaped systems have them in
 * the same rows; systems that are not shaped alike: pipamd_batch_load_matrices below).  The descriptor `d` describes the tableau AS IT IS SOLVED, as for the shifted entries:
 * d->ni == nrows + neq; shift == 0: nparm == 0, bigparm == -1; shift == +-1: nparm == 1, bigparm == nvar + 1.
 * pipamd_batch_load_system: input row r becomes tableau row r + (equalities before r), written as tab.c:342-377 writes it,
 *     shift == 0:  a_j | c        PIPAMD_SHIFT_MAX:  -a_j | c | +sum a_j        PIPAMD_SHIFT_URS:  a_j | c | -sum a_j
 * (the sum in the entry type, as pipamd_batch_load_shifted), and an equality is followed by its negation in EVERY column,
 * the constant and the big column included (tab.c:380-388).  With `simplify`, tab_simplify then runs on each of the ni
 * rows: g = the gcd of every column but the constant (the big one included); for g > 1 those columns are divided by g
 * and the constant is divided with the floor; a row with g of 0 or 1 stays.  pip_solve simplifies every integer problem
 * (piplib.c:848-849): a batch loaded without it takes another pivot sequence to the same answer.  Row tables, spare slots
 * and the job header as pipamd_batch_load; PIPAMD_T_ROWS_STAY is ignored (the caller's array is not the tableau; it may
 * be released once the load's work on `stream` is done).  The solve and the result entries are the existing ones
 * (pipamd_batch_results, or pipamd_batch_results_shifted for shift == +-1).
 * pipamd_batch_dual_system: Compute_dual for a batch loaded this way and solved with PIPAMD_T_DUAL, callable where
 * pipamd_batch_dual is; one kernel on `stream`, no synchronisation; `d_rows` is the array the batch was loaded from.
 * d_dual_num[b][r], d_dual_den[b][r], r < nrows: ONE pair per input row, as pip_solve's answer lists them -- the pair of
 * pipamd_batch_dual for the row's tableau row, in lowest terms (g = gcd(N, D): N / g, D / g); for an equality with the
 * values u (its row) and v (the negated row) u if u != 0, else -v, so an equality's value may be negative.  (0, 0)
 * throughout for a tableau whose status is not PIPAMD_ST_SOLUTION.  int64 each, or (low, high) pairs for
 * entier_bits == 128.  pipamd_batch_dual itself still refuses batches with a big parameter.
 * PIPAMD_E_INVALID, before any HIP call: a null engine, workspace, descriptor, `sys` or rows pointer; shift not 0, 1 or
 * -1; a descriptor that does not match the shift; nrows < 0; neq < 0 or > nrows; d->ni != nrows + neq; eq_rows null with
 * neq > 0, not strictly increasing or out of range; simplify not 0 or 1, or 1 without PIPAMD_T_INT; first / count
 * outside the batch; for the dual entries a null output array, no PIPAMD_T_DUAL, or PIPAMD_T_INT.  PIPAMD_E_TOOLARGE for
 * the dual entries: d->ni above 8,192, as pipamd_batch_dual. */
typedef struct pipamd_system {
  int32_t nrows;          /* rows of the caller's system (PipMatrix NbRows), nvar + 1 int64 each: unknowns | constant */
  int32_t neq;            /* how many of them are equalities */
  const int32_t *eq_rows; /* HOST array of their indices, strictly increasing, the same for every system of the batch;
                             read before the call returns (the caller may free it at once); NULL when neq == 0 */
  int32_t shift;          /* 0, PIPAMD_SHIFT_MAX or PIPAMD_SHIFT_URS */
  int32_t simplify;       /* 1: tab_simplify on the tableau, as pip_solve does whenever Nq; needs PIPAMD_T_INT */
} pipamd_system;
int pipamd_batch_load_system(pipamd_engine *e, void *d_workspace, const pipamd_batch_desc *d, const pipamd_system *sys,
                             const int64_t *d_rows, void *stream);
int pipamd_batch_load_system_part(pipamd_engine *e, void *d_workspace, const pipamd_batch_desc *d, const pipamd_system *sys,
                                  const int64_t *d_rows, int first, int count, void *stream);
int pipamd_batch_dual_system(pipamd_engine *e, const void *d_workspace, const pipamd_batch_desc *d, const pipamd_system *sys,
                             const int64_t *d_rows, int64_t *d_dual_num, int64_t *d_dual_den, void *stream);
int pipamd_batch_dual_system_part(pipamd_engine *e, const void *d_workspace, const pipamd_batch_desc *d,
                                  const pipamd_system *sys, const int64_t *d_rows, int first, int count, int64_t *d_dual_num,
                                  int64_t *d_dual_den, void *stream);

/* The same for systems that are NOT shaped alike: what pip_solve literally takes, a PolyLib matrix per system, each with
 * its own number of rows and its equalities wherever they fell.  `d_rows` is batch x max_rows x (nvar + 2) int64: system
 * b has max_rows rows of room, of which the first nrows_b = d_nrows[b] are its rows, marker | a_0 .. a_(nvar-1) | c.  A row
 * whose marker is 0 is an equality, any other marker an inequality (piplib.c:769, tab.c:380); rows at and beyond nrows_b
 * are never read.  Row counts and markers stay on the device with the rows: no host list, no class of systems per call.
 * The descriptor describes the tableau as it is solved, as for the system entries (shift == 0: nparm == 0,
 * bigparm == -1; shift == +-1: nparm == 1, bigparm == nvar + 1), except that d->ni is ROOM, not a row count: system b
 * becomes a tableau of ni_b = nrows_b + (its equalities) rows and needs ni_b <= d->ni; the spare rows behind it are
 * cap_cuts plus d->ni - ni_b.
 * pipamd_batch_load_matrices: each system's tableau, row tables and job header (ni = ni_b) are exactly what
 * pipamd_batch_load_system builds for that system alone -- the row order, the shift, the negated twin of an equality,
 * tab_simplify with `simplify` --, spare slots cleared from slot ni_b on; PIPAMD_T_ROWS_STAY is ignored.  A system with
 * nrows_b < 1, nrows_b > max_rows or ni_b > d->ni is BAD: the load finishes it itself -- an empty tableau (ni = 0) with
 * status PIPAMD_ST_BADINPUT, nothing outside its own max_rows x (nvar + 2) room read.  pipamd_batch_solve skips it (it
 * is not PIPAMD_ST_RUN) and solves the other tableaux as if it were not there; the result entries give it zeros.  The
 * solve and the result entries are the existing ones.
 * pipamd_batch_dual_matrices: as pipamd_batch_dual_system, callable where that is; `d_rows` and `d_nrows` are the arrays
 * the batch was loaded from, unchanged.  d_dual_num[b][r], d_dual_den[b][r], r < max_rows: for r < nrows_b the pair
 * pipamd_batch_dual_system computes for that system alone (an equality: u if u != 0, else -v), (0, 0) for r >= nrows_b,
 * and (0, 0) throughout for a tableau that is not PIPAMD_ST_SOLUTION.
 * _part: the tableaux first .. first + count - 1; `d_rows` and `d_nrows` hold the `count` systems of the part, the dual
 * arrays are the whole batch's.
 * PIPAMD_E_INVALID, before any HIP call: a null engine, workspace, descriptor, `m` or rows pointer; shift not 0, 1 or
 * -1; a descriptor that does not match the shift; max_rows < 1 or d->ni < 1; reserved != 0; simplify not 0 or 1, or 1
 * without PIPAMD_T_INT; first / count outside the batch; for the dual entries a null output array, no PIPAMD_T_DUAL, or
 * PIPAMD_T_INT.  PIPAMD_E_TOOLARGE: max_rows above the engine's 16,000 rows; for the dual entries d->ni above 8,192. */
typedef struct pipamd_matrices {
  int32_t max_rows;       /* rows of room per system in d_rows (>= 1, <= the engine's 16,000) */
  int32_t shift;          /* 0, PIPAMD_SHIFT_MAX or PIPAMD_SHIFT_URS */
  int32_t simplify;       /* as pipamd_system.simplify; needs PIPAMD_T_INT */
  int32_t reserved;       /* 0 */
  const int32_t *d_nrows; /* DEVICE array, one int32 per system: its row count.  NULL: every system has max_rows rows */
} pipamd_matrices;        /* 24 bytes, offsets 0 4 8 12 16 */
int pipamd_batch_load_matrices(pipamd_engine *e, void *d_workspace, const pipamd_batch_desc *d, const pipamd_matrices *m,
                               const int64_t *d_rows, void *stream);
int pipamd_batch_load_matrices_part(pipamd_engine *e, void *d_workspace, const pipamd_batch_desc *d, const pipamd_matrices *m,
                                    const int64_t *d_rows, int first, int count, void *stream);
int pipamd_batch_dual_matrices(pipamd_engine *e, const void *d_workspace, const pipamd_batch_desc *d, const pipamd_matrices *m,
                               const int64_t *d_rows, int64_t *d_dual_num, int64_t *d_dual_den, void *stream);
int pipamd_batch_dual_matrices_part(pipamd_engine *e, const void *d_workspace, const pipamd_batch_desc *d,
                                    const pipamd_matrices *m, const int64_t *d_rows, int first, int count, int64_t *d_dual_num,
                                    int64_t *d_dual_den, void *stream);

/* The plain system of pipamd_batch_load_system as SPARSE rows: the constraint matrix a front end has, column / value pairs
 * with a row-pointer array (CSR), all three on the device.  `sys` is exactly the pipamd_system of the system entries
 * (nrows, neq, the HOST list eq_rows, shift, simplify) and the descriptor is theirs: d->ni == nrows + neq; shift == 0:
 * nparm == 0, bigparm == -1; shift == +-1: nparm == 1, bigparm == nvar + 1.  Row r of system s owns the entries
 * d_row_ptr[s * nrows + r] .. d_row_ptr[s * nrows + r + 1] - 1 of d_cols / d_vals; a column is 0 .. nvar - 1 for an
 * unknown and nvar for the constant; a row's columns are strictly increasing (canonical CSR); a stored 0 is allowed and
 * equals an absent entry.  Values are int64 for either entry width, as for the dense loads.
 * pipamd_batch_load_sparse: for every system the tableau, row tables, spare slots and job header are bit for bit what
 * pipamd_batch_load_system builds from the system's dense expansion (nrows x (nvar + 1), zero where nothing is stored):
 * the row order with an equality's negated twin, the shift, the big column summed in the entry type, tab_simplify.
 * PIPAMD_T_ROWS_STAY is ignored; the three arrays may be released once the load's work on `stream` is done.  The solve
 * and the result entries are the existing ones.
 * A system the load cannot take is BAD and handled as pipamd_batch_load_matrices handles its bad systems: the load
 * finishes it itself -- an empty tableau (ni = 0) with status PIPAMD_ST_BADINPUT --, pipamd_batch_solve skips it, the
 * result and dual entries give it zeros, and the other systems are not disturbed.  Bad is: a row pointer of the system
 * outside [0, nnz] or below its predecessor; a row of more than nvar + 1 entries; a column outside 0 .. nvar; a row whose
 * columns are not strictly increasing.  A system's pointers are checked before any entry is read through them, and
 * nothing of d_cols / d_vals is read outside [0, nnz).
 * pipamd_batch_dual_sparse: pipamd_batch_dual_system for a batch loaded this way, callable where that is; one kernel on
 * `stream`, no synchronisation; `s` names the arrays the batch was loaded from.  d_dual_num[b][r], d_dual_den[b][r],
 * r < nrows: one reduced pair per input row, an equality's two values merged (u if u != 0, else -v); (0, 0) throughout
 * for a tableau that is not PIPAMD_ST_SOLUTION, a bad system among them.
 * _part: the tableaux first .. first + count - 1; the three arrays and nnz describe the `count` systems of the part
 * (d_row_ptr has count * nrows + 1 offsets into the part's d_cols / d_vals), the dual arrays are the whole batch's.
 * PIPAMD_E_INVALID, before any HIP call: everything pipamd_batch_load_system / pipamd_batch_dual_system refuse, with the
 * same rules on `sys`, the descriptor and first / count; a null `s` or d_row_ptr; nnz < 0; null d_cols or d_vals with
 * nnz > 0.  PIPAMD_E_TOOLARGE as for the system entries. */
typedef struct pipamd_sparse {
  pipamd_system sys;        /* nrows, neq, eq_rows (HOST list), shift, simplify: exactly as pipamd_batch_load_system */
  int64_t nnz;              /* entries in d_cols / d_vals (of the call: the whole batch, or the part) */
  const int64_t *d_row_ptr; /* DEVICE, systems * nrows + 1 offsets */
  const int32_t *d_cols;    /* DEVICE: column of each entry, 0 .. nvar-1 an unknown, nvar the constant */
  const int64_t *d_vals;    /* DEVICE: its value */
} pipamd_sparse;            /* 56 bytes, offsets 0 24 32 40 48 */
int pipamd_batch_load_sparse(pipamd_engine *e, void *d_workspace, const pipamd_batch_desc *d, const pipamd_sparse *s,
                             void *stream);
int pipamd_batch_load_sparse_part(pipamd_engine *e, void *d_workspace, const pipamd_batch_desc *d, const pipamd_sparse *s,
                                  int first, int count, void *stream);
int pipamd_batch_dual_sparse(pipamd_engine *e, const void *d_workspace, const pipamd_batch_desc *d, const pipamd_sparse *s,
                             int64_t *d_dual_num, int64_t *d_dual_den, void *stream);
int pipamd_batch_dual_sparse_part(pipamd_engine *e, const void *d_workspace, const pipamd_batch_desc *d, const pipamd_sparse *s,
                                  int first, int count, int64_t *d_dual_num, int64_t *d_dual_den, void *stream);

/* INSTANCES of one parametric system: PipLib's native input -- one system whose right-hand sides depend on parameters --
 * solved at many parameter points (tile sizes or loop bounds to explore, sample points to hold a quast against, many
 * right-hand sides of one constraint matrix) without parameters in the tableaux.  d_matrix is ONE matrix on the device,
 * nrows x (nvar + nparm + 1) int64: unknowns | parameters | constant, a PolyLib row of pip_solve's inequnk without its
 * marker column; d_points gives system b its parameter values theta_b0 .. theta_b(nparm-1).  System b is the plain
 * system whose row r is a_r0 .. a_r(nvar-1) | c_r + sum_k p_rk * theta_bk, substituted on the device: N instances cost
 * nrows x (nvar + nparm + 1) + N x nparm words of input instead of N x nrows x (nvar + 1).  `sys` is exactly the
 * pipamd_system of the system entries (nrows, neq, the HOST list eq_rows, shift, simplify) and the descriptor is theirs,
 * the tableau as it is solved: d->ni == nrows + neq; shift == 0: d->nparm == 0, bigparm == -1; shift == +-1:
 * d->nparm == 1, bigparm == nvar + 1.  in->nparm, the parameters of the shared system, is NOT d->nparm.
 * pipamd_batch_load_instances: for every system the tableau, row tables, spare slots and job header are bit for bit what
 * pipamd_batch_load_system builds from that system's dense rows: the row order with an equality's negated twin, the
 * shift, the big column as the sum of the unknowns' coefficients only, tab_simplify.  PIPAMD_T_ROWS_STAY is ignored; the
 * two arrays may be released once the load's work on `stream` is done.  The solve and the result entries are the
 * existing ones.
 * The constant is computed EXACTLY, not stepwise in the entry type: a system is good whenever every one of its constants
 * fits the entry type (int64 for entier_bits 0 / 64, __int128 for 128), even when single products or partial sums do
 * not; nothing wraps anywhere in the substitution.  A system with a constant that does not fit is BAD and handled as
 * pipamd_batch_load_matrices and _sparse handle their bad systems: the load finishes it itself -- an empty tableau
 * (ni = 0) with status PIPAMD_ST_BADINPUT, nothing of it stored before that is known --, pipamd_batch_solve skips it, the
 * result and dual entries give it zeros, and the other systems are not disturbed.
 * Points are any int64 values.  PIP's convention that parameters are non-negative, and any context on them, are the
 * caller's business: they are the caller's choice of points, nothing here looks at them.
 * pipamd_batch_dual_instances: pipamd_batch_dual_system for a batch loaded this way, callable where that is; one kernel on
 * `stream`, no synchronisation; `in` names the arrays the batch was loaded from.  d_dual_num[b][r], d_dual_den[b][r],
 * r < nrows: one reduced pair per input row, an equality's two values merged (u if u != 0, else -v); (0, 0) throughout
 * for a tableau that is not PIPAMD_ST_SOLUTION, a bad system among them.
 * _part: the tableaux first .. first + count - 1; d_points holds the `count` points of the part and d_matrix is the
 * part's matrix -- parts of one batch may use different matrices of the same shape --, the dual arrays are the whole
 * batch's.
 * PIPAMD_E_INVALID, before any HIP call: everything pipamd_batch_load_system / pipamd_batch_dual_system refuse, with the
 * same rules on `sys`, the descriptor and first / count; a null `in` or d_matrix; nparm < 0; reserved != 0; null d_points
 * with nparm > 0.  PIPAMD_E_TOOLARGE as for the system entries, and for nvar + nparm + 1 above 512 (the reference's
 * MAXCOL). */
typedef struct pipamd_instances {
  pipamd_system sys;       /* nrows, neq, eq_rows (HOST list), shift, simplify: exactly as pipamd_batch_load_system */
  int32_t nparm;           /* parameters of the shared system that the points give values to (>= 0) */
  int32_t reserved;        /* 0 */
  const int64_t *d_matrix; /* DEVICE, nrows x (nvar + nparm + 1): unknowns | parameters | constant; ONE matrix for the
                              batch (or the part) */
  const int64_t *d_points; /* DEVICE, systems x nparm: the parameter values of each system; may be NULL when nparm == 0 */
} pipamd_instances;        /* 48 bytes, offsets 0 24 28 32 40 */
int pipamd_batch_load_instances(pipamd_engine *e, void *d_workspace, const pipamd_batch_desc *d, const pipamd_instances *in,
                                void *stream);
int pipamd_batch_load_instances_part(pipamd_engine *e, void *d_workspace, const pipamd_batch_desc *d, const pipamd_instances *in,
                                     int first, int count, void *stream);
int pipamd_batch_dual_instances(pipamd_engine *e, const void *d_workspace, const pipamd_batch_desc *d, const pipamd_instances *in,
                                int64_t *d_dual_num, int64_t *d_dual_den, void *stream);
int pipamd_batch_dual_instances_part(pipamd_engine *e, const void *d_workspace, const pipamd_batch_desc *d,
                                     const pipamd_instances *in, int first, int count, int64_t *d_dual_num, int64_t *d_dual_den,
                                     void *stream);

/* Batch totals, device memory, 4 x uint64: [0] pivots (calls of pivoter), [1] Gomory cuts,
 * [2] rows rewritten by pivots (rows whose pivot-column entry is zero and that are already
 * reduced are left untouched -- same result as the reference's multiply-by-one pass),
 * [3] tableaux finished (solution or nil). */
int pipamd_batch_counters(pipamd_engine *e, const void *d_workspace, const pipamd_batch_desc *d,
                          uint64_t *d_out4, void *stream);

/* Bytes ONE pivot of one tableau of this shape moves when every real row is read and written,
 * as the reference's loop does (traiter.c:467-502): 2 * ni * ncol * sizeof(Entier).  The engine
 * itself only touches the rows that change; bench.py's `roofline` uses that smaller figure --
 * 8 * ncol * (2 * rows_rewritten + 2 * pivots) from pipamd_batch_counters -- and reports this one
 * as `dense_equivalent_GBps` and for `roofline_dense_mode` (PIPAMD_T_NOSKIP). */
size_t pipamd_dense_pivot_bytes(const pipamd_batch_desc *d);

/* Sum of the pivot-kernel launch durations of the last pipamd_batch_solve in milliseconds,
 * measured with HIP events on the launch stream, and the number of those launches. */
int pipamd_last_solve_ms(pipamd_engine *e, float *ms);
/* The events cost four runtime calls per solve, which shows on batches of a few hundred small
 * tableaux: off = pipamd_batch_solve records none (pipamd_last_solve_ms then fails).  Default on. */
int pipamd_engine_set_timing(pipamd_engine *e, int on);
int pipamd_last_solve_launches(pipamd_engine *e);
/* pipamd_batch_solve serves a batch of >= 2048 tableaux with two queue-fed launches and no host
 * round trip in between: a bulk launch of persistent one-wave workgroups that draw tableaux from
 * a device queue and give one up when it is finished, has used `pivots` pivots (default 96; 128 where a second lean launch follows the first) or
 * `rows` Gomory-cut rows (default 48: the bulk launch's LDS image holds the input rows plus that
 * many, so that 24 tableaux fit a CU), and a tail launch that runs what is left to completion
 * with four waves per tableau. */
int pipamd_engine_set_round_pivots(pipamd_engine *e, int pivots);
int pipamd_engine_set_round_rows(pipamd_engine *e, int rows);
/* Smaller batches skip the bulk launch (few tableaux fill the GPU better with four waves each).
 * A caller that keeps several small batches in flight on separate streams -- together they do fill
 * the GPU -- lowers the threshold (default 2048 tableaux). */
int pipamd_engine_set_bulk_min(pipamd_engine *e, int tableaux);

/* ------------------------------------------------------------------ layer 3 */
/* The solution tape.  traiter() does not return a value: it pushes cells onto the tape of
 * source/sol.c (struct S, sol.c:52-59: flags, param1, param2) through sol_nil / sol_if / sol_list /
 * sol_forme / sol_new / sol_div / sol_val (sol.c:104-209), and the reference's front ends read
 * that tape afterwards: sol_edit (sol.c:291) prints it, sol_quast_edit (sol.c:664) turns it into a
 * PipQuast.  The engine hands the same cells out, in the order the reference would have pushed
 * them, so those readers keep working unchanged (INTEGRATION.md shows the few lines that replay
 * the cells into sol.c; bindings/piplib_traiter_hook.c is that code, compiled and run by the tests). */
#define PIPAMD_SOL_NIL 1  /* sol_nil()                       sol.c:42-50 */
#define PIPAMD_SOL_IF 2   /* sol_if()                                    */
#define PIPAMD_SOL_LIST 3 /* sol_list(param1)                            */
#define PIPAMD_SOL_FORM 4 /* sol_forme(param1)                           */
#define PIPAMD_SOL_NEW 5  /* sol_new(param1)                             */
#define PIPAMD_SOL_DIV 6  /* sol_div()                                   */
#define PIPAMD_SOL_VAL 7  /* sol_val(param1, param2): numerator, denominator, not reduced */
typedef struct pipamd_sol_cell {
  int32_t kind, reserved;
  int64_t param1, param2;
} pipamd_sol_cell;

/* traiter(tp, ctxt, nvar, nparm, ni, nc, bigparm, flags) -- reference source/traiter.c:628, as
 * called from pip_solve (piplib.c:858), maind.c:205 and for the empty-context test
 * (piplib.c:848, maind.c:198).  `tableau` = the ni inequality rows of `tp` (host, row-major,
 * nvar+nparm+1 int64 each, PIP column order unknowns|constant|parameters; Unknown rows with
 * denominator 1, as tab_get / tab_Matrix2Tableau build them), `context` = the nc rows of `ctxt`
 * (nparm+1 each), flags = 0, PIPAMD_T_INT or PIPAMD_T_DUAL (funcall.h:32-33), deepest_cut = the
 * reference's global of that name (piplib.c:53).  The quast decision tree runs on the host, every
 * pivot on the GPU.  On success *cells is a malloc'ed array of *n_cells cells (free with
 * pipamd_free).  Where the reference would have exit()ed ("Integer overflow", ...) the call
 * returns PIPAMD_E_SOLVER and *status holds the PIPAMD_ST_* reason. */
int pipamd_traiter(pipamd_engine *e, int nvar, int nparm, int ni, int nc, int bigparm, int flags, int deepest_cut,
                   const int64_t *tableau, const int64_t *context, pipamd_sol_cell **cells, size_t *n_cells,
                   int *status, int64_t *pivots);

/* The same on 128-bit entries -- the reference's overflow-safe flavour is a whole-library build
 * with a wider Entier (include/piplib/piplib.h:42-88): device tableaux, context, parametric cuts
 * and tape all carry __int128 here; the input rows are int64, the cells' parameters come back as
 * (low, high) int64 pairs.  Tableaux must fit a workgroup's LDS (about 1,600 rows of <= 128
 * columns).  Small problems run their whole decision tree on the device in this flavour too (the 128-bit instantiations
 * of csrc/pip_quast.hip, up to 128 columns: the box at pipamd_engine_set_device_tree), many problems go through pipamd_solve_tableaux128 / pipamd_solve_tableaux_lockstep128. */
typedef struct pipamd_sol_cell128 {
  int32_t kind, reserved;
  int64_t param1_lo, param1_hi, param2_lo, param2_hi;
} pipamd_sol_cell128;
int pipamd_traiter128(pipamd_engine *e, int nvar, int nparm, int ni, int nc, int bigparm, int flags, int deepest_cut,
                      const int64_t *tableau, const int64_t *context, pipamd_sol_cell128 **cells, size_t *n_cells,
                      int *status, int64_t *pivots);
int pipamd_solve_tableau128(pipamd_engine *e, int nvar, int nparm, int ni, int nc, int bigparm, int nq,
                            const int64_t *ineq, const int64_t *ctx, int simplify, int deepest_cut,
                            pipamd_sol_cell128 **cells, size_t *n_cells, int *status, int64_t *pivots);

/* One problem in PIP's native tableau form (what maind.c reads from a .dat file): the whole of
 * maind.c:190-231 -- tab_simplify (tab.c:396) first when nq != 0 and `simplify`, the
 * empty-context test, then traiter.  An empty tape (*n_cells == 0) with PIPAMD_OK is maind.c's
 * "void" (empty context). */
int pipamd_solve_tableau(pipamd_engine *e, int nvar, int nparm, int ni, int nc, int bigparm, int nq,
                         const int64_t *ineq, const int64_t *ctx, int simplify, int deepest_cut,
                         pipamd_sol_cell **cells, size_t *n_cells, int *status, int64_t *pivots);
void pipamd_free(void *p);

/* The same for `n` independent problems: `nthreads` host threads, each with its own decision
 * tree, device arena and HIP stream, share the GPU (their launches overlap).  cells[i] /
 * n_cells[i] / rcs[i] / statuses[i] / pivots[i] are what pipamd_solve_tableau returns for
 * problem i (statuses and pivots may be NULL). */
typedef struct pipamd_problem {
  int32_t nvar, nparm, ni, nc, bigparm, nq;
  const int64_t *ineq; /* ni x (nvar+nparm+1) */
  const int64_t *ctx;  /* nc x (nparm+1) */
} pipamd_problem;
int pipamd_solve_tableaux(pipamd_engine *e, int n, const pipamd_problem *problems, int simplify,
                          int deepest_cut, int nthreads, pipamd_sol_cell **cells, size_t *n_cells, int *rcs,
                          int *statuses, int64_t *pivots);

/* The same on 128-bit entries (small problems on the device first, then one TreeT<__int128> per host thread; cells as
 * pipamd_traiter128 hands them out); the lock-step scheduler has a 128-bit entry too (pipamd_solve_tableaux_lockstep128). */
int pipamd_solve_tableaux128(pipamd_engine *e, int n, const pipamd_problem *problems, int simplify,
                             int deepest_cut, int nthreads, pipamd_sol_cell128 **cells, size_t *n_cells, int *rcs,
                             int *statuses, int64_t *pivots);

/* traiter() for `n` independent calls at once: for every i what pipamd_traiter(e, problems[i]'s shape and rows, flags[i],
 * deepest_cut, ...) returns -- the same cells in the same order, the same rc, status and pivot count.  No empty-context
 * test and no tab_simplify (this is traiter(), not maind.c): problems[i].nq is ignored, flags[i] says integer or rational.
 * flags[i] is 0, PIPAMD_T_INT or PIPAMD_T_DUAL; flags == NULL stands for all 0; any other value gives that problem
 * PIPAMD_E_INVALID in rcs[i] and does not fail the call.  statuses and pivots may be NULL.  The problems in the device
 * tree's box (below) run in one launch of the device-resident traiter(), each with its own flags; the others, and those
 * it hands back, go to `nthreads` host threads with a decision tree each, as in pipamd_solve_tableaux.  The lock-step
 * scheduler is not used (it starts at the context test and has no dual).  pipamd_last_device_tree answers for the call.
 * A front end with many pip_solve calls gathers their traiter() calls into one of these. */
int pipamd_traiter_many(pipamd_engine *e, int n, const pipamd_problem *problems, const int *flags, int deepest_cut,
                        int nthreads, pipamd_sol_cell **cells, size_t *n_cells, int *rcs, int *statuses,
                        int64_t *pivots);
/* The same on 128-bit entries: cells as pipamd_traiter128 hands them out. */
int pipamd_traiter_many128(pipamd_engine *e, int n, const pipamd_problem *problems, const int *flags, int deepest_cut,
                           int nthreads, pipamd_sol_cell128 **cells, size_t *n_cells, int *rcs, int *statuses,
                           int64_t *pivots);

/* pip_solve(inequnk, ineqpar, Bg, options) (piplib.c:722-880) for `n` independent calls at once, straight from the PolyLib
 * matrices (added since interface version 500).  A front end that has the matrices need not build a tableau: the engine
 * does the integer bookkeeping of piplib.c:758-797 on the host, uploads the matrices in one copy, and a kernel
 * (csrc/pip_m2t.hip) writes, for every problem, what tab_Matrix2Tableau (tab.c:292-393) returns at piplib.c:813 (the
 * context) and piplib.c:846 (the domain): the constant moved behind the first series of columns, the unknowns negated
 * under Maximize, the sum of the unknowns' coefficients in the big column (a fresh column when Bg is -1, added to the
 * given one otherwise; sums wrap in 64 bits as in the reference's long long build), the negated copies of the parameters
 * for Urs_parms with the `pos <= Bg` skip of tab.c:358-365, a zero column in the context where a new big parameter goes,
 * and the negated twin behind every equality (marker 0; Nl and Nm count those twice, piplib.c:767-770, 808-811).  The
 * device-resident traiter() then solves the problems of its box from that device buffer; the others, and those it hands
 * back, have their built rows copied back and go to `nthreads` host trees.  Either side does what pip_solve does:
 * tab_simplify on both tableaux when Nq, the context test as a TRAITER_INT call of its own (piplib.c:818-826), then
 * traiter() with the problem's flags. */
#define PIPAMD_PIP_NQ 1           /* options->Nq: integer solution (tab_simplify, TRAITER_INT: piplib.c:815, 848-853) */
#define PIPAMD_PIP_MAXIMIZE 2     /* options->Maximize: Shift = 1, SOL_MAX (piplib.c:777-779) */
#define PIPAMD_PIP_URS_PARMS 4    /* options->Urs_parms: Np - (Bg >= 0) negated parameter copies (piplib.c:785-788) */
#define PIPAMD_PIP_URS_UNKNOWNS 8 /* options->Urs_unknowns: Shift = -1, SOL_SHIFT; ignored under MAXIMIZE (piplib.c:777-783) */
#define PIPAMD_PIP_DUAL 16        /* options->Compute_dual: TRAITER_DUAL, SOL_DUAL; ignored under NQ (piplib.c:852-857) */
typedef struct pipamd_pip_problem {
  int32_t nrows, ncols;       /* inequnk: NbRows, NbColumns = 1 + Nn + Np + 1 (marker | unknowns | parameters | constant) */
  int32_t ctx_rows, ctx_cols; /* ineqpar: NbRows, NbColumns = Np + 2; ctx_cols == 0: ineqpar is NULL, Np = 0 (piplib.c:758) */
  int32_t bg;                 /* Bg as pip_solve takes it: a tableau column Nn+1 .. Nn+Np, or -1 (then Maximize and
                                 Urs_unknowns make one at NbColumns - 1 and count it as a parameter, piplib.c:791-797) */
  int32_t options;            /* PIPAMD_PIP_* */
  const int64_t *inequnk;     /* host, row-major, marker column first; NULL: the answer is void (piplib.c:753-754) */
  const int64_t *ineqpar;     /* host, row-major; may be NULL when ctx_rows == 0 */
} pipamd_pip_problem;         /* 40 bytes, offsets 0 4 8 12 16 20 24 32 */
/* what traiter() was called with (piplib.c:858), and what sol_quast_edit (piplib.c:866) takes */
typedef struct pipamd_pip_info {
  int32_t nvar, nparm, ni, nc, bigparm, flags;   /* Nn, Np, Nl, Nm, Bg as traiter() gets them; flags: 0, PIPAMD_T_INT or
                                                    PIPAMD_T_DUAL (TRAITER_*, funcall.h:32-33) */
  int32_t sol_bg, urs_parms, sol_flags, is_void; /* Bg - Nn - 1, Urs_parms, the SOL_* bits as sol.h:36-50 numbers them
                                                    (SOL_SHIFT 1, SOL_NEGATE 2, SOL_REMOVE 4, SOL_DUAL 8); is_void: pip_solve
                                                    returns NULL (inequnk NULL, or the context is empty) */
  int64_t row_off;                               /* pipamd_pip_tableaux: where this problem's rows start in *rows */
} pipamd_pip_info;                               /* 48 bytes, offsets 0 .. 36 in steps of 4, 40 */
/* The many-problem form of tab_Matrix2Tableau: validation, upload and the build kernel only.  *rows is a malloc'ed array
 * of *n_words int64 (free with pipamd_free; NULL when there are none): problem i has its ni x (nvar + nparm + 1) domain
 * rows at info[i].row_off, then its nc x (nparm + 1) context rows -- the kernel's output bit for bit, not simplified.  A
 * problem that is void or malformed (info[i].nvar < 0) has no rows.  Returns PIPAMD_E_INVALID for a null array or n < 0
 * and when any problem is malformed (the others are still built). */
int pipamd_pip_tableaux(pipamd_engine *e, int n, const pipamd_pip_problem *p, pipamd_pip_info *info, int64_t **rows,
                        size_t *n_words);
/* cells[i] / n_cells[i]: the tape pip_solve has when traiter() returns at piplib.c:858 -- the cells the one-call hook
 * (bindings/piplib_traiter_hook.c) would replay, so a caller replays them into sol.c and calls sol_simplify /
 * sol_quast_edit(&xq, NULL, info[i].sol_bg, info[i].urs_parms, info[i].sol_flags) unchanged.  A void
 * answer is PIPAMD_OK with no cells and info[i].is_void = 1.  pivots[i] counts the context test's pivots too; statuses
 * and pivots may be NULL; deepest_cut and nthreads as in pipamd_traiter_many; pipamd_last_device_tree answers for the
 * call.  A malformed problem gets PIPAMD_E_INVALID in its own rcs[i] (before any HIP call) and does not fail the call:
 * unknown option bits, a negative count, ncols < 2, ctx_cols of 1, ctx_cols == 0 with ctx_rows > 0, Nn < 0, bg outside
 * -1 / Nn+1 .. Nn+Np, ineqpar NULL with ctx_rows > 0, a built tableau of more than 512 columns (MAXCOL).  The call
 * itself fails only for a null array or n < 0; n == 0 is PIPAMD_OK. */
int pipamd_pip_solve_many(pipamd_engine *e, int n, const pipamd_pip_problem *p, int deepest_cut, int nthreads,
                          pipamd_pip_info *info, pipamd_sol_cell **cells, size_t *n_cells, int *rcs, int *statuses,
                          int64_t *pivots);
/* The overflow-safe flavour on the same int64 tableaux (the kernel's 128-bit instantiation, TreeT<__int128>; cells as
 * pipamd_traiter128 hands them out).  A problem whose big column -- the sum, or its negation under an equality -- leaves
 * 64 bits gets rcs[i] = PIPAMD_E_SOLVER and statuses[i] = PIPAMD_ST_RANGE instead of a wrapped column (the build kernel
 * raises a flag per problem). */
int pipamd_pip_solve_many128(pipamd_engine *e, int n, const pipamd_pip_problem *p, int deepest_cut, int nthreads,
                             pipamd_pip_info *info, pipamd_sol_cell128 **cells, size_t *n_cells, int *rcs, int *statuses,
                             int64_t *pivots);

/* The same results from a lock-step scheduler: one explicit traiter() state machine per problem
 * and, per step, ONE clone / patch / pivot-kernel / gather sequence for the whole batch, so the
 * host <-> device latency is paid once per step instead of once per problem.  Problems that need
 * a rare path (tableau growth beyond the reserved block, deepest cuts) are finished by the
 * per-problem tree of pipamd_solve_tableau. */
int pipamd_solve_tableaux_lockstep(pipamd_engine *e, int n, const pipamd_problem *problems, int simplify,
                                   int deepest_cut, pipamd_sol_cell **cells, size_t *n_cells, int *rcs,
                                   int *statuses, int64_t *pivots);
/* The lock-step scheduler of the overflow-safe flavour (piplib.h:42-88, funcall.h:37-41: the flavour is a type choice):
 * device tableaux, contexts, parametric cuts and tape cells are 128-bit, one launch sequence per step serves the whole
 * batch; the 128-bit instantiation of the device-resident traiter() runs in front of it (the problems in its box, see
 * pipamd_device_tree_fits) and pipamd_last_device_tree reports what it served and handed back, as for the 64-bit entry;
 * rare paths go to a TreeT<__int128>. */
int pipamd_solve_tableaux_lockstep128(pipamd_engine *e, int n, const pipamd_problem *problems, int simplify,
                                      int deepest_cut, pipamd_sol_cell128 **cells, size_t *n_cells, int *rcs,
                                      int *statuses, int64_t *pivots);
/* Small problems are first given to the device-resident traiter() (csrc/pip_quast.hip), in both entry widths: at most 128
 * columns (a lane per column up to 64, two columns per lane beyond; the spare columns for new parameters -- up to 10 -- stay
 * within that width, so a problem of 127 or 128 columns that needs a new parameter is handed back), at most 104
 * inequalities (128 real rows with the cuts), a context of at most 64 columns with its spare ones, and an LDS image that fits
 * the limit of its width (up to 64 columns: 96 KB in 64 bits, 150 KB in 128 bits; beyond: 160 KB, a workgroup's LDS --
 * so the widest, tallest 128-bit shapes go to the host schedulers).  pipamd_device_tree_fits answers for one shape.  One wave per
 * problem runs the whole call tree -- pivots, compa_test sub-problems (traiter.c:162-243), forks of the
 * quast (traiter.c:695-759), cuts with new parameters (integrer.c:156-291) -- and writes the tape, with
 * no host round trip.  A problem in which a 64-bit operation would overflow, or that outgrows its
 * reserved rows, is handed back and served by the lock-step scheduler / the per-problem tree, which
 * reproduce the reference's wrap-around and "Integer overflow" behaviour.  pipamd_traiter,
 * pipamd_solve_tableau, pipamd_solve_tableaux and pipamd_traiter_many try it first too (since interface version 300 also
 * with PIPAMD_T_DUAL: the list of dual values behind every rational solution, for every shape of the box -- tab_sort_rows'
 * `pos` table has an entry for each of up to 128 inequalities of a call), and so do their 128-bit counterparts with the kernel's 128-bit instantiation (there every product and
 * sum is checked against 128 bits).  On by default (the environment
 * variable PIPAMD_NO_DEVICE_TREE switches it off for a process);
 * pipamd_last_device_tree reports how many problems of the last lock-step call each side served. */
int pipamd_engine_set_device_tree(pipamd_engine *e, int on);
int pipamd_last_device_tree(const pipamd_engine *e, int *served, int *handed_back);
/* 1 if the device-resident traiter() takes a problem of this shape in the flavour of `entier_bits` (64 or 128) -- it may
 * still hand it back at run time (overflow, rows, tape, stack) --, 0 if the shape goes straight to the host schedulers,
 * PIPAMD_E_INVALID for bad arguments.  Host only: needs neither an engine nor a GPU.  The same decision the solve entries
 * make (interface version 500). */
int pipamd_device_tree_fits(const pipamd_problem *p, int entier_bits);

/* ------------------------------------------------------------------ tapes at parameter points */
/* A parametric problem is solved ONCE; its tape -- the cells pipamd_traiter, pipamd_solve_tableau*, pipamd_traiter_many
 * or pipamd_pip_solve_many handed out -- is then EVALUATED at as many parameter points as the caller likes, a lane per
 * point (csrc/pip_tape.hip), instead of solving an instance per point (pipamd_batch_load_instances).  Added since
 * interface version 500.  The grammar, with P the parameters in scope, nparm at the root:
 *     item := NEW(n) DIV FORM(P+1) VAL x (P+1) VAL(D)   item
 *           | IF FORM(P+1) VAL x (P+1)   item   item
 *           | LIST(nvar) { FORM(P+1) VAL x (P+1) } x nvar  [ LIST(ndual) { FORM(1) VAL } x ndual ]
 *           | NIL
 * New parameter (integrer.c:171-180): n == P, every denominator 1, D > 0; its value is floor((sum c_j theta_j + c) / D),
 * a true floor, in scope for the one item behind it (the second item of an enclosing IF starts from the IF's own P
 * again).  Condition (traiter.c:719-737): one positive denominator; the first item is taken when
 * sum n_j theta_j + n_c >= 0 (0 included), the second otherwise.  Leaf (traiter.c:262-268, 282-290): per unknown the
 * parameters' coefficients, then the constant, over one positive denominator D_i; unknown i is N / D_i with
 * N = sum n_j theta_j + n_c, handed out in lowest terms -- g = gcd(|N|, D_i): (N / g, D_i / g), (0, 1) for N == 0.  With
 * ndual > 0 a second list of ndual constants follows (PIPAMD_T_DUAL), handed out in lowest terms too.  An empty tape is
 * the front ends' "void".
 * Arithmetic.  int64 cells: every sum n_j theta_j + n_c is formed exactly, whatever single products or partial sums do;
 * a point at which a new parameter's value or a numerator in lowest terms does not fit int64 ends PIPAMD_ST_RANGE.
 * 128-bit cells: points are int64, new parameters and results __int128; the products and the running sums of a form
 * are checked against 128 bits in cell order -- coefficients 0 .. P-1, then the constant -- and the first that leaves
 * them ends the point PIPAMD_ST_RANGE.  Such a point does not disturb the others of the call.
 * NOT done here, the caller's business: pipamd_tape_eval knows no context -- points outside the context the problem was
 * solved under, or negative ones, are evaluated like any other, as pipamd_batch_load_instances solves them
 * (pipamd_tape_sweep below tests the points of a box against the context's rows and marks them); and a big
 * parameter the CALLER gave is just another column of the points.  The edits pip_solve makes to its result
 * (sol_quast_edit, piplib.c:866) are applied by pipamd_tape_compile_pip below, with one limit: dual lists are handed out
 * one pair per tableau row as they stand (sol_quast_edit edits them with flags 0, sol.c:706-708); the merge of an
 * equality's two values (pip_quast_equalities_dual) needs the input's markers and is not done.
 * Limits.  PIPAMD_TAPE_MAX_SLOTS: the largest P + 1 of a tape, the root's nparm + 1 included (the kernel keeps a
 * workgroup's parameters in scope in LDS: 128 points x (slots - 1) values).  The compiled program must stay below 2^31
 * words.  The program is staged in LDS when 8 * info.words + 128 * (info.slots - 1) * (8 or 16 bytes per value) is at
 * most PIPAMD_TAPE_LDS_BYTES, and read from global memory otherwise (info.staged says which). */
#define PIPAMD_TAPE_MAX_SLOTS 32
#define PIPAMD_TAPE_LDS_BYTES 65536
typedef struct pipamd_tape_shape {
  int32_t nvar;     /* forms of a solution list */
  int32_t nparm;    /* parameters of the problem = values of a point */
  int32_t ndual;    /* forms of the dual list behind every solution list (the tableau's inequalities); 0: none */
  int32_t reserved; /* 0 */
} pipamd_tape_shape;
typedef struct pipamd_tape_info {
  int64_t leaves; /* LIST (solution lists) and NIL items; pipamd_tape_eval's d_leaf counts them in tape order from 0 */
  int64_t ifs;    /* IF cells */
  int64_t news;   /* NEW cells */
  int64_t words;  /* 8-byte words of the compiled program (csrc/pip_tape.h) */
  int32_t slots;  /* the largest P + 1 of any item, at least nparm + 1 */
  int32_t depth;  /* items nested: 1 for the root, one more for the items of an IF and the item behind a NEW; 0: empty */
  int32_t staged; /* 1: the kernel copies the program to LDS; 0: it reads it from global memory (or there is none) */
  int32_t reserved;
} pipamd_tape_info; /* 48 bytes, offsets 0 8 16 24 32 36 40 44 */
/* Validates a tape against the grammar and fills *info (which may be NULL).  Host only: needs neither an engine nor a
 * GPU.  PIPAMD_E_INVALID: a null shape, or null cells with n_cells > 0; a negative count or reserved != 0 in the shape; a
 * cell of unknown kind, or of another kind than the grammar has in its place; a truncated tape; cells behind the end of
 * the root item; a FORM whose length is not P + 1 (1 in a dual list); a LIST whose length is not nvar (ndual for the
 * second); no second LIST with ndual > 0 (one with ndual == 0 is read as the next item); NEW(n) with n != P; a
 * denominator <= 0; unequal denominators within a form; a DIV form or divisor with a denominator other than 1;
 * D <= 0.  PIPAMD_E_TOOLARGE: more than PIPAMD_TAPE_MAX_SLOTS slots, or a program of 2^31 words or more.  The empty
 * tape (n_cells == 0) is valid. */
int pipamd_tape_check(const pipamd_sol_cell *cells, size_t n_cells, const pipamd_tape_shape *shape, pipamd_tape_info *info);
int pipamd_tape_check128(const pipamd_sol_cell128 *cells, size_t n_cells, const pipamd_tape_shape *shape,
                         pipamd_tape_info *info);
/* The same check, then the tape as a flat program in the memory of the engine's device: nodes in tape order, their
 * coefficients beside them, every jump strictly forward and inside the program -- the kernel cannot loop or read outside
 * it, whatever the points are.  The cells are not needed afterwards.  PIPAMD_E_INVALID before any HIP call: a null
 * engine or `out`, and whatever pipamd_tape_check refuses.  Free with pipamd_tape_free (NULL is allowed); a tape must
 * not outlive evaluations still running on a stream. */
typedef struct pipamd_tape pipamd_tape;
int pipamd_tape_compile(pipamd_engine *e, const pipamd_sol_cell *cells, size_t n_cells, const pipamd_tape_shape *shape,
                        pipamd_tape **out);
int pipamd_tape_compile128(pipamd_engine *e, const pipamd_sol_cell128 *cells, size_t n_cells, const pipamd_tape_shape *shape,
                           pipamd_tape **out);
void pipamd_tape_free(pipamd_tape *t);
/* The tape at n_points points: d_points is n_points x nparm int64 (may be NULL when nparm == 0; a tape compiled with
 * an edit: pipamd_tape_point_cols columns in place of nparm).  Each of the six
 * outputs may be NULL.  d_status[k]: PIPAMD_ST_SOLUTION, PIPAMD_ST_NIL (a NIL item; every point of an empty tape) or
 * PIPAMD_ST_RANGE.  d_leaf[k]: the ordinal, in tape order, of the LIST or NIL item reached; -1 for an empty tape and a
 * RANGE point.  d_x_num / d_x_den: n_points x nvar, d_dual_num / d_dual_den: n_points x ndual -- int64 values, or
 * little-endian (low, high) int64 pairs for a tape of 128-bit cells; a point that is not PIPAMD_ST_SOLUTION gets (0, 0)
 * throughout.  One launch on `stream`, no synchronisation, like pipamd_batch_results; n_points == 0 is PIPAMD_OK without
 * a launch.  The tape is not changed: it may be evaluated any number of times, on any stream of its device, also
 * concurrently.  PIPAMD_E_INVALID before any HIP call: a null engine or tape, a tape of another device than the
 * engine's, n_points < 0, null d_points with nparm > 0 and n_points > 0.  PIPAMD_E_TOOLARGE: n_points of 2^38 and more. */
int pipamd_tape_eval(pipamd_engine *e, const pipamd_tape *t, int64_t n_points, const int64_t *d_points, int32_t *d_status,
                     int32_t *d_leaf, int64_t *d_x_num, int64_t *d_x_den, int64_t *d_dual_num, int64_t *d_dual_den,
                     void *stream);


/* pip_solve's result edits (added since interface version 500).  pipamd_pip_solve_many hands out the tape traiter() wrote
 * and, in pipamd_pip_info, what pip_solve then passes to sol_quast_edit (piplib.c:866): sol_bg, urs_parms, sol_flags.
 * pipamd_tape_compile_pip applies sol_vector_edit (sol.c:435-512) to every form, so the compiled tape evaluates to what
 * pip_solve's own answer gives at a point.  edit == NULL, or an edit of all zeros, is exactly pipamd_tape_check /
 * pipamd_tape_compile; the result is an ordinary pipamd_tape for pipamd_tape_eval.  shape.nparm stays the parameter
 * count of the tape as solved (info.nparm), and the grammar is checked on the cells as they are (NEW(n) with n the raw
 * count in scope, forms of the raw P + 1).  With P the raw parameters in scope, bg = sol_bg, U = urs_parms and
 * first_urs = U + (bg >= 0):
 *  - column j < nparm of a form is DROPPED when j == bg with SOL_REMOVE, or when first_urs <= j < first_urs + U (the
 *    negated copies of Urs_parms), whatever it holds; the kept columns are the slots, renumbered in order.  A point is
 *    pipamd_tape_point_cols = nparm - (REMOVE ? 1 : 0) - U values: the parameters as pip_solve's caller numbers them.
 *    NEW writes the slot behind the kept parameters in scope; info.slots and PIPAMD_TAPE_MAX_SLOTS count kept columns.
 *  - conditions and new-parameter forms: the dropping alone (sol.c:694, 714).
 *  - solution-list forms, unknown i over D_i: with SOL_SHIFT the coefficient at bg becomes n_bg - D_i before any drop;
 *    where that is not 0 the unknown is UNBOUNDED: its denominator is handed out as 0, the numerator kept -- the
 *    convention of pipamd_batch_results_shifted.  A shifted coefficient that does not fit the cell type:
 *    PIPAMD_E_TOOLARGE.  With SOL_NEGATE the unknown's exact value N is negated at the point, before the range check and
 *    the reduction (a value whose negation leaves the type: PIPAMD_ST_RANGE).  Handed out: (+-N / g, D_i / g or 0) with
 *    g = gcd(|N|, D_i); (0, 1) or (0, 0) for N == 0.
 *  - dual lists: as they stand (see "NOT done" above).
 * Any negative sol_bg means "no big parameter", as sol_vector_edit reads it (pipamd_pip_info has Bg - Nn - 1 there, which
 * is below -1 for Bg == -1).
 * PIPAMD_E_INVALID before any HIP call: reserved != 0; sol_flags outside bits 0-3; urs_parms < 0; sol_bg >= nparm;
 * SOL_SHIFT or SOL_REMOVE without sol_bg >= 0; first_urs + U > nparm; SOL_REMOVE of a column among the Urs
 * copies; and everything pipamd_tape_check refuses. */
#define PIPAMD_SOL_SHIFT 1  /* sol.h:36-50, the numbering pipamd_pip_info.sol_flags uses */
#define PIPAMD_SOL_NEGATE 2
#define PIPAMD_SOL_REMOVE 4
#define PIPAMD_SOL_DUAL 8   /* accepted and ignored: shape.ndual says whether dual lists follow */
typedef struct pipamd_tape_edit {
  int32_t sol_bg, urs_parms, sol_flags, reserved; /* the three fields of pipamd_pip_info; reserved 0 */
} pipamd_tape_edit;
int pipamd_tape_check_pip(const pipamd_sol_cell *cells, size_t n_cells, const pipamd_tape_shape *shape,
                          const pipamd_tape_edit *edit, pipamd_tape_info *info);
int pipamd_tape_check_pip128(const pipamd_sol_cell128 *cells, size_t n_cells, const pipamd_tape_shape *shape,
                             const pipamd_tape_edit *edit, pipamd_tape_info *info);
int pipamd_tape_compile_pip(pipamd_engine *e, const pipamd_sol_cell *cells, size_t n_cells, const pipamd_tape_shape *shape,
                            const pipamd_tape_edit *edit, pipamd_tape **out);
int pipamd_tape_compile_pip128(pipamd_engine *e, const pipamd_sol_cell128 *cells, size_t n_cells,
                               const pipamd_tape_shape *shape, const pipamd_tape_edit *edit, pipamd_tape **out);
/* int64 values per point that pipamd_tape_eval reads from d_points (PIPAMD_E_INVALID for NULL) */
int pipamd_tape_point_cols(const pipamd_tape *t);

/* A set of tapes evaluated in one launch (added since interface version 500): the many small quasts of
 * pipamd_pip_solve_many, each at a handful of points.  pipamd_tape_set_create takes n >= 1 compiled tapes (edited or
 * not) of the engine's device and of one cell width -- PIPAMD_E_INVALID otherwise, before any HIP call, as for a null
 * engine, array, entry or `out`; programs of 2^31 words or more together: PIPAMD_E_TOOLARGE -- and copies their programs
 * into one device buffer beside a device table per tape.  The tapes may be freed afterwards.  The set is immutable:
 * pipamd_tape_set_eval is one launch without synchronisation and needs no per-call host table, so it may be called
 * concurrently on several streams.  *info (may be NULL) gets the strides below. */
typedef struct pipamd_tape_set pipamd_tape_set;
typedef struct pipamd_tape_set_info {
  int64_t words;                                   /* all programs together, < 2^31 */
  int32_t n, bits, point_cols, nvar, ndual, slots; /* tapes, 64 or 128, and the four maxima over the tapes */
} pipamd_tape_set_info;                            /* 32 bytes */
int pipamd_tape_set_create(pipamd_engine *e, int n, const pipamd_tape *const *tapes, pipamd_tape_set **out,
                           pipamd_tape_set_info *info);
void pipamd_tape_set_free(pipamd_tape_set *s);
/* Point k belongs to tape d_tape[k]; points need not be sorted by tape.  The arrays are padded to the set's maxima:
 * d_points is n_points x info.point_cols (a tape reads its first pipamd_tape_point_cols columns), d_x_* is
 * n_points x info.nvar, d_dual_* is n_points x info.ndual; entries beyond the tape's own counts get (0, 0).  Statuses,
 * leaf ordinals (per tape) and values are what pipamd_tape_eval gives for that tape.  d_tape[k] outside 0 .. n-1:
 * PIPAMD_ST_BADINPUT, leaf -1 and (0, 0) throughout; nothing is read through it and the other points are not disturbed.
 * PIPAMD_E_INVALID before any HIP call: as pipamd_tape_eval (d_points may be NULL when info.point_cols == 0), and a
 * null d_tape with n_points > 0.  PIPAMD_E_TOOLARGE: n_points of 2^38 and more. */
int pipamd_tape_set_eval(pipamd_engine *e, const pipamd_tape_set *s, int64_t n_points, const int32_t *d_tape,
                         const int64_t *d_points, int32_t *d_status, int32_t *d_leaf, int64_t *d_x_num, int64_t *d_x_den,
                         int64_t *d_dual_num, int64_t *d_dual_den, void *stream);

/* A tape swept over a box of integer points, under a context, with a summary reduced on the device (added since
 * interface version 500).  The kernel makes the points itself -- nothing is uploaded for the box --, tests each against
 * the context's rows exactly, walks the tape as pipamd_tape_eval does, and reduces integer figures on chip; the six
 * per-point arrays are optional, so a box far larger than memory for its answers can still be counted.
 *
 * pipamd_tape_sweep_plan is host only: it needs neither an engine nor a GPU; `info` comes from pipamd_tape_check*,
 * `bits` (64 or 128) is the tape's cell width, `point_cols` what pipamd_tape_point_cols gives (nparm without an edit).
 * PIPAMD_E_INVALID: null info or plan; bits not 64 or 128; point_cols outside 0 .. PIPAMD_TAPE_MAX_SLOTS - 1; null lo or
 * hi with point_cols > 0; any lo[c] > hi[c].  PIPAMD_E_TOOLARGE: n_points >= 2^38, pipamd_tape_eval's limit; the product
 * is formed without wrapping (lo = INT64_MIN, hi = INT64_MAX in one column is a legal question, answered TOOLARGE).
 * plan.binned: 1 exactly when 16 * (info.leaves + 4) bytes fit within PIPAMD_TAPE_LDS_BYTES beside the slots
 * (128 * (info.slots - 1) values of bits / 8 bytes) and beside the program (8 * info.words) where info.staged. */
struct pipamd_tape_sweep_plan { /* (a struct tag only: the function below has the name, so no typedef can) */
  int64_t n_points;      /* prod (hi[c] - lo[c] + 1); 1 when point_cols == 0 */
  int64_t summary_words; /* 8 + 2 * info->leaves */
  int32_t binned;        /* 1: per-leaf figures are gathered in LDS per workgroup; 0: wave-aggregated global atomics */
  int32_t reserved;
}; /* 24 bytes */
int pipamd_tape_sweep_plan(const pipamd_tape_info *info, int bits, int point_cols, const int64_t *lo, const int64_t *hi,
                           struct pipamd_tape_sweep_plan *plan);
/* The summary: plan.summary_words int64 on the device, L = info.leaves.  Counts of the points that ended SOLUTION, NIL,
 * RANGE, OUTSIDE; the smallest k with that status (-1: none); per leaf ordinal (LIST and NIL items, as d_leaf counts
 * them) the points that reached it, and the smallest such k (-1: none).  All figures are order-independent integers:
 * the summary is deterministic.  A caller can rely on: words 0..3 sum to n_points; the leaf counts sum to SOLUTION + NIL
 * (for an empty tape every inside point is NIL with leaf -1, and the leaf counts sum to 0). */
#define PIPAMD_SWEEP_COUNT 0            /* + PIPAMD_SWEEP_SOLUTION .. PIPAMD_SWEEP_OUTSIDE */
#define PIPAMD_SWEEP_FIRST 4            /* + the same */
#define PIPAMD_SWEEP_SOLUTION 0
#define PIPAMD_SWEEP_NIL 1
#define PIPAMD_SWEEP_RANGE 2
#define PIPAMD_SWEEP_OUTSIDE 3
#define PIPAMD_SWEEP_LEAF_COUNT(L) 8    /* + leaf ordinal */
#define PIPAMD_SWEEP_LEAF_FIRST(L) (8 + (L)) /* + leaf ordinal */
#define PIPAMD_SWEEP_WORDS(L) (8 + 2 * (L))
/* Box: lo and hi are HOST arrays of pipamd_tape_point_cols(t) values, bounds inclusive.  Point k of 0 .. n_points-1 is
 * the box in row-major order, the last column fastest: column c holds lo[c] + digit_c(k) -- the order and the values of
 * numpy.indices / itertools.product.
 * Context: d_ctx is a DEVICE array of n_ctx x ctx_cols int64 laid out as PolyLib lays out ineqpar: marker, point_cols
 * coefficients, constant; ctx_cols must be point_cols + 2 when n_ctx > 0.  Marker 0: the row is an equality; any other
 * marker: >= 0 (the reference's piplib_int_zero(p[i][0]), piplib.c:671).  Coefficients are int64 for tapes of either
 * cell width, and a row's value sum a_j theta_j + b is decided exactly whatever single products or partial sums do.  A
 * point that fails any row ends PIPAMD_ST_OUTSIDE, leaf -1, (0, 0) throughout; the tape is not walked for it.
 * n_ctx == 0: every point is inside.  The columns are the point columns: pip_solve's ineqpar can be passed as it stands
 * when the tape was compiled with pip_solve's edit (pipamd_tape_compile_pip) or when that edit drops no column (no big
 * parameter removed, no Urs_parms); for a tape compiled without an edit the rows must be given over the tape's own
 * nparm columns.
 * Outputs: the six arrays of pipamd_tape_eval, indexed by k; each may be NULL, and all may be.  For every point that is
 * not OUTSIDE they hold what pipamd_tape_eval writes for that point, bit for bit.  d_summary (may be NULL) is
 * initialised by the call on `stream` before the kernel: callers need not, and two calls do not accumulate.
 * A fill of the summary and one kernel on `stream`, no synchronisation; the call may run concurrently on several
 * streams with different output buffers.  PIPAMD_E_INVALID before any HIP call: whatever the planner refuses; a null
 * engine or tape; a tape of another device; n_ctx < 0; n_ctx > 0 with a null d_ctx or ctx_cols != point_cols + 2.
 * PIPAMD_E_TOOLARGE as the planner. */
int pipamd_tape_sweep(pipamd_engine *e, const pipamd_tape *t, const int64_t *lo, const int64_t *hi, int n_ctx, int ctx_cols,
                      const int64_t *d_ctx, int64_t *d_summary, int32_t *d_status, int32_t *d_leaf, int64_t *d_x_num,
                      int64_t *d_x_den, int64_t *d_dual_num, int64_t *d_dual_den, void *stream);

/* Two tapes compared point by point on the device (added since interface version 500): do two answers to the same
 * problem agree, and if not, where?  The tapes may be of different shape (other forks, other new parameters) and of
 * different cell widths; they are compared by value at points, never by cells or leaf ordinals.  Per point, sa and sb
 * are the statuses pipamd_tape_eval gives tape a and tape b there, each evaluated in its own width with its own edit
 * marks and PIPAMD_ST_RANGE rules, and the class is, in this order: RANGE if either status is PIPAMD_ST_RANGE; STATUS if
 * sa != sb; VALUE if any unknown's handed-out (numerator, denominator) pair differs; SAME otherwise.  Pairs are compared
 * as integers, int64 widened to 128 bits: both tapes hand out lowest terms over a positive denominator, or over 0 for
 * an unbounded unknown, so equal pairs are equal values, and (0, 1) differs from (0, 0).  Every unknown of both leaves is
 * evaluated whatever was found before: a later unknown that leaves the range makes the point RANGE.  With
 * PIPAMD_CMP_DUAL the ndual dual pairs are compared behind the unknowns. */
#define PIPAMD_CMP_SAME 0    /* both NIL, or both SOLUTION with every handed-out pair equal */
#define PIPAMD_CMP_STATUS 1  /* one SOLUTION, the other NIL */
#define PIPAMD_CMP_VALUE 2   /* both SOLUTION, some pair differs */
#define PIPAMD_CMP_RANGE 3   /* either tape ends PIPAMD_ST_RANGE at the point: undecided */
#define PIPAMD_CMP_OUTSIDE 4 /* pipamd_tape_compare_sweep alone: the point fails a row of the context */
#define PIPAMD_CMP_WORDS 10  /* the summary: 5 counts by class, then 5 firsts (the smallest k of the class, -1: none) */
#define PIPAMD_CMP_DUAL 1    /* flags: compare the dual lists too */
/* pipamd_tape_compare_plan is host only (neither an engine nor a GPU): the infos come from pipamd_tape_check*, bits_a and
 * bits_b are the cell widths, point_cols, lo and hi as for pipamd_tape_sweep_plan.  PIPAMD_E_INVALID: a null info or
 * plan, a width other than 64 and 128, whatever pipamd_tape_sweep_plan refuses of a box.  PIPAMD_E_TOOLARGE: 2^38 points
 * or more; a pair whose slot areas together -- 128 * (slots - 1) values of bits / 8 bytes for either tape -- exceed
 * PIPAMD_TAPE_LDS_BYTES: a lane keeps the parameters in scope of BOTH tapes on chip, so e.g. two 128-bit tapes of 32
 * slots each (2 x 63,488 bytes) cannot be compared, while each can be evaluated alone.  plan.staged: 1 exactly when both
 * programs (8 * words each) fit beside the slot areas too; otherwise both are read from global memory. */
struct pipamd_tape_compare_plan {
  int64_t n_points; /* prod (hi[c] - lo[c] + 1); 1 when point_cols == 0 */
  int32_t staged;
  int32_t reserved;
}; /* 16 bytes */
int pipamd_tape_compare_plan(const pipamd_tape_info *a, int bits_a, const pipamd_tape_info *b, int bits_b, int point_cols,
                             const int64_t *lo, const int64_t *hi, struct pipamd_tape_compare_plan *plan);
/* The list form: n_points points in d_points as pipamd_tape_eval takes them (no context: never OUTSIDE).  The sweep
 * form: box, row-major order of k and context rows exactly as pipamd_tape_sweep has them; an OUTSIDE point is walked by
 * neither tape.  An empty tape is NIL at every (inside) point.  Outputs, each may be NULL and all may be:
 *   d_class[k]     int32, PIPAMD_CMP_*
 *   d_where[k]     int32: the smallest unknown index whose pair differs; nvar + i for the first differing dual pair i
 *                  when all unknowns agree (PIPAMD_CMP_DUAL); -1 whenever the class is not PIPAMD_CMP_VALUE
 *   d_status_a[k], d_status_b[k]  int32: sa and sb; both PIPAMD_ST_OUTSIDE for a point outside the context
 *   d_summary      PIPAMD_CMP_WORDS int64, initialised by the call on `stream` (two calls do not accumulate): the
 *                  counts sum to n_points; order-independent integers throughout, so the summary is deterministic.
 * A fill of the summary and one kernel on `stream`, no synchronisation; may run concurrently on several streams with
 * different output buffers; neither tape is changed.  PIPAMD_E_INVALID before any HIP call: a null engine or tape; a tape
 * of another device than the engine's; nvar or pipamd_tape_point_cols differing between the tapes; PIPAMD_CMP_DUAL with
 * differing ndual; unknown flag bits; and what pipamd_tape_eval (list form) or pipamd_tape_sweep (sweep form) refuse for
 * their points, box and context.  PIPAMD_E_TOOLARGE: as the planner.  pipamd_debug_tape_sweep_blocks bounds the sweep
 * form's grid too. */
int pipamd_tape_compare(pipamd_engine *e, const pipamd_tape *a, const pipamd_tape *b, int flags, int64_t n_points,
                        const int64_t *d_points, int64_t *d_summary, int32_t *d_class, int32_t *d_where,
                        int32_t *d_status_a, int32_t *d_status_b, void *stream);
int pipamd_tape_compare_sweep(pipamd_engine *e, const pipamd_tape *a, const pipamd_tape *b, int flags, const int64_t *lo,
                              const int64_t *hi, int n_ctx, int ctx_cols, const int64_t *d_ctx, int64_t *d_summary,
                              int32_t *d_class, int32_t *d_where, int32_t *d_status_a, int32_t *d_status_b, void *stream);

/* A sweep's values reduced per unknown on the device (added since interface version 500): over a whole box, what values
 * does unknown i take -- its smallest, its largest, where they are attained, and the exact total?  The box, the order
 * of k, the context rows, the statuses, the RANGE rules, the edit marks and the empty tape are exactly
 * pipamd_tape_sweep's; nothing per point is written, so the box may be far larger than memory for its answers.
 * The summary: PIPAMD_VALUES_WORDS(nvar) int64 on the device.  Words 0..7 are bit for bit the words 0..7 pipamd_tape_sweep
 * writes for the same call (counts and firsts by status).  Behind them one record of PIPAMD_VALUES_REC words per unknown,
 * unknown i at word PIPAMD_VALUES_HEAD + PIPAMD_VALUES_REC * i:
 *   0 n_int        PIPAMD_ST_SOLUTION points at which unknown i is handed out over denominator 1
 *   1 n_frac       ... over a denominator > 1
 *   2 n_unbounded  ... over denominator 0 (an edited tape's unbounded unknown)
 *   3 0
 *   4,5 min (low, high: two's complement 128 bits; an int64 tape's value sign-extended)     6 k_min
 *   7,8 max (low, high)                                                                     9 k_max
 *   10,11,12 sum: 192 bits two's complement, little-endian limbs
 *   13..15 0
 * Only points that end PIPAMD_ST_SOLUTION take part, and RANGE is a status of the point as in pipamd_tape_eval: one
 * unknown out of range drops the whole point from every record.  For such a point unknown i is the pair
 * pipamd_tape_eval hands out: over denominator 1 the numerator enters n_int, min, max and sum; over a larger
 * denominator it is counted in n_frac and nothing else; over 0 in n_unbounded and nothing else.  k_min / k_max: the
 * smallest k of the box (k counts every point, outside ones included) at which the min / max is attained.  With
 * n_int == 0, min, max and sum are 0 and both k are -1.  The sum is exact: fewer than 2^38 values below 2^127 in
 * magnitude cannot leave 192 bits.  Every figure is an order-independent integer, and no record word is ever the target
 * of an atomic: the summary is bit-identical from run to run and for every grid size.
 * Two stages in memory the caller gives: the sweep kernel leaves a partial record per wave and unknown in d_work, a
 * second small kernel on the same stream folds them into d_summary.  The layout of d_work is private; plan.work_bytes
 * says how much a call needs:
 *     96 * nvar * 2 * min(ceil(n_points / 128), 2048)  bytes
 * -- 96 bytes a partial record, two waves a workgroup, a workgroup per chunk of 128 points up to the grid's cap of 2048
 * workgroups: 24 MiB at most (nvar 64).  d_work is read and written as int64 words: it must be 8-byte aligned, as
 * whatever hipMalloc returns is (a caller that sub-allocates keeps to it).  Neither d_summary nor d_work needs initialising, two calls do not accumulate,
 * and calls on several streams with different buffers may run concurrently.
 * pipamd_tape_sweep_values_plan is host only, as pipamd_tape_sweep_plan; nvar is the tape's shape.nvar.
 * PIPAMD_E_INVALID: whatever that planner refuses; nvar < 0.  PIPAMD_E_TOOLARGE: what that planner answers so; nvar above
 * PIPAMD_VALUES_MAX_NVAR (lane i of a wave keeps unknown i's record in registers).  nvar == 0 is legal: eight words.
 * plan.staged: 1 exactly when info.staged and the program (8 * info.words) fits PIPAMD_TAPE_LDS_BYTES beside the slots
 * (128 * (info.slots - 1) values of bits / 8 bytes) and beside the LDS of the value reduction -- which is none: its
 * accumulators are registers, so today the switch is info.staged's; a call reads the plan, not info.  Otherwise the
 * program is read from global memory.
 * pipamd_tape_sweep_values: a fill of the head words and two kernels on `stream`, no synchronisation.  PIPAMD_E_INVALID
 * before any HIP call: what pipamd_tape_sweep refuses; a null d_summary or d_work; a d_work that is not 8-byte aligned;
 * work_bytes below the plan's.
 * PIPAMD_E_TOOLARGE as the planner.  pipamd_debug_tape_sweep_blocks bounds this grid too. */
#define PIPAMD_VALUES_MAX_NVAR 64
#define PIPAMD_VALUES_HEAD 8 /* the sweep's words 0..7: PIPAMD_SWEEP_COUNT + status, PIPAMD_SWEEP_FIRST + status */
#define PIPAMD_VALUES_REC 16 /* int64 words per unknown */
#define PIPAMD_VALUES_WORDS(nvar) (8 + 16 * (nvar))
struct pipamd_tape_values_plan {
  int64_t n_points;      /* prod (hi[c] - lo[c] + 1); 1 when point_cols == 0 */
  int64_t summary_words; /* PIPAMD_VALUES_WORDS(nvar) */
  int64_t work_bytes;    /* see above */
  int32_t staged;
  int32_t reserved;
}; /* 32 bytes, offsets 0 8 16 24 28 */
int pipamd_tape_sweep_values_plan(const pipamd_tape_info *info, int bits, int nvar, int point_cols, const int64_t *lo,
                                  const int64_t *hi, struct pipamd_tape_values_plan *plan);
int pipamd_tape_sweep_values(pipamd_engine *e, const pipamd_tape *t, const int64_t *lo, const int64_t *hi, int n_ctx,
                             int ctx_cols, const int64_t *d_ctx, int64_t *d_summary, void *d_work, size_t work_bytes,
                             void *stream);

/* Every tape of a set swept over its own box in one launch (added since interface version 500): the census per answer
 * of pipamd_pip_solve_many's many small problems -- over this problem's parameter box, under the context it was solved
 * with, how many points have a solution, how many are NIL, which leaves are reached and where first.  A JOB is a tape of
 * a set, a box and a context; a launch takes any number of jobs and writes one pipamd_tape_sweep summary per job.
 * Meaning: with summary_off as below, words summary_off[j] .. summary_off[j + 1] - 1 of the summary are the
 * PIPAMD_SWEEP_WORDS(L_j) words pipamd_tape_sweep writes for job j's tape, box and context, bit for bit: k counts inside
 * the job's own box, and the statuses, the RANGE rules, the edit marks, the empty tape (every inside point NIL, leaf -1)
 * and the exact context test are the single sweep's.  Nothing per point is written: values per point of a set are what
 * pipamd_tape_set_eval is for.  A tape may appear in several jobs -- a large box cut into tiles, whose summaries merge by
 * adding the counts and taking the smallest first + offset -- and tapes may be left out.
 *
 * pipamd_tape_set_tape_info: what the set keeps of tape i on the host -- its pipamd_tape_info as compiled (leaves sizes
 * the summary), pipamd_tape_point_cols, nvar and ndual; each output may be NULL.  PIPAMD_E_INVALID: a null set, i outside
 * 0 .. n - 1.
 *
 * pipamd_tape_set_sweep_plan is host only: it needs neither an engine nor a GPU.  leaves[j] and point_cols[j] are those
 * of job j's tape (the planner does not read jobs[j].tape).  points[j]: the product of the extents of job j's box, 1
 * for 0 columns.  summary_off[0 .. n_jobs]: the running sums of PIPAMD_SWEEP_WORDS(leaves[j]); summary_off[n_jobs] words
 * is the summary a run needs.  chunk_off[0 .. n_jobs] (may be NULL): the running sums of ceil(points[j] / 128), the
 * units of work the kernel deals out.  Products and sums are formed without wrapping.  PIPAMD_E_INVALID, naming the
 * job: whatever pipamd_tape_sweep_plan refuses of a box (point_cols outside 0 .. PIPAMD_TAPE_MAX_SLOTS - 1, null lo or
 * hi with point_cols > 0, any lo[c] > hi[c]); n_ctx < 0; a null ctx with n_ctx > 0; leaves[j] outside 0 .. 2^31 - 1;
 * and n_jobs < 0, a null summary_off, and with n_jobs > 0 a null jobs, leaves, point_cols or points.
 * PIPAMD_E_TOOLARGE: more than 2^20 jobs (answered before any array is read); a job of 2^38 points or more; all jobs
 * up to some job together reaching 2^38 points.  Jobs are checked in order and the first refusal is the answer.
 *
 * pipamd_tape_set_sweep_create runs the planner's checks with the set's own leaves and point_cols and also refuses,
 * PIPAMD_E_INVALID: a null engine, set or `out`; a set of another device than the engine's; jobs[j].tape outside
 * 0 .. n - 1 -- all before any HIP call.  It then copies everything the kernel needs per job -- the tape's table index,
 * lo and the extents, n_ctx and the context rows (ragged: job j's rows have its own point_cols + 2 columns), the point
 * count, the summary offset, leaves, the chunk prefix -- into ONE device buffer.  The host arrays may be freed when the
 * call returns; the object is immutable; the SET MUST OUTLIVE IT.  summary_off (n_jobs + 1 values, may be NULL) is the
 * planner's.  n_jobs == 0 is legal.  Free with pipamd_tape_set_sweep_free (NULL is allowed), not while a run is still
 * on a stream.
 *
 * pipamd_tape_set_sweep_run: a fill of the summary_off[n_jobs] words of d_summary (counts 0, firsts -1, per job) and one
 * kernel on `stream`; no synchronisation and no per-call host table, so it may run concurrently on several streams
 * with different summaries; two calls do not accumulate.  n_jobs == 0: PIPAMD_OK without a launch.  PIPAMD_E_INVALID
 * before any HIP call: a null engine or sweep, a sweep of another device, a null d_summary with n_jobs > 0.
 * pipamd_debug_tape_sweep_blocks bounds this grid too.  Every figure is an order-independent integer (64-bit adds and
 * unsigned minima): the summary is deterministic. */
typedef struct pipamd_tape_sweep_job {
  int32_t tape;       /* index into the set */
  int32_t n_ctx;      /* rows of this job's context */
  const int64_t *lo;  /* HOST, pipamd_tape_point_cols of that tape values, inclusive; NULL allowed when 0 columns */
  const int64_t *hi;
  const int64_t *ctx; /* HOST, n_ctx x (point_cols + 2): marker, coefficients, constant, as ineqpar; NULL when n_ctx == 0 */
} pipamd_tape_sweep_job; /* 32 bytes, offsets 0 4 8 16 24 */
typedef struct pipamd_tape_set_sweep pipamd_tape_set_sweep;
int pipamd_tape_set_tape_info(const pipamd_tape_set *s, int i, pipamd_tape_info *info, int32_t *point_cols, int32_t *nvar,
                              int32_t *ndual);
int pipamd_tape_set_sweep_plan(int n_jobs, const pipamd_tape_sweep_job *jobs, const int64_t *leaves, const int32_t *point_cols,
                               int64_t *points, int64_t *summary_off, int64_t *chunk_off);
int pipamd_tape_set_sweep_create(pipamd_engine *e, const pipamd_tape_set *s, int n_jobs, const pipamd_tape_sweep_job *jobs,
                                 pipamd_tape_set_sweep **out, int64_t *summary_off);
int pipamd_tape_set_sweep_run(pipamd_engine *e, const pipamd_tape_set_sweep *w, int64_t *d_summary, void *stream);
void pipamd_tape_set_sweep_free(pipamd_tape_set_sweep *w);

#ifdef __cplusplus
}
#endif
#endif /* PIPLIB_AMD_H */
