// piplib_amd/csrc/pip_host.cpp -- host side of the C ABI (include/piplib_amd.h), layers 1-2.
//
// Owns no algorithmic work: shapes, workspace layout, launches, timing.  The
// decision-tree host (layer 3) lives in pip_tree.cpp.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <vector>

#include "pip_host.h"
#include "pip_source.h"
#include "pip_wide.h"

static thread_local char g_err[512];
void pipamd_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
extern "C" const char *pipamd_last_error(void) { return g_err; }
extern "C" int pipamd_version(void) { return PIPAMD_VERSION; }

#define HIPCHK(call)                                                                    \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess) {                                                             \
      pipamd_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      return PIPAMD_E_HIP;                                                              \
    }                                                                                   \
  } while (0)

extern "C" int pipamd_engine_create(pipamd_engine **out, int device) {
  if (!out) return PIPAMD_E_INVALID;
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (n <= 0 || device < 0 || device >= n) {
    pipamd_set_error("no such HIP device %d (count %d): the HIP path is mandatory, there is no CPU fallback", device, n);
    return PIPAMD_E_HIP;
  }
  HIPCHK(hipSetDevice(device));
  pipamd_engine *e = (pipamd_engine *)calloc(1, sizeof *e);
  if (!e) return PIPAMD_E_NOMEM;
  e->device = device;
  e->iter_limit = PIPAMD_DETLOG;
  if (hipDeviceGetAttribute(&e->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || e->cus < 1) e->cus = 1;
  {
    const char *nl = getenv("PIPAMD_NO_LEAN");  // measurement aid, like pipamd_debug_lean(e, 0)
    e->no_lean = nl && nl[0] == '1';
    const char *n2 = getenv("PIPAMD_NO_LEAN2");  // measurement aid: the general one-wave kernel as the second bulk launch
    e->no_lean2 = n2 && n2[0] == '1';
    const char *sr = getenv("PIPAMD_NO_SPARE_REPLAY");  // measurement aid, like pipamd_engine_set_spare_replay(e, 0)
    e->no_spare_replay = sr && sr[0] == '1';
    const char *lw = getenv("PIPAMD_LEAN2_WAVES");  // measurement aid, like pipamd_engine_set_lean2_waves(e, 1)
    e->lean2_one_wave = lw && lw[0] == '1';
  }
  pthread_mutex_init(&e->dt_lock, nullptr);
  *out = e;
  return PIPAMD_OK;
}

extern "C" void pipamd_engine_destroy(pipamd_engine *e) {
  if (!e) return;
  for (int i = 0; i < 2 * e->nev; i++) hipEventDestroy(e->ev[i]);
  if (e->d_q) hipFree(e->d_q);
  if (e->h_run) hipHostFree(e->h_run);
  if (e->d_scratch) hipFree(e->d_scratch);
  for (void *b : e->d_side)
    if (b) hipFree(b);
  for (int i = 0; i < e->nretired; i++) hipFree(e->retired[i]);
  if (e->d_side_count) hipFree(e->d_side_count);
  free(e->run);
  for (void *b : e->dt_buf)
    if (b) hipFree(b);
  if (e->dt_host) hipHostFree(e->dt_host);
  free(e->dt_rec);
  pthread_mutex_destroy(&e->dt_lock);
  free(e);
}

// ------------------------------------------------------------------ layer 1
static int round_even(int x) { return (x + 1) & ~1; }

int pipamd_batch_layout(const pipamd_batch_desc *d, PipBatchLayout *lay, size_t *jobs_bytes) {
  if (!d || d->batch <= 0 || d->nvar < 0 || d->nparm < 0 || d->ni < 0 || d->cap_cuts < 0 || d->cap_newparm < 0) {
    pipamd_set_error("invalid batch descriptor");
    return PIPAMD_E_INVALID;
  }
  const int ncol = d->nvar + d->nparm + 1;
  const int ebits = d->entier_bits == 128 ? 128 : 64;
  if (d->entier_bits != 0 && d->entier_bits != 64 && d->entier_bits != 128) {
    pipamd_set_error("entier_bits must be 0 (= 64), 64 or 128");
    return PIPAMD_E_INVALID;
  }
  const int ew = ebits / 64;
  lay->ebits = ebits;
  lay->batch = d->batch;
  lay->nvar = d->nvar;
  lay->nparm = d->nparm;
  lay->ni = d->ni;
  lay->bigparm = d->bigparm;
  lay->tflags = d->tflags & ~(PIPAMD_T_ROWS_STAY | PIPAMD_T_FRESHROWS);  // the load sets FRESHROWS itself
  lay->pad = 0;
  lay->S = d->ni + d->cap_cuts;
  lay->W = ebits == 128 ? ncol + d->cap_newparm : round_even(ncol + d->cap_newparm);
  const int wp = ebits == 128 ? (lay->W <= 64 ? 64 : (lay->W <= 128 ? 128 : (lay->W <= 256 ? 256 : 512)))
                              : (lay->W <= 128 ? 128 : (lay->W <= 256 ? 256 : 512));
  lay->blk = pip_block_layout(d->nvar, lay->S, lay->W, ew, (int64_t)d->nvar * (d->nparm + d->cap_newparm + 1) + d->nvar, wp / 64);
  // 64-bit tableaux whose row tables outgrow LDS run with the tables in HBM; 128-bit ones must fit
  if (lay->blk.L > PIPAMD_LMAX || lay->S > PIPAMD_SMAX || lay->W > PIPAMD_MAXCOL || lay->S < 1 ||
      (ebits == 128 && pipk_advance_lds_bytes((lay->blk.L + 3) & ~3, (lay->S + 3) & ~3, lay->W, ebits) > PIPAMD_LDS_BUDGET)) {
    pipamd_set_error("batch shape exceeds engine limits (L=%d<=%d, S=%d<=%d, W=%d<=%d, LDS image %zu<=%d bytes)", lay->blk.L,
                     PIPAMD_LMAX, lay->S, PIPAMD_SMAX, lay->W, PIPAMD_MAXCOL,
                     pipk_advance_lds_bytes((lay->blk.L + 3) & ~3, (lay->S + 3) & ~3, lay->W, ebits), PIPAMD_LDS_BUDGET);
    return PIPAMD_E_TOOLARGE;
  }
  if (d->bigparm >= ncol || (d->bigparm >= 0 && d->bigparm <= d->nvar)) {
    pipamd_set_error("bigparm must be -1 or a parameter column (nvar < bigparm < ncol)");
    return PIPAMD_E_INVALID;
  }
  lay->arena_off = 0;
  *jobs_bytes = ((size_t)d->batch * sizeof(PipJob) + 255) & ~(size_t)255;
  return PIPAMD_OK;
}

extern "C" size_t pipamd_batch_workspace_bytes(const pipamd_batch_desc *d) {
  PipBatchLayout lay;
  size_t jb;
  if (pipamd_batch_layout(d, &lay, &jb) != PIPAMD_OK) return 0;
  return jb + (size_t)lay.blk.words * (size_t)d->batch * sizeof(int64_t);
}

extern "C" size_t pipamd_dense_pivot_bytes(const pipamd_batch_desc *d) {
  // one pivot reads and writes every real row once: 2 * ni * ncol * sizeof(Entier)
  return 2ull * (size_t)d->ni * (size_t)(d->nvar + d->nparm + 1) * (d->entier_bits == 128 ? 16 : 8);
}

// What every entry that works on a loaded batch starts with: the layout of the descriptor, the tableaux first ..
// first + count - 1 held against the batch, the engine's device made current, the workspace split into its job headers
// and its arena.  Argument errors are reported before the first HIP call.
struct BatchView {
  PipBatchLayout lay;
  PipJob *jobs;
  long long *arena;
};

// (batch_view without the device: an empty part of a front end is checked like any other, then launches nothing and makes
// no HIP call)
static int part_view(const char *who, const pipamd_engine *e, const void *d_ws, const pipamd_batch_desc *d, int first, int count,
                     BatchView *v) {
  if (!e || !d_ws || !d) {
    pipamd_set_error("%s: null engine, workspace or descriptor", who);
    return PIPAMD_E_INVALID;
  }
  size_t jb;
  int rc = pipamd_batch_layout(d, &v->lay, &jb);
  if (rc) return rc;
  if (first < 0 || count < 0 || first > v->lay.batch - count) {
    pipamd_set_error("%s_part: tableaux %d..%d outside the batch of %d", who, first, first + count, v->lay.batch);
    return PIPAMD_E_INVALID;
  }
  v->jobs = (PipJob *)d_ws;
  v->arena = (long long *)((char *)d_ws + jb);
  return PIPAMD_OK;
}

static int batch_view(const char *who, const pipamd_engine *e, const void *d_ws, const pipamd_batch_desc *d, int first, int count,
                      BatchView *v) {
  int rc = part_view(who, e, d_ws, d, first, count, v);
  if (rc) return rc;
  return hipSetDevice(e->device) == hipSuccess ? PIPAMD_OK : PIPAMD_E_HIP;  // HIP's current device is per host thread
}

extern "C" int pipamd_batch_load_part(pipamd_engine *e, void *d_ws, const pipamd_batch_desc *d, const int64_t *d_rows,
                                      int first, int count, void *stream) {
  if (!d_rows) return PIPAMD_E_INVALID;
  BatchView v;
  int rc = batch_view("batch_load", e, d_ws, d, first, count, &v);
  if (rc) return rc;
  // PIPAMD_T_ROWS_STAY: no copy pass, the first pivot launch reads the caller's rows (whole 16-byte units)
  const int ncol = d->nvar + d->nparm + 1;
  v.lay.pad = (d->tflags & PIPAMD_T_ROWS_STAY) && v.lay.ebits != 128 && ncol % 2 == 0 && ((uintptr_t)d_rows & 15) == 0;
  HIPCHK(pipk_launch_batch_load(v.jobs, v.arena, (const long long *)d_rows, v.lay, first, count, (hipStream_t)stream));
  return PIPAMD_OK;
}

extern "C" int pipamd_batch_load(pipamd_engine *e, void *d_ws, const pipamd_batch_desc *d, const int64_t *d_rows,
                                 void *stream) {
  if (!d) return PIPAMD_E_INVALID;
  return pipamd_batch_load_part(e, d_ws, d, d_rows, 0, d->batch, stream);
}

// The launch sequence of pipamd_batch_solve is decided in pip_plan.h (pip_plan_batch, pip_plan_tail); BatchRun issues it.
#define Q_CTRL 3 /* control words per launch: out_count, out_maxni, the number of listed jobs that are out of rows */
// Control words (out_count, out_maxni per launch) must be zero when a launch starts.  They come
// from a pool of Q_POOL solves x Q_FAST launches that one memset zeroes every Q_POOL solves (a
// solve of a small batch is a handful of runtime calls: this was a fifth of them); the rare
// launches beyond Q_FAST of one solve use an overflow area zeroed on demand.
enum { Q_POOL = 64, Q_FAST = 8, Q_NPOOL = Q_CTRL * Q_FAST * Q_POOL, Q_NCTRL = Q_NPOOL + Q_CTRL * PIPAMD_MAX_ROUNDS };

// One pipamd_batch_solve in progress: everything the launch sequence needs between its asynchronous first part
// (bulk + first tail launch + the copy of the tail's control words, pipamd_batch_solve_async) and its completion
// (pipamd_batch_wait: further tail launches / re-housing while tableaux are left).
struct BatchRun {
  pipamd_engine *e;
  pipamd_batch_desc d;
  PipBatchLayout lay;
  PipJob *jobs;
  long long *arena;
  hipStream_t st;
  int *pool, *over, *list[2];
  bool over_zeroed, have_list, active, finishing, replay_pending;
  PipPlanIn in;    // what the launch sequence was decided from, and the decision (pip_plan.h)
  PipPlan plan;
  int stage;       // launches issued
  int curS;        // row capacity of the largest block in play (grows when tableaux are re-housed)
  int grow_round;
  int upper;       // what the host knows about the length of the next input list

  int *ctrl_of(int stg) const { return stg < Q_FAST ? pool + Q_CTRL * stg : over + Q_CTRL * (stg - Q_FAST); }

  int next_stage() {
    if (stage >= PIPAMD_MAX_ROUNDS) {
      pipamd_set_error("batch_solve: more than %d launches", PIPAMD_MAX_ROUNDS);
      return PIPAMD_E_SOLVER;
    }
    if (stage >= Q_FAST && !over_zeroed) {
      HIPCHK(hipMemsetAsync(over, 0, (size_t)Q_CTRL * PIPAMD_MAX_ROUNDS * sizeof(int), st));
      over_zeroed = true;
    }
    return PIPAMD_OK;
  }

  // expanser (traiter.c:55-88, called by integrer when the tableau is full, integrer.c:410-415) for the `n` jobs of
  // the last launch's out list: those at PIPAMD_ST_CAPACITY move into blocks of twice the row capacity in a side arena
  // of the engine and go on; the others are passed through.  A stage like a launch: it consumes the list and writes
  // the next one.  When the engine's limits (16-bit row codes; 128-bit entries: the LDS image) allow no larger
  // block, the pass only drops the jobs that are at the limit from the list: they keep PIPAMD_ST_CAPACITY.
  int rehouse(int n, int ncap) {
    pipamd_batch_desc d2 = d;
    int newS = curS * 2 > curS + 32 ? curS * 2 : curS + 32;
    if (e->grow_step > 0) newS = curS + e->grow_step;  // testing aid: many small growth rounds
    // the caller's row budget (pipamd_engine_set_max_rows); never below what the batch was loaded with
    const int budget = e->max_rows > 0 ? (e->max_rows > lay.S ? e->max_rows : lay.S) : PIPAMD_SMAX;
    if (newS > budget) newS = budget;
    if (newS < curS) newS = curS;  // == curS: nothing larger is allowed -- the pass drops the jobs that are at the limit
    PipBatchLayout nl;
    size_t jb2;
    // the side arena holds the jobs that are out of rows (`ncap`, counted by the launch that listed them), not the whole
    // list: that also carries the jobs merely paused
    if (ncap < 1) ncap = 1;
    if (ncap > n) ncap = n;
    d2.batch = ncap;
    for (;;) {
      d2.cap_cuts = newS - d.ni;
      if (pipamd_batch_layout(&d2, &nl, &jb2) == PIPAMD_OK) break;
      if (newS <= curS) return PIPAMD_E_SOLVER;  // the shape the batch was loaded with (or grew to): cannot fail
      newS = curS + (newS - curS) / 2;
    }
    int rc2 = next_stage();
    if (rc2) return rc2;
    const bool room = grow_round < PIPAMD_MAX_GROW;
    const size_t per_job_bytes = (size_t)nl.blk.words * sizeof(int64_t);
    const size_t need = per_job_bytes * (size_t)ncap + 16;
    int side_cap = 0;
    if (room) {
      if (e->side_bytes[grow_round] < need) {
        // grown geometrically; the outgrown arena is kept until the engine goes (hipFree in mid-stream would wait for
        // every other batch in flight on the device); if the device has no room the jobs that do not fit the arena that
        // is there keep PIPAMD_ST_CAPACITY -- the batch is not failed for them
        size_t want = 2 * e->side_bytes[grow_round] > need ? 2 * e->side_bytes[grow_round] : need;
        void *nb = nullptr;
        if (hipMalloc(&nb, want) != hipSuccess) {
          (void)hipGetLastError();
          want = need;
          if (hipMalloc(&nb, want) != hipSuccess) {
            (void)hipGetLastError();
            nb = nullptr;
          }
        }
        if (nb) {
          if (e->d_side[grow_round]) {
            if (e->nretired < (int)(sizeof e->retired / sizeof e->retired[0]))
              e->retired[e->nretired++] = e->d_side[grow_round];
            else
              HIPCHK(hipFree(e->d_side[grow_round]));
          }
          e->d_side[grow_round] = nb;
          e->side_bytes[grow_round] = want;
        }
      }
      const size_t fit = e->side_bytes[grow_round] > 16 ? (e->side_bytes[grow_round] - 16) / per_job_bytes : 0;
      side_cap = fit < (size_t)ncap ? (int)fit : ncap;
    }
    if (!e->d_side_count) HIPCHK(hipMalloc((void **)&e->d_side_count, sizeof(int)));
    HIPCHK(hipMemsetAsync(e->d_side_count, 0, sizeof(int), st));
    // job offsets are in int64 units from `arena`, rows 16-byte aligned
    const char *side = (room && e->d_side[grow_round]) ? (const char *)e->d_side[grow_round] : (const char *)arena;
    if (((side - (const char *)arena) & 15) != 0) side += 8;
    nl.arena_off = (int64_t)((side - (const char *)arena) / (ptrdiff_t)sizeof(int64_t));
    int *c = ctrl_of(stage);
    void *q5[5] = {list[(stage - 1) & 1], ctrl_of(stage - 1), list[stage & 1], c, c + 1};
    HIPCHK(pipk_launch_rehouse(jobs, arena, q5, n, nl, e->d_side_count, side_cap, st));
    stage++;
    if (room) grow_round++;
    curS = newS;
    e->last_rehoused += ncap;
    return PIPAMD_OK;
  }

  int launch(const PipStep &s) {
    int rcs = next_stage();
    if (rcs) return rcs;
    const int smax = s.smax > curS ? curS : s.smax;
    int *c = ctrl_of(stage);
    void *q5[5] = {nullptr, nullptr, list[stage & 1], c, c + 1};
    if (have_list) {
      q5[0] = list[(stage - 1) & 1];
      q5[1] = ctrl_of(stage - 1);
    }
    if (!e->no_timing) {
      if (e->nlaunch >= e->nev) {
        HIPCHK(hipEventCreate(&e->ev[2 * e->nev]));
        HIPCHK(hipEventCreate(&e->ev[2 * e->nev + 1]));
        e->nev++;
      }
      HIPCHK(hipEventRecord(e->ev[2 * e->nlaunch], st));
    }
    void *big[2] = {&e->d_scratch, &e->scratch_bytes};
    const int hints = (s.full ? PIPK_HINT_FULL : 0) |
                      (s.kernel == PIP_K_LEAN64 ? PIPK_HINT_LEAN64
                       : s.kernel == PIP_K_LEAN_BIG ? PIPK_HINT_LEAN | PIPK_HINT_BIG
                       : s.kernel == PIP_K_LEAN ? PIPK_HINT_LEAN : 0) |
                      (s.replay_behind ? 0 : PIPK_HINT_NO_REPLAY) | (s.spare_replay ? PIPK_HINT_SPARE_REPLAY : 0);
    HIPCHK(pipk_launch_advance_q(jobs, arena, lay.batch, lay.nvar + smax, smax, lay.W, s.budget, s.waves, lay.ebits, q5,
                                 s.whole_batch ? lay.batch : upper, big, hints, e->d_prof, st));
    if (!e->no_timing) HIPCHK(hipEventRecord(e->ev[2 * e->nlaunch + 1], st));
    e->nlaunch++;
    stage++;
    have_list = true;
    return PIPAMD_OK;
  }

  // the one replay of the logs the launches so far left (pip_plan.h), if any, then the copy of the last launch's
  // control words to the host
  int replay_and_report(bool replay) {
    if (replay) HIPCHK(pipk_launch_replay_all(jobs, arena, lay.batch, lay.ebits, plan.catchall_waves, st));
    replay_pending = false;
    HIPCHK(hipMemcpyAsync(e->h_run, ctrl_of(stage - 1), Q_CTRL * sizeof(int), hipMemcpyDeviceToHost, st));
    return PIPAMD_OK;
  }

  // a tail launch over what is left (pip_plan_tail), and the copy of its control words to the host
  int tail() {
    int rc = launch(pip_plan_tail(in, plan.tail_waves, curS, upper, replay_pending));
    return rc ? rc : replay_and_report(replay_pending);
  }

  int begin(pipamd_engine *e_, void *d_ws, const pipamd_batch_desc *d_, void *stream) {
    e = e_;
    size_t jb;
    int rc = pipamd_batch_layout(d_, &lay, &jb);
    if (rc) return rc;
    d = *d_;
    jobs = (PipJob *)d_ws;
    arena = (long long *)((char *)d_ws + jb);
    st = (hipStream_t)stream;
    if (!e->h_run) HIPCHK(hipHostMalloc((void **)&e->h_run, Q_CTRL * sizeof(int), hipHostMallocDefault));
    if (!e->d_q || e->q_cap < lay.batch) {
      if (e->d_q) HIPCHK(hipFree(e->d_q));
      e->d_q = nullptr;
      HIPCHK(hipMalloc((void **)&e->d_q, ((size_t)Q_NCTRL + 2 * (size_t)lay.batch) * sizeof(int)));
      e->q_cap = lay.batch;
      e->solve_seq = 0;
    }
    if (e->solve_seq % Q_POOL == 0 || e->pool_stream != st) {
      HIPCHK(hipMemsetAsync(e->d_q, 0, (size_t)Q_NPOOL * sizeof(int), st));
      e->solve_seq = 0;
      e->pool_stream = st;
    }
    pool = e->d_q + Q_CTRL * Q_FAST * (e->solve_seq % Q_POOL);
    over = e->d_q + Q_NPOOL;
    e->solve_seq++;
    over_zeroed = false;
    list[0] = e->d_q + Q_NCTRL;
    list[1] = e->d_q + Q_NCTRL + e->q_cap;
    e->nlaunch = 0;
    e->last_rehoused = 0;
    stage = 0;
    have_list = false;
    finishing = false;
    curS = lay.S;
    grow_round = 0;
    upper = lay.batch;
    in = PipPlanIn{lay.batch, lay.nvar, lay.nparm, lay.bigparm, lay.ni, lay.S, lay.W, lay.ebits, lay.tflags,
                   e->round_pivots, e->round_rows, e->bulk_min, e->iter_limit, e->waves_per_job, e->tail_waves,
                   e->lone_batches, e->no_spare_replay, e->lean2_one_wave, e->no_lean, e->no_lean2, e->lean64, e->lean_big,
                   e->single_launch, false};
    if (in.lean64) {
      const int s64 = pip_plan_lean64_rows(lay.S);
      in.lean64_fits = pipk_lean64_lds_bytes(s64, lay.nvar + s64) <= PIPAMD_LDS_BUDGET;
    }
    plan = pip_plan_batch(in);
    replay_pending = false;
    for (int i = 0; i < plan.nsteps; i++) {
      rc = launch(plan.step[i]);
      if (rc) return rc;
    }
    replay_pending = plan.pending;
    rc = plan.stop ? replay_and_report(plan.stop_replay) : tail();
    if (rc) return rc;
    active = true;
    return PIPAMD_OK;
  }

  int wait_stream() {
    if (e->blocking_wait) {  // sleep between looks at the stream instead of spinning on it (pipamd_engine_set_blocking_wait)
      hipError_t q;
      const struct timespec nap = {0, 40000};
      while ((q = hipStreamQuery(st)) == hipErrorNotReady) nanosleep(&nap, nullptr);
      HIPCHK(q);
    } else {
      HIPCHK(hipStreamSynchronize(st));
    }
    return PIPAMD_OK;
  }

  // What the launches enqueued so far left behind (the stream must be idle): 1 = every tableau has its final status,
  // 0 = more work was enqueued (a further tail launch, after re-housing the tableaux that are out of rows), < 0 error.
  int advance() {
    if (finishing) {  // the solutions of re-housed tableaux are back in the caller's workspace
      finishing = false;
      active = false;
      e->timed = !e->no_timing;
      return 1;
    }
    if (e->h_run[0] > 0 && !e->single_launch) {
      upper = e->h_run[0];
      if (e->h_run[1] & PIPAMD_Q_CAPFLAG) {  // some of them have spent their spare rows
        int rc = rehouse(upper, e->h_run[2]);
        if (rc) return rc;
      }
      int rc = tail();
      return rc ? rc : 0;
    }
    if (grow_round > 0) {  // the side arenas serve the engine's next solve: the solve ends when the copy-back has
      HIPCHK(pipk_launch_rehouse_finish(jobs, arena, lay.batch, (int)(lay.blk.state - lay.blk.sol), st));
      finishing = true;
      return 0;
    }
    active = false;
    e->timed = !e->no_timing;
    return 1;
  }

  int finish() {
    for (;;) {
      int rc = wait_stream();
      if (rc) {
        active = false;
        return rc;
      }
      rc = advance();
      if (rc < 0) active = false;
      if (rc != 0) return rc < 0 ? rc : PIPAMD_OK;
    }
  }
};

static int batch_begin(pipamd_engine *e, void *d_ws, const pipamd_batch_desc *d, void *stream) {
  if (e && hipSetDevice(e->device) != hipSuccess) return PIPAMD_E_HIP;  // HIP's current device is per host thread
  if (!e || !d_ws || !d) return PIPAMD_E_INVALID;
  if (!e->run) {
    e->run = (BatchRun *)calloc(1, sizeof(BatchRun));
    if (!e->run) return PIPAMD_E_NOMEM;
  }
  if (e->run->active) {
    pipamd_set_error("this engine already has a batch solve in flight: pipamd_batch_wait first (one per engine; engines are cheap)");
    return PIPAMD_E_INVALID;
  }
  return e->run->begin(e, d_ws, d, stream);
}

extern "C" int pipamd_batch_solve(pipamd_engine *e, void *d_ws, const pipamd_batch_desc *d, void *stream) {
  int rc = batch_begin(e, d_ws, d, stream);
  if (rc) {
    if (e && e->run) e->run->active = false;
    return rc;
  }
  return e->run->finish();
}

extern "C" int pipamd_batch_solve_async(pipamd_engine *e, void *d_ws, const pipamd_batch_desc *d, void *stream) {
  int rc = batch_begin(e, d_ws, d, stream);
  if (rc && e && e->run) e->run->active = false;
  return rc;
}

extern "C" int pipamd_batch_wait(pipamd_engine *e) {
  if (e && hipSetDevice(e->device) != hipSuccess) return PIPAMD_E_HIP;
  if (!e) return PIPAMD_E_INVALID;
  if (!e->run || !e->run->active) return PIPAMD_OK;  // nothing in flight
  return e->run->finish();
}

extern "C" int pipamd_batch_poll(pipamd_engine *e) {
  if (!e) return PIPAMD_E_INVALID;
  if (!e->run || !e->run->active) return 1;
  if (hipSetDevice(e->device) != hipSuccess) return PIPAMD_E_HIP;
  hipError_t q = hipStreamQuery(e->run->st);
  if (q == hipErrorNotReady) return 0;
  if (q != hipSuccess) {
    pipamd_set_error("hipStreamQuery failed: %s", hipGetErrorString(q));
    e->run->active = false;
    return PIPAMD_E_HIP;
  }
  // the launches enqueued so far have ended: done, or the next ones go out now (never blocks)
  int rc = e->run->advance();
  if (rc < 0) e->run->active = false;
  return rc;
}

// Row budget of pipamd_batch_solve: a tableau is re-housed (expanser) while its row capacity stays within `rows`
// (0 = the default: only the engine's own limit); beyond it the tableau ends PIPAMD_ST_CAPACITY.  The reference grows
// without bound, and so does the default here; a caller that feeds tableaux on which Gomory cuts converge slowly
// (thousands of cut rows, each pivot then rewriting thousands of rows) bounds the memory and time of a batch with it.
extern "C" int pipamd_engine_set_max_rows(pipamd_engine *e, int rows) {
  if (!e || rows < 0) return PIPAMD_E_INVALID;
  e->max_rows = rows;
  return PIPAMD_OK;
}

// Testing aid: a tableau that has spent its spare rows is re-housed with `rows` more instead of twice as many, so
// that a test sees many growth rounds on small inputs (0 = the default doubling).
extern "C" int pipamd_debug_grow_step(pipamd_engine *e, int rows) {
  if (!e || rows < 0) return PIPAMD_E_INVALID;
  e->grow_step = rows;
  return PIPAMD_OK;
}

// Measurement aid (bench.py's per-launch roofline): the solve stops after its first launch -- the one-wave bulk
// launch when the batch has one -- leaving unfinished tableaux at PIPAMD_ST_RUN; pipamd_batch_counters then tells
// what that launch alone did.
extern "C" int pipamd_debug_single_launch(pipamd_engine *e, int on) {
  if (!e) return PIPAMD_E_INVALID;
  // 1: after the bulk launches, 2: after the lean launch alone, 3: as 1 but without the determinant replay behind them
  // (testing aid: statuses are then not final, an overflow the replay would find is not reported)
  e->single_launch = on < 0 ? 0 : (on > 3 ? 1 : on);
  return PIPAMD_OK;
}

// Measurement / testing aid: without the lean kernel every tableau of a bulk launch runs in pip_advance_kernel.
extern "C" int pipamd_debug_lean(pipamd_engine *e, int on) {
  if (!e) return PIPAMD_E_INVALID;
  e->no_lean = on ? 0 : 1;
  return PIPAMD_OK;
}

// The lean kernel of the 128-bit flavour (pip_lean64_kernel, csrc/pip_lean.h) as the first launch of pipamd_batch_solve on batches it can
// take (no parameters, 129 ... 256 columns, at least 128 tableaux); default off.
extern "C" int pipamd_engine_set_lean64(pipamd_engine *e, int on) {
  if (!e) return PIPAMD_E_INVALID;
  e->lean64 = on ? 1 : 0;
  return PIPAMD_OK;
}

// The lean kernel's BIG flavour (pip_lean_kernel<SC, false, true>, csrc/pip_lean.h) for the bulk launches of batches whose one
// parameter is the big one (nparm == 1, bigparm == nvar + 1, at most 128 columns of 64-bit entries); default off: such a
// batch then takes the launches it always took.  pipamd_debug_lean(e, 0) / PIPAMD_NO_LEAN switch it off like the plain flavour.
extern "C" int pipamd_engine_set_lean_big(pipamd_engine *e, int on) {
  if (!e) return PIPAMD_E_INVALID;
  e->lean_big = on ? 1 : 0;
  return PIPAMD_OK;
}

extern "C" int pipamd_engine_set_timing(pipamd_engine *e, int on) {
  if (!e) return PIPAMD_E_INVALID;
  e->no_timing = !on;
  return PIPAMD_OK;
}

// Sum of the advance-kernel launch durations of the last pipamd_batch_solve (HIP events on
// the launch stream) and their number.
extern "C" int pipamd_last_solve_ms(pipamd_engine *e, float *ms) {
  if (!e || !ms || !e->timed) return PIPAMD_E_INVALID;
  float tot = 0;
  for (int i = 0; i < e->nlaunch; i++) {
    float t = 0;
    HIPCHK(hipEventSynchronize(e->ev[2 * i + 1]));
    HIPCHK(hipEventElapsedTime(&t, e->ev[2 * i], e->ev[2 * i + 1]));
    tot += t;
  }
  *ms = tot;
  return PIPAMD_OK;
}

extern "C" int pipamd_last_solve_launches(pipamd_engine *e) { return e ? e->nlaunch : 0; }

// Duration of launch `i` of the last pipamd_batch_solve (diagnostics, tools/).
extern "C" int pipamd_last_launch_ms(pipamd_engine *e, int i, float *ms) {
  if (!e || !ms || !e->timed || i < 0 || i >= e->nlaunch) return PIPAMD_E_INVALID;
  HIPCHK(hipEventSynchronize(e->ev[2 * i + 1]));
  HIPCHK(hipEventElapsedTime(ms, e->ev[2 * i], e->ev[2 * i + 1]));
  return PIPAMD_OK;
}

extern "C" int pipamd_engine_set_round_pivots(pipamd_engine *e, int pivots) {
  if (!e || pivots < 1) return PIPAMD_E_INVALID;
  e->round_pivots = pivots;
  return PIPAMD_OK;
}

extern "C" int pipamd_engine_set_tail_waves(pipamd_engine *e, int waves) {
  if (!e || (waves != 4 && waves != 8)) return PIPAMD_E_INVALID;
  e->tail_waves = waves;
  return PIPAMD_OK;
}

extern "C" int pipamd_engine_set_lone_batches(pipamd_engine *e, int on) {
  if (!e) return PIPAMD_E_INVALID;
  e->lone_batches = on ? 1 : 0;
  return PIPAMD_OK;
}

extern "C" int pipamd_engine_set_spare_replay(pipamd_engine *e, int on) {
  if (!e) return PIPAMD_E_INVALID;
  e->no_spare_replay = on ? 0 : 1;
  return PIPAMD_OK;
}

extern "C" int pipamd_engine_set_lean2_waves(pipamd_engine *e, int waves) {
  if (!e || (waves != 1 && waves != 4)) return PIPAMD_E_INVALID;
  e->lean2_one_wave = waves == 1;
  return PIPAMD_OK;
}

extern "C" int pipamd_engine_set_blocking_wait(pipamd_engine *e, int on) {
  if (!e) return PIPAMD_E_INVALID;
  e->blocking_wait = on ? 1 : 0;
  return PIPAMD_OK;
}
extern "C" int pipamd_engine_set_device_tree(pipamd_engine *e, int on) {
  if (!e) return PIPAMD_E_INVALID;
  e->no_device_tree = on ? 0 : 1;
  return PIPAMD_OK;
}
extern "C" int pipamd_last_device_tree(const pipamd_engine *e, int *served, int *handed_back) {
  if (!e) return PIPAMD_E_INVALID;
  if (served) *served = e->dt_served;
  if (handed_back) *handed_back = e->dt_fallback;
  return PIPAMD_OK;
}

extern "C" int pipamd_engine_set_bulk_min(pipamd_engine *e, int tableaux) {
  if (!e || tableaux < 1) return PIPAMD_E_INVALID;
  e->bulk_min = tableaux;
  return PIPAMD_OK;
}

extern "C" int pipamd_engine_set_round_rows(pipamd_engine *e, int rows) {
  if (!e || rows < 1) return PIPAMD_E_INVALID;
  e->round_rows = rows;
  return PIPAMD_OK;
}

extern "C" int pipamd_batch_results(pipamd_engine *e, const void *d_ws, const pipamd_batch_desc *d, int32_t *d_status,
                                    int32_t *d_pivots, int32_t *d_cuts, int64_t *d_sol_num, int64_t *d_sol_den,
                                    void *stream) {
  BatchView v;
  int rc = batch_view("batch_results", e, d_ws, d, 0, 0, &v);
  if (rc) return rc;
  HIPCHK(pipk_launch_batch_results(v.jobs, v.arena, v.lay.batch, v.lay.nvar, v.lay.nparm, v.lay.ebits, d_status, d_pivots,
                                   d_cuts, (void *)d_sol_num, (void *)d_sol_den, (hipStream_t)stream));
  return PIPAMD_OK;
}

// The batch layer's front ends (header comments: include/piplib_amd.h): the tableau's dual, Maximize / Urs_unknowns, pip_solve's
// plain system, PolyLib matrices, sparse rows and the instances of one parametric system, each as a load and a dual entry,
// whole and _part.  An entry runs its form's check (pip_source.h), which fills the PipBatchSource, then load_from or
// dual_from.  Everything is checked before the first HIP call; the one launch goes on `stream` and nothing here waits for it.
static int load_from(const char *who, pipamd_engine *e, void *d_ws, const pipamd_batch_desc *d, const PipBatchSource *src,
                     int first, int count, void *stream) {
  BatchView v;
  int rc = (count ? batch_view : part_view)(who, e, d_ws, d, first, count, &v);
  if (rc || count == 0) return rc;
  HIPCHK(pipk_launch_batch_load_source(v.jobs, v.arena, v.lay, src, first, count, (hipStream_t)stream));
  return PIPAMD_OK;
}

static int dual_from(const char *who, pipamd_engine *e, const void *d_ws, const pipamd_batch_desc *d, const PipBatchSource *src,
                     int first, int count, int64_t *d_dual_num, int64_t *d_dual_den, void *stream) {
  int rc = dual_check(who, d, src, d_dual_num, d_dual_den);
  if (rc) return rc;
  BatchView v;
  rc = (count ? batch_view : part_view)(who, e, d_ws, d, first, count, &v);
  if (rc || count == 0) return rc;
  HIPCHK(pipk_launch_batch_dual_source(v.jobs, v.arena, v.lay, src, first, count, (void *)d_dual_num, (void *)d_dual_den,
                                       (hipStream_t)stream));
  return PIPAMD_OK;
}

extern "C" int pipamd_batch_load_shifted_part(pipamd_engine *e, void *d_ws, const pipamd_batch_desc *d, const int64_t *d_rows,
                                              int shift, int first, int count, void *stream) {
  PipBatchSource src;
  int rc = shifted_source("batch_load_shifted", e, d_ws, d, d_rows, shift, &src);
  return rc ? rc : load_from("batch_load_shifted", e, d_ws, d, &src, first, count, stream);
}

extern "C" int pipamd_batch_load_shifted(pipamd_engine *e, void *d_ws, const pipamd_batch_desc *d, const int64_t *d_rows, int shift,
                                         void *stream) {
  return pipamd_batch_load_shifted_part(e, d_ws, d, d_rows, shift, 0, d ? d->batch : 0, stream);
}

extern "C" int pipamd_batch_results_shifted(pipamd_engine *e, const void *d_ws, const pipamd_batch_desc *d, int shift,
                                            int32_t *d_status, int32_t *d_pivots, int32_t *d_cuts, int64_t *d_x_num,
                                            int64_t *d_x_den, void *stream) {
  int rc = shifted_check("batch_results_shifted", e, d_ws, d, shift);
  if (rc) return rc;
  BatchView v;
  rc = batch_view("batch_results_shifted", e, d_ws, d, 0, 0, &v);
  if (rc) return rc;
  HIPCHK(pipk_launch_batch_results_shifted(v.jobs, v.arena, v.lay.batch, v.lay.nvar, v.lay.ebits, shift, d_status, d_pivots,
                                           d_cuts, (void *)d_x_num, (void *)d_x_den, (hipStream_t)stream));
  return PIPAMD_OK;
}

// Compute_dual of a batch loaded by pipamd_batch_load: the tableau rows are the one source without a check of its own
extern "C" int pipamd_batch_dual_part(pipamd_engine *e, const void *d_ws, const pipamd_batch_desc *d, const int64_t *d_rows,
                                      int first, int count, int64_t *d_dual_num, int64_t *d_dual_den, void *stream) {
  PipBatchSource src;
  src.kind = PIP_SRC_TABLEAU;
  src.rows = d_rows;
  return dual_from("batch_dual", e, d_ws, d, &src, first, count, d_dual_num, d_dual_den, stream);
}

extern "C" int pipamd_batch_dual(pipamd_engine *e, const void *d_ws, const pipamd_batch_desc *d, const int64_t *d_rows,
                                 int64_t *d_dual_num, int64_t *d_dual_den, void *stream) {
  return pipamd_batch_dual_part(e, d_ws, d, d_rows, 0, d ? d->batch : 0, d_dual_num, d_dual_den, stream);
}

extern "C" int pipamd_batch_load_system_part(pipamd_engine *e, void *d_ws, const pipamd_batch_desc *d, const pipamd_system *sys,
                                             const int64_t *d_rows, int first, int count, void *stream) {
  PipBatchSource src;
  int rc = system_check("batch_load_system", e, d_ws, d, sys, d_rows, &src);
  return rc ? rc : load_from("batch_load_system", e, d_ws, d, &src, first, count, stream);
}

extern "C" int pipamd_batch_load_system(pipamd_engine *e, void *d_ws, const pipamd_batch_desc *d, const pipamd_system *sys,
                                        const int64_t *d_rows, void *stream) {
  return pipamd_batch_load_system_part(e, d_ws, d, sys, d_rows, 0, d ? d->batch : 0, stream);
}

extern "C" int pipamd_batch_dual_system_part(pipamd_engine *e, const void *d_ws, const pipamd_batch_desc *d,
                                             const pipamd_system *sys, const int64_t *d_rows, int first, int count,
                                             int64_t *d_dual_num, int64_t *d_dual_den, void *stream) {
  PipBatchSource src;
  int rc = system_check("batch_dual_system", e, d_ws, d, sys, d_rows, &src);
  return rc ? rc : dual_from("batch_dual_system", e, d_ws, d, &src, first, count, d_dual_num, d_dual_den, stream);
}

extern "C" int pipamd_batch_dual_system(pipamd_engine *e, const void *d_ws, const pipamd_batch_desc *d, const pipamd_system *sys,
                                        const int64_t *d_rows, int64_t *d_dual_num, int64_t *d_dual_den, void *stream) {
  return pipamd_batch_dual_system_part(e, d_ws, d, sys, d_rows, 0, d ? d->batch : 0, d_dual_num, d_dual_den, stream);
}

extern "C" int pipamd_batch_load_sparse_part(pipamd_engine *e, void *d_ws, const pipamd_batch_desc *d, const pipamd_sparse *s,
                                             int first, int count, void *stream) {
  PipBatchSource src;
  int rc = sparse_check("batch_load_sparse", e, d_ws, d, s, &src);
  return rc ? rc : load_from("batch_load_sparse", e, d_ws, d, &src, first, count, stream);
}

extern "C" int pipamd_batch_load_sparse(pipamd_engine *e, void *d_ws, const pipamd_batch_desc *d, const pipamd_sparse *s,
                                        void *stream) {
  return pipamd_batch_load_sparse_part(e, d_ws, d, s, 0, d ? d->batch : 0, stream);
}

extern "C" int pipamd_batch_dual_sparse_part(pipamd_engine *e, const void *d_ws, const pipamd_batch_desc *d, const pipamd_sparse *s,
                                             int first, int count, int64_t *d_dual_num, int64_t *d_dual_den, void *stream) {
  PipBatchSource src;
  int rc = sparse_check("batch_dual_sparse", e, d_ws, d, s, &src);
  return rc ? rc : dual_from("batch_dual_sparse", e, d_ws, d, &src, first, count, d_dual_num, d_dual_den, stream);
}

extern "C" int pipamd_batch_dual_sparse(pipamd_engine *e, const void *d_ws, const pipamd_batch_desc *d, const pipamd_sparse *s,
                                        int64_t *d_dual_num, int64_t *d_dual_den, void *stream) {
  return pipamd_batch_dual_sparse_part(e, d_ws, d, s, 0, d ? d->batch : 0, d_dual_num, d_dual_den, stream);
}

extern "C" int pipamd_batch_load_instances_part(pipamd_engine *e, void *d_ws, const pipamd_batch_desc *d, const pipamd_instances *in,
                                                int first, int count, void *stream) {
  PipBatchSource src;
  int rc = instances_check("batch_load_instances", e, d_ws, d, in, &src);
  return rc ? rc : load_from("batch_load_instances", e, d_ws, d, &src, first, count, stream);
}

extern "C" int pipamd_batch_load_instances(pipamd_engine *e, void *d_ws, const pipamd_batch_desc *d, const pipamd_instances *in,
                                           void *stream) {
  return pipamd_batch_load_instances_part(e, d_ws, d, in, 0, d ? d->batch : 0, stream);
}

extern "C" int pipamd_batch_dual_instances_part(pipamd_engine *e, const void *d_ws, const pipamd_batch_desc *d,
                                                const pipamd_instances *in, int first, int count, int64_t *d_dual_num,
                                                int64_t *d_dual_den, void *stream) {
  PipBatchSource src;
  int rc = instances_check("batch_dual_instances", e, d_ws, d, in, &src);
  return rc ? rc : dual_from("batch_dual_instances", e, d_ws, d, &src, first, count, d_dual_num, d_dual_den, stream);
}

extern "C" int pipamd_batch_dual_instances(pipamd_engine *e, const void *d_ws, const pipamd_batch_desc *d, const pipamd_instances *in,
                                           int64_t *d_dual_num, int64_t *d_dual_den, void *stream) {
  return pipamd_batch_dual_instances_part(e, d_ws, d, in, 0, d ? d->batch : 0, d_dual_num, d_dual_den, stream);
}

extern "C" int pipamd_batch_load_matrices_part(pipamd_engine *e, void *d_ws, const pipamd_batch_desc *d, const pipamd_matrices *m,
                                               const int64_t *d_rows, int first, int count, void *stream) {
  PipBatchSource src;
  int rc = matrices_check("batch_load_matrices", e, d_ws, d, m, d_rows, &src);
  return rc ? rc : load_from("batch_load_matrices", e, d_ws, d, &src, first, count, stream);
}

extern "C" int pipamd_batch_load_matrices(pipamd_engine *e, void *d_ws, const pipamd_batch_desc *d, const pipamd_matrices *m,
                                          const int64_t *d_rows, void *stream) {
  return pipamd_batch_load_matrices_part(e, d_ws, d, m, d_rows, 0, d ? d->batch : 0, stream);
}

extern "C" int pipamd_batch_dual_matrices_part(pipamd_engine *e, const void *d_ws, const pipamd_batch_desc *d,
                                               const pipamd_matrices *m, const int64_t *d_rows, int first, int count,
                                               int64_t *d_dual_num, int64_t *d_dual_den, void *stream) {
  PipBatchSource src;
  int rc = matrices_check("batch_dual_matrices", e, d_ws, d, m, d_rows, &src);
  return rc ? rc : dual_from("batch_dual_matrices", e, d_ws, d, &src, first, count, d_dual_num, d_dual_den, stream);
}

extern "C" int pipamd_batch_dual_matrices(pipamd_engine *e, const void *d_ws, const pipamd_batch_desc *d, const pipamd_matrices *m,
                                          const int64_t *d_rows, int64_t *d_dual_num, int64_t *d_dual_den, void *stream) {
  return pipamd_batch_dual_matrices_part(e, d_ws, d, m, d_rows, 0, d ? d->batch : 0, d_dual_num, d_dual_den, stream);
}

// ------------------------------------------------------------------ tapes at parameter points
// (header comment: include/piplib_amd.h; the program: pip_tape.h.)  One walk over the cells serves the check and the
// compile: it validates the grammar, counts, applies pip_solve's result edit if there is one (TapeEdit), and -- given a
// vector -- emits the program.  The walk keeps its own stack of
// items still to come (an IF pushes its two, a NEW the one behind it), so a deep tape costs heap, not the thread's stack.
static inline i128 tape_p1(const pipamd_sol_cell &c) { return c.param1; }
static inline i128 tape_p2(const pipamd_sol_cell &c) { return c.param2; }
static inline i128 tape_wide(int64_t lo, int64_t hi) { return (i128)(((unsigned __int128)(uint64_t)hi << 64) | (uint64_t)lo); }
static inline i128 tape_p1(const pipamd_sol_cell128 &c) { return tape_wide(c.param1_lo, c.param1_hi); }
static inline i128 tape_p2(const pipamd_sol_cell128 &c) { return tape_wide(c.param2_lo, c.param2_hi); }

// pip_solve's result edit (sol_vector_edit, sol.c:435-512) as the walk applies it.  Without one: no column is dropped.
struct TapeEdit {
  int bg = -1, urs = 0, first_urs = 0, nparm = 0;
  bool shift = false, negate = false, remove = false;
  int ndrop() const { return (remove ? 1 : 0) + urs; }
  // column j of a form is not kept: the big parameter's under SOL_REMOVE, the Urs_parms copies (j >= nparm: a new
  // parameter or the constant, always kept)
  bool dropped(int64_t j) const { return (remove && j == bg) || (first_urs <= j && j < first_urs + urs); }
};

template <class Cell>
struct TapeWalk {
  enum { EW = sizeof(Cell) == sizeof(pipamd_sol_cell) ? 1 : 2 };
  const Cell *cells;
  size_t n, pos = 0;
  std::vector<long long> *prog;  // null: check only
  long long words = 0;
  const char *why = nullptr;
  TapeEdit ed;
  bool toolarge = false;  // a shifted coefficient left the cell type

  bool fail(const char *w) {
    if (!why) why = w;
    return false;
  }
  void emit_word(long long w) {
    if (prog) prog->push_back(w);
    words++;
  }
  void emit(i128 v) {
    emit_word((long long)(uint64_t)(unsigned __int128)v);
    if (EW == 2) emit_word((long long)(uint64_t)((unsigned __int128)v >> 64));
  }
  const Cell *take(int kind, const char *w) {
    if (pos >= n || cells[pos].kind != kind) {
      fail(w);
      return nullptr;
    }
    return &cells[pos++];
  }
  // FORM(len) and its VALs: one positive denominator (1 if `one`); the numerators of the kept columns are emitted, *den
  // gets the denominator.  `unbounded` (a solution list's form): under SOL_SHIFT the big parameter's coefficient becomes
  // n - D before any drop, and *unbounded says whether that is not 0 (sol.c:479-483).
  bool form(int64_t len, bool one, i128 *den, const char *w, bool *unbounded = nullptr) {
    const Cell *f = take(PIPAMD_SOL_FORM, w);
    if (!f) return false;
    if (tape_p1(*f) != (i128)len) return fail(w);
    i128 d = 1;
    if (unbounded) *unbounded = false;
    for (int64_t j = 0; j < len; j++) {
      const Cell *v = take(PIPAMD_SOL_VAL, w);
      if (!v) return false;
      if (j == 0) d = tape_p2(*v);
      if (tape_p2(*v) != d || d <= 0 || (one && d != 1)) return fail(w);
      i128 n = tape_p1(*v);
      if (unbounded && ed.shift && j == ed.bg) {
        if (__builtin_sub_overflow(n, d, &n) || (EW == 1 && n != (i128)(int64_t)n)) toolarge = true;
        if (n != 0) *unbounded = true;
      }
      if (j < ed.nparm && ed.dropped(j)) continue;
      emit(n);
    }
    *den = d;
    return true;
  }
};

static unsigned __int128 tape_gcd(unsigned __int128 x, unsigned __int128 y) {
  while (y) {
    const unsigned __int128 r = x % y;
    x = y;
    y = r;
  }
  return x;
}

template <class Cell>
static int tape_walk(const char *who, const Cell *cells, size_t n_cells, const pipamd_tape_shape *sh,
                     const pipamd_tape_edit *edit, pipamd_tape_info *info, std::vector<long long> *prog) {
  if (!sh || (!cells && n_cells > 0)) {
    pipamd_set_error("%s: null shape, or null cells with n_cells > 0", who);
    return PIPAMD_E_INVALID;
  }
  if (sh->nvar < 0 || sh->nparm < 0 || sh->ndual < 0 || sh->reserved != 0) {
    pipamd_set_error("%s: negative count (nvar %d, nparm %d, ndual %d) or reserved (%d) not 0", who, sh->nvar, sh->nparm,
                     sh->ndual, sh->reserved);
    return PIPAMD_E_INVALID;
  }
  enum { EW = TapeWalk<Cell>::EW };
  TapeWalk<Cell> w{cells, n_cells};
  w.prog = prog;
  // (an edit of all zeros is no edit: bg 0 without a flag and without Urs_parms changes nothing)
  if (edit && (edit->sol_bg || edit->urs_parms || edit->sol_flags || edit->reserved)) {
    const int bg = edit->sol_bg, U = edit->urs_parms, fl = edit->sol_flags;
    const int64_t first_urs = (int64_t)U + (bg >= 0);
    const bool rm = (fl & PIPAMD_SOL_REMOVE) != 0;
    // (any negative sol_bg is "no big parameter", as sol_vector_edit reads it: pipamd_pip_info has Bg - Nn - 1 there)
    if (edit->reserved != 0 || (fl & ~15) || U < 0 || bg >= sh->nparm ||
        ((fl & (PIPAMD_SOL_SHIFT | PIPAMD_SOL_REMOVE)) && bg < 0) || first_urs + U > sh->nparm ||
        (rm && U > 0 && bg >= first_urs && bg < first_urs + U)) {
      pipamd_set_error("%s: edit (sol_bg %d, urs_parms %d, sol_flags %d, reserved %d) does not fit nparm %d", who, bg, U, fl,
                       edit->reserved, sh->nparm);
      return PIPAMD_E_INVALID;
    }
    w.ed.bg = bg;
    w.ed.urs = U;
    w.ed.first_urs = (int)first_urs;
    w.ed.nparm = sh->nparm;
    w.ed.shift = (fl & PIPAMD_SOL_SHIFT) != 0;
    w.ed.negate = (fl & PIPAMD_SOL_NEGATE) != 0;
    w.ed.remove = rm;
  }
  const int ndrop = w.ed.ndrop();  // P of the cells counts every column; slots and headers count the kept ones
  struct Todo {
    int64_t P;
    int64_t depth;
    long long patch;  // word of the IF header whose else item this is, or -1
  };
  std::vector<Todo> todo;
  pipamd_tape_info I;
  memset(&I, 0, sizeof I);
  int64_t slots = (int64_t)sh->nparm - ndrop + 1, depth = 0;
  if (n_cells) todo.push_back({sh->nparm, 1, -1});
  bool ok = true;
  while (ok && !todo.empty()) {
    const Todo t = todo.back();
    todo.pop_back();
    const int64_t P = t.P;
    if (t.patch >= 0 && prog) (*prog)[t.patch] |= w.words << 32;
    if (P - ndrop + 1 > slots) slots = P - ndrop + 1;
    if (t.depth > depth) depth = t.depth;
    if (w.pos >= w.n) {
      ok = w.fail("truncated: an item is missing");
      break;
    }
    // (P beyond the limit: the walk goes on to tell an invalid tape from a large one, but emits headers of a fixed P)
    const int hp = P - ndrop < TAPE_MAX_SLOTS ? (int)(P - ndrop) : TAPE_MAX_SLOTS;
    const Cell &c = cells[w.pos++];
    i128 den;
    switch (c.kind) {
      case PIPAMD_SOL_NEW: {
        if (tape_p1(c) != (i128)P) {
          ok = w.fail("newparm whose number is not the count of parameters in scope");
          break;
        }
        w.emit_word(tape_header(TAPE_NEW, hp, 0));
        const Cell *d = w.take(PIPAMD_SOL_DIV, "no div behind a newparm");
        if (!d) {
          ok = false;
          break;
        }
        // the program has the divisor in front of the form: it is looked up behind the form's cells first
        const size_t at = w.pos + (size_t)P + 2;
        if (at >= w.n || cells[at].kind != PIPAMD_SOL_VAL || tape_p2(cells[at]) != 1 || tape_p1(cells[at]) <= 0) {
          ok = w.fail("div: truncated, or a divisor that is not a positive integer");
          break;
        }
        w.emit(tape_p1(cells[at]));
        ok = w.form(P + 1, true, &den, "div: a form of P + 1 integers is expected");
        if (!ok) break;
        w.pos++;  // the divisor
        I.news++;
        todo.push_back({P + 1, t.depth + 1, -1});
        break;
      }
      case PIPAMD_SOL_IF: {
        const long long at = w.words;
        w.emit_word(tape_header(TAPE_IF, hp, 0));
        ok = w.form(P + 1, false, &den, "if: a form of P + 1 values over one positive denominator is expected");
        if (!ok) break;
        I.ifs++;
        todo.push_back({P, t.depth + 1, at});
        todo.push_back({P, t.depth + 1, -1});
        break;
      }
      case PIPAMD_SOL_LIST: {
        if (tape_p1(c) != (i128)sh->nvar) {
          ok = w.fail("a solution list whose length is not nvar");
          break;
        }
        w.emit_word(tape_header(TAPE_LEAF, hp, I.leaves) | (w.ed.negate ? TAPE_LEAF_NEGATE : 0));
        for (int i = 0; ok && i < sh->nvar; i++) {
          // the denominator goes in front of its numerators: a place is kept, the form emitted, the place filled --
          // negated for an unbounded unknown (pip_tape.h)
          const size_t at = prog ? prog->size() : 0;
          bool unbounded = false;
          w.emit(0);
          ok = w.form(P + 1, false, &den, "list: forms of P + 1 values over one positive denominator are expected", &unbounded);
          if (unbounded) den = -den;
          if (ok && prog) {
            (*prog)[at] = (long long)(uint64_t)(unsigned __int128)den;
            if (EW == 2) (*prog)[at + 1] = (long long)(uint64_t)((unsigned __int128)den >> 64);
          }
        }
        if (!ok) break;
        if (sh->ndual > 0) {
          const Cell *l = w.take(PIPAMD_SOL_LIST, "no dual list behind a solution list");
          if (!l || tape_p1(*l) != (i128)sh->ndual) {
            ok = w.fail("a dual list whose length is not ndual");
            break;
          }
          for (int i = 0; ok && i < sh->ndual; i++) {
            const Cell *f = w.take(PIPAMD_SOL_FORM, "dual list: forms of one value are expected");
            const Cell *v = f && tape_p1(*f) == 1 ? w.take(PIPAMD_SOL_VAL, "dual list: forms of one value are expected") : nullptr;
            if (!v || tape_p2(*v) <= 0) {
              ok = w.fail("dual list: forms of one value over a positive denominator are expected");
              break;
            }
            const i128 num = tape_p1(*v), dd = tape_p2(*v);
            const unsigned __int128 mag = num < 0 ? (unsigned __int128)0 - (unsigned __int128)num : (unsigned __int128)num;
            const unsigned __int128 g = tape_gcd(mag, (unsigned __int128)dd);
            const unsigned __int128 q = mag / g;
            w.emit(num < 0 ? (i128)((unsigned __int128)0 - q) : (i128)q);
            w.emit((i128)((unsigned __int128)dd / g));
          }
          if (!ok) break;
        }
        I.leaves++;
        break;
      }
      case PIPAMD_SOL_NIL:
        w.emit_word(tape_header(TAPE_NIL, hp, I.leaves));
        I.leaves++;
        break;
      default:
        ok = w.fail("a cell of a kind that cannot start an item");
    }
    if (w.words >= (1ll << 31)) break;
  }
  if (ok && w.words < (1ll << 31) && w.pos != w.n) ok = w.fail("cells behind the end of the root item");
  if (!ok) {
    pipamd_set_error("%s: cell %zu of %zu: %s", who, w.pos, n_cells, w.why ? w.why : "invalid tape");
    return PIPAMD_E_INVALID;
  }
  if (slots > TAPE_MAX_SLOTS || w.words >= (1ll << 31)) {
    pipamd_set_error("%s: %lld slots (at most %d), or a program of 2^31 words or more", who, (long long)slots, TAPE_MAX_SLOTS);
    return PIPAMD_E_TOOLARGE;
  }
  if (w.toolarge) {
    pipamd_set_error("%s: a big parameter's coefficient minus its denominator (SOL_SHIFT) does not fit the cell type", who);
    return PIPAMD_E_TOOLARGE;
  }
  I.words = w.words;
  I.slots = (int32_t)slots;
  I.depth = (int32_t)depth;
  const int bits = 64 * EW;
  I.staged = n_cells > 0 && 8 * (size_t)w.words + tape_slot_bytes(I.slots, bits) <= (size_t)TAPE_LDS_BYTES;
  if (info) *info = I;
  return PIPAMD_OK;
}

struct pipamd_tape {
  int device, bits;
  pipamd_tape_shape shape;
  pipamd_tape_info info;
  int point_cols;     // values of a point: shape.nparm less the columns an edit drops
  int marks;          // the program holds a mark of an edit (pip_tape.h)
  long long *d_prog;
  long long *h_prog;  // the same words on the host, for pipamd_tape_set_create
};

extern "C" int pipamd_tape_check(const pipamd_sol_cell *cells, size_t n_cells, const pipamd_tape_shape *shape,
                                 pipamd_tape_info *info) {
  return tape_walk("tape_check", cells, n_cells, shape, nullptr, info, nullptr);
}
extern "C" int pipamd_tape_check128(const pipamd_sol_cell128 *cells, size_t n_cells, const pipamd_tape_shape *shape,
                                    pipamd_tape_info *info) {
  return tape_walk("tape_check128", cells, n_cells, shape, nullptr, info, nullptr);
}
extern "C" int pipamd_tape_check_pip(const pipamd_sol_cell *cells, size_t n_cells, const pipamd_tape_shape *shape,
                                     const pipamd_tape_edit *edit, pipamd_tape_info *info) {
  return tape_walk("tape_check_pip", cells, n_cells, shape, edit, info, nullptr);
}
extern "C" int pipamd_tape_check_pip128(const pipamd_sol_cell128 *cells, size_t n_cells, const pipamd_tape_shape *shape,
                                        const pipamd_tape_edit *edit, pipamd_tape_info *info) {
  return tape_walk("tape_check_pip128", cells, n_cells, shape, edit, info, nullptr);
}

// The promise to the kernel, held against `words` words themselves (a program, or a tape's part of a set's buffer that
// starts at word `base`): known operations, the negate mark on leaves alone, no denominator of 0, every else target
// behind its IF and inside these words, and a node behind every NEW and IF.  -1, or the first word that breaks it.
static long long tape_program_breach(const long long *prog, long long base, long long words, int ew, int nvar, int ndual,
                                     int slots, bool *marks = nullptr) {
  for (long long pc = 0; pc < words;) {
    const long long hdr = prog[base + pc];
    const int op = (int)(hdr & 0xff), P = (int)((hdr >> 8) & 0xffff), mark = (int)((hdr >> 24) & 0xff);
    const long long aux = (hdr >> 32) - base;
    long long len = 1;
    if (op == TAPE_NEW) len += ew * (P + 2);
    else if (op == TAPE_IF) len += ew * (P + 1);
    else if (op == TAPE_LEAF) len += ew * ((long long)nvar * (P + 2) + 2ll * ndual);
    if ((op != TAPE_NEW && op != TAPE_IF && op != TAPE_LEAF && op != TAPE_NIL) || hdr < 0 || P + 1 > slots || pc + len > words ||
        (op == TAPE_LEAF ? mark > 1 : mark != 0) || (op == TAPE_IF && (aux < pc + len || aux >= words)) ||
        ((op == TAPE_NEW || op == TAPE_IF) && pc + len >= words))
      return pc;
    if (op == TAPE_LEAF)
      for (int i = 0; i < nvar; i++) {
        const long long *d = prog + base + pc + 1 + (long long)i * ew * (P + 2);
        if (d[0] == 0 && (ew == 1 || d[1] == 0)) return pc;
        if (marks && (mark || d[ew - 1] < 0)) *marks = true;  // (what the kernel looks for: pip_tape.h)
      }
    pc += len;
  }
  return -1;
}

template <class Cell>
static int tape_compile(const char *who, pipamd_engine *e, const Cell *cells, size_t n_cells, const pipamd_tape_shape *shape,
                        const pipamd_tape_edit *edit, pipamd_tape **out) {
  if (!e || !out) {
    pipamd_set_error("%s: null engine or result pointer", who);
    return PIPAMD_E_INVALID;
  }
  *out = nullptr;
  pipamd_tape_info info;
  int rc = tape_walk(who, cells, n_cells, shape, edit, &info, nullptr);
  if (rc) return rc;
  std::vector<long long> prog;
  prog.reserve((size_t)info.words);
  rc = tape_walk(who, cells, n_cells, shape, edit, &info, &prog);
  if (rc) return rc;
  if ((long long)prog.size() != info.words) {
    pipamd_set_error("%s: internal: %zu words emitted, %lld counted", who, prog.size(), (long long)info.words);
    return PIPAMD_E_INVALID;
  }
  const int ew = sizeof(Cell) == sizeof(pipamd_sol_cell) ? 1 : 2;
  bool marks = false;
  const long long breach = tape_program_breach(prog.data(), 0, info.words, ew, shape->nvar, shape->ndual, info.slots, &marks);
  if (breach >= 0) {
    pipamd_set_error("%s: internal: word %lld of the program breaks the kernel's contract", who, breach);
    return PIPAMD_E_INVALID;
  }
  // (the walk accepted the edit: the columns it drops are distinct and inside nparm)
  int ndrop = 0;
  if (edit) ndrop = ((edit->sol_flags & PIPAMD_SOL_REMOVE) ? 1 : 0) + edit->urs_parms;
  if (hipSetDevice(e->device) != hipSuccess) return PIPAMD_E_HIP;
  pipamd_tape *t = (pipamd_tape *)calloc(1, sizeof *t);
  if (!t) return PIPAMD_E_NOMEM;
  t->device = e->device;
  t->bits = sizeof(Cell) == sizeof(pipamd_sol_cell) ? 64 : 128;
  t->shape = *shape;
  t->info = info;
  t->point_cols = shape->nparm - ndrop;
  t->marks = marks ? 1 : 0;
  if (info.words) {
    t->h_prog = (long long *)malloc((size_t)info.words * 8);
    if (!t->h_prog) {
      free(t);
      return PIPAMD_E_NOMEM;
    }
    memcpy(t->h_prog, prog.data(), (size_t)info.words * 8);
    hipError_t he = hipMalloc((void **)&t->d_prog, (size_t)info.words * 8);
    if (he == hipSuccess) he = hipMemcpy(t->d_prog, prog.data(), (size_t)info.words * 8, hipMemcpyHostToDevice);
    if (he != hipSuccess) {
      pipamd_set_error("%s: the program's %lld words on the device: %s", who, (long long)info.words, hipGetErrorString(he));
      if (t->d_prog) hipFree(t->d_prog);
      free(t->h_prog);
      free(t);
      return PIPAMD_E_HIP;
    }
  }
  *out = t;
  return PIPAMD_OK;
}

extern "C" int pipamd_tape_compile(pipamd_engine *e, const pipamd_sol_cell *cells, size_t n_cells, const pipamd_tape_shape *shape,
                                   pipamd_tape **out) {
  return tape_compile("tape_compile", e, cells, n_cells, shape, nullptr, out);
}
extern "C" int pipamd_tape_compile128(pipamd_engine *e, const pipamd_sol_cell128 *cells, size_t n_cells,
                                      const pipamd_tape_shape *shape, pipamd_tape **out) {
  return tape_compile("tape_compile128", e, cells, n_cells, shape, nullptr, out);
}
extern "C" int pipamd_tape_compile_pip(pipamd_engine *e, const pipamd_sol_cell *cells, size_t n_cells,
                                       const pipamd_tape_shape *shape, const pipamd_tape_edit *edit, pipamd_tape **out) {
  return tape_compile("tape_compile_pip", e, cells, n_cells, shape, edit, out);
}
extern "C" int pipamd_tape_compile_pip128(pipamd_engine *e, const pipamd_sol_cell128 *cells, size_t n_cells,
                                          const pipamd_tape_shape *shape, const pipamd_tape_edit *edit, pipamd_tape **out) {
  return tape_compile("tape_compile_pip128", e, cells, n_cells, shape, edit, out);
}
extern "C" int pipamd_tape_point_cols(const pipamd_tape *t) { return t ? t->point_cols : PIPAMD_E_INVALID; }

extern "C" void pipamd_tape_free(pipamd_tape *t) {
  if (!t) return;
  if (t->d_prog && hipSetDevice(t->device) == hipSuccess) hipFree(t->d_prog);
  free(t->h_prog);
  free(t);
}

// Testing aid: the words of a compiled tape's program, copied back from its device (tests hold them unchanged by
// evaluations).  host_out may be NULL to ask for the count alone; the copy waits for the device.
extern "C" int pipamd_debug_tape_program(const pipamd_tape *t, int64_t *host_out, int64_t cap, int64_t *words) {
  if (!t || !words || (host_out && cap < t->info.words)) return PIPAMD_E_INVALID;
  *words = t->info.words;
  if (host_out && t->info.words) {
    if (hipSetDevice(t->device) != hipSuccess) return PIPAMD_E_HIP;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(host_out, t->d_prog, (size_t)t->info.words * 8, hipMemcpyDeviceToHost));
  }
  return PIPAMD_OK;
}

extern "C" int pipamd_tape_eval(pipamd_engine *e, const pipamd_tape *t, int64_t n_points, const int64_t *d_points,
                                int32_t *d_status, int32_t *d_leaf, int64_t *d_x_num, int64_t *d_x_den, int64_t *d_dual_num,
                                int64_t *d_dual_den, void *stream) {
  if (!e || !t || n_points < 0 || t->device != e->device || (n_points > 0 && t->point_cols > 0 && !d_points)) {
    pipamd_set_error("tape_eval: null engine or tape, a tape of another device, n_points < 0, or parameters without points");
    return PIPAMD_E_INVALID;
  }
  if (n_points >= (1ll << 38)) {
    pipamd_set_error("tape_eval: %lld points, at most 2^38 - 1 a call", (long long)n_points);
    return PIPAMD_E_TOOLARGE;
  }
  if (n_points == 0) return PIPAMD_OK;
  if (hipSetDevice(e->device) != hipSuccess) return PIPAMD_E_HIP;
  TapeLaunch L;
  L.prog = t->d_prog;
  L.words = t->info.words;
  L.bits = t->bits;
  L.staged = t->info.staged;
  L.marks = t->marks;
  L.nvar = t->shape.nvar;
  L.nparm = t->point_cols;
  L.ndual = t->shape.ndual;
  L.slots = t->info.slots;
  L.n_points = n_points;
  L.points = (const long long *)d_points;
  L.status = d_status;
  L.leaf = d_leaf;
  L.x_num = d_x_num;
  L.x_den = d_x_den;
  L.dual_num = d_dual_num;
  L.dual_den = d_dual_den;
  HIPCHK(pipk_launch_tape_eval(&L, (hipStream_t)stream));
  return PIPAMD_OK;
}

// ------------------------------------------------------------------ a tape swept over a box of points
// The box's arithmetic, shared by the planner and the sweep: extents and their product, formed without wrapping.
static int tape_sweep_box(const char *who, int point_cols, const int64_t *lo, const int64_t *hi, unsigned long long *ext,
                          int64_t *n_points) {
  if (point_cols < 0 || point_cols > TAPE_MAX_SLOTS - 1 || (point_cols > 0 && (!lo || !hi))) {
    pipamd_set_error("%s: %d point columns (0 .. %d), or a box without bounds", who, point_cols, TAPE_MAX_SLOTS - 1);
    return PIPAMD_E_INVALID;
  }
  for (int c = 0; c < point_cols; c++)
    if (lo[c] > hi[c]) {
      pipamd_set_error("%s: column %d: lo %lld above hi %lld", who, c, (long long)lo[c], (long long)hi[c]);
      return PIPAMD_E_INVALID;
    }
  unsigned __int128 n = 1;  // (stays below 2^38 * 2^64)
  for (int c = 0; c < point_cols; c++) {
    // hi - lo in unsigned arithmetic is exact; + 1 wraps to 0 for the full range alone
    const unsigned long long span = (unsigned long long)hi[c] - (unsigned long long)lo[c];
    n *= (unsigned __int128)span + 1;
    if (n >= ((unsigned __int128)1 << 38)) {
      pipamd_set_error("%s: the box has 2^38 points or more (at most 2^38 - 1 a call)", who);
      return PIPAMD_E_TOOLARGE;
    }
    if (ext) ext[c] = span + 1;
  }
  *n_points = (int64_t)n;
  return PIPAMD_OK;
}

extern "C" int pipamd_tape_sweep_plan(const pipamd_tape_info *info, int bits, int point_cols, const int64_t *lo,
                                      const int64_t *hi, struct pipamd_tape_sweep_plan *plan) {
  if (!info || !plan || (bits != 64 && bits != 128)) {
    pipamd_set_error("tape_sweep_plan: null info or plan, or bits other than 64 and 128");
    return PIPAMD_E_INVALID;
  }
  int64_t n = 0;
  const int rc = tape_sweep_box("tape_sweep_plan", point_cols, lo, hi, nullptr, &n);
  if (rc) return rc;
  plan->n_points = n;
  plan->summary_words = PIPAMD_SWEEP_WORDS(info->leaves);
  const unsigned __int128 lds = (unsigned __int128)tape_slot_bytes(info->slots > 0 ? info->slots : 1, bits) +
                                (info->staged ? (unsigned __int128)8 * (unsigned long long)info->words : 0) +
                                (unsigned __int128)16 * ((unsigned long long)info->leaves + 4);
  plan->binned = info->leaves >= 0 && lds <= (unsigned __int128)TAPE_LDS_BYTES;
  plan->reserved = 0;
  return PIPAMD_OK;
}

static int g_tape_sweep_blocks;  // pipamd_debug_tape_sweep_blocks
// Testing aid: at most n workgroups for the sweeps that follow (0: the default bound), so that small boxes drive the
// kernel's grid-stride loop.
extern "C" int pipamd_debug_tape_sweep_blocks(int n) {
  if (n < 0) return PIPAMD_E_INVALID;
  g_tape_sweep_blocks = n;
  return PIPAMD_OK;
}

// The context's rows as the sweeps take them: none, or an array of point_cols + 2 columns
static inline bool tape_ctx_ok(int n_ctx, int ctx_cols, const int64_t *d_ctx, int point_cols) {
  return n_ctx >= 0 && (n_ctx == 0 || (d_ctx && ctx_cols == point_cols + 2));
}

extern "C" int pipamd_tape_sweep(pipamd_engine *e, const pipamd_tape *t, const int64_t *lo, const int64_t *hi, int n_ctx,
                                 int ctx_cols, const int64_t *d_ctx, int64_t *d_summary, int32_t *d_status, int32_t *d_leaf,
                                 int64_t *d_x_num, int64_t *d_x_den, int64_t *d_dual_num, int64_t *d_dual_den, void *stream) {
  if (!e || !t || t->device != e->device || !tape_ctx_ok(n_ctx, ctx_cols, d_ctx, t->point_cols)) {
    pipamd_set_error("tape_sweep: null engine or tape, a tape of another device, n_ctx < 0, or context rows without an "
                     "array of point_cols + 2 columns");
    return PIPAMD_E_INVALID;
  }
  TapeSweepLaunch L;
  memset(&L, 0, sizeof L);
  struct pipamd_tape_sweep_plan plan;
  int rc = tape_sweep_box("tape_sweep", t->point_cols, lo, hi, L.ext, &plan.n_points);
  if (rc) return rc;
  rc = pipamd_tape_sweep_plan(&t->info, t->bits, t->point_cols, lo, hi, &plan);
  if (rc) return rc;
  if (hipSetDevice(e->device) != hipSuccess) return PIPAMD_E_HIP;
  L.t.prog = t->d_prog;
  L.t.words = t->info.words;
  L.t.bits = t->bits;
  L.t.staged = t->info.staged;
  L.t.marks = t->marks;
  L.t.nvar = t->shape.nvar;
  L.t.nparm = t->point_cols;
  L.t.ndual = t->shape.ndual;
  L.t.slots = t->info.slots;
  L.t.n_points = plan.n_points;
  L.t.status = d_status;
  L.t.leaf = d_leaf;
  L.t.x_num = d_x_num;
  L.t.x_den = d_x_den;
  L.t.dual_num = d_dual_num;
  L.t.dual_den = d_dual_den;
  L.n_ctx = n_ctx;
  L.ctx = (const long long *)d_ctx;
  L.summary = (long long *)d_summary;
  L.leaves = t->info.leaves;
  L.binned = plan.binned;
  for (int c = 0; c < t->point_cols; c++) L.lo[c] = lo[c];
  L.cus = e->cus;
  L.max_blocks = g_tape_sweep_blocks;
  HIPCHK(pipk_launch_tape_sweep(&L, (hipStream_t)stream));
  return PIPAMD_OK;
}

// ------------------------------------------------------------------ a sweep's values reduced per unknown
// The planner's work for `who`: the refusals, the box (its extents into `ext` where that is not NULL) and the plan
static int tape_values_plan(const char *who, const pipamd_tape_info *info, int bits, int nvar, int point_cols, const int64_t *lo,
                            const int64_t *hi, unsigned long long *ext, struct pipamd_tape_values_plan *plan) {
  if (!info || !plan || (bits != 64 && bits != 128) || nvar < 0) {
    pipamd_set_error("%s: null info or plan, bits other than 64 and 128, or nvar < 0", who);
    return PIPAMD_E_INVALID;
  }
  int64_t n = 0;
  const int rc = tape_sweep_box(who, point_cols, lo, hi, ext, &n);
  if (rc) return rc;
  if (nvar > PIPAMD_VALUES_MAX_NVAR) {
    pipamd_set_error("%s: %d unknowns, at most %d (a lane of a wave keeps one unknown's record)", who, nvar, PIPAMD_VALUES_MAX_NVAR);
    return PIPAMD_E_TOOLARGE;
  }
  plan->n_points = n;
  plan->summary_words = PIPAMD_VALUES_WORDS(nvar);
  plan->work_bytes = (int64_t)tape_values_work_bytes(n, nvar);
  // (the reduction keeps its accumulators in registers: beside the slots the program alone asks for LDS)
  const unsigned __int128 lds = (unsigned __int128)tape_slot_bytes(info->slots > 0 ? info->slots : 1, bits) +
                                (unsigned __int128)8 * (unsigned long long)info->words;
  plan->staged = info->staged && info->words > 0 && lds <= (unsigned __int128)TAPE_LDS_BYTES;
  plan->reserved = 0;
  return PIPAMD_OK;
}

extern "C" int pipamd_tape_sweep_values_plan(const pipamd_tape_info *info, int bits, int nvar, int point_cols,
                                             const int64_t *lo, const int64_t *hi, struct pipamd_tape_values_plan *plan) {
  return tape_values_plan("tape_sweep_values_plan", info, bits, nvar, point_cols, lo, hi, nullptr, plan);
}

extern "C" int pipamd_tape_sweep_values(pipamd_engine *e, const pipamd_tape *t, const int64_t *lo, const int64_t *hi, int n_ctx,
                                        int ctx_cols, const int64_t *d_ctx, int64_t *d_summary, void *d_work, size_t work_bytes,
                                        void *stream) {
  if (!e || !t || t->device != e->device || !tape_ctx_ok(n_ctx, ctx_cols, d_ctx, t->point_cols) || !d_summary || !d_work ||
      ((uintptr_t)d_work & 7)) {
    pipamd_set_error("tape_sweep_values: null engine, tape, summary or work buffer, a work buffer that is not 8-byte aligned, "
                     "a tape of another device, n_ctx < 0, or context rows without an array of point_cols + 2 columns");
    return PIPAMD_E_INVALID;
  }
  TapeValuesLaunch L;
  memset(&L, 0, sizeof L);
  struct pipamd_tape_values_plan plan;
  const int rc = tape_values_plan("tape_sweep_values", &t->info, t->bits, t->shape.nvar, t->point_cols, lo, hi, L.ext, &plan);
  if (rc) return rc;
  if ((unsigned __int128)work_bytes < (unsigned __int128)plan.work_bytes) {
    pipamd_set_error("tape_sweep_values: a work buffer of %zu bytes, the plan asks for %lld", work_bytes, (long long)plan.work_bytes);
    return PIPAMD_E_INVALID;
  }
  if (hipSetDevice(e->device) != hipSuccess) return PIPAMD_E_HIP;
  L.t.prog = t->d_prog;
  L.t.words = t->info.words;
  L.t.bits = t->bits;
  L.t.staged = plan.staged;
  L.t.marks = t->marks;
  L.t.nvar = t->shape.nvar;
  L.t.nparm = t->point_cols;
  L.t.slots = t->info.slots;
  L.t.n_points = plan.n_points;
  L.n_ctx = n_ctx;
  L.ctx = (const long long *)d_ctx;
  L.summary = (long long *)d_summary;
  L.work = (long long *)d_work;
  for (int c = 0; c < t->point_cols; c++) L.lo[c] = lo[c];
  L.cus = e->cus;
  L.max_blocks = g_tape_sweep_blocks;
  HIPCHK(pipk_launch_tape_values(&L, (hipStream_t)stream));
  return PIPAMD_OK;
}

// ------------------------------------------------------------------ two tapes compared point by point
// The LDS of a pair: both slot areas must fit (TOOLARGE otherwise); staged: both programs fit beside them too.
static int tape_compare_lds(const char *who, const pipamd_tape_info *a, int bits_a, const pipamd_tape_info *b, int bits_b,
                            int *staged) {
  if (!a || !b || (bits_a != 64 && bits_a != 128) || (bits_b != 64 && bits_b != 128)) {
    pipamd_set_error("%s: null info, or bits other than 64 and 128", who);
    return PIPAMD_E_INVALID;
  }
  const unsigned __int128 slots = (unsigned __int128)tape_slot_bytes(a->slots > 0 ? a->slots : 1, bits_a) +
                                  (unsigned __int128)tape_slot_bytes(b->slots > 0 ? b->slots : 1, bits_b);
  if (slots > (unsigned __int128)TAPE_LDS_BYTES) {
    pipamd_set_error("%s: %d slots of %d bits and %d slots of %d bits: the two slot areas exceed %d bytes of LDS", who,
                     a->slots, bits_a, b->slots, bits_b, TAPE_LDS_BYTES);
    return PIPAMD_E_TOOLARGE;
  }
  *staged = a->words >= 0 && b->words >= 0 &&
            slots + (unsigned __int128)8 * ((unsigned __int128)a->words + (unsigned __int128)b->words) <= (unsigned __int128)TAPE_LDS_BYTES;
  return PIPAMD_OK;
}

extern "C" int pipamd_tape_compare_plan(const pipamd_tape_info *a, int bits_a, const pipamd_tape_info *b, int bits_b,
                                        int point_cols, const int64_t *lo, const int64_t *hi,
                                        struct pipamd_tape_compare_plan *plan) {
  if (!plan) {
    pipamd_set_error("tape_compare_plan: null plan");
    return PIPAMD_E_INVALID;
  }
  int staged = 0;
  int rc = tape_compare_lds("tape_compare_plan", a, bits_a, b, bits_b, &staged);
  if (rc == PIPAMD_E_INVALID) return rc;
  int64_t n = 0;
  const int rb = tape_sweep_box("tape_compare_plan", point_cols, lo, hi, nullptr, &n);
  if (rb) return rb;
  if (rc) return tape_compare_lds("tape_compare_plan", a, bits_a, b, bits_b, &staged);  // (its message again)
  plan->n_points = n;
  plan->staged = staged;
  plan->reserved = 0;
  return PIPAMD_OK;
}

// What both entries refuse of their handles and flags, then the pair's part of the launch
static int tape_compare_pair(const char *who, pipamd_engine *e, const pipamd_tape *a, const pipamd_tape *b, int flags,
                             TapeCompareLaunch *L) {
  if (flags & ~PIPAMD_CMP_DUAL) {
    pipamd_set_error("%s: unknown flag bits in %d", who, flags);
    return PIPAMD_E_INVALID;
  }
  if (!e || !a || !b || a->device != e->device || b->device != e->device) {
    pipamd_set_error("%s: null engine or tape, or a tape of another device than the engine's", who);
    return PIPAMD_E_INVALID;
  }
  if (a->shape.nvar != b->shape.nvar || a->point_cols != b->point_cols ||
      ((flags & PIPAMD_CMP_DUAL) && a->shape.ndual != b->shape.ndual)) {
    pipamd_set_error("%s: the tapes differ in nvar (%d, %d), in point columns (%d, %d) or -- PIPAMD_CMP_DUAL -- in ndual (%d, %d)",
                     who, a->shape.nvar, b->shape.nvar, a->point_cols, b->point_cols, a->shape.ndual, b->shape.ndual);
    return PIPAMD_E_INVALID;
  }
  memset(L, 0, sizeof *L);
  L->prog_a = a->d_prog, L->prog_b = b->d_prog;
  L->words_a = a->info.words, L->words_b = b->info.words;
  L->bits_a = a->bits, L->bits_b = b->bits;
  L->slots_a = a->info.slots, L->slots_b = b->info.slots;
  L->nvar = a->shape.nvar;
  L->nparm = a->point_cols;
  L->ndual = (flags & PIPAMD_CMP_DUAL) ? a->shape.ndual : 0;
  L->cus = e->cus;
  return PIPAMD_OK;
}

extern "C" int pipamd_tape_compare(pipamd_engine *e, const pipamd_tape *a, const pipamd_tape *b, int flags, int64_t n_points,
                                   const int64_t *d_points, int64_t *d_summary, int32_t *d_class, int32_t *d_where,
                                   int32_t *d_status_a, int32_t *d_status_b, void *stream) {
  TapeCompareLaunch L;
  int rc = tape_compare_pair("tape_compare", e, a, b, flags, &L);
  if (rc) return rc;
  if (n_points < 0 || (n_points > 0 && a->point_cols > 0 && !d_points)) {
    pipamd_set_error("tape_compare: n_points < 0, or parameters without points");
    return PIPAMD_E_INVALID;
  }
  if (n_points >= (1ll << 38)) {
    pipamd_set_error("tape_compare: %lld points, at most 2^38 - 1 a call", (long long)n_points);
    return PIPAMD_E_TOOLARGE;
  }
  rc = tape_compare_lds("tape_compare", &a->info, a->bits, &b->info, b->bits, &L.staged);
  if (rc) return rc;
  if (n_points == 0 && !d_summary) return PIPAMD_OK;
  if (hipSetDevice(e->device) != hipSuccess) return PIPAMD_E_HIP;
  L.n_points = n_points;
  L.points = (const long long *)d_points;
  L.summary = (long long *)d_summary;
  L.cls = d_class, L.where = d_where, L.status_a = d_status_a, L.status_b = d_status_b;
  HIPCHK(pipk_launch_tape_compare(&L, (hipStream_t)stream));
  return PIPAMD_OK;
}

extern "C" int pipamd_tape_compare_sweep(pipamd_engine *e, const pipamd_tape *a, const pipamd_tape *b, int flags,
                                         const int64_t *lo, const int64_t *hi, int n_ctx, int ctx_cols, const int64_t *d_ctx,
                                         int64_t *d_summary, int32_t *d_class, int32_t *d_where, int32_t *d_status_a,
                                         int32_t *d_status_b, void *stream) {
  TapeCompareLaunch L;
  int rc = tape_compare_pair("tape_compare_sweep", e, a, b, flags, &L);
  if (rc) return rc;
  if (!tape_ctx_ok(n_ctx, ctx_cols, d_ctx, a->point_cols)) {
    pipamd_set_error("tape_compare_sweep: n_ctx < 0, or context rows without an array of point_cols + 2 columns");
    return PIPAMD_E_INVALID;
  }
  int64_t n = 0;
  rc = tape_sweep_box("tape_compare_sweep", a->point_cols, lo, hi, L.ext, &n);
  if (rc) return rc;
  rc = tape_compare_lds("tape_compare_sweep", &a->info, a->bits, &b->info, b->bits, &L.staged);
  if (rc) return rc;
  if (hipSetDevice(e->device) != hipSuccess) return PIPAMD_E_HIP;
  L.box = 1;
  L.n_points = n;
  for (int c = 0; c < a->point_cols; c++) L.lo[c] = lo[c];
  L.n_ctx = n_ctx;
  L.ctx = (const long long *)d_ctx;
  L.max_blocks = g_tape_sweep_blocks;
  L.summary = (long long *)d_summary;
  L.cls = d_class, L.where = d_where, L.status_a = d_status_a, L.status_b = d_status_b;
  HIPCHK(pipk_launch_tape_compare(&L, (hipStream_t)stream));
  return PIPAMD_OK;
}

// ------------------------------------------------------------------ a set of tapes in one launch
struct pipamd_tape_set {
  int device, bits;
  pipamd_tape_set_info info;
  long long *d_prog;      // info.words words: the programs one behind the other, else targets relocated
  TapeSetEntry *d_table;  // info.n entries
  TapeSetEntry *h_table;     // the same entries on the host, and every tape's own counts (pipamd_tape_set_tape_info,
  pipamd_tape_info *h_info;  // pipamd_tape_set_sweep_create)
};

extern "C" int pipamd_tape_set_create(pipamd_engine *e, int n, const pipamd_tape *const *tapes, pipamd_tape_set **out,
                                      pipamd_tape_set_info *info) {
  if (out) *out = nullptr;
  if (!e || !out || n < 1 || !tapes) {
    pipamd_set_error("tape_set_create: null engine, tapes or result pointer, or n < 1");
    return PIPAMD_E_INVALID;
  }
  pipamd_tape_set_info I;
  memset(&I, 0, sizeof I);
  I.n = n;
  I.slots = 1;
  for (int i = 0; i < n; i++) {
    const pipamd_tape *t = tapes[i];
    if (!t || t->device != e->device || t->bits != tapes[0]->bits) {
      pipamd_set_error("tape_set_create: tape %d is null, of another device than the engine's, or of another cell width", i);
      return PIPAMD_E_INVALID;
    }
    I.words += t->info.words;
    if (t->point_cols > I.point_cols) I.point_cols = t->point_cols;
    if (t->shape.nvar > I.nvar) I.nvar = t->shape.nvar;
    if (t->shape.ndual > I.ndual) I.ndual = t->shape.ndual;
    if (t->info.slots > I.slots) I.slots = t->info.slots;
    if (I.words >= (1ll << 31)) {
      pipamd_set_error("tape_set_create: programs of 2^31 words or more together");
      return PIPAMD_E_TOOLARGE;
    }
  }
  I.bits = tapes[0]->bits;
  const int ew = I.bits / 64;
  std::vector<long long> prog((size_t)I.words);
  std::vector<TapeSetEntry> table((size_t)n);
  long long at = 0;
  for (int i = 0; i < n; i++) {
    const pipamd_tape *t = tapes[i];
    const long long words = t->info.words;
    TapeSetEntry &en = table[i];
    memset(&en, 0, sizeof en);
    en.start = (int)at;
    en.words = (int)words;
    en.point_cols = t->point_cols;
    en.nvar = t->shape.nvar;
    en.ndual = t->shape.ndual;
    // the tape's own words, every else target moved by the tape's start (node lengths as tape_compile checked them)
    for (long long pc = 0; pc < words;) {
      const long long hdr = t->h_prog[pc];
      const int op = (int)(hdr & 0xff), P = (int)((hdr >> 8) & 0xffff);
      long long len = 1;
      if (op == TAPE_NEW) len += ew * (P + 2);
      else if (op == TAPE_IF) len += ew * (P + 1);
      else if (op == TAPE_LEAF) len += ew * ((long long)en.nvar * (P + 2) + 2ll * en.ndual);
      if (pc + len > words) len = words - pc;  // (cannot be: the re-check below refuses it)
      memcpy(&prog[(size_t)(at + pc)], t->h_prog + pc, (size_t)len * 8);
      if (op == TAPE_IF) prog[(size_t)(at + pc)] = hdr + (at << 32);
      pc += len;
    }
    // the promise to the kernel again, on the concatenation: every jump forward and inside its own tape's words
    const long long breach = tape_program_breach(prog.data(), at, words, ew, en.nvar, en.ndual, t->info.slots);
    if (breach >= 0) {
      pipamd_set_error("tape_set_create: internal: word %lld of tape %d breaks the kernel's contract", breach, i);
      return PIPAMD_E_INVALID;
    }
    at += words;
  }
  if (hipSetDevice(e->device) != hipSuccess) return PIPAMD_E_HIP;
  pipamd_tape_set *s = (pipamd_tape_set *)calloc(1, sizeof *s);
  if (!s) return PIPAMD_E_NOMEM;
  s->device = e->device;
  s->bits = I.bits;
  s->info = I;
  s->h_table = (TapeSetEntry *)malloc((size_t)n * sizeof(TapeSetEntry));
  s->h_info = (pipamd_tape_info *)malloc((size_t)n * sizeof(pipamd_tape_info));
  if (!s->h_table || !s->h_info) {
    free(s->h_table);
    free(s->h_info);
    free(s);
    return PIPAMD_E_NOMEM;
  }
  memcpy(s->h_table, table.data(), (size_t)n * sizeof(TapeSetEntry));
  for (int i = 0; i < n; i++) s->h_info[i] = tapes[i]->info;
  hipError_t he = hipMalloc((void **)&s->d_table, (size_t)n * sizeof(TapeSetEntry));
  if (he == hipSuccess) he = hipMemcpy(s->d_table, table.data(), (size_t)n * sizeof(TapeSetEntry), hipMemcpyHostToDevice);
  if (he == hipSuccess && I.words) he = hipMalloc((void **)&s->d_prog, (size_t)I.words * 8);
  if (he == hipSuccess && I.words) he = hipMemcpy(s->d_prog, prog.data(), (size_t)I.words * 8, hipMemcpyHostToDevice);
  if (he != hipSuccess) {
    pipamd_set_error("tape_set_create: %d tapes, %lld words on the device: %s", n, (long long)I.words, hipGetErrorString(he));
    if (s->d_table) hipFree(s->d_table);
    if (s->d_prog) hipFree(s->d_prog);
    free(s->h_table);
    free(s->h_info);
    free(s);
    return PIPAMD_E_HIP;
  }
  if (info) *info = I;
  *out = s;
  return PIPAMD_OK;
}

extern "C" void pipamd_tape_set_free(pipamd_tape_set *s) {
  if (!s) return;
  if (hipSetDevice(s->device) == hipSuccess) {
    if (s->d_prog) hipFree(s->d_prog);
    if (s->d_table) hipFree(s->d_table);
  }
  free(s->h_table);
  free(s->h_info);
  free(s);
}

extern "C" int pipamd_tape_set_eval(pipamd_engine *e, const pipamd_tape_set *s, int64_t n_points, const int32_t *d_tape,
                                    const int64_t *d_points, int32_t *d_status, int32_t *d_leaf, int64_t *d_x_num,
                                    int64_t *d_x_den, int64_t *d_dual_num, int64_t *d_dual_den, void *stream) {
  if (!e || !s || n_points < 0 || s->device != e->device ||
      (n_points > 0 && (!d_tape || (s->info.point_cols > 0 && !d_points)))) {
    pipamd_set_error("tape_set_eval: null engine or set, a set of another device, n_points < 0, points without tape indices, "
                     "or parameters without points");
    return PIPAMD_E_INVALID;
  }
  if (n_points >= (1ll << 38)) {
    pipamd_set_error("tape_set_eval: %lld points, at most 2^38 - 1 a call", (long long)n_points);
    return PIPAMD_E_TOOLARGE;
  }
  if (n_points == 0) return PIPAMD_OK;
  if (hipSetDevice(e->device) != hipSuccess) return PIPAMD_E_HIP;
  TapeSetLaunch L;
  L.prog = s->d_prog;
  L.table = s->d_table;
  L.n = s->info.n;
  L.bits = s->bits;
  L.point_cols = s->info.point_cols;
  L.nvar = s->info.nvar;
  L.ndual = s->info.ndual;
  L.slots = s->info.slots;
  L.n_points = n_points;
  L.tape = d_tape;
  L.points = (const long long *)d_points;
  L.status = d_status;
  L.leaf = d_leaf;
  L.x_num = d_x_num;
  L.x_den = d_x_den;
  L.dual_num = d_dual_num;
  L.dual_den = d_dual_den;
  HIPCHK(pipk_launch_tape_set_eval(&L, (hipStream_t)stream));
  return PIPAMD_OK;
}

extern "C" int pipamd_tape_set_tape_info(const pipamd_tape_set *s, int i, pipamd_tape_info *info, int32_t *point_cols,
                                         int32_t *nvar, int32_t *ndual) {
  if (!s || i < 0 || i >= s->info.n) {
    pipamd_set_error("tape_set_tape_info: a null set, or tape %d outside 0 .. n - 1", i);
    return PIPAMD_E_INVALID;
  }
  if (info) *info = s->h_info[i];
  if (point_cols) *point_cols = s->h_table[i].point_cols;
  if (nvar) *nvar = s->h_table[i].nvar;
  if (ndual) *ndual = s->h_table[i].ndual;
  return PIPAMD_OK;
}

// ------------------------------------------------------------------ every tape of a set swept over its own box
enum { TAPE_SET_SWEEP_MAX_JOBS = 1 << 20 };
// The checks and the arithmetic the planner and pipamd_tape_set_sweep_create share: per job the box (tape_sweep_box)
// and the context's shape; the running sums of points, summary words and chunks, none of which can wrap: fewer than
// 2^38 points in all, at most 2^20 jobs, a tape's leaves below 2^31 as its program's words are.  Each output may be NULL.
static int tape_set_sweep_check(const char *who, int n_jobs, const pipamd_tape_sweep_job *jobs, const int64_t *leaves,
                                const int32_t *point_cols, int64_t *points, int64_t *summary_off, int64_t *chunk_off) {
  if (n_jobs < 0 || (n_jobs > 0 && (!jobs || !leaves || !point_cols))) {
    pipamd_set_error("%s: n_jobs < 0, or jobs without their array, leaves or point_cols", who);
    return PIPAMD_E_INVALID;
  }
  if (n_jobs > TAPE_SET_SWEEP_MAX_JOBS) {
    pipamd_set_error("%s: %d jobs, at most 2^20 a call", who, n_jobs);
    return PIPAMD_E_TOOLARGE;
  }
  int64_t all = 0, words = 0, chunks = 0;
  if (summary_off) summary_off[0] = 0;
  if (chunk_off) chunk_off[0] = 0;
  for (int j = 0; j < n_jobs; j++) {
    char job[96];
    snprintf(job, sizeof job, "%s: job %d", who, j);
    const pipamd_tape_sweep_job &q = jobs[j];
    if (q.n_ctx < 0 || (q.n_ctx > 0 && !q.ctx) || leaves[j] < 0 || leaves[j] >= (1ll << 31)) {
      pipamd_set_error("%s: n_ctx < 0, context rows without an array, or leaves outside 0 .. 2^31 - 1", job);
      return PIPAMD_E_INVALID;
    }
    int64_t n = 0;
    const int rc = tape_sweep_box(job, point_cols[j], q.lo, q.hi, nullptr, &n);
    if (rc) return rc;
    all += n;
    if (all >= (1ll << 38)) {
      pipamd_set_error("%s: 2^38 points or more in the jobs up to this one (at most 2^38 - 1 a call)", job);
      return PIPAMD_E_TOOLARGE;
    }
    words += PIPAMD_SWEEP_WORDS(leaves[j]);
    chunks += (n + TAPE_BLOCK - 1) / TAPE_BLOCK;
    if (points) points[j] = n;
    if (summary_off) summary_off[j + 1] = words;
    if (chunk_off) chunk_off[j + 1] = chunks;
  }
  return PIPAMD_OK;
}

extern "C" int pipamd_tape_set_sweep_plan(int n_jobs, const pipamd_tape_sweep_job *jobs, const int64_t *leaves,
                                          const int32_t *point_cols, int64_t *points, int64_t *summary_off, int64_t *chunk_off) {
  if (!summary_off || (n_jobs > 0 && !points)) {
    pipamd_set_error("tape_set_sweep_plan: null summary_off, or jobs without points");
    return PIPAMD_E_INVALID;
  }
  return tape_set_sweep_check("tape_set_sweep_plan", n_jobs, jobs, leaves, point_cols, points, summary_off, chunk_off);
}

struct pipamd_tape_set_sweep {
  const pipamd_tape_set *set;
  int device, n_jobs, blocks;
  long long chunks, words;
  long long *d_buf;  // the buffer pip_tape.h describes (TapeSetSweepLaunch)
};

extern "C" int pipamd_tape_set_sweep_create(pipamd_engine *e, const pipamd_tape_set *s, int n_jobs,
                                            const pipamd_tape_sweep_job *jobs, pipamd_tape_set_sweep **out, int64_t *summary_off) {
  if (out) *out = nullptr;
  if (!e || !s || !out || s->device != e->device) {
    pipamd_set_error("tape_set_sweep_create: null engine, set or result pointer, or a set of another device");
    return PIPAMD_E_INVALID;
  }
  if (n_jobs < 0 || (n_jobs > 0 && !jobs)) {
    pipamd_set_error("tape_set_sweep_create: n_jobs < 0, or jobs without their array");
    return PIPAMD_E_INVALID;
  }
  if (n_jobs > TAPE_SET_SWEEP_MAX_JOBS) {
    pipamd_set_error("tape_set_sweep_create: %d jobs, at most 2^20 a call", n_jobs);
    return PIPAMD_E_TOOLARGE;
  }
  std::vector<int64_t> leaves((size_t)n_jobs), points((size_t)n_jobs), sum_off((size_t)n_jobs + 1), chunk_off((size_t)n_jobs + 1);
  std::vector<int32_t> cols((size_t)n_jobs);
  for (int j = 0; j < n_jobs; j++) {
    const int t = jobs[j].tape;
    if (t < 0 || t >= s->info.n) {
      pipamd_set_error("tape_set_sweep_create: job %d: tape %d outside 0 .. %d", j, t, s->info.n - 1);
      return PIPAMD_E_INVALID;
    }
    leaves[j] = s->h_info[t].leaves;
    cols[j] = s->h_table[t].point_cols;
  }
  const int rc = tape_set_sweep_check("tape_set_sweep_create", n_jobs, jobs, leaves.data(), cols.data(), points.data(),
                                      sum_off.data(), chunk_off.data());
  if (rc) return rc;
  // the buffer: chunk_off, summary_off, the jobs' records, then per job lo, extents and context rows
  const size_t head = 2 * ((size_t)n_jobs + 1) + (size_t)n_jobs * (sizeof(TapeSetSweepJob) / 8);
  size_t total = head;
  for (int j = 0; j < n_jobs; j++) total += 2 * (size_t)cols[j] + (size_t)jobs[j].n_ctx * ((size_t)cols[j] + 2);
  std::vector<long long> buf(total);
  TapeSetSweepJob *rec = (TapeSetSweepJob *)(buf.data() + 2 * ((size_t)n_jobs + 1));
  size_t at = head;
  for (int j = 0; j <= n_jobs; j++) buf[(size_t)j] = chunk_off[j], buf[(size_t)n_jobs + 1 + j] = sum_off[j];
  for (int j = 0; j < n_jobs; j++) {
    const pipamd_tape_sweep_job &q = jobs[j];
    TapeSetSweepJob &r = rec[j];
    memset(&r, 0, sizeof r);
    r.tape = q.tape;
    r.n_ctx = q.n_ctx;
    r.box = (long long)at;
    for (int c = 0; c < cols[j]; c++) {
      buf[at + c] = q.lo[c];
      buf[at + cols[j] + c] = (long long)((unsigned long long)q.hi[c] - (unsigned long long)q.lo[c] + 1);  // (below 2^38)
    }
    at += 2 * (size_t)cols[j];
    r.ctx = (long long)at;
    const size_t ctx_words = (size_t)q.n_ctx * ((size_t)cols[j] + 2);
    if (ctx_words) memcpy(&buf[at], q.ctx, ctx_words * 8);
    at += ctx_words;
    r.n_points = points[j];
    r.summary_off = sum_off[j];
    r.leaves = leaves[j];
    r.chunk_off = chunk_off[j];
  }
  if (hipSetDevice(e->device) != hipSuccess) return PIPAMD_E_HIP;
  pipamd_tape_set_sweep *w = (pipamd_tape_set_sweep *)calloc(1, sizeof *w);
  if (!w) return PIPAMD_E_NOMEM;
  w->set = s;
  w->device = e->device;
  w->n_jobs = n_jobs;
  w->chunks = chunk_off[n_jobs];
  w->words = sum_off[n_jobs];
  if (n_jobs) {
    w->blocks = pipk_tape_set_sweep_blocks(s->bits, s->info.slots, e->cus);
    hipError_t he = hipMalloc((void **)&w->d_buf, total * 8);
    if (he == hipSuccess) he = hipMemcpy(w->d_buf, buf.data(), total * 8, hipMemcpyHostToDevice);
    if (he != hipSuccess) {
      pipamd_set_error("tape_set_sweep_create: %d jobs, %zu words on the device: %s", n_jobs, total, hipGetErrorString(he));
      if (w->d_buf) hipFree(w->d_buf);
      free(w);
      return PIPAMD_E_HIP;
    }
  }
  if (summary_off) memcpy(summary_off, sum_off.data(), ((size_t)n_jobs + 1) * 8);
  *out = w;
  return PIPAMD_OK;
}

extern "C" void pipamd_tape_set_sweep_free(pipamd_tape_set_sweep *w) {
  if (!w) return;
  if (w->d_buf && hipSetDevice(w->device) == hipSuccess) hipFree(w->d_buf);
  free(w);
}

extern "C" int pipamd_tape_set_sweep_run(pipamd_engine *e, const pipamd_tape_set_sweep *w, int64_t *d_summary, void *stream) {
  if (!e || !w || w->device != e->device || (w->n_jobs > 0 && !d_summary)) {
    pipamd_set_error("tape_set_sweep_run: null engine or sweep, a sweep of another device, or jobs without a summary");
    return PIPAMD_E_INVALID;
  }
  if (w->n_jobs == 0) return PIPAMD_OK;
  if (hipSetDevice(e->device) != hipSuccess) return PIPAMD_E_HIP;
  TapeSetSweepLaunch L;
  memset(&L, 0, sizeof L);
  L.prog = w->set->d_prog;
  L.table = w->set->d_table;
  L.buf = w->d_buf;
  L.n_jobs = w->n_jobs;
  L.bits = w->set->bits;
  L.slots = w->set->info.slots;
  L.blocks = w->blocks;
  L.max_blocks = g_tape_sweep_blocks;
  L.chunks = w->chunks;
  L.words = w->words;
  L.summary = (long long *)d_summary;
  HIPCHK(pipk_launch_tape_set_sweep(&L, (hipStream_t)stream));
  return PIPAMD_OK;
}

extern "C" int pipamd_batch_counters(pipamd_engine *e, const void *d_ws, const pipamd_batch_desc *d, uint64_t *d_out4,
                                     void *stream) {
  if (!d_out4) return PIPAMD_E_INVALID;
  BatchView v;
  int rc = batch_view("batch_counters", e, d_ws, d, 0, 0, &v);
  if (rc) return rc;
  HIPCHK(pipk_launch_batch_counters(v.jobs, v.lay.batch, (unsigned long long *)d_out4, (hipStream_t)stream));
  return PIPAMD_OK;
}

// Diagnostic only: per-phase cycle sums of the advance kernel (needs a -DPIP_PROFILE build).
extern "C" int pipamd_debug_profile(pipamd_engine *e, int enable, uint64_t *host_out10) {
  if (!e) return PIPAMD_E_INVALID;
  if (enable && !e->d_prof) {
    HIPCHK(hipMalloc((void **)&e->d_prof, 64 * sizeof(unsigned long long)));
    HIPCHK(hipMemset(e->d_prof, 0, 64 * sizeof(unsigned long long)));
  }
  if (host_out10 && e->d_prof) {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(host_out10, e->d_prof, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(e->d_prof, 0, 64 * sizeof(unsigned long long)));
  }
  return PIPAMD_OK;
}

extern "C" int pipamd_engine_set_waves_per_job(pipamd_engine *e, int waves) {
  if (!e || (waves != 0 && waves != 1 && waves != 4 && waves != 8)) return PIPAMD_E_INVALID;
  e->waves_per_job = waves;
  return PIPAMD_OK;
}

extern "C" int pipamd_engine_set_iter_limit(pipamd_engine *e, int pivots_per_launch) {
  if (!e || pivots_per_launch < 1) return PIPAMD_E_INVALID;
  // a launch logs (pivot, denominator) per pivot for the determinant replay: PIPAMD_DETLOG entries per job
  e->iter_limit = pivots_per_launch < PIPAMD_DETLOG ? pivots_per_launch : PIPAMD_DETLOG;
  return PIPAMD_OK;
}

extern "C" void pipamd_free(void *p) { free(p); }
