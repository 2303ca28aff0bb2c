// piplib_amd/csrc/pip_host.h -- internal host-side declarations.
#ifndef PIP_HOST_H
#define PIP_HOST_H
#include <hip/hip_runtime.h>
#include <pthread.h>

#include "pip_job.h"
#include "pip_plan.h"
#include "pip_tape.h"

#define PIPAMD_MAX_ROUNDS 512
#define PIPAMD_MAX_GROW 24 /* growth rounds of one solve: the row capacity at least doubles per round, up to PIPAMD_SMAX */

struct pipamd_engine {
  int device;
  hipEvent_t ev[2 * PIPAMD_MAX_ROUNDS];
  int nev, nlaunch;
  int timed;
  int round_pivots;  /* pivot budget per tableau in the bulk launch (0 = default) */
  int round_rows;    /* spare rows (Gomory cuts) in the bulk launch's LDS image (0 = default) */
  int bulk_min;      /* batches of at least this many tableaux start with the one-wave bulk launch (0 = default 2048) */
  int single_launch; /* debug: stop after one launch */
  int lone_batches;  /* 1: no general one-wave launch between the lean launch and the tail (pipamd_engine_set_lone_batches) */
  int no_spare_replay; /* 1: the second lean launch's spare blocks replay no determinant logs (pipamd_engine_set_spare_replay) */
  int lean2_one_wave; /* 1: the second lean launch runs one wave per tableau, not four (pipamd_engine_set_lean2_waves) */
  int no_lean;       /* 1: bulk launches without the lean kernel (pip_lean.h) */
  int lean64;        /* 1: 128-bit batches of 129 ... 256 columns start with pip_lean64_kernel (pip_lean.h; pipamd_engine_set_lean64) */
  int lean_big;      /* 1: bulk batches whose one parameter is the big one start with the lean kernel's BIG flavour (pipamd_engine_set_lean_big) */
  int no_lean2;      /* 1: the second one-wave bulk launch is the general kernel even where the lean kernel could resume */
  int *h_run;        /* pinned: {jobs still running, their largest row count | PIPAMD_Q_CAPFLAG, how many of them are out of rows} */
  int *d_q;          /* launch-list control words (a pool, see pipamd_batch_solve) and the two job lists */
  unsigned solve_seq; /* solves since the control pool was last zeroed */
  hipStream_t pool_stream; /* the stream that zeroing was ordered on */
  int no_timing;     /* 1: no HIP events around the launches */
  int q_cap;         /* jobs the lists hold */
  int iter_limit;
  int waves_per_job; /* 0 = choose by batch size */
  int tail_waves;    /* waves per tableau of the tail launch when waves_per_job is 0 (0 = default 4) */
  int blocking_wait;   /* 1: pipamd_batch_solve naps between looks at its stream instead of spinning on it */
  int no_device_tree; /* 1: pipamd_solve_tableaux_lockstep skips the device-resident traiter() (pip_quast.hip) */
  void *dt_buf[10];    /* device tree: device buffers kept between calls (problems, rows, stacks, tapes, results, ...;
                          7-9: pipamd_pip_*: built tableaux, uploaded matrices, range flags) */
  size_t dt_cap[10];
  int dt_small[10];     /* calls in a row that needed less than a quarter of the buffer (it is given back after eight) */
  pthread_mutex_t dt_lock; /* the device-tree buffers below serve one call at a time */
  void *dt_host;       /* device tree: pinned staging buffer for the problems' rows */
  size_t dt_host_cap;
  int dt_served, dt_fallback; /* problems the device tree finished / handed back in the last lock-step call */
  int dt_record;       /* testing aid (pipamd_debug_device_tree_record): keep the device tree's result words of the last call */
  int *dt_rec;         /* Q_OUT ints per problem of that call, by input index; -1 throughout where the device tree was not given it */
  int dt_rec_n;
  unsigned long long *d_prof; /* diagnostic builds only (-DPIP_PROFILE) */
  void *d_scratch;
  size_t scratch_bytes;
  /* expanser for the batch layer (pipamd_batch_solve): side arenas for tableaux that spent their spare rows, one
   * per growth round of a solve (a round doubles the row capacity), kept between solves; the block counter */
  void *d_side[PIPAMD_MAX_GROW];
  size_t side_bytes[PIPAMD_MAX_GROW];
  int *d_side_count;
  void *retired[128]; /* side arenas outgrown while batches were in flight: freed with the engine (hipFree waits for the device) */
  int nretired;
  int max_rows;      /* row budget per tableau of pipamd_batch_solve's growth (0 = the engine's limit) */
  int grow_step;     /* testing aid: rows added per growth round (0 = double) */
  int last_rehoused; /* tableaux the last pipamd_batch_solve re-housed (all rounds) */
  struct BatchRun *run; /* the batch solve in progress (pipamd_batch_solve_async .. pipamd_batch_wait) */
  int cus;           /* compute units of the device: the bound of pipamd_tape_sweep's persistent grid */
};

/* pipk_launch_advance_q's `hints`: what the caller knows about the jobs of a launch, and what the launch is to do */
enum {
  PIPK_HINT_FULL = 1,      /* every job has no parameters, no big parameter and nvar + 1 == W == the wave's column coverage (the caller knows its batch is uniform): see FULL */
  PIPK_HINT_LEAN = 2,      /* the lean kernel of pip_lean.h (one wave per job, 64-bit entries, at most 128 columns and pipk_lean_class(Smax) != 0, else refused): it runs the jobs it can (no parameters, entries below 2^15) and leaves the others PIPAMD_ST_RUN on the output list for a launch without this bit; waves_per_job == 4 with it, where pipk_lean_waves_class(Smax) and not PIPK_HINT_BIG: the same kernel with four waves per tableau, 256-thread blocks, for a launch over a few paused tableaux */
  PIPK_HINT_NO_REPLAY = 4, /* no determinant replay behind the launch (see pipk_launch_replay_all) */
  PIPK_HINT_LEAN64 = 8,    /* the lean kernel of pip_lean.h on long long rows (one wave per job, 128-bit entries, 129 ... 256 columns, pipk_lean64_lds_bytes(Smax, Lmax) within the LDS budget, else refused): it runs the jobs it can (no parameters, entries below 2^63) and leaves the others on the output list */
  PIPK_HINT_BIG = 16,      /* with PIPK_HINT_LEAN: every job has nparm == 1 and bigparm == nvar + 1 -- the lean kernel's BIG flavour */
  PIPK_HINT_SPARE_REPLAY = 32 /* with PIPK_HINT_LEAN and an input list: the launch's workgroups beyond the list replay the determinant logs of the finished jobs that are not on it (PipQueue.replay_spare; `grid` is then the batch, not the list's bound) */
};

void pipamd_set_error(const char *fmt, ...);
int pipamd_batch_layout(const pipamd_batch_desc *d, PipBatchLayout *lay, size_t *jobs_bytes);

extern "C" {
/* bytes of the LDS image a launch over jobs of at most (Lmax, Smax, Wmax) needs; a job only fits
 * the engine if this stays within the 159 KiB a workgroup can get (PIPAMD_LDS_BUDGET) */
size_t pipk_advance_lds_bytes(int Lmax, int Smax, int Wmax, int ebits);
int pipk_static_class(int smax);
int pipk_lean_class(int smax);
int pipk_lean_waves_class(int smax);
hipError_t pipk_launch_advance(PipJob *jobs, long long *arena, int njobs, int Lmax, int Smax, int Wmax, int iter_limit,
                               int waves_per_job, int ebits, unsigned long long *prof, hipStream_t stream);
size_t pipk_lean64_lds_bytes(int Smax, int Lmax);
hipError_t pipk_launch_advance_q(PipJob *jobs, long long *arena, int njobs, int Lmax, int Smax, int Wmax, int iter_limit,
                                 int waves_per_job, int ebits, void *const *q5, int grid, void **big, int hints,
                                 unsigned long long *prof,
                                 hipStream_t stream);
hipError_t pipk_launch_replay_all(PipJob *jobs, long long *arena, int njobs, int ebits, int wave_per_job, hipStream_t stream);
hipError_t pipk_launch_batch_load(PipJob *jobs, long long *arena, const long long *rows, PipBatchLayout lay, int first,
                                  int count, hipStream_t stream);
hipError_t pipk_launch_batch_results_shifted(const PipJob *jobs, const long long *arena, int njobs, int nvar, int ebits,
                                             int shift, int *status, int *pivots, int *cuts, void *x_num, void *x_den,
                                             hipStream_t stream);
hipError_t pipk_launch_batch_results(const PipJob *jobs, const long long *arena, int njobs, int nvar, int nparm,
                                     int ebits, int *status, int *pivots, int *cuts, void *sol_num, void *sol_den,
                                     hipStream_t stream);
int pipk_batch_dual_max_ni(void); /* inequalities per tableau pip_batch_dual_kernel sorts in LDS */
/* the load and the dual of the batch layer's front ends, from the one source (pip_job.h) the entry's check has filled */
hipError_t pipk_launch_batch_load_source(PipJob *jobs, long long *arena, PipBatchLayout lay, const PipBatchSource *src, int first,
                                         int count, hipStream_t stream);
hipError_t pipk_launch_batch_dual_source(const PipJob *jobs, const long long *arena, PipBatchLayout lay, const PipBatchSource *src,
                                         int first, int count, void *dual_num, void *dual_den, hipStream_t stream);
hipError_t pipk_launch_rehouse(PipJob *jobs, long long *arena, void *const *q5, int grid, PipBatchLayout nl, int *side_count,
                               int side_cap, hipStream_t stream);
hipError_t pipk_launch_rehouse_finish(PipJob *jobs, long long *arena, int njobs, int sol_words, hipStream_t stream);
hipError_t pipk_launch_clone(long long *arena, const long long *list, int n, hipStream_t stream);
hipError_t pipk_launch_patch(long long *arena, const int *buf, const long long *index, int n, hipStream_t stream);
hipError_t pipk_launch_fresh(long long *arena, const long long *buf, const long long *index, int n, int ebits, hipStream_t stream);
hipError_t pipk_launch_gather(const PipJob *jobs, const long long *arena, int njobs, long long *out,
                              const long long *off, int ebits, hipStream_t stream);
hipError_t pipk_launch_batch_counters(const PipJob *jobs, int njobs, unsigned long long *out, hipStream_t stream);
}
#endif
