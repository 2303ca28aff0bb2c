// piplib_amd/csrc/pip_plan.h -- which launches a pipamd_batch_solve sends out: the decision as a pure function.
//
// Host only, no HIP header and no engine: pip_host.cpp fills a PipPlanIn from the batch layout and the engine's
// switches, pip_plan_batch() says which kernels go out, in which order, with which budgets, and who replays the
// determinant logs; BatchRun (pip_host.cpp) issues that plan.  tests/batch_plan_main.cpp includes this header alone.
#ifndef PIP_PLAN_H
#define PIP_PLAN_H
#include "pip_job.h"

// Row-capacity class of the one-wave kernels with a compile-time LDS image for a launch of `smax` row slots: the
// smallest class that holds it if that costs at most an eighth more LDS than its exact size (occupancy is LDS-bound
// at 24 tableaux per CU); 0 = none.
inline int pip_static_class(int smax) {
  const int s = (smax + 3) & ~3;
  if (s <= 64) return 64;
  if (s > 84 && s <= 96) return 96;
  if (s > 98 && s <= 112) return 112;
  if (s > 112 && s <= 128) return 128;
  if (s > 140 && s <= 160) return 160;
  return 0;
}
// Row-capacity class of the lean kernel (pip_lean.h) for `smax` row slots: the smallest that holds them (a class too
// large costs a little occupancy, no class costs the lean launch); 0 = none.
inline int pip_lean_class(int smax) {
  const int s = (smax + 3) & ~3;
  return s <= 64 ? 64 : (s <= 96 ? 96 : (s <= 112 ? 112 : (s <= 128 ? 128 : (s <= 160 ? 160 : 0))));
}
// 1 where the lean kernel's class for `smax` row slots also comes with four waves per tableau (pip_lean.h, NW = 4; the
// plain flavour only): the classes a second lean launch over paused headline-sized tableaux lands in
inline int pip_lean_waves_class(int smax) {
  const int sc = pip_lean_class(smax);
  return sc == 128 || sc == 160;
}

/* Pivot budget per tableau of the first bulk launch where a second lean launch follows it (pip_plan_batch takes it for
 * that sequence alone, every other bulk launch has 96; pipamd_engine_set_round_pivots overrides both).  A tableau that has
 * spent it waits for the whole launch to end, is widened, listed and re-packed by the second lean launch (four waves
 * per tableau since round 7: the budget was measured with one, and was not measured again); of 256
 * headline tableaux nine spend a budget of 96 and one a budget of 128 (tests/test_gpu_first_launch_budget.py).  Measured
 * against 96, 160 and 256 with 16 batches in flight on 4 and on 16 hardware queues (DESIGN.md section 5 round 6,
 * profiles/r06_ab.txt): 128 is ahead of 96 in every round; 160 and 256 are no better with batches in flight and lose
 * 8-11 % for a batch on its own. */
#ifndef PIPAMD_ROUND_PIVOTS
#define PIPAMD_ROUND_PIVOTS 128
#endif

// What the decision reads, and nothing else: the batch's layout (PipBatchLayout) and the engine's switches.
struct PipPlanIn {
  int batch, nvar, nparm, bigparm, ni, S, W, ebits, tflags;
  int round_pivots, round_rows, bulk_min, iter_limit, waves_per_job, tail_waves, lone_batches, no_spare_replay,
      lean2_one_wave, no_lean, no_lean2, lean64, lean_big, single_launch;
  // pipk_lean64_lds_bytes(s, nvar + s) <= PIPAMD_LDS_BUDGET for s = pip_plan_lean64_rows(S) (the image's size is the
  // device code's to tell); looked at only where `lean64` is on
  bool lean64_fits;
};

enum PipKernelFamily {
  PIP_K_GENERAL,   // pip_advance_kernel
  PIP_K_LEAN,      // pip_lean_kernel, the plain flavour
  PIP_K_LEAN_BIG,  // pip_lean_kernel's BIG flavour: every job's one parameter is the big one
  PIP_K_LEAN64     // pip_lean64_kernel: the 128-bit flavour on long long rows
};

// One launch of a pivot kernel.
struct PipStep {
  int kernel;          // PipKernelFamily
  int waves;           // per tableau
  int budget;          // pivots per tableau
  int smax;            // row slots of the launch's image
  bool whole_batch;    // a workgroup per tableau of the batch; else: per entry the input list can have
  bool replay_behind;  // the launch's determinant logs are replayed right behind it, over its own jobs
  bool spare_replay;   // its workgroups beyond the input list replay the logs of the finished jobs not on it
  bool full;           // a uniform batch without parameters whose rows fill a wave's 128 columns exactly: FULL kernels
};

// The bulk launches of a solve and what follows them.
struct PipPlan {
  PipStep step[2];  // (the lean64 launch stands alone; else a first one-wave launch and a second)
  int nsteps;
  bool pending;     // the bulk launches left their determinant logs to one replay behind them
  bool spare_went;  // the second lean launch's spare blocks replayed the logs of the jobs the first one finished
  bool catchall_waves;  // that one replay goes out a wave per job, not a lane per job
  int tail_waves;
  // pipamd_debug_single_launch: the sequence ends behind the bulk launches (the tableaux they left stay
  // PIPAMD_ST_RUN), with that one replay before the stop or without it.  A batch without a bulk launch takes its
  // first tail launch and stops there (BatchRun::advance).
  bool stop, stop_replay;
};

inline int pip_plan_lean64_rows(int S) { return S < 448 ? S : 448; }  // (448 rows: an image of 30 KB, five tableaux per CU)

inline bool pip_plan_full(const PipPlanIn &in) { return in.nparm == 0 && in.bigparm < 0 && in.nvar + 1 == 128 && in.W == 128; }

// traiter() for the whole batch, as a short sequence of launches without a host round trip in
// between (each launch writes the list of tableaux it left unfinished, the next one reads it):
//   bulk  (batches of >= `bulk_min` tableaux, default 2048): one wave per tableau; a tableau's workgroup ends when the
//         tableau is finished, has spent `round_pivots` pivots or has filled the LDS image (sized
//         for the rows it has plus `round_rows` Gomory cuts, so that 24 tableaux fit a CU).  The
//         workgroup dispatcher starts the next tableau in its place, so every CU stays busy until
//         all have had their turn.  Where the lean kernel (pip_lean.h) takes the batch, a second lean launch follows
//         over the list of the tableaux the first one paused: a few hundred, four waves per tableau where the row
//         capacity has that kernel (pipamd_engine_set_lean2_waves), its blocks beyond the list replaying determinant logs.
//   tail  : what the bulk launch left unfinished (the few tableaux that need many more pivots or
//         rows) runs to completion with four waves per tableau and an image for every spare row:
//         little parallelism is left, so the latency of a pivot is what counts (pip_plan_tail).
// Only then the host looks at the number of tableaux still running (normally 0; tableaux that
// hit the per-launch pivot limit `iter_limit` go through further tail launches).
inline PipPlan pip_plan_batch(const PipPlanIn &in) {
  PipPlan p{};
  const bool integer = (in.tflags & PIPAMD_T_INT) != 0;
  // (the default budget of the first bulk launch is 96; only where a second lean launch takes what the first leaves it
  // is PIPAMD_ROUND_PIVOTS, chosen below once `lean2` is known -- the general one-wave launches of 128-bit batches and
  // of batches with parameters, and an engine in lone-batches mode, keep 96)
  const int K1 = in.round_pivots > 0 ? in.round_pivots : 96;
  const int KA = !integer ? 0 : (in.round_rows > 0 ? in.round_rows : 48);
  const bool full = pip_plan_full(in);
  const bool one_wave_ok = in.waves_per_job != 4 && in.waves_per_job != 8;
  p.tail_waves = in.waves_per_job ? in.waves_per_job : (in.tail_waves ? in.tail_waves : 4);
  p.catchall_waves = in.lone_batches != 0;
  // The 128-bit flavour on rows of 129 ... 256 columns without parameters can start with pip_lean64_kernel (pip_lean.h),
  // one wave per tableau over the whole batch: it finishes the tableaux whose stored entries stay below 2^63 (two in
  // three of BASELINE's configs[4]) and leaves the others to the tail.  Opt-in (pipamd_engine_set_lean64):
  // measured on that batch it is no faster than pip_advance_kernel's four waves per tableau.
  // A batch with PIPAMD_T_DUAL takes no lean launch: a tableau the lean kernels finish keeps its rows packed, and
  // pip_batch_dual_kernel reads logical row 0 in the general format (pipamd_batch_dual, include/piplib_amd.h)
  const bool dual = (in.tflags & PIPAMD_T_DUAL) != 0;
  if (!dual && in.lean64 && !in.no_lean && in.ebits == 128 && in.nparm == 0 && in.bigparm < 0 && in.W > 128 && in.W <= 256 &&
      !(in.tflags & (PIPAMD_T_NOSKIP | PIPAMD_T_DEEPEST)) && in.batch >= (in.bulk_min > 0 ? in.bulk_min : 128) && one_wave_ok) {
    const int smax = pip_plan_lean64_rows(in.S);
    if (smax >= in.ni && in.lean64_fits) {
      // (it replays behind itself; any single_launch level: the lean launch on its own)
      p.step[p.nsteps++] = PipStep{PIP_K_LEAN64, 1, in.iter_limit, smax, true, true, false, full};
      p.stop = in.single_launch != 0;
      return p;
    }
  }
  if (in.batch < (in.bulk_min > 0 ? in.bulk_min : 2048) || !one_wave_ok) return p;  // straight to the tail
  int budget, smax;
  bool lean, lean2;
  // no parameters, at most 128 columns of 64-bit entries, rows skipped, plain cuts: the lean kernel (pip_lean.h) goes
  // first -- it finishes the tableaux whose entries stay below 2^15 and leaves the others to the general kernel's launch
  // ... and its BIG flavour for the batches whose one parameter is the big one (lexicographic maxima, unknowns of either
  // sign: pipamd_batch_load_shifted), which need no host decision either.  Opt-in (pipamd_engine_set_lean_big):
  // measured, it is ahead by 13-35 % except for a lone Urs_unknowns batch, where it is 3 % behind
  const bool plain = in.nparm == 0 && in.bigparm < 0;
  const bool bigone = in.lean_big && in.nparm == 1 && in.bigparm == in.nvar + 1 && in.nvar + 2 <= in.W;
  const int lean_kernel = in.bigparm >= 0 ? PIP_K_LEAN_BIG : PIP_K_LEAN;
  const int smax2 = in.ni + 96 < in.S ? in.ni + 96 : in.S;
  // The second one-wave launch: the lean kernel again where it can resume its own paused jobs (below), with a budget
  // of its own; else the general kernel with the first launch's.
  // The first launch's budget: PIPAMD_ROUND_PIVOTS is tried first and kept only if the two lean launches go out with
  // it; every other sequence is shaped with 96.
  for (int k = in.round_pivots > 0 ? K1 : PIPAMD_ROUND_PIVOTS;; k = K1) {
    budget = in.iter_limit < k ? in.iter_limit : k;
    smax = in.ni + (KA < budget ? KA : budget);
    if (smax > in.S) smax = in.S;
    lean = !dual && !in.no_lean && in.ebits != 128 && (plain || bigone) && in.W <= 128 && !(in.W & 1) &&
           !(in.tflags & (PIPAMD_T_NOSKIP | PIPAMD_T_DEEPEST)) && pip_lean_class(smax) != 0;
    lean2 = lean && !in.lone_batches && !in.no_lean2 && pip_lean_class(smax2) != 0;
    if (lean2 || k == K1) break;
  }
  const int b2 = lean2 ? (in.iter_limit < 160 ? in.iter_limit : 160) : budget;
  // The bulk launches leave their determinant logs to the replay behind the first tail launch when the two of them
  // together cannot fill a tableau's log: budget + b2 pivots against the PIPAMD_DETLOG entries it holds.  (A kernel
  // pauses a tableau whose log is full, so nothing is lost beyond that either: the first launch, and a general second
  // one, then replay behind themselves.  A second lean launch never does: its log then holds its own pivots alone, at
  // most 160, and waits for the replay behind the tail.)
  const bool defer = budget + b2 <= PIPAMD_DETLOG;
  p.stop = in.single_launch != 0;
  if (lean) {
    p.step[p.nsteps++] = PipStep{lean_kernel, 1, budget, smax, true, !defer, false, full};
    p.pending = defer;
  }
  // Then what the lean launch left (on the headline: the 6 % of the tableaux that spent its pivot budget) in a second
  // one-wave launch: the lean kernel again, which resumes its own paused jobs, with the largest row-capacity class and
  // a budget that covers the longest tableaux -- and leaves what it cannot take (rows beyond ints, more rows than its
  // image) to the tail.  Where the shape has no lean kernel: the general one-wave kernel.  (Measured with 14 batches
  // in flight: sending those tableaux straight to the four-wave tail instead costs 10 % of the throughput.)
  // (pipamd_engine_set_lone_batches: straight to the tail launches; single_launch 2: the lean launch on its own)
  if (!(lean && (in.lone_batches || in.single_launch == 2))) {
    if (lean2) {
      // (a block per tableau of the batch over the list of the paused ones: the blocks beyond the list replay the
      // logs the first launch left behind its finished tableaux, pip_lean.h lean_spare_replay)
      p.spare_went = p.pending && !in.no_spare_replay;
      // (four waves per tableau where that row capacity and flavour have the kernel: the launch is a few hundred
      // tableaux, each a chain of pivots that lasts as long as the rows of a pivot take one after the other)
      const int w2 = !in.lean2_one_wave && in.bigparm < 0 && pip_lean_waves_class(smax2) ? 4 : 1;
      p.step[p.nsteps++] = PipStep{lean_kernel, w2, b2, smax2, true, false, p.spare_went, full};
      p.pending = true;
    } else {
      p.step[p.nsteps++] = PipStep{PIP_K_GENERAL, 1, budget, smax, true, !defer, false, full};
      p.pending = defer;
    }
  }
  // Where the second lean launch's spare blocks have replayed the logs of the jobs the first one finished, the one
  // replay is the catch-all for what is left -- the few hundred tableaux of the second launch and the tail, every other
  // log is empty -- and goes out a wave per job, the form with the shortest latency.  It does so whenever spare blocks
  // went, also where they could reach little or nothing because the list covers most of the batch (a first-launch
  // budget of a few pivots): correct, since this replay takes every log that is left, but that case was not measured.
  p.catchall_waves = in.lone_batches || p.spare_went;
  // (single_launch 3: without the catch-all replay -- the logs stay as the launches left them, so that a test sees
  // which of them the second lean launch's spare blocks replayed)
  p.stop_replay = p.stop && p.pending && in.single_launch != 3;
  return p;
}

// A tail launch over what is left: at most `upper` listed tableaux in blocks of `curS` row slots.
// The determinant logs of the bulk launches are replayed once, behind the first tail launch, for all tableaux
// (pipk_launch_replay_all): a replay kernel between two launches is a tiny launch that waits milliseconds for a
// turn on a device busy with other batches' bulk launches, and nothing in the pivot launches depends on it -- a
// tableau that overflowed goes on pivoting until the replay says so, its status and pivot count are the same (also
// where it meanwhile ended in a pivot without a column, counted and not logged: det_unlogged, pip_advance.h).
// The bulk launches together log fewer pivots per tableau than the log holds (`defer` in pip_plan_batch).
// (128-bit entries: a list shorter than the GPU has CUs gets a CU per tableau -- sixteen waves; what is left after the
// first tail launch are the few tableaux of hundreds of pivots and rows, each a latency chain of its own)
inline PipStep pip_plan_tail(const PipPlanIn &in, int tail_waves, int curS, int upper, bool pending) {
  const bool wide16 = in.ebits == 128 && in.W <= 256 && upper <= 256 && !in.waves_per_job && !in.tail_waves;
  return PipStep{PIP_K_GENERAL, wide16 ? 16 : tail_waves, in.iter_limit, curS, false, !pending, false, pip_plan_full(in)};
}

#endif
