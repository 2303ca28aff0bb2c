// piplib_amd/csrc/pip_quast.h -- the device-resident traiter() of pip_quast.hip: launch interface.
#ifndef PIP_QUAST_H
#define PIP_QUAST_H
#include <hip/hip_runtime.h>
#include <stddef.h>

// one problem: its rows sit at input[in_off]: ni x (nvar+nparm+1) inequalities, then nc x (nparm+1) context rows
struct QProb {
  long long in_off;
  int nvar, nparm, ni, nc, bigparm, nq;
  int flags, pad;  // Q_NO_CONTEXT_TEST: traiter() proper (the front ends test the context in a call of its own)
};
enum { Q_NO_CONTEXT_TEST = 1,
       Q_DUAL = 2 };  // Compute_dual (traiter.c:273-294): the list of dual values behind every (rational) solution
// capacities of one launch (every problem of the launch gets the same LDS image and HBM regions)
struct QCaps {
  int R, S, W;    // main tableau: logical rows, real-row slots, columns (W <= 128: two column blocks beyond 64; S <= 128)
  int CR, CW;     // context: rows, columns (parameters | constant; CW <= 64)
  int SR, SS;     // compa_test sub-problems: logical rows, real-row slots (their width is CW)
  int depth;      // frames of the fork stack
  int cells;      // tape cells
  int deepest;    // deepest-cut option (integrer.c:417-438)
  int simplify;   // tab_simplify on the inputs of integer problems (maind.c:190-196)
};
// out[Q_OUT*i]: result; +1: cells; +2: pivots; +3: why a problem was handed back (Q_WHY_* bits);
// +4: run time of the problem's wave in 10 ns units; +5: cells written when it stopped
enum { Q_DONE = 0, Q_VOID = 1, Q_FALLBACK = 2 };
enum { Q_OUT = 6 };
enum {
  Q_WHY_OVERFLOW = 1,  // a 64-bit product / sum overflowed, or the determinant did ("Integer overflow")
  Q_WHY_ROWS = 2,      // rows, columns or context rows reserved for the problem ran out
  Q_WHY_TAPE = 4,      // SOL_SIZE cells
  Q_WHY_STACK = 8,     // fork depth
  Q_WHY_OTHER = 16     // too many parameters, iteration guard, assert(ok_var), ...
};

// ---- testing aid (pip_probe.hip, pipamd_debug_quast_step; tests/test_gpu_quast_step_probe.py): one wave-level step of the
// device tree -- classify_rows, sort_rows, pivot_step, make_cut, deepen, find_quotient, build_sub, solve_plain -- on a
// tableau the caller gives.  `in`: words 0, 1 the lengths of `in` and `out` in words, then the cases' offsets into `in`
// (ncases words) and into `out` (ncases words), then the cases.  A case, in int64 words (a value of the instantiation's
// entry type is one word, or two, low then high):
//   the QS_HDR header words in the order of QStepCase (two reserved words behind them)
//   flag[R], ref[R], pos[128]                                                    a word each
//   det[4], den[R], val[S * W], ctx[CR * CW], cutv[CW + 2]                       values
// out: status (1: the step ran), its return value (the lanes' values or-ed), aux (bits 0..2 ok_var, ok_const, ok_parm of
// make_cut; bits 8.. the `bad` that deepen / find_quotient left), ldet; flag[R], ref[R], pos[128], skey[128] a word each;
// det[4], den[R], val[S * W], ctx[CR * CW], cutv[CW + 2] and the cut vector (64 values per column block) as values.
// pivi is the pivot row of QS_PIVOT and the row i of the cut steps; QS_DEEPEN reads the cut vector from row i itself, and
// QS_BUILD_SUB its extra row (a lane per column, as compa_test hands it over) from cutv.
enum { QS_CLASSIFY, QS_SORT, QS_PIVOT, QS_MAKE_CUT, QS_DEEPEN, QS_CUT_CHAIN, QS_FIND_QUOTIENT, QS_BUILD_SUB, QS_SOLVE_PLAIN, QS_NFN };
enum { QS_HDR = 20, QS_POS = 128, QS_SKEY = 128, QS_SKEY_FILL = -2,
       QS_OPT_POS = 1, QS_OPT_SKEY = 2, QS_OPT_EXTRA = 4,  // `opts`: hand sort_rows pos / skey; build_sub gets the extra row
       QS_LDS_MAX = 65536 };                               // the dynamic LDS a kernel gets without asking for more
struct QStepCase {
  int fn, W, S, R, nvar, ncol, nligne, ni, bigparm, pivi, CR, CW, nc, nparm, deepest, budget, opts, ldet;
};
static inline __host__ __device__ void qstep_read(const long long *c, QStepCase *g) {
  int *f = &g->fn;
  for (int k = 0; k < 18; k++) f[k] = (int)c[k];
}
// values of a case's image in LDS and in `in`, and the bytes of the image; EB bytes a value
static inline __host__ __device__ size_t qstep_values(const QStepCase &g) {
  return 4 + (size_t)g.R + (size_t)g.S * g.W + (size_t)g.CR * g.CW + (size_t)g.CW + 2;
}
static inline __host__ __device__ size_t qstep_lds_bytes(const QStepCase &g, size_t EB) {
  return EB * qstep_values(g) + 8 * (size_t)g.R + 16 + 4 * QS_SKEY + QS_POS;
}
static inline __host__ __device__ size_t qstep_in_words(const QStepCase &g, size_t EW) {
  return QS_HDR + 2 * (size_t)g.R + QS_POS + EW * qstep_values(g);
}
static inline __host__ __device__ size_t qstep_out_words(const QStepCase &g, size_t EW, int NB) {
  return 4 + 2 * (size_t)g.R + QS_POS + QS_SKEY + EW * (qstep_values(g) + 64 * (size_t)NB);
}

extern "C" {
// inst: 0 <long long, 1>, 1 <long long, 2>, 2 <__int128, 1>, 3 <__int128, 2>; shm: the largest image among the cases
hipError_t pipk_launch_quast_step(int inst, const long long *in, long long *out, int ncases, size_t shm, hipStream_t stream);
// ebits: the entry width of the launch, 64 (the reference's long long build) or 128 (the overflow-safe flavour)
size_t pipk_quast_lds_bytes(const QCaps *c, int ebits);
size_t pipk_quast_frame_words(const QCaps *c, int ebits);  // entries of one stack frame
hipError_t pipk_launch_quast(const QProb *probs, const long long *input, void *stack, void *cells, int *out, int nprob,
                             const QCaps *cap, int ebits, hipStream_t stream);
hipError_t pipk_launch_quast_pack(const long long *cells, const long long *off, long long *packed, int nprob,
                                  int cells_cap, int ebits, hipStream_t stream);
}
#endif
