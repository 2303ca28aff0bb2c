// piplib_amd/csrc/pip_m2t.h -- tab_Matrix2Tableau (tab.c:292-393) for a ragged set of problems, on the device
// (pip_m2t.hip): launch interface.
#ifndef PIP_M2T_H
#define PIP_M2T_H
#include <hip/hip_runtime.h>
#include <stddef.h>

enum { M2T_MAXCOL = 512 };  // MAXCOL, type.h: the widest tableau the build kernel writes

// One pip_solve() call (piplib.c:722): its PolyLib matrices sit at input[src_off] -- nrows x ncols of inequnk, then
// crows x ccols of ineqpar, marker column first --, its tableaux are written to output[out_off] in QProb::in_off layout:
// ni x (nn + np + 1) domain rows, then nc x (np + 1) context rows, np = np0 + isnew + urs.
struct M2TProb {
  long long src_off, out_off;
  int nrows, ncols;  // inequnk
  int crows, ccols;  // ineqpar (0 x 0: NULL)
  int nn, np0;       // unknowns; parameters of the matrices (ineqpar's NbColumns - 2)
  int bg;            // Bg as traiter() gets it: a column of the domain tableau, or -1
  int shift;         // 1 Maximize, -1 Urs_unknowns, 0 neither (piplib.c:777-783)
  int urs;           // Urs_parms: negated copies of the parameters behind the last column (piplib.c:785-788)
  int isnew;         // bignum_is_new (tab.c:311-313): Bg is a fresh column, the context gets a zero column there
  int ni, nc;        // rows of the two tableaux, equalities counted twice (piplib.c:767-770, 808-811)
};

extern "C" {
// range[i] = 1 where the big column of problem i, or its twin under an equality, leaves 64 bits (the value written is
// the reference's wrapped one), else 0
hipError_t pipk_launch_m2t(const M2TProb *probs, const long long *input, long long *output, int *range, int nprob,
                           hipStream_t stream);
}
#endif
