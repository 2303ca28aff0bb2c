// tests/batch_source_main.cpp -- piplib_amd/csrc/pip_source.h on its own, for tests/test_batch_source_host.py: built with the
// host compiler under the address and undefined-behaviour sanitizers.  One case per input line, every field an integer:
//   form(0 shifted, 1 system, 2 sparse, 3 instances, 4 matrices, 5 tableau) dual e ws d nvar nparm ni bigparm tflags
//   desc rows nrows shift simplify a b c num den eq_list neq n r_0 .. r_(n-1)
// e, ws, d, desc, rows, num, den, eq_list: 1 = the pointer is there.  a, b, c: nnz, cols, vals (sparse); nparm, reserved, points
// (instances); reserved, d_nrows (matrices).  dual: dual_check runs behind the form's check.  The device pointers are
// addresses of nothing -- a check that looked behind one would fault -- and the equality list is a heap block of exactly
// n ints.  Answer: "rc | message" and, for rc 0, " | kind shift simplify nrows | rows row_ptr cols vals nnz matrix points
// nparm markers.nrows max_rows | the mask's rows" with the pointers as 0 / 1.
#include <stdarg.h>
#include <stdio.h>

#include <vector>

#include "../piplib_amd/csrc/pip_source.h"

static char g_err[512];
void pipamd_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
extern "C" int pipk_batch_dual_max_ni(void) { return 8192; }

template <class P>
static P *fake(int there, uintptr_t a) { return there ? (P *)a : nullptr; }

int main() {
  static const char *const who[] = {"batch_load_shifted", "batch_load_system", "batch_load_sparse", "batch_load_instances",
                                    "batch_load_matrices", "batch_dual"};
  int form, dual, e, ws, dp, nvar, nparm, ni, bigparm, tflags, desc, rows, nrows, shift, simplify, a, b, c, num, den, eql, neq, n;
  while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &form, &dual, &e, &ws, &dp, &nvar, &nparm, &ni,
               &bigparm, &tflags, &desc, &rows, &nrows, &shift, &simplify, &a, &b, &c, &num, &den, &eql, &neq, &n) == 23) {
    std::vector<int32_t> *list = new std::vector<int32_t>(n);  // (a block of its own: a read past n is the sanitizer's)
    for (int i = 0; i < n; i++)
      if (scanf("%d", &(*list)[i]) != 1) return 2;
    const pipamd_batch_desc d = {4, nvar, nparm, ni, bigparm, tflags, 4, 0, 64};
    const pipamd_system sys = {nrows, neq, eql ? list->data() : nullptr, shift, simplify};
    const pipamd_sparse sp = {sys, a, fake<const int64_t>(rows, 0x3000), fake<const int32_t>(b, 0x4000), fake<const int64_t>(c, 0x5000)};
    const pipamd_instances in = {sys, a, b, fake<const int64_t>(rows, 0x3000), fake<const int64_t>(c, 0x6000)};
    const pipamd_matrices m = {nrows, shift, simplify, a, fake<const int32_t>(b, 0x7000)};
    const void *E = fake<void>(e, 0x1000), *W = fake<void>(ws, 0x2000);
    const pipamd_batch_desc *D = dp ? &d : nullptr;
    const int64_t *R = fake<const int64_t>(rows, 0x3000);
    PipBatchSource *src = new PipBatchSource;  // (heap, not zeroed: a member of the kind left unfilled prints as garbage)
    g_err[0] = 0;
    int rc = 0;
    switch (form) {
      case 0: rc = shifted_source(who[0], E, W, D, R, shift, src); break;
      case 1: rc = system_check(who[1], E, W, D, desc ? &sys : nullptr, R, src); break;
      case 2: rc = sparse_check(who[2], E, W, D, desc ? &sp : nullptr, src); break;
      case 3: rc = instances_check(who[3], E, W, D, desc ? &in : nullptr, src); break;
      case 4: rc = matrices_check(who[4], E, W, D, desc ? &m : nullptr, R, src); break;
      default: src->kind = PIP_SRC_TABLEAU, src->rows = R; break;
    }
    if (!rc && dual) rc = dual_check(who[form], D, src, fake<void>(num, 0x8000), fake<void>(den, 0x9000));
    printf("%d | %s", rc, g_err);
    if (!rc) {
      const int k = src->kind;
      const bool masked = k == PIP_SRC_DENSE || k == PIP_SRC_CSR || k == PIP_SRC_INSTANCES;
      if (k == PIP_SRC_TABLEAU)
        printf(" | %d 0 0 0 | %d", k, src->rows != nullptr);
      else
        printf(" | %d %d %d %d | %d", k, src->shift, src->simplify, src->nrows, src->rows != nullptr);
      if (k == PIP_SRC_CSR)
        printf(" %d %d %d %lld", src->csr.row_ptr != nullptr, src->csr.cols != nullptr, src->csr.vals != nullptr, (long long)src->csr.nnz);
      else
        printf(" 0 0 0 0");
      if (k == PIP_SRC_INSTANCES)
        printf(" %d %d %d", src->inst.matrix != nullptr, src->inst.points != nullptr, src->inst.nparm);
      else
        printf(" 0 0 0");
      if (k == PIP_SRC_MATRICES)
        printf(" %d %d |", src->markers.nrows != nullptr, src->markers.max_rows);
      else
        printf(" 0 0 |");
      for (int r = 0; masked && r < 64 * (int)(sizeof src->mask.w / sizeof src->mask.w[0]); r++)
        if (src->mask.w[r >> 6] >> (r & 63) & 1) printf(" %d", r);
    }
    printf("\n");
    delete src;
    delete list;
  }
  return 0;
}
