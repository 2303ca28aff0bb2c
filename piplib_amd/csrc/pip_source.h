// piplib_amd/csrc/pip_source.h -- what the batch layer's front ends refuse, and the PipBatchSource (pip_job.h) they launch from.
// Host only and free of HIP calls (tests/batch_source_main.cpp builds it alone): every entry of pip_host.cpp runs its form's
// check here, which reports a refusal under the entry's name `who` and otherwise fills the source in place; load_from /
// dual_from then launch from it.  Header comments of the entries: include/piplib_amd.h.
#ifndef PIP_SOURCE_H
#define PIP_SOURCE_H
#include <string.h>

#include "pip_job.h"

void pipamd_set_error(const char *fmt, ...);
extern "C" int pipk_batch_dual_max_ni(void); /* inequalities per tableau pip_batch_dual_kernel sorts in LDS */

// the members every kind but the tableau rows fills
static void source_fill(PipBatchSource *src, int kind, int shift, int simplify, int nrows, const int64_t *rows) {
  src->kind = kind;
  src->shift = shift;
  src->simplify = simplify;
  src->nrows = nrows;
  src->rows = rows;
}

// Maximize / Urs_unknowns: what the shifted load and the shifted results refuse alike
static int shifted_check(const char *who, const void *e, const void *d_ws, const pipamd_batch_desc *d, int shift) {
  if (!e || !d_ws || !d) {
    pipamd_set_error("%s: null engine, workspace or descriptor", who);
    return PIPAMD_E_INVALID;
  }
  if (shift != PIPAMD_SHIFT_MAX && shift != PIPAMD_SHIFT_URS) {
    pipamd_set_error("%s: shift must be PIPAMD_SHIFT_MAX (1) or PIPAMD_SHIFT_URS (-1), not %d", who, shift);
    return PIPAMD_E_INVALID;
  }
  if (d->nparm != 1 || d->bigparm != d->nvar + 1) {
    pipamd_set_error("%s: the descriptor must describe the shifted tableau (nparm == 1, bigparm == nvar + 1)", who);
    return PIPAMD_E_INVALID;
  }
  return PIPAMD_OK;
}

// the shifted load is the load of a dense system of d->ni rows without equalities, not simplified
static int shifted_source(const char *who, const void *e, const void *d_ws, const pipamd_batch_desc *d, const int64_t *d_rows,
                          int shift, PipBatchSource *src) {
  int rc = shifted_check(who, e, d_ws, d, shift);
  if (rc) return rc;
  if (!d_rows) {
    pipamd_set_error("%s: null rows pointer", who);
    return PIPAMD_E_INVALID;
  }
  source_fill(src, PIP_SRC_DENSE, shift, 0, d->ni, d_rows);
  memset(&src->mask, 0, sizeof src->mask);
  return PIPAMD_OK;
}

// What the dual entries refuse on top of their form's check; `src` is pipamd_batch_dual's when it gets here unchecked:
// tableau rows, which may still be null and which only a batch without parameters is read against.
static int dual_check(const char *who, const pipamd_batch_desc *d, const PipBatchSource *src, const void *d_dual_num,
                      const void *d_dual_den) {
  const bool tableau = src->kind == PIP_SRC_TABLEAU;
  if (!d || (tableau && !src->rows) || !d_dual_num || !d_dual_den) {
    pipamd_set_error("%s: null descriptor, rows or output array", who);
    return PIPAMD_E_INVALID;
  }
  if (!(d->tflags & PIPAMD_T_DUAL) || (d->tflags & PIPAMD_T_INT)) {
    pipamd_set_error("%s: the batch must have been solved with PIPAMD_T_DUAL and without PIPAMD_T_INT (the dual needs a "
                     "rational solve)", who);
    return PIPAMD_E_INVALID;
  }
  if (d->ni > pipk_batch_dual_max_ni()) {
    pipamd_set_error("%s: %d inequalities per tableau, the dual kernel sorts at most %d", who, d->ni, pipk_batch_dual_max_ni());
    return PIPAMD_E_TOOLARGE;
  }
  if (tableau && (d->nparm != 0 || d->bigparm >= 0)) {
    pipamd_set_error("%s: nparm must be 0 and bigparm -1 (the batch layer finishes only such batches on its own)", who);
    return PIPAMD_E_INVALID;
  }
  return PIPAMD_OK;
}

// pip_solve's plain system: equalities, tab_simplify and the dual as pip_solve hands it out.
// What the system and the matrices entries refuse alike: null pointers (`desc`: the system or matrices description), the
// shift and the descriptor against it ...
static int plain_check(const char *who, const void *e, const void *d_ws, const pipamd_batch_desc *d, const void *desc,
                       const void *d_rows, int shift) {
  if (!e || !d_ws || !d || !desc || !d_rows) {
    pipamd_set_error("%s: null engine, workspace, descriptor, system or rows pointer", who);
    return PIPAMD_E_INVALID;
  }
  if (shift != 0 && shift != PIPAMD_SHIFT_MAX && shift != PIPAMD_SHIFT_URS) {
    pipamd_set_error("%s: shift must be 0, PIPAMD_SHIFT_MAX (1) or PIPAMD_SHIFT_URS (-1), not %d", who, shift);
    return PIPAMD_E_INVALID;
  }
  if (shift ? (d->nparm != 1 || d->bigparm != d->nvar + 1) : (d->nparm != 0 || d->bigparm != -1)) {
    pipamd_set_error("%s: the descriptor must describe the tableau as it is solved (shift 0: nparm == 0, bigparm == -1; "
                     "otherwise nparm == 1, bigparm == nvar + 1)", who);
    return PIPAMD_E_INVALID;
  }
  return PIPAMD_OK;
}

// ... and simplify
static int simplify_check(const char *who, const pipamd_batch_desc *d, int simplify) {
  if (simplify != 0 && simplify != 1) {
    pipamd_set_error("%s: simplify must be 0 or 1, not %d", who, simplify);
    return PIPAMD_E_INVALID;
  }
  if (simplify && !(d->tflags & PIPAMD_T_INT)) {
    pipamd_set_error("%s: simplify without PIPAMD_T_INT (pip_solve simplifies integer problems only)", who);
    return PIPAMD_E_INVALID;
  }
  return PIPAMD_OK;
}

// the dense system; the caller's equality list is read into the source's mask, so nothing of it has to outlive the call
static int system_check(const char *who, const void *e, const void *d_ws, const pipamd_batch_desc *d, const pipamd_system *sys,
                        const int64_t *d_rows, PipBatchSource *src) {
  int rc = plain_check(who, e, d_ws, d, sys, d_rows, sys ? sys->shift : 0);
  if (rc) return rc;
  if (sys->nrows < 0 || sys->neq < 0 || sys->neq > sys->nrows || d->ni != sys->nrows + sys->neq) {
    pipamd_set_error("%s: %d rows with %d equalities do not make the descriptor's %d inequalities", who, sys->nrows, sys->neq,
                     d->ni);
    return PIPAMD_E_INVALID;
  }
  if (sys->nrows > PIPAMD_SMAX) {
    pipamd_set_error("%s: %d rows, the engine holds at most %d", who, sys->nrows, PIPAMD_SMAX);
    return PIPAMD_E_TOOLARGE;
  }
  if (sys->neq > 0 && !sys->eq_rows) {
    pipamd_set_error("%s: %d equalities and no list of them", who, sys->neq);
    return PIPAMD_E_INVALID;
  }
  rc = simplify_check(who, d, sys->simplify);
  if (rc) return rc;
  source_fill(src, PIP_SRC_DENSE, sys->shift, sys->simplify, sys->nrows, d_rows);
  memset(&src->mask, 0, sizeof src->mask);
  for (int i = 0; i < sys->neq; i++) {
    const int r = sys->eq_rows[i];
    if (r < 0 || r >= sys->nrows || (i > 0 && r <= sys->eq_rows[i - 1])) {
      pipamd_set_error("%s: eq_rows[%d] = %d is out of range or not above its predecessor", who, i, r);
      return PIPAMD_E_INVALID;
    }
    src->mask.w[r >> 6] |= (uint64_t)1 << (r & 63);
  }
  return PIPAMD_OK;
}

// The plain system as sparse rows: the system entries' checks on `sys` and the descriptor, with the row pointers in the
// place of the rows; what the arrays hold is checked on the device.
static int sparse_check(const char *who, const void *e, const void *d_ws, const pipamd_batch_desc *d, const pipamd_sparse *s,
                        PipBatchSource *src) {
  int rc = system_check(who, e, d_ws, d, s ? &s->sys : nullptr, s ? s->d_row_ptr : nullptr, src);
  if (rc) return rc;
  if (s->nnz < 0 || (s->nnz > 0 && (!s->d_cols || !s->d_vals))) {
    pipamd_set_error("%s: nnz (%lld) below 0, or entries without a column or a value array", who, (long long)s->nnz);
    return PIPAMD_E_INVALID;
  }
  src->kind = PIP_SRC_CSR;
  src->rows = nullptr;
  src->csr.row_ptr = s->d_row_ptr;
  src->csr.cols = s->d_cols;
  src->csr.vals = s->d_vals;
  src->csr.nnz = s->nnz;
  return PIPAMD_OK;
}

// The instances of one parametric system: the system entries' checks on `sys` and the descriptor, with the shared matrix
// in the place of the rows; the substitution, and whether a system's constants fit the entry type, is the device's business.
static int instances_check(const char *who, const void *e, const void *d_ws, const pipamd_batch_desc *d, const pipamd_instances *in,
                           PipBatchSource *src) {
  int rc = system_check(who, e, d_ws, d, in ? &in->sys : nullptr, in ? in->d_matrix : nullptr, src);
  if (rc) return rc;
  if (in->nparm < 0 || in->reserved != 0 || (in->nparm > 0 && !in->d_points)) {
    pipamd_set_error("%s: nparm (%d) below 0, reserved (%d) not 0, or parameters without an array of points", who, in->nparm,
                     in->reserved);
    return PIPAMD_E_INVALID;
  }
  if ((int64_t)d->nvar + in->nparm + 1 > PIPAMD_MAXCOL) {
    pipamd_set_error("%s: a matrix row of %d unknowns, %d parameters and the constant, at most %d columns", who, d->nvar,
                     in->nparm, PIPAMD_MAXCOL);
    return PIPAMD_E_TOOLARGE;
  }
  src->kind = PIP_SRC_INSTANCES;
  src->rows = nullptr;
  src->inst.matrix = in->d_matrix;
  src->inst.points = in->d_points;
  src->inst.nparm = in->nparm;
  return PIPAMD_OK;
}

// PolyLib matrices with a row count and markers per system.  Which rows are equalities and how many rows a system has is
// found on the device; what is left to refuse here is the description.
static int matrices_check(const char *who, const void *e, const void *d_ws, const pipamd_batch_desc *d, const pipamd_matrices *m,
                          const int64_t *d_rows, PipBatchSource *src) {
  int rc = plain_check(who, e, d_ws, d, m, d_rows, m ? m->shift : 0);
  if (rc) return rc;
  if (m->max_rows < 1 || d->ni < 1 || m->reserved != 0) {
    pipamd_set_error("%s: max_rows (%d) and the descriptor's ni (%d) must be at least 1, reserved (%d) must be 0", who, m->max_rows,
                     d->ni, m->reserved);
    return PIPAMD_E_INVALID;
  }
  if (m->max_rows > PIPAMD_SMAX) {
    pipamd_set_error("%s: %d rows of room per system, the engine holds at most %d", who, m->max_rows, PIPAMD_SMAX);
    return PIPAMD_E_TOOLARGE;
  }
  rc = simplify_check(who, d, m->simplify);
  if (rc) return rc;
  source_fill(src, PIP_SRC_MATRICES, m->shift, m->simplify, m->max_rows, d_rows);
  src->markers.nrows = m->d_nrows;
  src->markers.max_rows = m->max_rows;
  return PIPAMD_OK;
}
#endif
