// piplib_amd/csrc/pip_tree_steps.h -- what the host decision trees of layer 3 compute between pivot runs, once: the
// wrap-around integer helpers, the context with its quotient parameters, and the formulas of the reference's compa_test,
// integrer() and traiter() that decide bit-for-bit parity.  Host only: no HIP, no device memory, no PipJob -- plain
// pointers and vectors in, a push(kind, a, b) callable for the solution tape.  The per-problem TreeT and the lock-step
// ForestT (pip_tree.cpp) call these; where a row comes from, how a result reaches the device and what happens when a
// block is full stays with them.  tests/tree_steps_main.cpp drives this header alone, on the CPU.
#ifndef PIP_TREE_STEPS_H
#define PIP_TREE_STEPS_H
#include <stddef.h>

#include <algorithm>
#include <vector>

#include "pip_job.h"
#include "pip_wide.h"

namespace pip_steps {

using ::i64;
using ::u64;
using ::i128;

// ---- wrap-around integer helpers (piplib.h:128-169, integrer.c:43-74), host side, for both
// entry widths: E = long long (the reference's int64 build) or __int128 (the overflow-safe one)
template <class E> struct UT;
template <> struct UT<i64> { typedef u64 type; };
template <> struct UT<i128> { typedef u128 type; };
using ::wadd;  // pip_wide.h's wrap-around overloads for both widths
using ::wsub;
using ::wneg;
using ::wmul;
template <class E> inline E wabs(E a) { return a < 0 ? wneg(a) : a; }
template <class E> inline E crem(E a, E b) { return (b == 0 || b == -1) ? (E)0 : a % b; }
template <class E> inline E cquo(E a, E b) { return b == 0 ? (E)0 : (b == -1 ? wneg(a) : a / b); }
template <class E> E gcd(E a, E b) {
  while (b) {
    E t = crem(a, b);
    a = b;
    b = t;
  }
  return wabs(a);
}
template <class E> inline E fmod_(E a, E b) {
  E m = crem(a, b);
  if (m < 0) m = wadd(m, wabs(b));
  return m;
}
template <class E> inline E floordiv(E a, E b) { return cquo(wsub(a, fmod_(a, b)), b); }
template <class E> E bezout(E x, E y, E delta) {  // integrer.c:98-150
  E a = 1, b = 0, c = 0, d = 1, u = y, v = delta;
  for (;;) {
    E q = floordiv(u, v), r = fmod_(u, v);
    if (r == 0) break;
    u = v;
    v = r;
    E e = wsub(a, wmul(q, c)), f = wsub(b, wmul(q, d));
    a = c;
    b = d;
    c = e;
    d = f;
  }
  if (v != 1) return 0;
  return fmod_(wmul(c, x), delta);
}

enum { S_FREE = 0, S_NIL, S_IF, S_LIST, S_FORM, S_NEW, S_DIV, S_VAL }; /* sol.c:42-50 */
template <class E> struct CellT {
  int kind;
  E a, b;
};

// context: rows of (parameters | constant), traiter.c keeps it as a Tableau
template <class E> struct CtxT {
  int nc = 0, width = 0;  // rows in use, columns allocated per row
  std::vector<E> v;
  E &at(int r, int c) { return v[(size_t)r * width + c]; }
  E at(int r, int c) const { return v[(size_t)r * width + c]; }
  void reserve(int rows, int cols) {
    if (cols > width) {
      std::vector<E> nv((size_t)std::max(rows, nc + 4) * cols, 0);
      for (int r = 0; r < nc; r++)
        for (int c = 0; c < width; c++) nv[(size_t)r * cols + c] = v[(size_t)r * width + c];
      v.swap(nv);
      width = cols;
    }
    if ((size_t)rows * width > v.size()) v.resize((size_t)(rows + 8) * width, 0);
  }

  // ---- parameters introduced by parametric cuts (integrer.c:156-291) ----
  // A cut with parameter part c.p + c0 over the denominator D needs q = floor(-(c.p + c0) / D),
  // i.e. the parameter q with 0 <= -(c.p + c0) - D q <= D - 1.  The context stores such a
  // definition as the two rows of that double inequality, with q in a column of its own:
  //     lower:  -c.p - D q - c0          >= 0
  //     upper:   c.p + D q + c0 + D - 1  >= 0
  struct Quotient {
    std::vector<E> c;  // coefficients of the nparm existing parameters
    E c0, D;           // constant, divisor
  };
  // is there a row  sign * (c on the columns before p | D in column p | 0 behind it)  with constant cst?
  bool has_row(int nparm, int p, const Quotient &k, bool negated, E cst) const {
    for (int r = 0; r < nc; r++) {
      if (at(r, p) != (negated ? wneg(k.D) : k.D) || at(r, nparm) != cst) continue;
      bool same = true;
      for (int col = p + 1; col < nparm && same; col++) same = at(r, col) == 0;
      for (int col = 0; col < p && same; col++) same = at(r, col) == (negated ? wneg(k.c[col]) : k.c[col]);
      if (same) return true;
    }
    return false;
  }
  // A parameter the cut does not use (trailing zero coefficients) whose two defining rows are the
  // ones this quotient would get: its column, or -1 (find_parm, integrer.c:258-291).
  int find_quotient(int nparm, const Quotient &k) const {
    const E upper_cst = wsub(wadd(k.c0, k.D), (E)1);
    for (int p = nparm - 1; p >= 0 && k.c[p] == 0; --p)
      if (has_row(nparm, p, k, false, upper_cst) && has_row(nparm, p, k, true, wneg(k.c0))) return p;
    return -1;
  }
  // The new parameter takes column nparm (the constants move one column right) and its two rows
  // are appended (add_parm, integrer.c:194-224).  Returns its column.
  int define_quotient(int nparm, const Quotient &k) {
    const int nr = nc;
    reserve(nr + 2, nparm + 2);
    for (int r = 0; r < nr; r++) {
      at(r, nparm + 1) = at(r, nparm);
      at(r, nparm) = 0;
    }
    for (int j = 0; j < nparm; j++) {
      at(nr, j) = wneg(k.c[j]);
      at(nr + 1, j) = k.c[j];
    }
    at(nr, nparm) = wneg(k.D);
    at(nr + 1, nparm) = k.D;
    at(nr, nparm + 1) = wneg(k.c0);
    at(nr + 1, nparm + 1) = wadd(wsub(k.c0, (E)1), k.D);
    nc += 2;
    return nparm;
  }
  // what the solution tape says about it (integrer.c:173-188): New k, Div, the form -c.p - c0, D
  template <class PUSH>
  static void announce_quotient(PUSH &&push, int nparm, const Quotient &k) {
    push(S_NEW, (E)nparm, (E)0);
    push(S_DIV, (E)0, (E)0);
    push(S_FORM, (E)(nparm + 1), (E)0);
    for (int j = 0; j < nparm; j++) push(S_VAL, wneg(k.c[j]), (E)1);
    push(S_VAL, wneg(k.c0), (E)1);
    push(S_VAL, k.D, (E)1);
  }
};

// ---- compa_test (traiter.c:162-243) ----
// The two rows that join the context, one per sub-problem, for an undecided row  row_parms.p + row_const:
// ex_plus is "row >= 1" (>= 0 if the row is critical), ex_minus is "-row >= 1"; nparm + 1 entries each, constant last.
template <class E>
void compa_rows(E row_const, const E *row_parms, int nparm, bool critic, E *ex_plus, E *ex_minus) {
  for (int j = 0; j < nparm; j++) {
    ex_plus[j] = row_parms[j];
    ex_minus[j] = wneg(row_parms[j]);
  }
  ex_plus[nparm] = critic ? row_const : wsub(row_const, (E)1);
  ex_minus[nparm] = wsub(wneg(row_const), (E)1);
}
// the sign of the row, from which of the two sub-problems have no solution
inline int compa_flag(bool plus_is_nil, bool minus_is_nil, bool critic) {
  if (!plus_is_nil && !minus_is_nil) return critic ? PIPAMD_F_CRITIC : PIPAMD_F_UNKNOWN;
  if (!minus_is_nil) return PIPAMD_F_MINUS;
  return !plus_is_nil ? PIPAMD_F_PLUS : PIPAMD_F_ZERO;
}

// ---- integrer() for one non-integral row (integrer.c:357-520) ----
enum CutKind {
  CUT_NONE = 0,  // case (b): the row admits no cut, the problem has no solution
  CUT_CONST,     // case (d): a cut in the unknowns and the constant alone
  CUT_PARM,      // case (e): a parametric cut; cut_row carries the divisor in column newcol
  CUT_NO_VAR     // case (c), the reference's assert(ok_var) -- reported after the quotient is defined, as there
};
// r: the row (nvar unknowns | constant | nparm parameters), D its denominator.  A parametric cut finds or defines its
// quotient in ctx (a new one is announced through push and takes parameter column nparm, which is then incremented).
// cut_row: the row to append, nvar + nparm + 1 entries with the new nparm; newcol: the quotient's column in it, or -1.
// deepest: the deepest-cut option (integrer.c:417-438), which only touches constant cuts.
template <class E, class PUSH>
CutKind parm_cut(const E *r, E D, int nvar, int &nparm, int bigparm, bool deepest, CtxT<E> &ctx, PUSH &&push,
                 std::vector<E> &cut_row, int &newcol) {
  const int ncol = nvar + nparm + 1;
  std::vector<E> &cut = cut_row;
  cut.assign(ncol, 0);
  bool ok_var = false, ok_parm = false;
  for (int j = 0; j < nvar; j++) {
    cut[j] = fmod_(r[j], D);
    if (cut[j] > 0) ok_var = true;
  }
  cut[nvar] = wneg(fmod_(wneg(r[nvar]), D));
  for (int j = nvar + 1; j < ncol; j++) {
    if (j == bigparm) {
      cut[j] = 0;
      continue;
    }
    cut[j] = wneg(fmod_(wneg(r[j]), D));
    if (cut[j] != 0) ok_parm = true;
  }
  newcol = -1;
  if (!ok_parm) {
    if (!ok_var) return CUT_NONE;
    if (deepest) {  // integrer.c:417-438
      E t = wneg(cut[nvar]), delta = gcd(t, D), tau = cquo(t, delta), dd = cquo(D, delta);
      t = wsub(dd, (E)1);
      E lambda = bezout(t, tau, dd);
      t = gcd(lambda, D);
      while (t != 1) {
        lambda = wadd(lambda, dd);
        t = gcd(lambda, D);
      }
      for (int j = 0; j < nvar; j++) cut[j] = fmod_(wmul(lambda, cut[j]), D);
      t = fmod_(wmul(cut[nvar], lambda), D);
      t = wsub(D, t);
      cut[nvar] = wneg(t);
    }
    return CUT_CONST;
  }
  typename CtxT<E>::Quotient k{std::vector<E>(cut.begin() + nvar + 1, cut.begin() + ncol), cut[nvar], D};
  int parm = ctx.find_quotient(nparm, k);
  if (parm == -1) {
    CtxT<E>::announce_quotient(push, nparm, k);
    parm = ctx.define_quotient(nparm, k);
    nparm++;
    cut.push_back(0);
  }
  if (!ok_var) return CUT_NO_VAR;  // assert(ok_var), integrer.c:499
  newcol = nvar + 1 + parm;
  cut[newcol] = wadd(cut[newcol], D);
  return CUT_PARM;
}

// ---- the quast forks on the sign of a row (traiter.c:695-759) ----
// The "then" branch: the row, divided by the gcd of its parameter part (and of the constant, for a rational solve),
// becomes context row ctx.nc -- written, not yet counted: the child's copy counts it -- and If / Form / Val cells say so.
template <class E, class PUSH>
void fork_row(E row_const, const E *row_parms, int nparm, bool integer, CtxT<E> &ctx, PUSH &&push) {
  push(S_IF, (E)0, (E)0);
  push(S_FORM, (E)(nparm + 1), (E)0);
  E g = 0;
  for (int j = 0; j < nparm; j++) g = gcd(g, row_parms[j]);
  if (!integer) g = gcd(g, row_const);
  const int nc = ctx.nc;
  ctx.reserve(nc + 1, nparm + 2);
  for (int j = 0; j < nparm; j++) {
    ctx.at(nc, j) = cquo(row_parms[j], g);
    push(S_VAL, ctx.at(nc, j), (E)1);
  }
  ctx.at(nc, nparm) = integer ? floordiv(row_const, g) : cquo(row_const, g);
  push(S_VAL, ctx.at(nc, nparm), (E)1);
}
// The "else" branch (traiter.c:751-758): the row fork_row wrote, negated (-row - 1 >= 0), now counted.
template <class E>
void fork_else(CtxT<E> &ctx, int nparm) {
  const int nc = ctx.nc;
  for (int j = 0; j < nparm; j++) ctx.at(nc, j) = wneg(ctx.at(nc, j));
  ctx.at(nc, nparm) = wneg(wadd(ctx.at(nc, nparm), (E)1));
  ctx.nc = nc + 1;
}

// ---- the solution list (traiter.c:255-271): num is nvar x (nparm + 1), den one denominator per unknown ----
template <class E, class PUSH>
void push_solution(PUSH &&push, int nvar, int nparm, const E *num, const E *den) {
  push(S_LIST, (E)nvar, (E)0);
  for (int i = 0; i < nvar; i++) {
    push(S_FORM, (E)(nparm + 1), (E)0);
    for (int j = 0; j <= nparm; j++) push(S_VAL, num[(size_t)i * (nparm + 1) + j], den[i]);
  }
}

}  // namespace pip_steps
#endif
