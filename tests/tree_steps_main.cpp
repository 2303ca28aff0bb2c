// tests/tree_steps_main.cpp -- drives piplib_amd/csrc/pip_tree_steps.h alone, on the CPU (tests/test_tree_steps.py builds
// it with the host compiler and the address / undefined-behaviour sanitizers and runs it as a child process).
// One case per line of stdin, "<bits> <command> <integers ...>", one line of results each; a context per width is kept
// between lines ("ctx" sets it, "cut" / "fork" / "else" change it).  Lists are separated by ";".
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>

#include "../piplib_amd/csrc/pip_tree_steps.h"

using namespace pip_steps;

template <class E>
struct Runner {
  typedef typename UT<E>::type U;
  CtxT<E> ctx;
  int ctx_nparm = 0;
  std::string out;

  static E parse(const std::string &s) {  // decimal, wrapped to the width
    U v = 0;
    size_t k = (s[0] == '-' || s[0] == '+') ? 1 : 0;
    for (; k < s.size(); k++) v = v * 10 + (U)(s[k] - '0');
    return (E)(s[0] == '-' ? (U)0 - v : v);
  }
  void put(E x) {
    U v = x < 0 ? (U)0 - (U)x : (U)x;
    std::string d;
    do {
      d.insert(d.begin(), (char)('0' + (int)(v % 10)));
      v /= 10;
    } while (v);
    out += (x < 0 ? " -" : " ") + d;
  }
  void sep() { out += " ;"; }
  E next(std::istringstream &in) {
    std::string s;
    in >> s;
    return parse(s);
  }
  std::vector<E> list(std::istringstream &in, int n) {
    std::vector<E> v(n);
    for (E &x : v) x = next(in);
    return v;
  }
  auto cells() {
    return [this](int kind, E a, E b) {
      put((E)kind);
      put(a);
      put(b);
    };
  }
  void put_ctx(int nparm) {  // rows in use x (nparm parameters | constant)
    put((E)ctx.nc);
    for (int r = 0; r < ctx.nc; r++)
      for (int c = 0; c <= nparm; c++) put(ctx.at(r, c));
  }

  void line(std::istringstream &in) {
    std::string cmd;
    in >> cmd;
    out.clear();
    if (cmd == "op") {
      std::string name;
      in >> name;
      const E a = next(in), b = next(in);
      if (name == "wadd") put(wadd(a, b));
      else if (name == "wsub") put(wsub(a, b));
      else if (name == "wmul") put(wmul(a, b));
      else if (name == "wneg") put(wneg(a));
      else if (name == "wabs") put(wabs(a));
      else if (name == "crem") put(crem(a, b));
      else if (name == "cquo") put(cquo(a, b));
      else if (name == "fmod") put(fmod_(a, b));
      else if (name == "gcd") put(gcd(a, b));
      else if (name == "floordiv") put(floordiv(a, b));
      else if (name == "bezout") put(bezout(a, b, next(in)));
      else out = " unknown op";
    } else if (cmd == "flag") {
      const int p = (int)next(in), m = (int)next(in), c = (int)next(in);
      put((E)compa_flag(p != 0, m != 0, c != 0));
    } else if (cmd == "rows") {
      const int nparm = (int)next(in), critic = (int)next(in);
      const E cst = next(in);
      const std::vector<E> parms = list(in, nparm);
      std::vector<E> plus(nparm + 1), minus(nparm + 1);
      compa_rows(cst, parms.data(), nparm, critic != 0, plus.data(), minus.data());
      for (E x : plus) put(x);
      sep();
      for (E x : minus) put(x);
    } else if (cmd == "ctx") {
      const int nparm = (int)next(in), nc = (int)next(in);
      ctx = CtxT<E>();
      ctx.reserve(nc + 4, nparm + 2);
      ctx.nc = nc;
      for (int r = 0; r < nc; r++)
        for (int c = 0; c <= nparm; c++) ctx.at(r, c) = next(in);
      put((E)nc);
    } else if (cmd == "cut") {
      const int nvar = (int)next(in);
      int nparm = (int)next(in);
      const int bigparm = (int)next(in), deepest = (int)next(in);
      const E D = next(in);
      const std::vector<E> r = list(in, nvar + nparm + 1);
      std::vector<E> row;
      std::string tape;
      int newcol = -2;
      out.swap(tape);
      const CutKind kind = parm_cut(r.data(), D, nvar, nparm, bigparm, deepest != 0, ctx, cells(), row, newcol);
      out.swap(tape);
      put((E)(int)kind);
      put((E)nparm);
      put((E)newcol);
      sep();
      if (kind == CUT_CONST || kind == CUT_PARM)
        for (E x : row) put(x);
      sep();
      out += tape;
      sep();
      put_ctx(nparm);
    } else if (cmd == "fork") {
      const int nparm = (int)next(in), integer = (int)next(in);
      const E cst = next(in);
      const std::vector<E> parms = list(in, nparm);
      fork_row(cst, parms.data(), nparm, integer != 0, ctx, cells());
      sep();
      for (int c = 0; c <= nparm; c++) put(ctx.at(ctx.nc, c));
      sep();
      put((E)ctx.nc);
    } else if (cmd == "else") {
      const int nparm = (int)next(in);
      fork_else(ctx, nparm);
      put_ctx(nparm);
    } else if (cmd == "sol") {
      const int nvar = (int)next(in), nparm = (int)next(in);
      const std::vector<E> num = list(in, nvar * (nparm + 1)), den = list(in, nvar);
      push_solution(cells(), nvar, nparm, num.data(), den.data());
    } else {
      out = " unknown command";
    }
    printf("%s\n", out.c_str() + (out.empty() ? 0 : 1));
  }
};

int main() {
  Runner<long long> r64;
  Runner<__int128> r128;
  std::string text;
  while (std::getline(std::cin, text)) {
    if (text.empty()) continue;
    std::istringstream in(text);
    int bits = 0;
    in >> bits;
    if (bits == 64)
      r64.line(in);
    else if (bits == 128)
      r128.line(in);
    else
      return 2;
  }
  return 0;
}
