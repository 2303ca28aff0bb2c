// tests/wide_main.cpp -- drives the host half of piplib_amd/csrc/pip_wide.h alone, on the CPU (tests/test_wide_host.py
// builds it with the host compiler and the address / undefined-behaviour sanitizers and runs it as a child process): the
// text the kernels compile, run where a sanitizer may run.
// One case per line of stdin, "<function> <operands ...>", one line of results each.  Every operand and every result is
// a 128-bit pattern in two hex words, low then high; narrower operands take its low bits, an int result is sign-extended,
// a double travels as its bit pattern.
#include <stdio.h>
#include <string.h>

#include <string_view>

#include "../piplib_amd/csrc/pip_wide.h"

static u128 arg[2];
static void put(u128 v) { printf(" %llx %llx", (u64)v, (u64)(v >> 64)); }
static void put_int(int v) { put((u128)(i128)v); }
static void put_divmod(PipDivMod d) {
  put(d.q);
  put(d.r);
}
static double as_double(u128 v) {
  const u64 w = (u64)v;
  double d;
  memcpy(&d, &w, sizeof d);
  return d;
}
static void put_double(double d) {
  u64 w;
  memcpy(&w, &d, sizeof w);
  put(w);
}

int main() {
  char fn[32];
  while (scanf("%31s", fn) == 1) {
    const int nargs = (!strncmp(fn, "divmod", 6) || !strncmp(fn, "wadd", 4) || !strncmp(fn, "wsub", 4) || !strncmp(fn, "wmul", 4)) ? 2 : 1;
    for (int k = 0; k < nargs; k++) {
      u64 lo, hi;
      if (scanf("%llx %llx", &lo, &hi) != 2) return 2;
      arg[k] = ((u128)hi << 64) | lo;
    }
    const u128 a = arg[0], b = arg[1];
    const std::string_view f(fn);
    if (f == "bitlen32") put_int(bitlen((unsigned)a));
    else if (f == "bitlen64") put_int(bitlen((u64)a));
    else if (f == "bitlen128") put_int(bitlen(a));
    else if (f == "ctz32") put_int(ctz((unsigned)a));
    else if (f == "ctz64") put_int(ctz((u64)a));
    else if (f == "ctz128") put_int(ctz(a));
    else if (f == "fits64") put_int(fits64((i128)a) ? 1 : 0);
    else if (f == "uabs32") put(uabs((int)(unsigned)a));
    else if (f == "uabs64") put(uabs((i64)(u64)a));
    else if (f == "uabs128") put(uabs((i128)a));
    else if (f == "inv32") put(inv_odd((unsigned)a));
    else if (f == "inv64") put(inv_odd((u64)a));
    else if (f == "inv128") put(inv_odd(a));
    else if (f == "todouble64") put_double(to_double((i64)(u64)a));
    else if (f == "todouble128") put_double(to_double((i128)a));
    else if (f == "trunc") put_int(trunc_x86(as_double(a)));
    else if (f == "divmod_native") put_divmod(udivmod<true>(a, b));
    else if (f == "divmod_wide") put_divmod(udivmod<false>(a, b));
    else if (f == "wneg64") put((u64)wneg((i64)(u64)a));
    else if (f == "wadd64") put((u64)wadd((i64)(u64)a, (i64)(u64)b));
    else if (f == "wsub64") put((u64)wsub((i64)(u64)a, (i64)(u64)b));
    else if (f == "wmul64") put((u64)wmul((i64)(u64)a, (i64)(u64)b));
    else if (f == "wneg128") put((u128)wneg((i128)a));
    else if (f == "wadd128") put((u128)wadd((i128)a, (i128)b));
    else if (f == "wsub128") put((u128)wsub((i128)a, (i128)b));
    else if (f == "wmul128") put((u128)wmul((i128)a, (i128)b));
    else return 3;
    printf("\n");
  }
  return 0;
}
