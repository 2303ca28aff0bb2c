// piplib_amd/csrc/pip_m2t.hip -- tab_Matrix2Tableau (tab.c:292-393) on the device, for a ragged set of pip_solve()
// calls: what piplib.c:813 and piplib.c:846 build on the way to traiter(), written where the device-resident traiter()
// (pip_quast.hip) reads its problems.
//
// One wave64 per problem.  A lane owns the output columns lane, lane + 64, ... of a row: for each it works out the
// matrix column it comes from and its sign, so a row is one coalesced load, one store, and a second store for the
// negated twin of an equality.  The sum that goes to the big column (Maximize / Urs_unknowns) is added up over the
// unknowns' lanes with a wave reduction -- wrap-around addition is associative, so the order does not matter -- and the
// lane that owns the big column stores it last.  The sum is carried in 128 bits beside the wrapped value so that the
// overflow-safe flavour can refuse a problem whose big column left 64 bits.  tab_simplify is not done here: the device
// tree and the host trees do it when they load the rows.
#include <hip/hip_runtime.h>

#include "pip_m2t.h"
#include "pip_wide.h"

namespace {
typedef i64 w64;  // an input coefficient: wneg() on it is piplib_int_oppose on long long, which wraps
typedef i128 w128;

// Output column c of the domain tableau, unknowns | constant | parameters | new big | urs copies: the matrix column it
// is copied from (-1: none, the new big column) and whether it is negated (tab.c:342-367).
__device__ __forceinline__ int dom_src(const M2TProb &P, int c, bool &neg) {
  neg = false;
  if (c < P.nn) {
    neg = P.shift > 0;
    return 1 + c;
  }
  if (c == P.nn) return P.ncols - 1;
  if (c <= P.nn + P.np0) return c;
  const int nb = P.nn + P.np0 + 1 + P.isnew;  // nb_columns
  if (c < nb) return -1;
  int pos = c - P.urs;  // tab.c:358-365
  if (pos <= P.bg) --pos;
  neg = true;
  return pos;
}
// The same for the context tableau, parameters | new big | urs copies | constant (Shift = 0, Bg - Nn - 1 for Bg).
__device__ __forceinline__ int ctx_src(const M2TProb &P, int c, bool &neg) {
  neg = false;
  if (c < P.np0) return 1 + c;
  const int nb = P.np0 + P.isnew;  // nb_columns - ctx
  if (c < nb) return -1;
  if (c == nb + P.urs) return P.ccols - 1;
  int pos = c - P.urs;
  if (pos <= (P.bg >= 0 ? P.bg - P.nn - 1 : -1)) --pos;
  neg = true;
  return 1 + pos;
}

// `rows` x `cols` of a matrix to at most `orows` x W of a tableau; returns true where the big column left 64 bits
template <bool CTX>
__device__ bool build_rows(const M2TProb &P, const w64 *m, int rows, int cols, w64 *out, int orows, int W, int lane) {
  const bool sum_on = !CTX && P.shift != 0;
  bool bad = false;
  for (int i = 0, o = 0; i < rows; i++) {
    const w64 *r = m + (size_t)i * cols;
    const bool eq = r[0] == 0;            // piplib.c:769, tab.c:335
    if (o + (eq ? 2 : 1) > orows) break;  // (the host counted the same markers: never taken)
    w64 *d = out + (size_t)o * W;
    w128 part = 0;
    w64 bigv = 0;
    for (int c = lane; c < W; c += 64) {
      bool neg;
      const int s = CTX ? ctx_src(P, c, neg) : dom_src(P, c, neg);
      w64 v = s >= 0 ? r[s] : 0;
      if (sum_on && c < P.nn) part += v;
      if (neg) v = wneg(v);
      if (sum_on && c == P.bg) {
        bigv = v;
      } else {
        d[c] = v;
        if (eq) d[W + c] = wneg(v);
      }
    }
    if (sum_on) {
      w128 sum = wave_sum(part);  // tab.c:346, 368-377
      if (P.shift < 0) sum = -sum;
      if (lane == (P.bg & 63)) {
        const w128 b = sum + bigv;
        const w64 w = (w64)(u64)(u128)b;
        bad |= b != (w128)w || (eq && w == (w64)(1ull << 63));
        d[P.bg] = w;
        if (eq) d[W + P.bg] = wneg(w);
      }
    }
    o += eq ? 2 : 1;
  }
  return bad;
}

__global__ __launch_bounds__(256) void pip_m2t_kernel(const M2TProb *probs, const w64 *in, w64 *out, int *range, int nprob) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= nprob) return;
  const M2TProb P = probs[k];
  const int np = P.np0 + P.isnew + P.urs, W = P.nn + np + 1;
  const w64 *m = in + P.src_off;
  w64 *t = out + P.out_off;
  bool bad = build_rows<false>(P, m, P.nrows, P.ncols, t, P.ni, W, lane);
  bad |= build_rows<true>(P, m + (size_t)P.nrows * P.ncols, P.crows, P.ccols, t + (size_t)P.ni * W, P.nc, np + 1, lane);
  const u64 any = __ballot(bad);
  if (lane == 0) range[k] = any != 0;
}
}  // namespace

extern "C" hipError_t pipk_launch_m2t(const M2TProb *probs, const long long *input, long long *output, int *range, int nprob,
                                      hipStream_t stream) {
  if (nprob <= 0) return hipSuccess;
  hipLaunchKernelGGL(pip_m2t_kernel, dim3((nprob + 3) / 4), dim3(256), 0, stream, probs, input, output, range, nprob);
  return hipGetLastError();
}
