// k_topk.hip — the K best entries of every row, in the arg-max's own order (PF_DECODE_TOPK, DESIGN.md §Top-k and n-best).
//
// Order: entry a ranks before entry b when y[a] > y[b], or y[a] == y[b] and a > b (the reference loop keeps the LARGER
// index of equal values, quirk Q4; -0.0 == +0.0).  NaN entries are never ranked.  n = min(K, non-NaN entries); slots
// r >= n hold id -1 and value -inf.  For a row without NaN rank 0 is what launch_argmax returns.
//
// One 256-thread workgroup per row, K selection rounds.  In round r a thread proposes its best entry that ranks STRICTLY
// AFTER the winner of round r - 1 — the order is total over (value, index), so "after the previous winner" is exactly
// "not taken yet": no taken flags, no atomics, no LDS copy of the row.  The 64 lanes reduce by shuffle, the four waves
// through LDS (two alternating slots: one barrier per round).  NV > 0: the row (V <= 256 * NV) is held in registers,
// entries at or beyond V as NaN, which no round can pick; NV == 0: the row is read again in every round (it stays in
// this CU's L1 / L2).  Nothing at or beyond V is read in a row and no row beyond `rows` is touched.
#include <climits>

#include "kernels.h"

namespace pf {

namespace {
struct TK { float v; int i; };            // i < 0: no entry
// the one of two distinct entries that ranks first
__device__ __forceinline__ TK tk_first(TK a, TK b) {
  if (b.i < 0) return a;
  if (a.i < 0) return b;
  if (a.v > b.v) return a;
  if (b.v > a.v) return b;
  return a.i > b.i ? a : b;
}
}  // namespace

template <int NV>
__global__ __launch_bounds__(256) void topk_kernel(const float* __restrict__ x, int V, int ldx, int K,
                                                   int64_t* __restrict__ ids, float* __restrict__ val,
                                                   int32_t* __restrict__ n_out) {
  __shared__ float s_v[2][4];
  __shared__ int s_i[2][4];
  const int64_t row = blockIdx.x;
  const float* xr = x + row * (int64_t)ldx;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float reg[NV > 0 ? NV : 1];
  if constexpr (NV > 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int k = tid + 256 * j;
      reg[j] = k < V ? xr[k] : __builtin_nanf("");
    }
  }
  float pv = INFINITY;                     // the previous round's winner; before round 0 everything ranks after it
  int pi = INT_MAX;
  int n = 0;
  for (int r = 0; r < K; ++r) {
    TK best = {-INFINITY, -1};
    // k ascends per thread, so ">=" keeps the larger index of equal values; NaN fails both compares
    auto visit = [&](float v, int k) __attribute__((always_inline)) {
      const bool after = v < pv || (v == pv && k < pi);
      if (after && (best.i < 0 || v >= best.v)) { best.v = v; best.i = k; }
    };
    if constexpr (NV > 0) {
#pragma unroll
      for (int j = 0; j < NV; ++j) visit(reg[j], tid + 256 * j);
    } else {
      for (int k = tid; k < V; k += 256) visit(xr[k], k);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      TK ob; ob.v = __shfl_xor(best.v, o, 64); ob.i = __shfl_xor(best.i, o, 64);
      best = tk_first(best, ob);
    }
    const int sl = r & 1;
    if (lane == 0) { s_v[sl][wv] = best.v; s_i[sl][wv] = best.i; }
    __syncthreads();
    TK w = {s_v[sl][0], s_i[sl][0]};
#pragma unroll
    for (int q = 1; q < 4; ++q) { TK o = {s_v[sl][q], s_i[sl][q]}; w = tk_first(w, o); }
    if (tid == 0) {
      ids[row * K + r] = w.i < 0 ? -1 : w.i;
      val[row * K + r] = w.i < 0 ? -INFINITY : w.v;
    }
    if (w.i < 0) { pi = -1; continue; }    // nothing left (block-uniform): the remaining rounds only write fill values
    ++n;
    pv = w.v; pi = w.i;
  }
  if (tid == 0) n_out[row] = n;
}

void launch_topk(hipStream_t s, const float* x, int64_t rows, int V, int ldx, int K, int64_t* ids, float* val, int32_t* n) {
  if (rows == 0) return;
  const dim3 g((unsigned)rows), b(256);
  if (V <= 256 * 36) hipLaunchKernelGGL((topk_kernel<36>), g, b, 0, s, x, V, ldx, K, ids, val, n);
  else if (V <= 256 * 100) hipLaunchKernelGGL((topk_kernel<100>), g, b, 0, s, x, V, ldx, K, ids, val, n);
  else hipLaunchKernelGGL((topk_kernel<0>), g, b, 0, s, x, V, ldx, K, ids, val, n);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
