// k_lm.hip — the language model's step on its own (pf_op_lm_score): the device twin of lm_score (lm.cpp), over the same image
// with the same text (lm_dev.h).  One thread walks one sequence: the walk is a chain of dependent lookups, and what is
// measured against the host is every g and every state on the way, bit for bit.
#include "kernels.h"
#include "lm_dev.h"

namespace pf {

// ids [B, L], lens [B] -> g [B, L], state [B, L] after every token p < lens[b]; later positions are not written
__global__ __launch_bounds__(64) void lm_walk_kernel(const int32_t* image, const int32_t* ids, const int32_t* lens, int B, int L,
                                                      double alpha, double beta, double* g_out, int32_t* state_out) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const LmView v = lm_view(image);
  const int n = min(max(lens[b], 0), L);
  double g = 0.0;
  int s = v.start;
  for (int p = 0; p < n; ++p) {
    const int64_t o = (int64_t)b * L + p;
    s = lm_step(v, s, ids[o], alpha, beta, true, g);
    g_out[o] = g;
    state_out[o] = s;
  }
}

void launch_lm_walk(hipStream_t s, const int32_t* image, const int32_t* ids, const int32_t* lens, int B, int L, float alpha, float beta,
                    double* g, int32_t* state) {
  PF_CHECK(image && B >= 0 && L >= 0, PF_ERR_INVALID_ARG, "lm_walk: bad arguments");
  if (B == 0 || L == 0) return;
  hipLaunchKernelGGL(lm_walk_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, image, ids, lens, B, L, (double)alpha, (double)beta,
                     g, state);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
