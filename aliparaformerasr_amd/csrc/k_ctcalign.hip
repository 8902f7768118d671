// k_ctcalign.hip — CTC forced alignment of known labelings (PF_DECODE_ALIGN).
//
// The definition is tests/ctcalign_ref.py, the host twin host_ctc_align (hostutil.cpp).  Per job (utterance b, target h)
// two recursions over the S = 2U + 1 states run side by side through the frames t < n_b: the best path in float32 (one
// add per cell, so the score is bit for bit the reference's) and the sum over all paths in float64 (lse).
//
// One workgroup of 256 threads per job, the frame loop inside the kernel.  A thread owns a contiguous run of R states
// (R = 1, 2, 4 or 8 by the launch's longest possible target), keeps their labels, skip flags and both values in
// registers and writes the values to the double-buffered state rows in LDS, from which only the two values below its
// run are read back.  The next frame's log-probs (one gather per odd state, the blank column for the even ones) are
// issued before the current frame is worked on.  One barrier per frame.
//
// Back-pointers take 2 bits per cell, 16 states per 32-bit word, T * ceil(S / 16) words per job in a global workspace.
// A thread leaves its cells' codes as bytes in a double-buffered LDS row; behind the frame's barrier the first
// ceil(S / 16) threads pack the previous frame's row into words while the next frame is computed, so packing needs no
// barrier of its own and no atomics.  The backtrace is a walk from the end state: a frame moves the state down by at most
// 2, so the 16 frames of a stretch touch at most 3 words per frame, known when the stretch begins; the first wave loads
// them in one go and one lane walks them out of LDS.  first / last land in LDS (the state rows are dead by then); the
// token scores are then a parallel pass over the tokens.
#include "kernels.h"

namespace pf {

namespace {

constexpr int kAlignThreads = 256;
constexpr int kAlignStates = 2048;                  // >= 2 * PF_ALIGN_MAX_TOKENS + 1
constexpr int kAlignStretch = 16;                   // frames per backtrace stretch
constexpr double kNegInf = -__builtin_huge_val();
constexpr float kNegInfF = -__builtin_huge_valf();

__device__ inline double align_lse(double a, double b) {
  if (a == kNegInf) return b;
  if (b == kNegInf) return a;
  const double m = a > b ? a : b;
  return m + log1p(exp(-fabs(a - b)));
}

}  // namespace

template <int R>
__global__ __launch_bounds__(kAlignThreads) void ctc_align_kernel(const float* lp, int64_t ld, int V, const int32_t* tgt,
                                                                  const int32_t* tlen, const int32_t* len, int T, int H, int cap,
                                                                  uint32_t* bp, int64_t bp_stride, float* path_score,
                                                                  double* loglik, int32_t* ok, int32_t* first, int32_t* last,
                                                                  float* tok_score) {
  __shared__ double ad[2][kAlignStates];
  __shared__ float af[2][kAlignStates];
  __shared__ uint32_t code[2][kAlignStates / 4];    // one byte per state
  __shared__ uint32_t stretch[kAlignStretch][4];
  __shared__ int s_walk;

  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int64_t job = (int64_t)b * H + h;
  const int U = tlen[job];
  const int nb = min(max(len[b], 0), T);
  const int32_t* y = tgt + job * cap;
  int32_t* first_o = first + job * cap;
  int32_t* last_o = last + job * cap;
  float* tok_o = tok_score + job * cap;

  // jobs without a frame loop: skipped (-1), too long, or no frames.  Block-uniform.
  if (U < 0 || U > cap || U > PF_ALIGN_MAX_TOKENS || nb == 0) {
    const bool empty_ok = U == 0 && nb == 0;
    for (int u = tid; u < cap; u += kAlignThreads) { first_o[u] = -1; last_o[u] = -1; tok_o[u] = 0.f; }
    if (tid == 0) {
      path_score[job] = empty_ok ? 0.f : kNegInfF;
      loglik[job] = empty_ok ? 0.0 : kNegInf;
      ok[job] = empty_ok ? 1 : 0;
    }
    return;
  }

  const int S = 2 * U + 1, nW = (S + 15) >> 4;
  const float* rows = lp + (int64_t)b * T * ld;
  uint32_t* bpj = bp + job * bp_stride;              // row t at bpj + t * nW, t >= 1
  const int s0 = tid * R;

  // labels and skip flags of this thread's states; a label outside the row reads nothing and poisons the job
  int lab[R];
  bool skip[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int s = s0 + r;
    lab[r] = -1;
    skip[r] = false;
    if (s < S) {
      const int c = (s & 1) ? y[s >> 1] : 0;
      lab[r] = (c >= 0 && c < V) ? c : -2;
      skip[r] = (s & 1) && s >= 3 && c != y[(s >> 1) - 1];
    }
  }
  auto gather = [&](int t, int r) -> float {
    return lab[r] >= 0 ? rows[(int64_t)t * ld + lab[r]] : (lab[r] == -2 ? __builtin_nanf("") : kNegInfF);
  };

  float vf[R], nx[R];
  double vd[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int s = s0 + r;
    const float x = gather(0, r);
    vf[r] = (s < 2 && s < S) ? x : kNegInfF;
    vd[r] = (s < 2 && s < S) ? (double)x : kNegInf;
    if (s < S) { af[0][s] = vf[r]; ad[0][s] = vd[r]; }
    nx[r] = nb > 1 ? gather(1, r) : 0.f;
  }
  __syncthreads();

  for (int t = 1; t < nb; ++t) {
    const int cur = (t - 1) & 1, nxt = t & 1;
    float cx[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      cx[r] = nx[r];
      if (t + 1 < nb) nx[r] = gather(t + 1, r);
    }
    // frame t - 1's codes, complete since the barrier, go out as words (frame 0 has none)
    if (t >= 2 && tid < nW) {
      uint32_t w = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t x = code[cur][tid * 4 + q];
        w |= ((x & 3u) | ((x >> 6) & 12u) | ((x >> 12) & 48u) | ((x >> 18) & 192u)) << (8 * q);
      }
      bpj[(int64_t)(t - 1) * nW + tid] = w;
    }
    if (s0 < S) {
      const float e1f = s0 >= 1 ? af[cur][s0 - 1] : kNegInfF, e2f = s0 >= 2 ? af[cur][s0 - 2] : kNegInfF;
      const double e1d = s0 >= 1 ? ad[cur][s0 - 1] : kNegInf, e2d = s0 >= 2 ? ad[cur][s0 - 2] : kNegInf;
      // downwards, so that the values below a state are still the previous frame's
#pragma unroll
      for (int r = R - 1; r >= 0; --r) {
        const int s = s0 + r;
        if (s < S) {
          const float p1 = r >= 1 ? vf[r >= 1 ? r - 1 : 0] : e1f;
          const float p2 = r >= 2 ? vf[r >= 2 ? r - 2 : 0] : (r == 1 ? e1f : e2f);
          const double q1 = r >= 1 ? vd[r >= 1 ? r - 1 : 0] : e1d;
          const double q2 = r >= 2 ? vd[r >= 2 ? r - 2 : 0] : (r == 1 ? e1d : e2d);
          float best = vf[r];
          uint32_t m = 0;
          if (p1 > best) { best = p1; m = 1; }
          if (skip[r] && p2 > best) { best = p2; m = 2; }
          double acc = align_lse(vd[r], q1);
          if (skip[r]) acc = align_lse(acc, q2);
          vf[r] = best + cx[r];
          vd[r] = acc + (double)cx[r];
          af[nxt][s] = vf[r];
          ad[nxt][s] = vd[r];
          ((unsigned char*)code[nxt])[s] = (unsigned char)m;
        }
      }
    }
    __syncthreads();
  }

  const int fin = (nb - 1) & 1;
  if (nb >= 2 && tid < nW) {
    uint32_t w = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t x = code[fin][tid * 4 + q];
      w |= ((x & 3u) | ((x >> 6) & 12u) | ((x >> 12) & 48u) | ((x >> 18) & 192u)) << (8 * q);
    }
    bpj[(int64_t)(nb - 1) * nW + tid] = w;
  }
  const float a1 = af[fin][S - 1], a2 = S > 1 ? af[fin][S - 2] : kNegInfF;
  const int s_end = (S > 1 && a2 > a1) ? S - 2 : S - 1;
  const float score = s_end == S - 1 ? a1 : a2;
  const bool good = score > kNegInfF;
  if (tid == 0) {
    path_score[job] = score;
    loglik[job] = S > 1 ? align_lse(ad[fin][S - 1], ad[fin][S - 2]) : ad[fin][0];
    ok[job] = good ? 1 : 0;
    s_walk = s_end;
  }
  __syncthreads();                                  // the state rows are dead from here; the words are visible to the block
  int* first_l = (int*)af[0];
  int* last_l = (int*)af[1];
  for (int u = tid; u < U; u += kAlignThreads) { first_l[u] = -1; last_l[u] = -1; }
  __syncthreads();

  if (good) {                                       // block-uniform: every thread read the same two LDS values
    for (int t_hi = nb - 1; t_hi >= 1; t_hi -= kAlignStretch) {
      const int sw = s_walk, w0 = sw >> 4;
      if (tid < kAlignStretch * 4) {
        const int f = tid >> 2, k = tid & 3, t = t_hi - f;
        if (k < 3 && t >= 1 && w0 - k >= 0) stretch[f][k] = bpj[(int64_t)t * nW + (w0 - k)];
      }
      __syncthreads();
      if (tid == 0) {
        int s = sw;
        for (int f = 0; f < kAlignStretch && t_hi - f >= 1; ++f) {
          const int t = t_hi - f;
          if (s & 1) {
            const int u = s >> 1;
            if (last_l[u] < 0) last_l[u] = t;
            first_l[u] = t;
          }
          s -= (int)((stretch[f][w0 - (s >> 4)] >> (2 * (s & 15))) & 3u);
        }
        s_walk = s;
      }
      __syncthreads();
    }
    if (tid == 0) {
      const int s = s_walk;                         // the state of frame 0
      if (s & 1) {
        const int u = s >> 1;
        if (last_l[u] < 0) last_l[u] = 0;
        first_l[u] = 0;
      }
    }
    __syncthreads();
  }

  for (int u = tid; u < cap; u += kAlignThreads) {
    int f = -1, l = -1;
    float sc = 0.f;
    if (good && u < U) {
      f = first_l[u];
      l = last_l[u];
      if (f >= 0) {
        const int c = y[u];
        sc = rows[(int64_t)f * ld + c];
        for (int t = f + 1; t <= l; ++t) sc = fmaxf(sc, rows[(int64_t)t * ld + c]);
      }
    }
    first_o[u] = f;
    last_o[u] = l;
    tok_o[u] = sc;
  }
}

// tgt [B, H, cap] / tlen [B, H] from the caller's targets (job 0 when c_len is given) and the beam's result block
__global__ __launch_bounds__(kAlignThreads) void ctc_align_jobs_kernel(const int32_t* c_tgt, const int32_t* c_len, int c_cap,
                                                                       const int32_t* b_ids, const int32_t* b_len,
                                                                       const int32_t* b_nhyp, int N, int b_cap, int H, int cap,
                                                                       int32_t* tgt, int32_t* tlen) {
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int64_t job = (int64_t)b * H + h;
  const int hc = c_len ? 1 : 0;
  int U = -1, src_cap = 0;
  const int32_t* src = nullptr;
  if (h < hc) {
    U = c_len[b];
    src = c_tgt + (int64_t)b * c_cap;
    src_cap = c_cap;
  } else {
    const int i = h - hc;
    if (i < min(b_nhyp[b], N)) {
      U = b_len[(int64_t)b * N + i];
      src = b_ids + ((int64_t)b * N + i) * b_cap;
      src_cap = b_cap;
    }
  }
  for (int p = tid; p < cap; p += kAlignThreads) tgt[job * cap + p] = (p < U && p < src_cap) ? src[p] : -1;
  if (tid == 0) tlen[job] = U < 0 ? -1 : (U > src_cap ? PF_ALIGN_MAX_TOKENS + 1 : U);
}

size_t ctc_align_bp_words(int T, int cap) {
  const int S = 2 * std::min(std::max(cap, 0), PF_ALIGN_MAX_TOKENS) + 1;
  return (size_t)std::max(T, 1) * (size_t)((S + 15) / 16);
}

void launch_ctc_align_jobs(hipStream_t s, const int32_t* c_tgt, const int32_t* c_len, int c_cap, const int32_t* b_ids,
                           const int32_t* b_len, const int32_t* b_nhyp, int N, int b_cap, int B, int H, int cap, int32_t* tgt,
                           int32_t* tlen) {
  PF_CHECK(H == (c_len ? 1 : 0) + N && cap >= 1 && N >= 0 && (N == 0 || (b_ids && b_len && b_nhyp)), PF_ERR_INVALID_ARG,
           "ctc_align_jobs: bad shape");
  if (B == 0 || H == 0) return;
  hipLaunchKernelGGL(ctc_align_jobs_kernel, dim3((unsigned)H, (unsigned)B), dim3(kAlignThreads), 0, s, c_tgt, c_len, c_cap, b_ids,
                     b_len, b_nhyp, N, b_cap, H, cap, tgt, tlen);
  PF_HIP(hipGetLastError());
}

void launch_ctc_align(hipStream_t s, const float* lp, int64_t ld, int V, const int32_t* tgt, const int32_t* tlen, const int32_t* len,
                      int B, int T, int H, int cap, uint32_t* bp, int64_t bp_stride, float* path_score, double* loglik, int32_t* ok,
                      int32_t* first, int32_t* last, float* tok_score) {
  PF_CHECK(B >= 0 && T >= 0 && H >= 0 && cap >= 1 && V >= 1 && ld >= V && B <= 65535, PF_ERR_INVALID_ARG, "ctc_align: bad shape");
  PF_CHECK(bp_stride >= (int64_t)ctc_align_bp_words(T, cap), PF_ERR_INVALID_ARG, "ctc_align: back-pointer workspace too small");
  if (B == 0 || H == 0) return;
  const int S = 2 * std::min(cap, PF_ALIGN_MAX_TOKENS) + 1;
  const dim3 grid((unsigned)H, (unsigned)B), block(kAlignThreads);
#define PF_ALIGN_LAUNCH(R)                                                                                                     \
  hipLaunchKernelGGL(ctc_align_kernel<R>, grid, block, 0, s, lp, ld, V, tgt, tlen, len, T, H, cap, bp, bp_stride, path_score, \
                     loglik, ok, first, last, tok_score)
  if (S <= kAlignThreads) PF_ALIGN_LAUNCH(1);
  else if (S <= 2 * kAlignThreads) PF_ALIGN_LAUNCH(2);
  else if (S <= 4 * kAlignThreads) PF_ALIGN_LAUNCH(4);
  else PF_ALIGN_LAUNCH(8);
#undef PF_ALIGN_LAUNCH
  PF_HIP(hipGetLastError());
}

}  // namespace pf
