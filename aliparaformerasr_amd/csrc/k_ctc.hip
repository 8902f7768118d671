// k_ctc.hip — CTC collapse of the per-frame arg-max ids on the device (PF_DECODE_CTC, DESIGN.md §CTC decoding).
//
// The reference leaves this step out: OfflineRecognizer.cs:153-168 (the merge of repeats is commented out, quirk Q6)
// and :151 (every timestamp {0, 0}).  The rule implemented here:
//   a token STARTS at frame t  when  y[t] != blank and (t == 0 or y[t] != y[t-1]),  and extends while y stays equal;
//   per token: id, first frame, last frame, score = fmaxf over the run of the frame's log-prob;
//   frames at or beyond len[b] are never read.
//
// One workgroup of ONE wave per utterance; the wave walks its row in chunks of 64 frames.  Inside a chunk everything is
// cross-lane (64-bit ballot, shuffles); between chunks three wave-uniform values are carried: the number of tokens
// started so far (the slot of an open token is that number - 1), the id of the chunk's last frame and the running
// maximum of the run that frame belongs to.  A run may therefore span any number of chunks: it starts a token once,
// and its `last` / `score` are written by the frame that ends it (the next frame differs, or it is frame len - 1).
// No atomics, no LDS; output order is frame order.  The next chunk is loaded before the current one is worked on.
#include "kernels.h"

namespace pf {

__global__ __launch_bounds__(64) void ctc_collapse_kernel(const int64_t* __restrict__ ids, const float* __restrict__ score,
                                                          const int32_t* __restrict__ len, int T, int blank, int cap,
                                                          int32_t* __restrict__ n_out, int64_t* __restrict__ ids_out,
                                                          int32_t* __restrict__ first_out, int32_t* __restrict__ last_out,
                                                          float* __restrict__ score_out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = min(max(len[b], 0), T);
  const int64_t* yr = ids + (int64_t)b * T;
  const float* sr = score + (int64_t)b * T;
  int64_t* io = ids_out + (int64_t)b * cap;
  int32_t* fo = first_out + (int64_t)b * cap;
  int32_t* lo = last_out + (int64_t)b * cap;
  float* so = score_out + (int64_t)b * cap;
  const long long bl = blank;
  const unsigned long long le = (2ull << lane) - 1ull;   // lanes <= this one (lane 63: all ones)

  int count = 0;                  // tokens started in the chunks before this one
  long long carry_y = bl;         // id of the previous chunk's last frame
  float carry_m = 0.f;            // running maximum of the run that frame belongs to

  long long y = lane < n ? (long long)yr[lane] : bl;
  float s = lane < n ? sr[lane] : 0.f;
  for (int c = 0; c < n; c += 64) {
    const int t = c + lane, tn = t + 64;
    const long long y_nx = tn < n ? (long long)yr[tn] : bl;
    const float s_nx = tn < n ? sr[tn] : 0.f;
    const bool valid = t < n, tok = valid && y != bl;

    long long prev = __shfl_up(y, 1, 64);
    if (lane == 0) prev = carry_y;
    long long next = __shfl_down(y, 1, 64);
    const long long nx0 = __shfl(y_nx, 0, 64);
    if (lane == 63) next = nx0;
    const bool differs = t == 0 || y != prev;             // a run (of a token or of blanks) begins at this frame
    const bool start = tok && differs;
    const bool end = tok && (t == n - 1 || y != next);    // lanes beyond n hold `blank`, so frame n - 1 also ends by value

    const unsigned long long smask = __ballot(start);
    const unsigned long long bmask = __ballot(differs) | 1ull;
    const int slot = count + __popcll(smask & le) - 1;    // of the token this frame belongs to (tok lanes only)
    const int head = 63 - __clzll(bmask & le);            // lane where this frame's run begins inside the chunk

    // inclusive maximum over [head, lane]
    float m = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float o = __shfl_up(m, d, 64);
      if (lane - d >= head) m = fmaxf(m, o);
    }
    // the run that crosses the chunk's lower edge also owns what the earlier chunks saw of it
    const long long y0 = __shfl(y, 0, 64);
    if (head == 0 && c > 0 && y0 == carry_y) m = fmaxf(m, carry_m);

    if (tok && slot < cap) {
      if (start) { io[slot] = y; fo[slot] = t; }
      if (end) { lo[slot] = t; so[slot] = m; }
    }
    count += __popcll(smask);
    carry_y = __shfl(y, 63, 64);
    carry_m = __shfl(m, 63, 64);
    y = y_nx; s = s_nx;
  }
  // slots past the last token: fixed values, so a fetched block never shows what an earlier forward left there
  for (int k = count + lane; k < cap; k += 64) { io[k] = -1; fo[k] = -1; lo[k] = -1; so[k] = 0.f; }
  if (lane == 0) n_out[b] = count;
}

void launch_ctc_collapse(hipStream_t s, const int64_t* ids, const float* score, const int32_t* len, int B, int T, int blank,
                         int cap, int32_t* n_out, int64_t* ids_out, int32_t* first_out, int32_t* last_out, float* score_out) {
  if (B == 0) return;
  hipLaunchKernelGGL(ctc_collapse_kernel, dim3((unsigned)B), dim3(64), 0, s, ids, score, len, T, blank, cap, n_out, ids_out,
                     first_out, last_out, score_out);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
