// k_ctcspot.hip — CTC phrase spotting: where in an utterance was each phrase of a list said.
//
// The definition is tests/ctcspot_ref.py, the host twin host_ctc_spot (hostutil.cpp).  Per (utterance b, phrase k) a Viterbi DP
// over the S = 2U - 1 states of the phrase (tokens with the blanks BETWEEN them) runs through the frames t < n_b with a restart
// of state 0 at every frame and an exit at every frame; the start frame travels with the value, so there is no back-trace.  All
// values are float32 with one add per cell: a score is bit for bit the reference's.
//
// LANE = STATE, several phrases per wave.  The host packer (spot_pack) lays the phrases' chains end to end into rows of 64
// lanes, a chain never straddling a row; a lane word holds the state's column and four flags (decode_blocks.h kSpot*).  One
// wave runs one row, a workgroup of 256 threads four rows of one utterance, the grid is (ceil(rows / 4), B).  The waves of a
// workgroup never need each other: no barrier, no LDS.
//
// NEIGHBOURS: v[s - 1], v[s - 2] and their starts come through four independent __shfl_up moves of the wave (value and start,
// by one and by two lanes).  The head flag cuts the chain: a head lane takes nothing from below (it restarts), the lane above
// it is an odd state and has no skip, and a skip flag is only ever set from state 2 on — so nothing of the chain below a head
// is looked at.
//
// LOG-PROBS: a lane only ever needs its own column.  It keeps the values of kSpotRing frames in registers (a fully unrolled
// ring) and, while the recurrence walks that stretch, the next stretch's gathers are in flight into a second set: the
// dependent chain of the recurrence never waits for a load but at a stretch's end, one stretch after the loads were issued.
// No load is issued for a frame at or beyond n_b, or by an idle lane.
//
// HITS: the exit lane of a chain owns its (b, k): it carries the open hit in registers, applies the selection rule every frame
// and stores a closed hit straight into its slots; after the last frame it closes the open hit, writes n_hits and fills the
// slots behind the stored hits.  One lane per (b, k): no atomics, no workspace.
#include "decode_blocks.h"
#include "kernels.h"

namespace pf {

namespace {

constexpr int kSpotThreads = kSpotLanes * kSpotRowsPerGroup;
constexpr float kSpotNegInf = -__builtin_huge_valf();

}  // namespace

__global__ __launch_bounds__(kSpotThreads) void ctc_spot_kernel(const float* __restrict__ lp, int64_t ld, const uint32_t* __restrict__ lanes,
                                                                const int32_t* __restrict__ lane_kw, int rows,
                                                                const int32_t* __restrict__ len, int T, int K, float thr, int max_hits,
                                                                int32_t* __restrict__ n_hits, int32_t* __restrict__ begin_end,
                                                                float* __restrict__ score) {
  const int row = (int)blockIdx.x * kSpotRowsPerGroup + (int)(threadIdx.x >> 6), b = (int)blockIdx.y;
  if (row >= rows) return;                            // wave-uniform
  const int lane = (int)(threadIdx.x & 63);
  const uint32_t w = lanes[(size_t)row * kSpotLanes + lane];
  const int kw = lane_kw[(size_t)row * kSpotLanes + lane];
  const bool head = (w & kSpotHead) != 0, skip = (w & kSpotSkip) != 0, exit_lane = (w & kSpotExit) != 0, idle = (w & kSpotIdle) != 0;
  const int nb = min(max(len[b], 0), T);
  const float* col = lp + (int64_t)b * T * ld + (w & kSpotLabel);   // this lane's column of the utterance's rows

  float v = kSpotNegInf;
  int st = -1;
  // the open hit and the count of closed ones (exit lanes)
  bool open = false;
  int n = 0, c_begin = 0, c_end = 0, c_dur = 0;
  float c_e = 0.f;
  int32_t* be_o = nullptr;
  float* sc_o = nullptr;
  if (exit_lane) {
    const int64_t x = (int64_t)b * K + kw;
    be_o = begin_end + x * max_hits * 2;
    sc_o = score + x * max_hits;
  }

  float cur[kSpotRing], nxt[kSpotRing];
#pragma unroll
  for (int j = 0; j < kSpotRing; ++j) cur[j] = (!idle && j < nb) ? col[(int64_t)j * ld] : kSpotNegInf;

  for (int t0 = 0; t0 < nb; t0 += kSpotRing) {
    // the next stretch's gathers, issued before this stretch's recurrence
#pragma unroll
    for (int j = 0; j < kSpotRing; ++j) {
      const int t = t0 + kSpotRing + j;
      nxt[j] = (!idle && t < nb) ? col[(int64_t)t * ld] : kSpotNegInf;
    }
#pragma unroll
    for (int j = 0; j < kSpotRing; ++j) {
      const int t = t0 + j;
      if (t < nb) {                                   // wave-uniform
        const float p1 = __shfl_up(v, 1), p2 = __shfl_up(v, 2);
        const int s1 = __shfl_up(st, 1), s2 = __shfl_up(st, 2);
        float best = v;
        int from = st;
        if (p1 > best) { best = p1; from = s1; }
        if (skip && p2 > best) { best = p2; from = s2; }
        if (head) { v = cur[j]; st = t; }
        else if (!idle) { v = cur[j] + best; st = from; }
        if (exit_lane) {
          const int dur = t - st + 1;
          const float fd = (float)dur;
          if (v > kSpotNegInf && v >= __fmul_rn(thr, fd)) {
            bool take = true;
            if (!open || st > c_end) {
              if (open) {
                if (n < max_hits) { be_o[2 * n] = c_begin; be_o[2 * n + 1] = c_end; sc_o[n] = c_e; }
                ++n;
              }
              open = true;
            } else {
              take = __fmul_rn(v, (float)c_dur) > __fmul_rn(c_e, fd);
            }
            if (take) { c_begin = st; c_end = t; c_dur = dur; c_e = v; }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kSpotRing; ++j) cur[j] = nxt[j];
  }

  if (exit_lane) {
    if (open) {
      if (n < max_hits) { be_o[2 * n] = c_begin; be_o[2 * n + 1] = c_end; sc_o[n] = c_e; }
      ++n;
    }
    n_hits[(int64_t)b * K + kw] = n;
    for (int i = min(n, max_hits); i < max_hits; ++i) { be_o[2 * i] = -1; be_o[2 * i + 1] = -1; sc_o[i] = 0.f; }
  }
}

void launch_ctc_spot(hipStream_t s, const float* lp, int64_t ld, int V, const uint32_t* lanes, const int32_t* lane_kw, int rows,
                     const int32_t* len, int B, int T, int K, float thr, int max_hits, int32_t* n_hits, int32_t* begin_end,
                     float* score) {
  PF_CHECK(B >= 0 && T >= 0 && K >= 0 && rows >= 0 && V >= 1 && ld >= V && B <= 65535 && max_hits >= 1 && max_hits <= PF_SPOT_MAX_HITS &&
               thr <= 0.f,
           PF_ERR_INVALID_ARG, "ctc_spot: bad shape");
  if (B == 0 || K == 0 || rows == 0) return;
  const dim3 grid((unsigned)((rows + kSpotRowsPerGroup - 1) / kSpotRowsPerGroup), (unsigned)B), block(kSpotThreads);
  hipLaunchKernelGGL(ctc_spot_kernel, grid, block, 0, s, lp, ld, lanes, lane_kw, rows, len, T, K, thr, max_hits, n_hits, begin_end, score);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
