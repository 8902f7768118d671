// k_vad.hip — voice-activity segmentation on the device (paraformer_hip.h "Voice-activity segmentation").
// The definition in numpy is tests/vad_ref.py, the host twin host_vad_levels / host_vad_segments (hostutil.cpp).  Every
// value past the clamp of step 1 is an integer, so the three agree exactly.
//
// vad_levels_kernel (step 1): a half-wave per fbank row.  A row of 80 mel bins is 320 bytes: 20 lanes load 16 bytes each
// (rows are 16-byte aligned when n_mels % 4 == 0; other widths take 4-byte loads), clamp, scale by 64, round half to even and
// add up as int32 through five shuffle steps.  Integer addition makes the order of the sum irrelevant.
//
// vad_segments_kernel (steps 2-6): one workgroup of ONE wave per utterance, B utterances per launch.
//   threshold   the k-th smallest level by a three-pass radix select (11 + 11 + 10 bits of the order-preserving key
//               e ^ 0x80000000) over a 2048-bin histogram in LDS: exact for any int32 level.
//   the walk    ONE forward pass over the utterance in chunks of 64 frames, everything inside a chunk cross-lane (64-bit
//               ballots), like k_ctc.hip.  Carried between chunks, all wave-uniform:
//                 hist[4]    the raw bits of the previous 256 frames (window <= 256)
//                 state      state[t] of the previous chunk's last frame
//                 last_one   the last frame with state 1 so far (-1: none)
//                 run_t      the frame at which the open padded run's first state-1 frame lies (its begin is run_t - pad_begin)
//               state[t] is "the last event at or before t wins": the highest event bit at or below the lane, else the carry.
//               Padding is done on runs, not frames: state runs [s0, s1) and [s2, s3) belong to one padded run iff
//               s2 - s1 <= pad_begin + pad_end (then [s0 - pad_begin, s1 + pad_end) and [s2 - pad_begin, ..) touch or
//               overlap).  So the first frame of a state run OPENS a padded run when no state-1 frame lies within that
//               distance behind it, and the same frame CLOSES the one before: [max(0, run_t - pad_begin), min(T, last_one +
//               1 + pad_end)).  The last run is closed after the walk.
//   emission    closing lanes are served one after another in lane order (a wave-uniform loop over the ballot), so the
//               output is ascending without a compaction pass: drop below min_speech, split above max_len with a wave-wide
//               arg-min over the search window (<= 1025 levels, ties to the largest t), store with lane 0.
// An hour of audio (360 000 frames) is 5 625 chunks per pass.  Nothing at or beyond T[b] is read; of seg only the first
// min(n[b], cap) rows are written.
#include "kdev.h"
#include "kernels.h"

namespace pf {

// ------------------------------------------------------------------ step 1: levels ------
__device__ __forceinline__ int vad_q(float x) {
  float v = x;
  if (!(v > -64.f)) v = -64.f;               // NaN and -inf land here
  if (v > 64.f) v = 64.f;
  return (int)rintf(v * 64.f);               // exact product; round half to even
}

__global__ __launch_bounds__(256) void vad_levels_kernel(const float* __restrict__ rows, int64_t T, int n_mels,
                                                         int32_t* __restrict__ levels) {
  const int sub = threadIdx.x & 31;
  const int64_t t = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  int acc = 0;
  if (t < T) {
    const float* r = rows + t * n_mels;
    if ((n_mels & 3) == 0) {
      for (int j = sub; j < (n_mels >> 2); j += 32) {
        const float4 v = *reinterpret_cast<const float4*>(r + 4 * j);
        acc += vad_q(v.x) + vad_q(v.y) + vad_q(v.z) + vad_q(v.w);
      }
    } else {
      for (int j = sub; j < n_mels; j += 32) acc += vad_q(r[j]);
    }
  }
#pragma unroll
  for (int d = 16; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 32);
  if (t < T && sub == 0) levels[t] = acc;
}

void launch_vad_levels(hipStream_t s, const float* rows, int64_t T, int n_mels, int32_t* levels) {
  if (T <= 0) return;
  hipLaunchKernelGGL(vad_levels_kernel, dim3((unsigned)((T + 7) / 8)), dim3(256), 0, s, rows, T, n_mels, levels);
  PF_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ steps 2-6: segments ------
// (vad_count_bits and vad_last_event_state, shared with k_endpoint.hip, are in kdev.h)

// one closed padded run [b, e) of utterance levels `lev`: drop, split, store.  All arguments are wave-uniform.
__device__ __forceinline__ void vad_emit_run(const int32_t* __restrict__ lev, int b, int e, const VadParams& p, int lane,
                                             int32_t* __restrict__ seg, int cap, int& count) {
  if (e - b < p.min_speech) return;
  while (e - b > p.max_len) {
    const int hi = min(b + p.max_len, e - p.min_speech), lo = hi - p.split_search;   // b < lo <= hi < e (the config's constraints)
    int best_v = INT32_MAX, best_t = -1;
    for (int t = lo + lane; t <= hi; t += 64) {
      const int v = lev[t];
      if (v <= best_v) { best_v = v; best_t = t; }           // ascending t: of equal levels the later one stays
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const int ov = __shfl_xor(best_v, d, 64), ot = __shfl_xor(best_t, d, 64);
      if (ot >= 0 && (best_t < 0 || ov < best_v || (ov == best_v && ot > best_t))) { best_v = ov; best_t = ot; }
    }
    if (lane == 0 && count < cap) *reinterpret_cast<int2*>(seg + 2 * (int64_t)count) = make_int2(b, best_t);
    ++count;
    b = best_t;
  }
  if (lane == 0 && count < cap) *reinterpret_cast<int2*>(seg + 2 * (int64_t)count) = make_int2(b, e);
  ++count;
}

__global__ __launch_bounds__(64) void vad_segments_kernel(const int32_t* __restrict__ levels, const int64_t* __restrict__ off,
                                                          const int32_t* __restrict__ Tn, VadParams p, int32_t* __restrict__ seg_out,
                                                          int cap, int32_t* __restrict__ n_out) {
  __shared__ int hist[2048];
  const int u = blockIdx.x, lane = threadIdx.x;
  const int T = Tn[u];
  const int32_t* lev = levels + off[u];
  int32_t* seg = seg_out + (int64_t)u * cap * 2;
  if (T <= 0) {
    if (lane == 0) n_out[u] = 0;
    return;
  }

  // ---- step 2: the threshold
  long long thr = p.abs_level;
  if (p.floor_pct >= 0) {
    int k = (int)min((long long)T - 1, (long long)T * p.floor_pct / 100);     // remaining rank inside the selected prefix
    unsigned prefix = 0;                                                     // the key's bits above `shift`, once chosen
    for (int pass = 0; pass < 3; ++pass) {
      const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0, bits = pass == 2 ? 10 : 11;
      for (int i = lane; i < 2048; i += 64) hist[i] = 0;
      __syncthreads();
      for (int t = lane; t < T; t += 64) {
        const unsigned key = (unsigned)lev[t] ^ 0x80000000u;
        if (pass == 0 || (key >> (shift + bits)) == prefix) atomicAdd(&hist[(key >> shift) & ((1u << bits) - 1u)], 1);
      }
      __syncthreads();
      // lane l owns bins [32 l, 32 l + 32): find the bin in which the cumulative count passes k
      int mine = 0;
      for (int i = 0; i < 32; ++i) mine += hist[32 * lane + i];
      int incl = mine;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
      }
      const unsigned long long hit = __ballot(k < incl);
      const int owner = __ffsll((long long)hit) - 1;                         // the counts add up to more than k: a lane hits
      int bin = 0, rest = 0;
      if (lane == owner) {
        int cum = incl - mine;
        for (int i = 0; i < 32; ++i) {
          const int h = hist[32 * lane + i];
          if (k < cum + h) { bin = 32 * lane + i; rest = k - cum; break; }
          cum += h;
        }
      }
      bin = __shfl(bin, owner, 64);
      k = __shfl(rest, owner, 64);
      prefix = (prefix << bits) | (unsigned)bin;
      __syncthreads();
    }
    const long long F = (long long)(int)(prefix ^ 0x80000000u);
    thr = max(F + (long long)p.margin_q * p.n_mels, (long long)p.abs_level);
  }

  // ---- steps 3-5: the walk
  const unsigned long long le = (2ull << lane) - 1ull;     // lanes <= this one (lane 63: all ones)
  const unsigned long long lt = le >> 1;                   // lanes below this one
  const int pads = p.pad_begin + p.pad_end;
  unsigned long long h[5] = {0, 0, 0, 0, 0};               // h[0..3]: raw bits of the 256 frames before the chunk, h[4]: the chunk
  int state_c = 0, last_one = -1, run_t = -1, count = 0;

  int e_cur = lane < T ? lev[lane] : 0;
  for (int c0 = 0; c0 < T; c0 += 64) {
    const int t = c0 + lane, tn = t + 64;
    const int e_nx = tn < T ? lev[tn] : 0;
    const bool valid = t < T;
    h[4] = __ballot(valid && (long long)e_cur > thr);

    // step 3: frames of the window before frame 0 are zero bits, so the count over `window` positions is c[t]
    const int cnt = vad_count_bits(h, 256 + lane - p.window + 1, 256 + lane);
    const int w = min(p.window, t + 1);
    const bool on = valid && cnt >= p.on_count;
    const bool offe = valid && !on && w - cnt >= p.off_count;
    const unsigned long long evm = __ballot(on || offe), onm = __ballot(on);
    const bool st = valid && vad_last_event_state(evm, onm, le, state_c != 0);
    const unsigned long long sm = __ballot(st);

    // step 4 on runs: the first frame of a state run opens a padded run when nothing lies within `pads` behind it
    const bool prev_st = lane == 0 ? state_c != 0 : ((sm >> (lane - 1)) & 1ull) != 0;
    const unsigned long long s_lt = sm & lt;
    const int prev_one = s_lt ? c0 + 63 - __clzll((long long)s_lt) : last_one;   // the last state-1 frame before this one
    const bool opens = st && !prev_st && (prev_one < 0 || t - (prev_one + 1) > pads);
    const unsigned long long om = __ballot(opens);
    const unsigned long long o_lt = om & lt;
    const int prev_open = o_lt ? c0 + 63 - __clzll((long long)o_lt) : run_t;     // where the run this frame closes was opened
    const int cb = max(prev_open - p.pad_begin, 0), ce = min(prev_one + 1 + p.pad_end, T);

    // step 5: the runs closed in this chunk, in frame order
    unsigned long long todo = __ballot(opens && prev_one >= 0);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      vad_emit_run(lev, __shfl(cb, src, 64), __shfl(ce, src, 64), p, lane, seg, cap, count);
    }

    if (sm) last_one = c0 + 63 - __clzll((long long)sm);
    if (om) run_t = c0 + 63 - __clzll((long long)om);
    state_c = (int)((sm >> 63) & 1ull);
    h[0] = h[1]; h[1] = h[2]; h[2] = h[3]; h[3] = h[4];
    e_cur = e_nx;
  }
  if (last_one >= 0) vad_emit_run(lev, max(run_t - p.pad_begin, 0), min(last_one + 1 + p.pad_end, T), p, lane, seg, cap, count);
  if (lane == 0) n_out[u] = count;
}

void launch_vad_segments(hipStream_t s, const int32_t* levels, const int64_t* off, const int32_t* T, int B, const VadParams& p,
                         int32_t* seg, int cap, int32_t* n) {
  if (B == 0) return;
  hipLaunchKernelGGL(vad_segments_kernel, dim3((unsigned)B), dim3(64), 0, s, levels, off, T, p, seg, cap, n);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
