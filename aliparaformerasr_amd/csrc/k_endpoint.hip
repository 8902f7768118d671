// k_endpoint.hip — the streaming endpoint detector on the device (paraformer_hip.h "Voice-activity endpointing, streaming",
// DESIGN.md §4.6o).  The definition in numpy is tests/endpoint_ref.py, the host twin host_endpoint_update (hostutil.cpp).  Every
// value is an integer, so the three agree exactly, the state block included.
//
// endpoint_update_kernel: one workgroup of ONE wave per stream, B streams per launch.  It is the chunked walk of
// vad_segments_kernel (k_vad.hip) with its wave-uniform carry made persistent: the carry is loaded from the stream's state block
// (16 words, lane j reads word j), the stream's n_new[b] new levels are walked in chunks of 64 frames, the block is stored back.
// The block of stream b is states[slot[b]] (slot null: states[b]; the slots of a launch are distinct), its levels start at
// levels + off[b] (off null: levels + b * ld).
//   floor       F[v] = min(e[v], F[v-1] + rise) is a (min, +) recurrence: inside a chunk lane j takes the inclusive prefix minimum
//               of e[i] - rise * i (six shuffle steps in int64), adds rise * j and meets the carry as carry + rise * (j + 1).
//               Everything is relative to the chunk: nothing grows with the stream's age.
//   hysteresis  the 64-bit-ballot form of k_vad.hip (vad_count_bits, vad_last_event_state in kdev.h).  A launch's last chunk may
//               hold fewer than 64 frames, so the 256-frame window moves on by the chunk's frame count, not by a word.
//   events      two kinds of frame can change the sentence: the first frame of a state run (opens one when none is open) and a
//               state-0 frame exactly end_silence behind the last state-1 frame (closes the open one).  Both are found per lane;
//               their ballot is served in lane order by a wave-uniform loop, as k_vad.hip serves its closing lanes.  The forced
//               cut depends on the begin of the open sentence, which those events move: the loop places it between them
//               (every cut at a frame before the next event, and at the chunk's end every cut up to its last frame).
//               Events therefore leave in ascending order from lane 0 through plain stores.
// Nothing at or beyond n_new[b] is read; of events only the first min(n, cap) rows of a stream are written; n_events, in_speech
// and open_begin are always written.  The kernel is latency-bound by construction (one wave per stream, a few chunks per call).
#include "kdev.h"
#include "kernels.h"

namespace pf {

__global__ __launch_bounds__(64) void endpoint_update_kernel(int32_t* __restrict__ states, const int32_t* __restrict__ slot,
                                                             const int32_t* __restrict__ levels, const int32_t* __restrict__ off, int64_t ld,
                                                             const int32_t* __restrict__ n_new, const int32_t* __restrict__ flush,
                                                             EndpointParams p, int32_t* __restrict__ events, int cap,
                                                             int32_t* __restrict__ n_events, int32_t* __restrict__ in_speech,
                                                             int32_t* __restrict__ open_begin) {
  const int u = blockIdx.x, lane = threadIdx.x;
  int32_t* sb = states + (int64_t)(slot ? slot[u] : u) * PF_ENDPOINT_STATE_INTS;
  const int32_t* lev = levels + (off ? (int64_t)off[u] : (int64_t)u * ld);
  int32_t* evo = events + (int64_t)u * cap * 3;

  // ---- the carry: lane j holds word j, every value below is wave-uniform
  const int sw = lane < PF_ENDPOINT_STATE_INTS ? sb[lane] : 0;
  auto word = [&](int j) { return __builtin_amdgcn_readlane(sw, j); };
  unsigned long long h[5];
#pragma unroll
  for (int k = 0; k < 4; ++k) h[k] = (unsigned long long)(unsigned)word(kEpHist + 2 * k) | ((unsigned long long)(unsigned)word(kEpHist + 2 * k + 1) << 32);
  h[4] = 0;
  int state_c = word(kEpState), last_one = word(kEpLastOne) - 1, run_first = word(kEpRunFirst) - 1, prev_end = word(kEpPrevEnd);
  int count = word(kEpCount), flushed = word(kEpFlushed);
  long long carry = (long long)((unsigned long long)(unsigned)word(kEpFloorLo) | ((unsigned long long)(unsigned)word(kEpFloorHi) << 32));
  const int n = flushed ? 0 : n_new[u];                          // (the host refuses frames after a flush; the kernel ignores them)
  const bool fl = !flushed && flush && flush[u] != 0;

  const unsigned long long le = (2ull << lane) - 1ull;          // lanes <= this one (lane 63: all ones)
  const unsigned long long lt = le >> 1;                        // lanes below this one
  const long long margin = (long long)p.margin_q * p.n_mels;
  int nev = 0;
  auto begin = [&] { return max(prev_end, run_first - p.pad_begin); };
  auto emit = [&](int b, int e, int kind) {
    if (lane == 0 && nev < cap) { evo[3 * nev] = b; evo[3 * nev + 1] = e; evo[3 * nev + 2] = kind; }
    ++nev;
  };

  int e_cur = lane < n ? lev[lane] : 0;
  for (int c0 = 0; c0 < n; c0 += 64) {
    const int nv = min(64, n - c0);                              // the chunk's frames: lanes [0, nv)
    const int e_nx = c0 + 64 + lane < n ? lev[c0 + 64 + lane] : 0;
    const bool valid = lane < nv;
    const int t = count + lane;                                  // count: the frames in front of the chunk

    // step 2': the floor and the threshold
    long long thr = p.abs_level;
    if (p.rise >= 0) {
      long long m = valid ? (long long)e_cur - (long long)p.rise * lane : 0;   // lanes past the chunk lie above every lane that counts
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(m, d, 64);
        if (lane >= d) m = min(m, o);
      }
      long long F = m + (long long)p.rise * lane;
      if (count > 0) F = min(F, carry + (long long)p.rise * (lane + 1));
      thr = max(F + margin, (long long)p.abs_level);
      carry = __shfl(F, nv - 1, 64);
    }
    h[4] = __ballot(valid && (long long)e_cur > thr);

    // step 3: as k_vad.hip (frames in front of frame 0 are zero bits)
    const int cnt = vad_count_bits(h, 256 + lane - p.window + 1, 256 + lane);
    const int w = min(p.window, t + 1);
    const bool on = valid && cnt >= p.on_count;
    const bool offe = valid && !on && w - cnt >= p.off_count;
    const unsigned long long evm = __ballot(on || offe), onm = __ballot(on);
    const bool st = valid && vad_last_event_state(evm, onm, le, state_c != 0);
    const unsigned long long sm = __ballot(st);

    // steps 4' and 5': the frames that can open or close a sentence, served in order; the forced cuts between them
    const bool prev_st = lane == 0 ? state_c != 0 : ((sm >> (lane - 1)) & 1ull) != 0;
    const unsigned long long s_lt = sm & lt;
    const int prev_one = s_lt ? count + 63 - __clzll((long long)s_lt) : last_one;      // the last state-1 frame before this one
    const bool starts = st && !prev_st;
    const bool closes = valid && !st && prev_one >= 0 && t - prev_one == p.end_silence;
    auto forced_until = [&](int tlim) {                          // every cut at a frame <= tlim (a frame of this chunk)
      while (run_first >= 0 && begin() + p.max_len - 1 <= tlim) {
        const int tf = begin() + p.max_len - 1;
        emit(begin(), tf + 1, PF_ENDPOINT_FORCED);
        prev_end = tf + 1;
        if (!((sm >> (tf - count)) & 1ull)) run_first = -1;
      }
    };
    unsigned long long todo = __ballot(starts || closes);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int tc = count + src, po = __shfl(prev_one, src, 64);
      forced_until(tc - 1);
      if ((sm >> src) & 1ull) {
        if (run_first < 0) run_first = tc;
      } else if (run_first >= 0) {
        const int b = begin(), en = po + 1 + p.pad_end;
        if (en - b >= p.min_speech) { emit(b, en, PF_ENDPOINT_SILENCE); prev_end = en; }
        run_first = -1;
      }
    }
    forced_until(count + nv - 1);

    if (sm) last_one = count + 63 - __clzll((long long)sm);
    state_c = (int)((sm >> (nv - 1)) & 1ull);
    if (nv == 64) {
      h[0] = h[1]; h[1] = h[2]; h[2] = h[3]; h[3] = h[4];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) h[k] = (h[k] >> nv) | (h[k + 1] << (64 - nv));
    }
    count += nv;
    e_cur = e_nx;
  }

  // step 6: the flush
  if (fl) {
    if (run_first >= 0) {
      const int b = begin(), en = min(count, last_one + 1 + p.pad_end);
      if (en - b >= p.min_speech) { emit(b, en, PF_ENDPOINT_FLUSH); prev_end = en; }
      run_first = -1;
    }
    flushed = 1;
  }

  // ---- the carry goes back the way it came: lane j stores word j
  if (lane < PF_ENDPOINT_STATE_INTS) {
    int v;
    if (lane < 8) {
      const unsigned long long hw = lane < 2 ? h[0] : lane < 4 ? h[1] : lane < 6 ? h[2] : h[3];
      v = (int)(unsigned)((lane & 1) ? hw >> 32 : hw);
    } else {
      v = lane == kEpState ? state_c : lane == kEpLastOne ? last_one + 1 : lane == kEpRunFirst ? run_first + 1
        : lane == kEpPrevEnd ? prev_end : lane == kEpCount ? count : lane == kEpFloorLo ? (int)(unsigned)(unsigned long long)carry
        : lane == kEpFloorHi ? (int)(unsigned)((unsigned long long)carry >> 32) : flushed;
    }
    sb[lane] = v;
  }
  if (lane == 0) {
    n_events[u] = nev;
    in_speech[u] = run_first >= 0 ? 1 : 0;
    open_begin[u] = run_first >= 0 ? begin() : -1;
  }
}

void launch_endpoint_update(hipStream_t s, int32_t* states, const int32_t* slot, const int32_t* levels, const int32_t* off, int64_t ld,
                            const int32_t* n_new, const int32_t* flush, int B, const EndpointParams& p, int32_t* events, int cap, int32_t* n_events, int32_t* in_speech,
                            int32_t* open_begin) {
  if (B == 0) return;
  hipLaunchKernelGGL(endpoint_update_kernel, dim3((unsigned)B), dim3(64), 0, s, states, slot, levels, off, ld, n_new, flush, p, events, cap, n_events,
                     in_speech, open_begin);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
