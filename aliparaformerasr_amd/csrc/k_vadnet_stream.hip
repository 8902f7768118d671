// k_vadnet_stream.hip — the FSMN-VAD model score in causal, stateful form (paraformer_hip.h "Voice-activity endpointing,
// streaming, model score").  The release schedule in Python is tests/vadnet_stream_ref.py, the host twin
// host_vad_model_stream (vadnet.cpp).  Its levels and logits are bit-equal to k_vadnet.hip's over the whole stream: the
// products are tile_rows.h's (a tile row's result depends on that row and on W alone), the FSMN sum, the softmax merge and the
// level formula are vadnet_dev.h's, shared with that kernel.
//
// ONE launch per call, one workgroup of four waves per stream.  A stream that has received n frames and now gets n_new has
// released rel0 = max(0, n - right) levels and releases up to rel1 = max(0, n + n_new - right), at a flush all n + n_new
// (right = lfr_m - 1 - left, left = (lfr_m - 1) / 2).  The workgroup walks [rel0, rel1) in tiles of at most 64 rows and runs all
// 1 + n_layers stages of a tile back to back:
//   head      LFR + CMVN from the state's row tail (the last lfr_m - 1 rows received) and the new rows; the upper clamp acts
//             only at the flush (before it the schedule keeps t + right inside the received frames)
//   in_linear1 -> in_linear2 + ReLU -> linear_0 -> p_0 into the fp32 window in LDS, behind the `reach` history rows of the state
//   per layer the FSMN sum over the window (absolute frame index t: a tap with d > t is skipped), the window's last `reach`
//             rows back to the state, affine + ReLU, the next linear into the window
//   tail      out_linear1 -> out_linear2 -> softmax -> level; the logits when asked for
// p never goes through global memory inside a tile; between tiles and between calls a layer's history is its `reach` rows of the
// state block, which this workgroup alone reads and writes (the barrier between the store and the next tile's load orders them).
//
// LDS: two f16 tiles [64, ld] and the window [(reach + 64), ldw] fp32, ldw = ldp + 4: the accumulator rows a lane half stores
// (float4 at a row stride of ldw) then start 4 banks apart instead of on one bank.  At the released dimensions (ld 408, ldp 128,
// reach 19): 104 448 + 43 824 bytes, and 3 072 of static reduction scratch.
// Rows of a tile at or beyond its count are computed from a zero head and never stored.  Nothing at or beyond a stream's n_new
// is read; only the released levels (and logits) are written; n_out is always written.
#include "kdev.h"
#include "kernels.h"
#include "tile_rows.h"
#include "vadnet_dev.h"

namespace pf {

__global__ __launch_bounds__(256) void vadnet_stream_kernel(VadNetStreamLaunch a) {
  extern __shared__ __attribute__((aligned(16))) char vs_lds[];
  __shared__ float red[4][VN_ROWS][3];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int ld = a.ld, ldp = a.ldp, ldw = a.ldw, reach = a.reach;
  half_t* buf0 = reinterpret_cast<half_t*>(vs_lds);
  half_t* buf1 = buf0 + (size_t)VN_ROWS * ld;
  float* win = reinterpret_cast<float*>(buf1 + (size_t)VN_ROWS * ld);
  const int b = blockIdx.x;

  // ---- the state block: history [n_layers, reach, ldp] | row tail [lfr_m - 1, n_mels] | ... | count | flushed (the last 8 bytes)
  char* sb = a.states + (int64_t)(a.slot ? a.slot[b] : b) * a.state_bytes;
  float* hist = reinterpret_cast<float*>(sb);
  float* rtail = hist + (size_t)a.n_layers * reach * ldp;
  int32_t* words = reinterpret_cast<int32_t*>(sb + a.words_off);
  const int keep = a.lfr_m - 1, left = keep >> 1, right = keep - left;
  const int n = words[0];
  const bool was_flushed = words[1] != 0;
  const int nn = was_flushed ? 0 : a.n_new[b];                   // (frames after a flush are refused on the host)
  const bool fl = was_flushed || (a.flush && a.flush[b] != 0);
  const int n1 = n + nn;
  const int rel0 = was_flushed ? n : (n > right ? n - right : 0);
  const int rel1 = fl ? n1 : (n1 > right ? n1 - right : 0);
  const float* __restrict__ xb = a.x + (a.off ? (int64_t)a.off[b] : (int64_t)b * a.ldx) * a.n_mels;
  if (tid == 0) a.n_out[b] = rel1 - rel0;

  const float* __restrict__ shift = reinterpret_cast<const float*>(a.img + a.shift_off);
  const float* __restrict__ scale = reinterpret_cast<const float*>(a.img + a.scale_off);
  const float* __restrict__ silf = reinterpret_cast<const float*>(a.img + a.sil_off);

  for (int t0 = rel0; t0 < rel1; t0 += VN_ROWS) {
    const int nr = rel1 - t0 < VN_ROWS ? rel1 - t0 : VN_ROWS;
    // ---- the head: column c = j * n_mels + m of level t is (x[clamp(t - left + j, 0, last)][m] + shift[c]) * scale[c]     (R1)
    // frame f < n comes from the row tail (row f - n + keep), a later one from the new rows; last = n1 - 1 binds at the flush only
    for (int row = wave; row < VN_ROWS; row += 4) {
      const int t = t0 + row;
      for (int c = lane; c < a.in1.Kpad; c += 64) {
        float v = 0.f;
        if (row < nr && c < a.in_dim) {
          const int j = c / a.n_mels, m = c - j * a.n_mels;
          int src = t - left + j;
          src = src < 0 ? 0 : (src > n1 - 1 ? n1 - 1 : src);
          int q = src - n + keep;
          q = q < 0 ? 0 : q;
          const float xv = src >= n ? xb[(int64_t)(src - n) * a.n_mels + m] : rtail[q * a.n_mels + m];
          v = (xv + shift[c]) * scale[c];
        }
        buf0[row * ld + c] = (half_t)v;
      }
    }
    __syncthreads();
    vn_stage(a.img, a.in1, false, buf0, buf1, ld, wave, lane);
    __syncthreads();
    vn_stage(a.img, a.in2, true, buf1, buf0, ld, wave, lane);
    __syncthreads();
    half_t* cur = buf0;
    half_t* nxt = buf1;
    for (int l = 0; l < a.n_layers; ++l) {
      float* hl = hist + (size_t)l * reach * ldp;
      // ---- the window: the history rows t0 - reach .. t0 - 1 in front, linear_l's rows (fp32, all ldp columns) behind them
      for (int i = tid; i < reach * ldp; i += 256) {
        const int hr = i / ldp;
        win[hr * ldw + (i - hr * ldp)] = hl[i];
      }
      tr_product(a.img, a.lin[l], cur, ld, wave, lane, [&](int nt, int i, const f16x& acc) {
        float* wr = win + (size_t)(reach + 32 * i + r) * ldw + 32 * nt + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<float4*>(wr + 8 * q) = make_float4(acc[4 * q + 0], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
      });
      __syncthreads();
      // ---- the FSMN sum (R4) into the other tile, and the window's last `reach` valid rows back as the new history
      const float* __restrict__ taps = reinterpret_cast<const float*>(a.img + a.taps_off[l]);
      const int head_w = a.aff[l].Kpad;
      for (int row = wave; row < VN_ROWS; row += 4)
        for (int c = lane; c < head_w; c += 64) {
          float v = 0.f;
          if (row < nr && c < ldp) v = vn_fsmn_sum(win + (size_t)(reach + row) * ldw + c, ldw, taps + c, ldp, (long long)t0 + row, a.lorder, a.lstride);
          nxt[row * ld + c] = (half_t)v;
        }
      for (int i = tid; i < reach * ldp; i += 256) {
        const int hr = i / ldp;
        hl[i] = win[(size_t)(nr + hr) * ldw + (i - hr * ldp)];
      }
      __syncthreads();
      vn_stage(a.img, a.aff[l], true, nxt, cur, ld, wave, lane);       // affine_l + ReLU (R5), back into `cur`
      __syncthreads();
    }
    vn_stage(a.img, a.out1, false, cur, nxt, ld, wave, lane);          // out_linear1 (R6)
    __syncthreads();
    const int64_t o0 = (int64_t)b * a.cap + (t0 - rel0);
    vn_softmax_merge(a.img, a.out2, nxt, ld, wave, lane, silf, a.out_dim, red,
                     [&](int j) -> float* { return a.logits && j < nr ? a.logits + (o0 + j) * a.out_dim : nullptr; });
    __syncthreads();
    if (tid < nr && a.levels) a.levels[o0 + tid] = vn_level(red, tid);
    __syncthreads();
  }

  // ---- the row tail (frames n1 - keep .. n1 - 1; a frame before 0 is zeros), the count and the flag.  The new tail is staged
  // in LDS first: it may read the rows it overwrites.
  if (nn > 0) {
    float* stage = reinterpret_cast<float*>(vs_lds);
    const int cells = keep * a.n_mels;
    for (int i = tid; i < cells; i += 256) {
      const int q = i / a.n_mels, m = i - q * a.n_mels;
      const int f = n1 - keep + q;
      stage[i] = f < 0 ? 0.f : (f >= n ? xb[(int64_t)(f - n) * a.n_mels + m] : rtail[(f - n + keep) * a.n_mels + m]);
    }
    __syncthreads();
    for (int i = tid; i < cells; i += 256) rtail[i] = stage[i];
  }
  if (tid == 0) {
    if (nn > 0) words[0] = n1;
    if (fl && !was_flushed) words[1] = 1;
  }
}

size_t vadnet_stream_lds_bytes(int ld, int ldp, int reach) {
  return (size_t)2 * VN_ROWS * ld * sizeof(half_t) + (size_t)(reach + VN_ROWS) * (ldp + 4) * sizeof(float);
}

void launch_vadnet_stream(hipStream_t s, const VadNetStreamLaunch& a, int B) {
  if (B <= 0) return;
  PF_CHECK(a.img && a.states && a.n_new && a.n_out && a.ld >= 24 && a.ld % 8 == 0 && a.ldp % 32 == 0 && a.ldw == a.ldp + 4 &&
               a.n_layers >= 1 && a.n_layers <= 8 && a.reach == (a.lorder - 1) * a.lstride && a.state_bytes % 4 == 0 && a.words_off % 4 == 0 && a.words_off + 8 <= a.state_bytes && a.n_mels >= 1 &&
               a.lfr_m >= 1 && a.in_dim == a.n_mels * a.lfr_m && a.in1.Kpad <= a.ld - 8 && a.cap >= 0,
           PF_ERR_INVALID_ARG, "vadnet_stream: missing operand");
  const size_t lds = vadnet_stream_lds_bytes(a.ld, a.ldp, a.reach);
  PF_CHECK(lds <= kVadStreamMaxLds, PF_ERR_UNSUPPORTED, "vadnet_stream: the model's tiles and history window do not fit the LDS");
  static DeviceOnce once;
  once.run([] { set_max_lds((const void*)vadnet_stream_kernel, (int)kVadStreamMaxLds); });
  hipLaunchKernelGGL(vadnet_stream_kernel, dim3((unsigned)B), dim3(256), lds, s, a);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
