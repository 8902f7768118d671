// k_vadnet.hip — the FSMN-VAD model score on the device (paraformer_hip.h "Voice-activity segmentation, model score",
// DESIGN.md §4.6k).  The definition in numpy float64 is tests/vadnet_ref.py, the host twin host_vad_model_* (vadnet.cpp).
//
// Rows are the concatenated 10 ms fbank frames of all B utterances (frame offsets off [B + 1]); a workgroup of four waves
// owns a tile of 64 consecutive rows, which may straddle utterance boundaries: every row looks up its own utterance, and the
// LFR clamp and the zero history of the FSMN taps are per utterance.  1 + n_layers launches of ONE kernel:
//   launch 0            LFR + CMVN -> in_linear1 -> in_linear2 + ReLU -> linear_0                       -> p_0
//   launch l = 1 .. n-1 FSMN taps over p_{l-1} (global memory, left halo) -> affine_{l-1} + ReLU -> linear_l -> p_l
//   launch n            FSMN taps over p_{n-1} -> affine_{n-1} + ReLU -> out_linear1 -> out_linear2 -> softmax -> level
// The only dependence between tiles is the tap halo, which a launch boundary covers: no grid barrier, nothing persistent.
//
// A product is the one of tile_rows.h: W fragments from the image as the A operand, the activation tile X [64, K] f16 in LDS as
// the B operand.  The tile's row stride is ld = the widest operand + 8 halves: an odd number of 16-byte chunks, so the rows of
// a read do not all start on one bank; it is not conflict-free: at the released size ld = 408 is 204 dwords = 12 mod 64, and
// rows r and r + 16 of a read share a bank.  The cost of that was not measured.
//
// Rounding points (everything else is fp32): R0 the weights, once, at attach time; R1 the LFR + CMVN input; R2 in_linear1's
// output; R3 in_linear2's after ReLU; R4 the FSMN sum m; R5 affine's output after ReLU; R6 out_linear1's output.  p is stored
// as fp32 [rows, ldp] (proj padded to 32; the padding columns hold zeros), the logits are fp32 and go to memory only when asked
// for.  Padded rows and columns of W are zeros, padded columns of X are written as zeros, so padding never changes a sum;
// columns at or beyond output_dim never enter the softmax.
//
// The softmax runs on the accumulators: every lane keeps (max, sum, silence sum) over its channels on line, the two lane
// halves are merged with one shuffle, the four waves through 3 KB of LDS; e = rint((1 - 2 s) * 16384), -16384 when that is
// not finite.  ReLU is x < 0 ? 0 : x, which keeps a NaN (fmaxf would drop it).
// The FSMN sum, the softmax merge and the level formula are vadnet_dev.h's, shared with k_vadnet_stream.hip.
// Nothing at or beyond an utterance's T is read; rows at or beyond the total are computed as zeros and never stored.
#include "kdev.h"
#include "kernels.h"
#include "tile_rows.h"
#include "vadnet_dev.h"

namespace pf {

namespace {

struct VnRowInfo {            // per tile row: the first row of its utterance and that utterance's length; T = 0: no such row
  long long start[VN_ROWS];
  int T[VN_ROWS];
};

}  // namespace

__global__ __launch_bounds__(256) void vadnet_kernel(VadNetLaunch a) {
  extern __shared__ __attribute__((aligned(16))) char vn_lds[];
  __shared__ VnRowInfo info;
  __shared__ float red[4][VN_ROWS][3];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int ld = a.ld;
  half_t* buf0 = reinterpret_cast<half_t*>(vn_lds);
  half_t* buf1 = buf0 + (size_t)VN_ROWS * ld;
  const long long g0 = (long long)blockIdx.x * VN_ROWS;

  tr_row_info(a.off, a.B, a.total, g0, tid, info.start, info.T);       // every row's utterance
  __syncthreads();

  // ---- the head: the first f16 tile in buf0, width a.head_w (a multiple of 16), zeros in its padding columns and in rows
  // at or beyond the total
  if (a.head == 0) {
    // LFR + CMVN: column c = j * n_mels + m of row t is (x[clamp(t - left + j, 0, T - 1)][m] + shift[c]) * scale[c]     (R1)
    const float* __restrict__ shift = reinterpret_cast<const float*>(a.img + a.shift_off);
    const float* __restrict__ scale = reinterpret_cast<const float*>(a.img + a.scale_off);
    const int left = (a.lfr_m - 1) >> 1;
    for (int row = wave; row < VN_ROWS; row += 4) {
      const int T = info.T[row];
      const long long start = info.start[row], t = g0 + row - start;
      for (int c = lane; c < a.head_w; c += 64) {
        float v = 0.f;
        if (T > 0 && c < a.in_dim) {
          const int j = c / a.n_mels, m = c - j * a.n_mels;
          long long src = t - left + j;
          src = src < 0 ? 0 : (src > T - 1 ? T - 1 : src);
          v = (a.x[(start + src) * a.n_mels + m] + shift[c]) * scale[c];
        }
        buf0[row * ld + c] = (half_t)v;
      }
    }
  } else {
    // the FSMN sum over p (fp32, row stride ldp): m[t] = p[t] + sum_k taps[k] * p[t - (lorder - 1 - k) * lstride]   (R4)
    const float* __restrict__ taps = reinterpret_cast<const float*>(a.img + a.taps_off);
    for (int row = wave; row < VN_ROWS; row += 4) {
      const int T = info.T[row];
      const long long g = g0 + row, t = g - info.start[row];
      for (int c = lane; c < a.head_w; c += 64) {
        float v = 0.f;
        if (T > 0 && c < a.ldp) v = vn_fsmn_sum(a.p_in + g * a.ldp + c, a.ldp, taps + c, a.ldp, t, a.lorder, a.lstride);
        buf0[row * ld + c] = (half_t)v;
      }
    }
  }
  __syncthreads();

  // ---- the products that stay in LDS
  half_t* cur = buf0;
  half_t* nxt = buf1;
  for (int s = 0; s < a.n_mid; ++s) {
    vn_stage(a.img, a.mid[s], a.mid_relu[s] != 0, cur, nxt, ld, wave, lane);
    __syncthreads();
    half_t* t = cur; cur = nxt; nxt = t;
  }

  const int r = lane & 31, h = lane >> 5;
  if (a.tail == 0) {
    // ---- linear_l: p rows to memory, fp32, all ldp columns (the padding ones are exact zeros)
    tr_product(a.img, a.last, cur, ld, wave, lane, [&](int nt, int i, const f16x& acc) {
      const long long g = g0 + 32 * i + r;
      if (g < a.total) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<float4*>(a.p_out + g * a.ldp + 32 * nt + 8 * q + 4 * h) =
              make_float4(acc[4 * q + 0], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
      }
    });
    return;
  }

  // ---- out_linear2, the softmax and the level
  const float* __restrict__ silf = reinterpret_cast<const float*>(a.img + a.sil_off);
  vn_softmax_merge(a.img, a.last, cur, ld, wave, lane, silf, a.out_dim, red, [&](int j) -> float* {
    const long long g = g0 + j;
    return a.logits && g < a.total ? a.logits + g * a.out_dim : nullptr;
  });
  __syncthreads();
  if (tid < VN_ROWS) {
    const long long g = g0 + tid;
    if (g < a.total && a.levels) a.levels[g] = vn_level(red, tid);
  }
}

size_t vadnet_lds_bytes(int ld) { return (size_t)2 * VN_ROWS * ld * sizeof(half_t); }

void launch_vadnet(hipStream_t s, const VadNetLaunch& a) {
  if (a.total <= 0 || a.B <= 0) return;
  PF_CHECK(a.img && a.off && a.ld >= 24 && a.ld % 8 == 0 && a.head_w % 16 == 0 && a.head_w <= a.ld - 8 && a.n_mid >= 0 && a.n_mid <= 2 &&
               a.ldp % 32 == 0 && (a.head == 0 ? (a.x != nullptr && a.n_mels >= 1) : (a.p_in != nullptr)) &&
               (a.tail == 0 ? a.p_out != nullptr : (a.levels != nullptr || a.logits != nullptr)),
           PF_ERR_INVALID_ARG, "vadnet: missing operand");
  const size_t lds = vadnet_lds_bytes(a.ld);
  PF_CHECK(lds <= 150 * 1024, PF_ERR_UNSUPPORTED, "vadnet: the model's widest operand does not fit the LDS");
  static DeviceOnce once;
  once.run([] { set_max_lds((const void*)vadnet_kernel, 150 * 1024); });
  hipLaunchKernelGGL(vadnet_kernel, dim3((unsigned)((a.total + VN_ROWS - 1) / VN_ROWS)), dim3(256), lds, s, a);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
