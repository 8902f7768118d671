// vadnet_dev.h — the device arithmetic the two FSMN-VAD kernels share (k_vadnet.hip: whole utterances, 1 + n_layers launches;
// k_vadnet_stream.hip: B streams with carried history, one launch).  The streaming levels and logits are defined as bit-equal
// to the offline ones, so the FSMN sum, the softmax merge and the level formula exist ONCE, here: same expression, same order.
// Everything is __forceinline__.
#pragma once
#include "kdev.h"
#include "tile_rows.h"

namespace pf {

constexpr int VN_ROWS = TR_ROWS;

// the f16 tile of the next product: Y [64, g.Npad], optional ReLU
__device__ __forceinline__ void vn_stage(const char* __restrict__ img, const TileGemm& g, bool relu, const half_t* x, half_t* y, int ld,
                                         int wave, int lane) {
  const int r = lane & 31, h = lane >> 5;
  tr_product(img, g, x, ld, wave, lane, [&](int nt, int i, const f16x& acc) { tr_put_f16(acc, relu, y, ld, i, nt, r, h); });
}

// the FSMN sum of ONE channel of frame t (the absolute frame index of its utterance or stream; R4 rounds the result):
//   m[t] = p[t] + sum_k taps[k] * p[t - (lorder - 1 - k) * lstride],  a tap whose source lies before frame 0 skipped.
// pt: that channel of row t of p, the rows before it at a stride of pstride floats (global memory or LDS); tc: the channel's
// column of taps [lorder, tstride]
__device__ __forceinline__ float vn_fsmn_sum(const float* pt, long long pstride, const float* __restrict__ tc, int tstride, long long t,
                                             int lorder, int lstride) {
  float v = pt[0];
  for (int k = 0; k < lorder; ++k) {
    const long long d = (long long)(lorder - 1 - k) * lstride;
    if (d <= t) v += tc[k * tstride] * pt[-d * pstride];
  }
  return v;
}

// out_linear2 and the softmax merge over the f16 tile x: every lane keeps (max, sum, silence sum) over its channels on line,
// the two lane halves are merged with one shuffle, and every wave leaves its share of tile row j in red[wave][j].  The caller
// synchronises, then vn_level merges the four waves.  logits_row(j): where tile row j's logits go (null: nowhere).
template <class RowPtr>
__device__ __forceinline__ void vn_softmax_merge(const char* __restrict__ img, const TileGemm& g, const half_t* x, int ld, int wave, int lane,
                                                 const float* __restrict__ silf, int out_dim, float (*red)[VN_ROWS][3], RowPtr&& logits_row) {
  const int r = lane & 31, h = lane >> 5;
  float mx[2] = {-INFINITY, -INFINITY}, sum[2] = {0.f, 0.f}, sil[2] = {0.f, 0.f};
  bool poisoned[2] = {false, false};
  tr_product(img, g, x, ld, wave, lane, [&](int nt, int i, const f16x& acc) {
    float* lrow = logits_row(32 * i + r);
    float tm = -INFINITY;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = 32 * nt + 8 * q + 4 * h;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n + e < out_dim) {
          const float v = acc[4 * q + e];
          if (v != v) poisoned[i] = true;
          tm = fmaxf(tm, v);
          if (lrow) lrow[n + e] = v;
        }
    }
    if (tm == -INFINITY) return;                         // no valid column in this block for this lane half, or all -inf
    const float nm = fmaxf(mx[i], tm);
    const float sc = mx[i] == -INFINITY ? 0.f : expf(mx[i] - nm);
    float s1 = sum[i] * sc, s2 = sil[i] * sc;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = 32 * nt + 8 * q + 4 * h;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n + e < out_dim) {
          const float ex = expf(acc[4 * q + e] - nm);
          s1 += ex;
          s2 += ex * silf[n + e];
        }
    }
    mx[i] = nm; sum[i] = s1; sil[i] = s2;
  });
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    // the other lane half holds the other channels of the same row
    const float om = __shfl_xor(mx[i], 32, 64), os = __shfl_xor(sum[i], 32, 64), oq = __shfl_xor(sil[i], 32, 64);
    const bool op = __shfl_xor((int)poisoned[i], 32, 64) != 0;
    const float nm = fmaxf(mx[i], om);
    const float ca = mx[i] == -INFINITY ? 0.f : expf(mx[i] - nm), cb = om == -INFINITY ? 0.f : expf(om - nm);
    float s1 = sum[i] * ca + os * cb, s2 = sil[i] * ca + oq * cb;
    if (poisoned[i] || op) s1 = NAN;
    if (h == 0) { red[wave][32 * i + r][0] = nm; red[wave][32 * i + r][1] = s1; red[wave][32 * i + r][2] = s2; }
  }
}

// the level of tile row j from the four waves' shares: e = rint((1 - 2 s) * 16384), -16384 when that is not finite
__device__ __forceinline__ int vn_level(const float (*red)[VN_ROWS][3], int j) {
  float nm = -INFINITY;
#pragma unroll
  for (int w = 0; w < 4; ++w) nm = fmaxf(nm, red[w][j][0]);
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const float m = red[w][j][0];
    const float c = m == -INFINITY ? 0.f : expf(m - nm);
    s1 += red[w][j][1] * c;
    s2 += red[w][j][2] * c;
  }
  const float v = (1.f - 2.f * (s2 / s1)) * 16384.f;
  return (v >= -16384.f && v <= 16384.f) ? (int)rintf(v) : -16384;
}

}  // namespace pf
