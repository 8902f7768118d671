// punc_dev.h — the device pieces the two forms of the CT-Transformer share (k_punc.hip: B windows, a launch per stage;
// k_punc_stream.hip: B streams with carried keys and values, one launch): the tile geometry, the LayerNorm of a row tile and
// the steps of the two-pass attention on one 32-key block.  Everything here is __forceinline__.
#pragma once
#include "kdev.h"
#include "tile_rows.h"

namespace pf {

constexpr int PR_ROWS = TR_ROWS, PR_D = 256, PR_XLD = 260, PR_LD = 264;
constexpr size_t PR_X_BYTES = (size_t)PR_ROWS * PR_XLD * 4, PR_BUF_BYTES = (size_t)PR_ROWS * PR_LD * 2;

// LayerNorm of the fp32 tile into an f16 tile: one wave per row, four channels per lane                          (R1)
__device__ __forceinline__ void pr_norm(const float* __restrict__ xs, const float* __restrict__ gam, const float* __restrict__ bet,
                                        half_t* __restrict__ y, int wave, int lane) {
  const float4 g4 = *reinterpret_cast<const float4*>(gam + 4 * lane), b4 = *reinterpret_cast<const float4*>(bet + 4 * lane);
  for (int row = wave; row < PR_ROWS; row += 4) {
    const float4 v = *reinterpret_cast<const float4a*>(xs + row * PR_XLD + 4 * lane);
    const float mu = wave_sum((v.x + v.y) + (v.z + v.w)) * (1.f / PR_D);
    const float d0 = v.x - mu, d1 = v.y - mu, d2 = v.z - mu, d3 = v.w - mu;
    const float var = wave_sum((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3)) * (1.f / PR_D);
    const float inv = 1.f / sqrtf(var + 1e-12f);
    h4 o;
    o[0] = (half_t)(d0 * inv * g4.x + b4.x); o[1] = (half_t)(d1 * inv * g4.y + b4.y);
    o[2] = (half_t)(d2 * inv * g4.z + b4.z); o[3] = (half_t)(d3 * inv * g4.w + b4.w);
    *reinterpret_cast<h4a*>(y + row * PR_LD + 4 * lane) = o;
  }
}

// ---- attention on one head of 32 channels.  S^T = K Q^T: 32 keys on the accumulator's rows, the lane's query on its column.
// Register e of the accumulator is key key0 + (e & 3) + 8 (e >> 2), key0 = the block's first key + 4 h.  A key at or beyond
// `lim` is masked: it takes no part in the maximum and contributes an exact zero to the sum and to O.
// kp: the lane's key row at the head's channel 8 h; qf: the lane's query, channels 16 s + 8 h + (0 .. 7)
__device__ __forceinline__ f16x pa_scores(const half_t* kp, const h8 (&qf)[2]) {
  const h8 k0 = *reinterpret_cast<const h8*>(kp), k1 = *reinterpret_cast<const h8*>(kp + 16);
  f16x z;
#pragma unroll
  for (int e = 0; e < 16; ++e) z[e] = 0.f;
  z = __builtin_amdgcn_mfma_f32_32x32x16_f16(k0, qf[0], z, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(k1, qf[1], z, 0, 0, 0);
}
// pass 1: the lane's share of the row maximum
__device__ __forceinline__ void pa_max(const f16x& S, int key0, int lim, float& mx) {
#pragma unroll
  for (int e = 0; e < 16; ++e)
    if (key0 + (e & 3) + 8 * (e >> 2) < lim) mx = fmaxf(mx, S[e]);
}
// the V^T fragment of a block: vrow = the lane's channel row of V^T [32, keys] in LDS at the block's first key + 4 h
__device__ __forceinline__ void pa_vfrag(const half_t* vrow, h8 (&vf)[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const half_t* vp = vrow + 16 * s;
    const h4 lo = *reinterpret_cast<const h4a*>(vp), hi = *reinterpret_cast<const h4a*>(vp + 8);
    vf[s] = h8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  }
}
// pass 2: exp(s - max) (R3 as the PV operand; the sum takes the fp32 values) and O^T += V^T P^T
__device__ __forceinline__ void pa_pv(const f16x& S, float mx, int key0, int lim, const h8 (&vf)[2], float& sum, f16x& O) {
  h8 pf[2];
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    float p = 0.f;
    if (key0 + (e & 3) + 8 * (e >> 2) < lim) p = expf(S[e] - mx);
    sum += p;
    pf[e >> 3][e & 7] = (half_t)p;                                                           // R3
  }
  O = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[0], pf[0], O, 0, 0, 0);
  O = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[1], pf[1], O, 0, 0, 0);
}

}  // namespace pf
