// pcm_dev.h — the PCM decode and down-mix of the intake kernels (k_pcm.hip, k_resample.hip), operation for operation the host's
// (hostutil.cpp pcm_decode and the (l + r) * 0.5f down-mix): value k of an utterance, sample j of its mono sequence, four values
// from one wide load.  Contraction is off inside each function, whatever the including file is compiled with.
#pragma once
#include "kernels.h"

namespace pf {

__device__ __forceinline__ float pcm_g711_mulaw(unsigned b) {
  const int u = (~b) & 0xFF;
  const int mag = ((((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84;
  return (float)((u & 0x80) ? -mag : mag) / 32768.0f;
}
__device__ __forceinline__ float pcm_g711_alaw(unsigned b) {
  const int a = (int)(b ^ 0x55u) & 0xFF, e = (a >> 4) & 7, m = a & 0x0F;
  const int mag = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);
  return (float)((a & 0x80) ? mag : -mag) / 32768.0f;
}

// value k of the utterance whose raw bytes start at `in`
template <int FMT>
__device__ __forceinline__ float pcm_value(const unsigned char* __restrict__ in, int64_t k) {
#pragma clang fp contract(off)
  if (FMT == PF_PCM_U8) return (float)in[k] / 128.0f - 1.0f;
  if (FMT == PF_PCM_S16) return (float)((const int16_t*)in)[k] / 32768.0f;
  if (FMT == PF_PCM_S24) {
    const unsigned char* q = in + 3 * k;
    const int32_t x = (int32_t)((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)(int32_t)(int8_t)q[2] << 16));
    return (float)x / 8388608.0f;
  }
  if (FMT == PF_PCM_S32) return (float)((const int32_t*)in)[k] / 2147483648.0f;
  if (FMT == PF_PCM_F32) return __uint_as_float(((const uint32_t*)in)[k]);
  if (FMT == PF_PCM_F64) return (float)((const double*)in)[k];
  if (FMT == PF_PCM_ALAW) return pcm_g711_alaw(in[k]);
  return pcm_g711_mulaw(in[k]);
}

// sample j of the (possibly down-mixed) mono sequence
template <int FMT>
__device__ __forceinline__ float pcm_mono(const unsigned char* __restrict__ in, int64_t j, bool downmix) {
#pragma clang fp contract(off)
  if (!downmix) return pcm_value<FMT>(in, j);
  const float l = pcm_value<FMT>(in, 2 * j), r = pcm_value<FMT>(in, 2 * j + 1);
  return (l + r) * 0.5f;
}

// four consecutive values from one wide load (1-, 2- and 4-byte formats; `in` + 4 k values is 4 / 8 / 16-byte aligned)
template <int FMT>
__device__ __forceinline__ float4 pcm_value4(const unsigned char* __restrict__ in, int64_t k) {
#pragma clang fp contract(off)
  float4 o;
  if (FMT == PF_PCM_S16) {
    const uint2 w = *(const uint2*)(in + 2 * k);
    o.x = (float)(int16_t)(w.x & 0xFFFF) / 32768.0f; o.y = (float)(int16_t)(w.x >> 16) / 32768.0f;
    o.z = (float)(int16_t)(w.y & 0xFFFF) / 32768.0f; o.w = (float)(int16_t)(w.y >> 16) / 32768.0f;
  } else if (FMT == PF_PCM_S32) {
    const int4 w = *(const int4*)(in + 4 * k);
    o.x = (float)w.x / 2147483648.0f; o.y = (float)w.y / 2147483648.0f;
    o.z = (float)w.z / 2147483648.0f; o.w = (float)w.w / 2147483648.0f;
  } else if (FMT == PF_PCM_F32) {
    const uint4 w = *(const uint4*)(in + 4 * k);
    o.x = __uint_as_float(w.x); o.y = __uint_as_float(w.y); o.z = __uint_as_float(w.z); o.w = __uint_as_float(w.w);
  } else {
    const uint32_t w = *(const uint32_t*)(in + k);
    const unsigned b0 = w & 0xFF, b1 = (w >> 8) & 0xFF, b2 = (w >> 16) & 0xFF, b3 = w >> 24;
    if (FMT == PF_PCM_U8) {
      o.x = (float)b0 / 128.0f - 1.0f; o.y = (float)b1 / 128.0f - 1.0f;
      o.z = (float)b2 / 128.0f - 1.0f; o.w = (float)b3 / 128.0f - 1.0f;
    } else if (FMT == PF_PCM_ALAW) {
      o.x = pcm_g711_alaw(b0); o.y = pcm_g711_alaw(b1); o.z = pcm_g711_alaw(b2); o.w = pcm_g711_alaw(b3);
    } else {
      o.x = pcm_g711_mulaw(b0); o.y = pcm_g711_mulaw(b1); o.z = pcm_g711_mulaw(b2); o.w = pcm_g711_mulaw(b3);
    }
  }
  return o;
}

}  // namespace pf
