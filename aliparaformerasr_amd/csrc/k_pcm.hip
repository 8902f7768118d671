// k_pcm.hip — PCM intake on the device (DESIGN.md §PCM intake): raw interleaved values of B utterances -> the float32 mono
// samples at the engine's rate that the fbank kernel reads.  One launch per batch from a per-utterance job table.
//
// Every stage restates the host code operation for operation (hostutil.cpp pcm_decode / resample_linear, the
// restatement of AliParaformerAsr.Examples/Utils/AudioHelper.cs GetFileSample :12-32 and Resample :223-279), so the
// result is bit for bit the host's:
//   decode    PCM8 b/128-1, PCM16 /32768, PCM24 sign-extended /8388608, PCM32 (float)x /2147483648, float32 bits as they
//             are, float64 narrowed (round to nearest), G.711 A-law / mu-law closed forms /32768;
//   down-mix  (l + r) * 0.5f in float32, add then multiply; a trailing unpaired value is never read;
//   resample  float64 pos = i * ratio, idx = (int)pos, fr = pos - idx; m[last] when idx >= last, else
//             (float)((1 - fr) * m[idx] + fr * m[idx + 1]) — two multiplies and one add, EACH rounded.  The x86 host
//             build has no FMA, so the unfused result is the definition: contraction is off for this file (the pragma below
//             and -ffp-contract=off in the Makefile; hipcc's default for device code is to fuse).
// The format is uniform per utterance (blockIdx.y), so the switch is a uniform branch.
//
// Loads: at the native rate without a down-mix each thread converts FOUR consecutive values of a 1-, 2- or 4-byte format
// from one 4-, 8- or 16-byte load and stores one float4 (utterances start on 16-byte boundaries of both buffers).  24-bit
// values are 3-byte aligned and float64 values are 8 bytes wide: they, the down-mix and the interpolation use the
// per-value loads — neighbouring lanes read neighbouring values, a 48 kHz stereo input with a stride of three frames.
//
// Out of scope (paraformer_hip.h): the streaming recognizer, pf_group_*, more than two channels, compressed containers,
// sinc / polyphase filtering — the reference's linear interpolation is the definition here, aliasing included.
#include "kernels.h"

namespace pf {

#pragma clang fp contract(off)

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

template <int FMT>
__device__ __forceinline__ void pcm_convert(const PcmJob& j, const unsigned char* __restrict__ in, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  const int64_t n_out = j.n_out;
  const bool downmix = j.downmix != 0;
  if (!j.resample) {
    int64_t done = 0;
    if (!downmix && FMT != PF_PCM_S24 && FMT != PF_PCM_F64) {
      const int64_t quads = n_out >> 2;
      for (int64_t q = tid; q < quads; q += nthr) *(float4*)(out + 4 * q) = pcm_value4<FMT>(in, 4 * q);
      done = quads << 2;
    }
    for (int64_t i = done + tid; i < n_out; i += nthr) out[i] = pcm_mono<FMT>(in, i, downmix);
    return;
  }
  const double ratio = j.ratio;
  const int last = (int)j.n_mono - 1;
  for (int64_t i = tid; i < n_out; i += nthr) {
    const double pos = (double)(int)i * ratio;
    const int idx = (int)pos;
    const double fr = pos - (double)idx;
    float v;
    if (idx >= last) {
      v = pcm_mono<FMT>(in, last < 0 ? 0 : last, downmix);
    } else {
      const double a = (double)pcm_mono<FMT>(in, idx, downmix), b = (double)pcm_mono<FMT>(in, (int64_t)idx + 1, downmix);
      const double wa = (1.0 - fr) * a, wb = fr * b;     // each rounded: see the header comment
      v = (float)(wa + wb);
    }
    out[i] = v;
  }
}

// jobs != null: the batch form, utterance blockIdx.y of a table in device memory.  jobs == null: ONE utterance whose job rides
// in the kernel arguments — OfflineStream.AddPcm launches behind its own upload and has no table to copy in front of it.
__global__ __launch_bounds__(256) void pcm_to_samples_kernel(const PcmJob* __restrict__ jobs, const PcmJob one,
                                                             const unsigned char* __restrict__ raw, float* __restrict__ samples) {
  const PcmJob j = jobs ? jobs[blockIdx.y] : one;
  if ((int64_t)blockIdx.x * blockDim.x >= (j.n_out > 0 ? j.n_out : 0)) return;     // (a quad loop never starts beyond it either)
  const unsigned char* in = raw + j.in_off;
  float* out = samples + j.out_off;
  switch (j.format) {
    case PF_PCM_U8: pcm_convert<PF_PCM_U8>(j, in, out); break;
    case PF_PCM_S16: pcm_convert<PF_PCM_S16>(j, in, out); break;
    case PF_PCM_S24: pcm_convert<PF_PCM_S24>(j, in, out); break;
    case PF_PCM_S32: pcm_convert<PF_PCM_S32>(j, in, out); break;
    case PF_PCM_F32: pcm_convert<PF_PCM_F32>(j, in, out); break;
    case PF_PCM_F64: pcm_convert<PF_PCM_F64>(j, in, out); break;
    case PF_PCM_ALAW: pcm_convert<PF_PCM_ALAW>(j, in, out); break;
    case PF_PCM_MULAW: pcm_convert<PF_PCM_MULAW>(j, in, out); break;
    default: break;
  }
}

// grid-stride over the output: at most 256 workgroups per utterance (eight values per thread at 30 s of 16 kHz audio)
static unsigned pcm_grid_x(int64_t max_n_out) {
  const int64_t want = (max_n_out + 255) / 256;
  return (unsigned)(want < 256 ? want : 256);
}

void launch_pcm_to_samples(hipStream_t s, const PcmJob* jobs, int B, int64_t max_n_out, const void* raw, float* samples) {
  if (B == 0 || max_n_out <= 0) return;
  hipLaunchKernelGGL(pcm_to_samples_kernel, dim3(pcm_grid_x(max_n_out), (unsigned)B), dim3(256), 0, s, jobs, PcmJob{},
                     (const unsigned char*)raw, samples);
  PF_HIP(hipGetLastError());
}

void launch_pcm_to_samples_one(hipStream_t s, const PcmJob& job, const void* raw, float* samples) {
  if (job.n_out <= 0) return;
  hipLaunchKernelGGL(pcm_to_samples_kernel, dim3(pcm_grid_x(job.n_out), 1u), dim3(256), 0, s, (const PcmJob*)nullptr, job,
                     (const unsigned char*)raw, samples);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
