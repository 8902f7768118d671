// k_cif_stream.hip — the streaming integrate-and-fire with its carried pair on the device, and the three small
// movers of the device-resident chunk step (Engine::online_step): the FSMN caches between a stream's slot and the decoder's
// batch, and the pack of the fired rows.  The host statement is online_cif_step (online.cpp, built on online_cif); the two agree
// bit for bit, the state block included.  This file is compiled with -ffp-contract=off and forms every product, sum and
// difference through exact.h: the host rounds them separately.
//
// cif_stream_kernel.  A stream's walk is [carry ; Tc chunk frames], at most 21 rows of 512 floats here: nothing to stream, only
// latency.  The fire chain (which entry fires, with what weight) is a scalar recurrence over the Tc + 1 alphas; every thread
// recomputes it in registers, so the threads of a stream exchange nothing and the channels are independent.  A workgroup is ONE
// wave whose lanes hold four channels each (kCifStreamGroup = 256 channels); the grid is (D / 256, B), so one stream of 512
// channels already runs on two CUs.  A thread issues the carry's and a tile's row loads (kTile = 20 rows, one float4 each) before
// it walks them; Tc <= 20 is one tile.  No LDS, no atomics, no barrier.  The integrate of the state block is kept once per
// channel group (decode_blocks.h CifStreamBlock): a workgroup reads and writes its own copy only.
//   entry 0      alpha = the carried integrate, hidden = the carried (divided) frame; entry j = chunk position j - 1
//   the mask     positions < lo and >= hi walk with alpha 0 (DynamicMask): their rows still enter, as 0 * h does on the host
//   fire         !(alpha + integrate < threshold): strict, so a sum that lands on the threshold fires
//   the carry    frames / integrate (IEEE division) when integrate > 0, else frames as they are
// A fire stores the thread's four channels of row `count`; behind the walk it zeroes its channels of the rows up to cap, and lane
// 0 of the first group writes count and the fire entries (-1 behind them).  count <= Tc + 1 <= cap (the launcher checks).
#include "exact.h"
#include "kdev.h"
#include "kernels.h"
#include "decode_blocks.h"

namespace pf {

namespace {
constexpr int kTile = 20;

__device__ __forceinline__ float4 mul4(float a, const float4& h) { return make_float4(mul_rn(a, h.x), mul_rn(a, h.y), mul_rn(a, h.z), mul_rn(a, h.w)); }
__device__ __forceinline__ float4 add4(const float4& f, const float4& p) { return make_float4(add_rn(f.x, p.x), add_rn(f.y, p.y), add_rn(f.z, p.z), add_rn(f.w, p.w)); }
}  // namespace

__global__ __launch_bounds__(64) void cif_stream_kernel(CifStreamLaunch a) {
  const int b = blockIdx.y, g = blockIdx.x, c4 = g * 64 + (int)threadIdx.x, D4 = a.D >> 2;
  if (c4 >= D4) return;
  char* sb = a.states + (int64_t)(a.slot ? a.slot[b] : b) * a.state_stride;
  float4* s_hidden = (float4*)sb + c4;                            // CifStreamBlock: hidden [D] | integrate [groups]
  float* s_integrate = (float*)sb + a.D + g;
  const bool fresh = a.reset && a.reset[b] != 0;
  const bool lead = g == 0 && threadIdx.x == 0;
  const float4* rows = (const float4*)(a.enc + (int64_t)b * a.Tc * a.D) + c4;
  const float* al = a.alphas + (int64_t)b * a.lda;
  float4* out = (float4*)(a.fired + (int64_t)b * a.cap * a.D) + c4;
  int32_t* ent = a.fire_entry + (int64_t)b * a.cap;
  const float thr = a.threshold;

  float integrate = 0.0f;
  float4 frames = make_float4(0.f, 0.f, 0.f, 0.f);
  int count = 0;
  auto step = [&](float alpha, const float4& h, int entry) {
    if (add_rn(alpha, integrate) < thr) {
      integrate = add_rn(integrate, alpha);
      frames = add4(frames, mul4(alpha, h));
    } else {
      frames = add4(frames, mul4(sub_rn(thr, integrate), h));
      if (count < a.cap) {
        out[(int64_t)count * D4] = frames;
        if (lead) ent[count] = entry;
      }
      ++count;
      integrate = add_rn(integrate, alpha);
      integrate = sub_rn(integrate, thr);
      frames = mul4(integrate, h);
    }
  };

  // the carry and the first tile's loads leave together
  float carry_a = 0.0f;
  float4 carry_h = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!fresh) { carry_a = *s_integrate; carry_h = *s_hidden; }
  for (int t0 = 0; t0 < a.Tc; t0 += kTile) {
    float4 h[kTile];
    float w[kTile];
#pragma unroll
    for (int i = 0; i < kTile; ++i) {
      const int t = t0 + i;
      const bool in = t < a.Tc;
      h[i] = in ? rows[(int64_t)t * D4] : make_float4(0.f, 0.f, 0.f, 0.f);
      w[i] = in && t >= a.lo && t < a.hi ? al[t] : 0.0f;
    }
    if (t0 == 0) step(carry_a, carry_h, 0);
#pragma unroll
    for (int i = 0; i < kTile; ++i)
      if (t0 + i < a.Tc) step(w[i], h[i], t0 + i + 1);
  }

  float4 keep = frames;
  if (integrate > 0.0f) keep = make_float4(frames.x / integrate, frames.y / integrate, frames.z / integrate, frames.w / integrate);
  *s_hidden = keep;
  if (threadIdx.x == 0) *s_integrate = integrate;
  for (int l = count; l < a.cap; ++l) out[(int64_t)l * D4] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (lead) {
    for (int l = count; l < a.cap; ++l) ent[l] = -1;
    a.counts[b] = count;
  }
}

void launch_cif_stream(hipStream_t s, const CifStreamLaunch& a) {
  PF_CHECK(a.B > 0 && a.Tc > 0 && a.D > 0 && a.D % 4 == 0 && a.cap >= a.Tc + 1, PF_ERR_INVALID_ARG,
           "cif_stream: B, Tc > 0, D % 4 == 0 and cap >= Tc + 1 expected");
  PF_CHECK(a.states && a.enc && a.alphas && a.fired && a.fire_entry && a.counts && a.lda >= a.Tc, PF_ERR_INVALID_ARG, "cif_stream: bad arguments");
  PF_CHECK(a.state_stride >= (int64_t)block_at_zero<CifStreamBlock>(a.D).bytes() && a.state_stride % 16 == 0, PF_ERR_INVALID_ARG,
           "cif_stream: the state stride does not hold a block");
  const unsigned groups = (unsigned)((a.D + (int)kCifStreamGroup - 1) / (int)kCifStreamGroup);
  hipLaunchKernelGGL(cif_stream_kernel, dim3(groups, (unsigned)a.B), dim3(64), 0, s, a);
  PF_HIP(hipGetLastError());
}

// ---- the FSMN caches: slot <-> the decoder's [nd, B, DC] batch (float4 cells; one thread per cell of one stream's cache)
__global__ __launch_bounds__(256) void cif_cache_gather_kernel(const char* __restrict__ states, int64_t state_stride, int64_t cache_off,
                                                               const int32_t* __restrict__ slot, const int32_t* __restrict__ reset, int B,
                                                               int nd, int DC4, float4* __restrict__ cin) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * DC4) return;
  const int b = (int)(i / DC4), c = (int)(i % DC4);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!(reset && reset[b] != 0)) v = ((const float4*)(states + (int64_t)slot[b] * state_stride + cache_off))[c];   // layer 0, for every layer
  for (int l = 0; l < nd; ++l) cin[((int64_t)l * B + b) * DC4 + c] = v;
}
__global__ __launch_bounds__(256) void cif_cache_scatter_kernel(char* __restrict__ states, int64_t state_stride, int64_t cache_off,
                                                                const int32_t* __restrict__ slot, int B, int nd, int DC4,
                                                                const float4* __restrict__ cout) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)nd * B * DC4) return;
  const int c = (int)(i % DC4), b = (int)((i / DC4) % B), l = (int)(i / ((int64_t)DC4 * B));
  ((float4*)(states + (int64_t)slot[b] * state_stride + cache_off))[(int64_t)l * DC4 + c] = cout[i];
}
void launch_cif_cache_gather(hipStream_t s, const char* states, int64_t state_stride, int64_t cache_off, const int32_t* slot,
                             const int32_t* reset, int B, int nd, int DC, float* cin) {
  PF_CHECK(states && slot && cin && B > 0 && nd > 0 && DC > 0 && DC % 4 == 0 && cache_off % 16 == 0 && state_stride % 16 == 0 &&
               state_stride >= cache_off + (int64_t)nd * DC * 4, PF_ERR_INVALID_ARG, "cif_cache_gather: bad arguments");
  const int64_t n = (int64_t)B * (DC / 4);
  hipLaunchKernelGGL(cif_cache_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, states, state_stride, cache_off, slot, reset, B,
                     nd, DC / 4, (float4*)cin);
  PF_HIP(hipGetLastError());
}
void launch_cif_cache_scatter(hipStream_t s, char* states, int64_t state_stride, int64_t cache_off, const int32_t* slot, int B, int nd,
                              int DC, const float* cout) {
  PF_CHECK(states && slot && cout && B > 0 && nd > 0 && DC > 0 && DC % 4 == 0 && cache_off % 16 == 0 && state_stride % 16 == 0 &&
               state_stride >= cache_off + (int64_t)nd * DC * 4, PF_ERR_INVALID_ARG, "cif_cache_scatter: bad arguments");
  const int64_t n = (int64_t)nd * B * (DC / 4);
  hipLaunchKernelGGL(cif_cache_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, states, state_stride, cache_off, slot, B, nd,
                     DC / 4, (const float4*)cout);
  PF_HIP(hipGetLastError());
}

// ---- the pack: fired [B, cap, D] -> dst [B, L, D]
__global__ __launch_bounds__(256) void cif_pack_kernel(const float4* __restrict__ fired, int B, int cap, int L, int D4, float4* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * L * D4) return;
  const int64_t per = (int64_t)L * D4;
  const int b = (int)(i / per);
  dst[i] = fired[(int64_t)b * cap * D4 + (i - (int64_t)b * per)];
}
void launch_cif_pack(hipStream_t s, const float* fired, int B, int cap, int L, int D, float* dst) {
  PF_CHECK(fired && dst && B > 0 && L > 0 && L <= cap && D > 0 && D % 4 == 0, PF_ERR_INVALID_ARG, "cif_pack: bad arguments");
  const int64_t n = (int64_t)B * L * (D / 4);
  hipLaunchKernelGGL(cif_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float4*)fired, B, cap, L, D / 4, (float4*)dst);
  PF_HIP(hipGetLastError());
}

// ---- counts and fire entries into pinned host memory (the route of export_plan_kernel, k_misc.hip)
__global__ void export_words_kernel(const int32_t* __restrict__ src, int n, volatile int32_t* dst) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
  __threadfence_system();
}
void launch_export_words(hipStream_t s, const int32_t* src, int n, int32_t* dst_dev) {
  if (n <= 0) return;
  hipLaunchKernelGGL(export_words_kernel, dim3(1), dim3(256), 0, s, src, n, dst_dev);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
