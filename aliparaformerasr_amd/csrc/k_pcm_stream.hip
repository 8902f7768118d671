// k_pcm_stream.hip — the PCM intake of the streaming recognizer: for every PCM-fed stream of a GetResults call,
// the stream's next chunk of up to 9600 samples at the engine's rate, from the raw bytes that arrived since its last step and a
// tail of decoded frames carried on the device.  The host statement is PcmStream::take (hostutil.cpp), whose total is
// pcm_to_samples over the concatenated bytes; this kernel is bit for bit that, for every way of cutting the bytes into calls:
//   copy          out[i] = m[i];
//   linear        k_pcm.hip's statement with the GLOBAL output index: pos = (double)i * ratio, idx, fr, two products and a sum,
//                 each rounded (contraction is off), m[last] for idx >= last once the total is known;
//   band-limited  k_resample.hip's chain: acc = fmaf(h[p][k], m[b - H + 1 + k], acc), k ascending, one accumulator, +0 outside
//                 the sequence multiplied in.  That order is the definition: no tree, no split sum, no matrix instruction.
// m is the stream's mono sequence; frame g of it is +0 outside [0, n_total), a cell of the carried tail below in_first, else
// decoded from the step's raw frames (pcm_dev.h, as the offline kernels).
//
// Launch: 256 threads, blockIdx.y = the stream's job (read through scalar loads: every field is wave-uniform, the format switch
// a uniform branch), blockIdx.x walks the row's tiles of job.tile outputs.  Per tile the input span is assembled ONCE in LDS —
// tail cells, decoded frames, zeros — neighbouring lanes taking neighbouring frames; then one output per lane and pass.
// The coefficient rows are read from global memory: a chunk is about ten tiles, shared by as many workgroups, so a workgroup
// would copy a whole bank (91 KB at 44.1 kHz, 179 KB with 32 zero crossings at 11.025 kHz: more than the LDS) for ONE tile of
// 1024 chains; the rows a tile reads are at most the bank and stay in L2.  For L == 1 every lane reads the same coefficient:
// the one row sits in LDS, a broadcast.
// The tail: a stream's block holds two buffers.  Every workgroup reads only buffer tail_parity; workgroup 0 of the stream writes
// frames [next_first, next_first + next_len) — old tail cells and newly decoded frames — into the other one, which the host
// names as current in the next step.  No workgroup reads what another writes, no atomics, no wait between workgroups.
#include "kernels.h"
#pragma clang fp contract(off)
#include "decode_blocks.h"
#include "pcm_dev.h"

namespace pf {

static_assert(kPcmStreamTail == PF_RESAMPLE_MAX_TAPS, "the carried tail holds one window of the widest filter");
constexpr int kPsThreads = 256;
constexpr int kPsMaxLds = 160 * 1024;

template <int FMT>
__device__ __forceinline__ float ps_frame(const PcmStreamJob& j, const float* __restrict__ tail, const unsigned char* __restrict__ in,
                                          int64_t g) {
  if (g < 0 || (j.n_total >= 0 && g >= j.n_total)) return 0.0f;
  const int64_t r = g - j.in_first;
  if (r < 0) {
    const int64_t c = r + j.tail_len;
    return c >= 0 ? tail[c] : 0.0f;
  }
  return r < (int64_t)j.n_new ? pcm_mono<FMT>(in, r, j.downmix != 0) : 0.0f;
}

// the chain of one output: taps fused multiply-adds in k order (taps is even)
__device__ __forceinline__ float ps_chain(const float* __restrict__ h, const float* __restrict__ x, int taps) {
  float acc = 0.0f;
#pragma unroll 4
  for (int k = 0; k < taps; k += 2) {
    acc = __fmaf_rn(h[k], x[k], acc);
    acc = __fmaf_rn(h[k + 1], x[k + 1], acc);
  }
  return acc;
}

template <int FMT>
__device__ __forceinline__ void ps_stream(const PcmStreamJob& j, const unsigned char* __restrict__ raw, char* __restrict__ states,
                                          int64_t state_stride, float* __restrict__ samples, float* __restrict__ xs, int xs_cap) {
#pragma clang fp contract(off)
  const unsigned char* in = raw + j.raw_off;
  float* blk = (float*)(states + (int64_t)j.slot * state_stride);
  const float* tail = blk + (size_t)j.tail_parity * kPcmStreamTail;
  float* out = samples + (int64_t)j.row * kPcmStreamRow;
  float* hs = xs + xs_cap;
  const int tid = (int)threadIdx.x;
  if (blockIdx.x == 0 && j.write_tail) {
    float* nt = blk + (size_t)(j.tail_parity ^ 1) * kPcmStreamTail;
    for (int i = tid; i < j.next_len; i += kPsThreads) nt[i] = ps_frame<FMT>(j, tail, in, j.next_first + i);
  }
  const int tile = j.tile, ntiles = (kPcmStreamRow + tile - 1) / tile;
  const int L = j.L, taps = 2 * j.H;
  const float* __restrict__ hg = j.bank;
  if (j.rule == 2 && L == 1)                                 // (the first tile's barriers order it before any read)
    for (int i = tid; i < taps; i += kPsThreads) hs[i] = hg[i];
  for (int t = (int)blockIdx.x; t < ntiles; t += (int)gridDim.x) {
    const int ol = t * tile;
    const int cells = kPcmStreamRow - ol < tile ? kPcmStreamRow - ol : tile;
    const int left = j.n_out - ol;
    const int n = left <= 0 ? 0 : (left < cells ? left : cells);
    for (int i = n + tid; i < cells; i += kPsThreads) out[ol + i] = 0.0f;     // behind the stream's outputs: +0, as InputFinished pads
    if (n == 0) continue;
    const int64_t gi = j.o0 + ol;
    if (j.rule == 0) {
      for (int jj = tid; jj < n; jj += kPsThreads) out[ol + jj] = ps_frame<FMT>(j, tail, in, gi + jj);
      continue;
    }
    int64_t lo;
    int span;
    unsigned p0 = 0;
    if (j.rule == 2) {
      const int64_t pos0 = gi * (int64_t)j.M;
      p0 = (unsigned)(pos0 % L);
      lo = pos0 / L - j.H + 1;
      span = (int)((unsigned)(n - 1) * (unsigned)(j.M / L) + (p0 + (unsigned)(n - 1) * (unsigned)(j.M % L)) / (unsigned)L) + taps;
    } else {
      lo = (int64_t)((double)gi * j.ratio);
      span = (int)((int64_t)((double)(gi + n - 1) * j.ratio) - lo) + 2;
    }
    if (span > xs_cap) continue;                             // never (ps_span bounds this span): such a tile is left unwritten, not read short
    __syncthreads();                                         // the previous tile has been read
    for (int i = tid; i < span; i += kPsThreads) xs[i] = ps_frame<FMT>(j, tail, in, lo + i);
    __syncthreads();
    if (j.rule == 2) {
      const unsigned qM = (unsigned)(j.M / L), rM = (unsigned)(j.M % L), stride = (unsigned)j.stride;
      if (L == 1) {
        for (int jj = tid; jj < n; jj += kPsThreads) out[ol + jj] = ps_chain(hs, xs + (unsigned)jj * qM, taps);
      } else {
        for (int jj = tid; jj < n; jj += kPsThreads) {
          const unsigned e = p0 + (unsigned)jj * rM;
          out[ol + jj] = ps_chain(hg + (e % (unsigned)L) * stride, xs + (unsigned)jj * qM + e / (unsigned)L, taps);
        }
      }
    } else {
      const int64_t last = j.n_total - 1;
      for (int jj = tid; jj < n; jj += kPsThreads) {
        const double pos = (double)(gi + jj) * j.ratio;
        const int64_t idx = (int64_t)pos;
        const double fr = pos - (double)idx;
        float v;
        if (j.n_total >= 0 && idx >= last) {
          v = ps_frame<FMT>(j, tail, in, last < 0 ? 0 : last);
        } else {
          const int o = (int)(idx - lo);
          const double a = (double)xs[o], b = (double)xs[o + 1];
          const double wa = (1.0 - fr) * a, wb = fr * b;      // each rounded: see k_pcm.hip
          v = (float)(wa + wb);
        }
        out[ol + jj] = v;
      }
    }
  }
}

__global__ __launch_bounds__(kPsThreads) void pcm_stream_kernel(const PcmStreamJob* __restrict__ jobs, const unsigned char* __restrict__ raw,
                                                                char* __restrict__ states, int64_t state_stride,
                                                                float* __restrict__ samples, int xs_cap) {
  extern __shared__ __align__(16) float ps_lds[];
  const PcmStreamJob j = jobs[blockIdx.y];
  switch (j.format) {
    case PF_PCM_U8: ps_stream<PF_PCM_U8>(j, raw, states, state_stride, samples, ps_lds, xs_cap); break;
    case PF_PCM_S16: ps_stream<PF_PCM_S16>(j, raw, states, state_stride, samples, ps_lds, xs_cap); break;
    case PF_PCM_S24: ps_stream<PF_PCM_S24>(j, raw, states, state_stride, samples, ps_lds, xs_cap); break;
    case PF_PCM_S32: ps_stream<PF_PCM_S32>(j, raw, states, state_stride, samples, ps_lds, xs_cap); break;
    case PF_PCM_F32: ps_stream<PF_PCM_F32>(j, raw, states, state_stride, samples, ps_lds, xs_cap); break;
    case PF_PCM_F64: ps_stream<PF_PCM_F64>(j, raw, states, state_stride, samples, ps_lds, xs_cap); break;
    case PF_PCM_ALAW: ps_stream<PF_PCM_ALAW>(j, raw, states, state_stride, samples, ps_lds, xs_cap); break;
    case PF_PCM_MULAW: ps_stream<PF_PCM_MULAW>(j, raw, states, state_stride, samples, ps_lds, xs_cap); break;
    default: break;
  }
}

// the LDS floats a tile of n outputs can need (an upper bound of the kernel's span).
// Linear rule: the kernel's span is floor(a) - floor(b) + 2 with a = fl((gi + n - 1) ratio), b = fl(gi ratio).  Every position is
// below 2^31 frames, so each product is off by at most 2^-22 (half an ulp of a double below 2^31), and
// floor(a) - floor(b) < a - b + 1 <= X + 1 + 2^-21 with X = (n - 1) ratio exactly; the span is an integer below X + 3 + 2^-21, hence at
// most ceil(X) + 3.  fl(X) as formed here can lie 2^-38 under X (X <= 1023 * 6 at the steepest ratio that fits), which can make
// the ceil one too small; + 4 covers that as well.  One cell more than is ever read.
static int64_t ps_span(const PcmStreamJob& j, int64_t n) {
  if (j.rule == 0) return 0;
  if (j.rule == 1) return (int64_t)std::ceil((double)(n - 1) * j.ratio) + 4;
  return (n - 1) * (int64_t)(j.M / j.L) + ((int64_t)j.L - 1 + (n - 1) * (int64_t)(j.M % j.L)) / j.L + 2 * (int64_t)j.H;
}

void pcm_stream_fit(PcmStreamJob& j) {
  int tile = PF_RESAMPLE_TILE;
  while (tile > 1 && ps_span(j, tile) > kResampleInCap) tile >>= 1;
  j.tile = tile;
}

static int ps_frame_bytes(const PcmStreamJob& j) {
  const int bps = j.format == PF_PCM_S16 ? 2 : j.format == PF_PCM_S24 ? 3 : (j.format == PF_PCM_S32 || j.format == PF_PCM_F32) ? 4 : j.format == PF_PCM_F64 ? 8 : 1;
  return bps * (j.downmix ? 2 : 1);
}

void launch_pcm_stream(hipStream_t s, const PcmStreamJob* jobs_dev, const PcmStreamJob* jobs_host, int B, const void* raw, int64_t raw_bytes,
                       char* states, int64_t state_stride, int n_slots, float* samples, int n_rows) {
  PF_CHECK(jobs_dev && jobs_host && B > 0 && states && samples && (raw || raw_bytes == 0), PF_ERR_INVALID_ARG, "pcm_stream: bad arguments");
  PF_CHECK(state_stride >= (int64_t)block_at_zero<PcmStreamBlock>().bytes() && state_stride % 4 == 0, PF_ERR_INVALID_ARG,
           "pcm_stream: the state stride does not hold a block");
  int64_t xs_cap = 0;
  int gx = 1;
  for (int b = 0; b < B; ++b) {                                  // every index the kernel forms is checked here
    const PcmStreamJob& j = jobs_host[b];
    const int64_t tail_first = j.in_first - j.tail_len;
    PF_CHECK(j.format >= PF_PCM_U8 && j.format <= PF_PCM_MULAW && j.rule >= 0 && j.rule <= 2 && j.row >= 0 && j.row < n_rows && j.slot >= 0 &&
                 j.slot < n_slots && j.n_out >= 0 && j.n_out <= kPcmStreamRow && j.n_new >= 0 && j.o0 >= 0 && j.in_first >= 0 &&
                 (j.tail_parity == 0 || j.tail_parity == 1) && j.tail_len >= 0 && j.tail_len <= (int)kPcmStreamTail && tail_first >= 0 &&
                 j.raw_off >= 0 && j.raw_off % 16 == 0 && j.raw_off + (int64_t)j.n_new * ps_frame_bytes(j) <= raw_bytes &&
                 j.tile >= 1 && j.tile <= PF_RESAMPLE_TILE && (j.tile & (j.tile - 1)) == 0,
             PF_ERR_INVALID_ARG, "pcm_stream: bad job");
    PF_CHECK(!j.write_tail || (j.next_len >= 0 && j.next_len <= (int)kPcmStreamTail && j.next_first >= tail_first &&
                               j.next_first + j.next_len <= j.in_first + j.n_new),
             PF_ERR_INVALID_ARG, "pcm_stream: bad next tail");
    if (j.rule == 1) PF_CHECK(j.ratio > 0.0 && std::isfinite(j.ratio), PF_ERR_INVALID_ARG, "pcm_stream: bad ratio");
    if (j.rule == 2)
      PF_CHECK(j.bank && j.L >= 1 && j.L <= PF_RESAMPLE_MAX_PHASES && j.M >= 1 && j.H >= 1 && 2 * j.H <= PF_RESAMPLE_MAX_TAPS && j.stride > 2 * j.H,
               PF_ERR_INVALID_ARG, "pcm_stream: bad bank");
    PF_CHECK(ps_span(j, j.tile) <= kResampleInCap, PF_ERR_UNSUPPORTED, "pcm_stream: one output's input span does not fit the LDS");
    xs_cap = std::max(xs_cap, ps_span(j, j.tile));
    gx = std::max(gx, (kPcmStreamRow + j.tile - 1) / j.tile);
  }
  static DeviceOnce once;
  once.run([] { set_max_lds((const void*)pcm_stream_kernel, kPsMaxLds); });
  const size_t lds = ((size_t)xs_cap + PF_RESAMPLE_MAX_TAPS) * sizeof(float);
  hipLaunchKernelGGL(pcm_stream_kernel, dim3((unsigned)std::min(gx, 256), (unsigned)B), dim3(kPsThreads), lds, s, jobs_dev,
                     (const unsigned char*)raw, states, state_stride, samples, (int)xs_cap);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
