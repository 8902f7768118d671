// k_resample.hip — PCM intake with PF_PCM_RESAMPLE_SINC: raw interleaved values of the flagged utterances of
// a batch -> float32 mono samples at the engine's rate through a polyphase Kaiser-windowed sinc filter.  The definition is
// tests/resample_ref.py; the host twin is hostutil.cpp resample_sinc_mono, bit for bit:
//   output i:  b = (i M) / L, p = (i M) % L,  acc = +0;  for k = 0 .. taps - 1:  acc = fmaf(h[p][k], m[b - H + 1 + k], acc)
// with m = the decoded, down-mixed mono sequence (pcm_dev.h, as k_pcm.hip) and +0 outside it — multiplied in, not skipped.
// The bank h is DATA (hostutil.cpp resample_bank, float64 rounded to float32 once): the only arithmetic here is __fmaf_rn, in k
// order, one accumulator per output.  That order is the definition, so there is no tree, no split sum and no matrix instruction.
//
// Launch: 256 threads, blockIdx.y = the utterance (a job table, or ONE job in the kernel arguments for OfflineStream.AddPcm),
// blockIdx.x < job.gx workgroups that walk the utterance's tiles of job.tile outputs (PF_RESAMPLE_TILE unless the rate ratio is so
// steep that the tile's input would not fit).  Per tile:
//   1. the input span [floor(o0 M / L) - H + 1, floor((o0 + n - 1) M / L) + H] is decoded and down-mixed ONCE into LDS,
//      neighbouring lanes reading neighbouring frames, zeros outside [0, n_mono);
//   2. lane j computes output o0 + j (+ 256, ...): its window starts at j * (M div L) + (p0 + j * (M mod L)) / L of the tile —
//      32-bit arithmetic per output, one 64-bit division per tile.
// The bank sits in LDS behind the input tile when both fit in the CU's 160 KB (copied once per workgroup, row stride odd);
// otherwise its rows are read from global memory (at most 4 MB, L2-resident).  For L == 1 every lane reads the same coefficient:
// an LDS broadcast.
#include "kernels.h"
#include "hostutil.h"
#include "pcm_dev.h"

#include <map>
#include <mutex>

namespace pf {

constexpr int kRsThreads = 256;
constexpr int kRsMaxLds = 160 * 1024;

template <int FMT>
__device__ __forceinline__ void rs_fill(float* __restrict__ xs, const unsigned char* __restrict__ in, int64_t lo, int span,
                                        int64_t n_mono, bool downmix) {
  for (int i = threadIdx.x; i < span; i += kRsThreads) {
    const int64_t g = lo + i;
    xs[i] = (g >= 0 && g < n_mono) ? pcm_mono<FMT>(in, g, downmix) : 0.0f;
  }
}

// the chain of one output: taps fused multiply-adds in k order (taps is even)
__device__ __forceinline__ float rs_chain(const float* __restrict__ h, const float* __restrict__ x, int taps) {
  float acc = 0.0f;
#pragma unroll 4
  for (int k = 0; k < taps; k += 2) {
    acc = __fmaf_rn(h[k], x[k], acc);
    acc = __fmaf_rn(h[k + 1], x[k + 1], acc);
  }
  return acc;
}

// TABLE: the batch form, utterance blockIdx.y of a table in device memory; else ONE utterance whose job rides in the kernel
// arguments.  Either way the job is read through scalar loads: every field is wave-uniform.
template <bool TABLE>
__global__ __launch_bounds__(kRsThreads) void resample_sinc_kernel(const ResampleJob* __restrict__ jobs, const ResampleJob one,
                                                                   const unsigned char* __restrict__ raw, float* __restrict__ samples) {
  extern __shared__ __align__(16) float rs_lds[];
  const ResampleJob j = TABLE ? jobs[blockIdx.y] : one;
  const int64_t ntiles = j.n_out > 0 ? (j.n_out + j.tile - 1) / j.tile : 0;
  if ((int)blockIdx.x >= j.gx || (int64_t)blockIdx.x >= ntiles) return;
  const unsigned char* in = raw + j.in_off;
  float* out = samples + j.out_off;
  float* xs = rs_lds;
  float* hs = rs_lds + j.in_cap;
  const int L = j.L, taps = 2 * j.H, stride = j.stride;
  const unsigned qM = (unsigned)(j.M / L), rM = (unsigned)(j.M % L);
  const float* __restrict__ hg = j.bank;
  if (j.bank_lds)                                          // (the first tile's barriers order it before any read)
    for (int i = threadIdx.x; i < L * stride; i += kRsThreads) hs[i] = hg[i];
  const bool downmix = j.downmix != 0;
  for (int64_t t = blockIdx.x; t < ntiles; t += j.gx) {
    const int64_t o0 = t * j.tile, pos0 = o0 * (int64_t)j.M;
    const int64_t b0 = pos0 / L;
    const unsigned p0 = (unsigned)(pos0 % L);
    const int n = (int)(j.n_out - o0 < (int64_t)j.tile ? j.n_out - o0 : (int64_t)j.tile);
    const int span = (int)((unsigned)(n - 1) * qM + (p0 + (unsigned)(n - 1) * rM) / (unsigned)L) + taps;     // <= in_cap
    const int64_t lo = b0 - j.H + 1;
    __syncthreads();                                       // the previous tile has been read
    switch (j.format) {
      case PF_PCM_U8: rs_fill<PF_PCM_U8>(xs, in, lo, span, j.n_mono, downmix); break;
      case PF_PCM_S16: rs_fill<PF_PCM_S16>(xs, in, lo, span, j.n_mono, downmix); break;
      case PF_PCM_S24: rs_fill<PF_PCM_S24>(xs, in, lo, span, j.n_mono, downmix); break;
      case PF_PCM_S32: rs_fill<PF_PCM_S32>(xs, in, lo, span, j.n_mono, downmix); break;
      case PF_PCM_F32: rs_fill<PF_PCM_F32>(xs, in, lo, span, j.n_mono, downmix); break;
      case PF_PCM_F64: rs_fill<PF_PCM_F64>(xs, in, lo, span, j.n_mono, downmix); break;
      case PF_PCM_ALAW: rs_fill<PF_PCM_ALAW>(xs, in, lo, span, j.n_mono, downmix); break;
      case PF_PCM_MULAW: rs_fill<PF_PCM_MULAW>(xs, in, lo, span, j.n_mono, downmix); break;
      default: break;
    }
    __syncthreads();
    if (j.bank_lds) {
      for (int jj = threadIdx.x; jj < n; jj += kRsThreads) {
        const unsigned e = p0 + (unsigned)jj * rM;
        out[o0 + jj] = rs_chain(hs + (e % (unsigned)L) * (unsigned)stride, xs + (unsigned)jj * qM + e / (unsigned)L, taps);
      }
    } else {
      for (int jj = threadIdx.x; jj < n; jj += kRsThreads) {
        const unsigned e = p0 + (unsigned)jj * rM;
        out[o0 + jj] = rs_chain(hg + (e % (unsigned)L) * (unsigned)stride, xs + (unsigned)jj * qM + e / (unsigned)L, taps);
      }
    }
  }
}

static size_t rs_lds_bytes(const ResampleJob& j) {
  return ((size_t)j.in_cap + (j.bank_lds ? (size_t)j.L * j.stride : 0)) * sizeof(float);
}

static void rs_launch(hipStream_t s, const ResampleJob* jobs_dev, const ResampleJob* jobs_host, int B, const void* raw, float* samples) {
  size_t lds = 0;
  int gx = 0;
  for (int b = 0; b < B; ++b) {
    const ResampleJob& j = jobs_host[b];
    PF_CHECK(j.L >= 1 && j.L <= PF_RESAMPLE_MAX_PHASES && j.H >= 1 && 2 * j.H <= PF_RESAMPLE_MAX_TAPS && j.stride > 2 * j.H && j.tile >= 1 &&
                 j.tile <= PF_RESAMPLE_TILE && j.in_cap >= 2 * j.H && j.in_cap <= kResampleInCap && j.bank && j.n_mono >= 0 &&
                 rs_lds_bytes(j) <= (size_t)kRsMaxLds,
             PF_ERR_INVALID_ARG, "resample: bad job");
    if (j.n_out <= 0) continue;
    lds = std::max(lds, rs_lds_bytes(j));
    gx = std::max(gx, j.gx);
  }
  if (gx <= 0) return;
  static DeviceOnce once;
  once.run([] {
    set_max_lds((const void*)resample_sinc_kernel<true>, kRsMaxLds);
    set_max_lds((const void*)resample_sinc_kernel<false>, kRsMaxLds);
  });
  if (jobs_dev)
    hipLaunchKernelGGL(resample_sinc_kernel<true>, dim3((unsigned)gx, (unsigned)B), dim3(kRsThreads), lds, s, jobs_dev, ResampleJob{},
                       (const unsigned char*)raw, samples);
  else
    hipLaunchKernelGGL(resample_sinc_kernel<false>, dim3((unsigned)gx, 1u), dim3(kRsThreads), lds, s, jobs_dev, jobs_host[0],
                       (const unsigned char*)raw, samples);
  PF_HIP(hipGetLastError());
}

void launch_resample_sinc(hipStream_t s, const ResampleJob* jobs_dev, const ResampleJob* jobs_host, int B, const void* raw, float* samples) {
  if (B > 0) rs_launch(s, jobs_dev, jobs_host, B, raw, samples);
}

void launch_resample_sinc_one(hipStream_t s, const ResampleJob& job, const void* raw, float* samples) {
  rs_launch(s, nullptr, &job, 1, raw, samples);
}

// ---- the banks ----
struct ResampleBanks::Impl {
  std::mutex mu;
  pf_resample_config cfg = resample_default();
  std::map<int, ResampleBankDev> banks;                    // by input rate (one engine rate per owner)
};

ResampleBanks::ResampleBanks() : d_(new Impl) {}
ResampleBanks::~ResampleBanks() { clear(); delete d_; }

void ResampleBanks::clear() {
  std::lock_guard<std::mutex> lk(d_->mu);
  for (auto& kv : d_->banks) (void)hipFree(kv.second.dev);    // (waits for the kernels that read it)
  d_->banks.clear();
}

void ResampleBanks::set(const pf_resample_config* cfg) {
  const pf_resample_config c = resample_check(cfg);
  clear();
  std::lock_guard<std::mutex> lk(d_->mu);
  d_->cfg = c;
}

pf_resample_config ResampleBanks::config() {
  std::lock_guard<std::mutex> lk(d_->mu);
  return d_->cfg;
}

ResampleJob ResampleBanks::job(int sample_rate, int fs, int format, bool downmix, int64_t n_mono, int64_t n_out, int64_t in_off,
                               int64_t out_off, int sharers) {
  ResampleBankDev bk;
  {
    std::lock_guard<std::mutex> lk(d_->mu);
    auto it = d_->banks.find(sample_rate);
    if (it == d_->banks.end()) {
      const ResampleBank hb = resample_bank(sample_rate, fs, d_->cfg);
      ResampleBankDev nb{hb.L, hb.M, hb.H, hb.stride, nullptr};
      PF_HIP(hipMalloc((void**)&nb.dev, hb.h.size() * sizeof(float)));
      const hipError_t e = hipMemcpy(nb.dev, hb.h.data(), hb.h.size() * sizeof(float), hipMemcpyHostToDevice);
      if (e != hipSuccess) { (void)hipFree(nb.dev); PF_HIP(e); }
      it = d_->banks.emplace(sample_rate, nb).first;
    }
    bk = it->second;
  }
  ResampleJob j{};
  j.in_off = in_off; j.out_off = out_off; j.n_mono = n_mono; j.n_out = n_out; j.bank = bk.dev;
  j.L = bk.L; j.M = bk.M; j.H = bk.H; j.stride = bk.stride; j.format = format; j.downmix = downmix ? 1 : 0;
  const int64_t qM = bk.M / bk.L, rM = bk.M % bk.L, taps = 2 * bk.H;
  auto span = [&](int64_t tile) { return (tile - 1) * qM + (bk.L - 1 + (tile - 1) * rM) / bk.L + taps; };
  int tile = PF_RESAMPLE_TILE;
  while (tile > 1 && span(tile) > kResampleInCap) tile >>= 1;
  j.tile = tile; j.in_cap = (int)span(tile);
  j.bank_lds = ((size_t)j.in_cap + (size_t)bk.L * bk.stride) * sizeof(float) <= (size_t)kRsMaxLds ? 1 : 0;
  const int64_t ntiles = n_out > 0 ? (n_out + tile - 1) / tile : 0;
  // a workgroup that copies a bank into LDS should amortise it over many tiles: about one workgroup per CU over the launch
  const int64_t cap = j.bank_lds ? std::max(1, device_cu_count() / std::max(sharers, 1)) : 256;
  j.gx = (int)std::min(ntiles, cap);
  return j;
}

}  // namespace pf
