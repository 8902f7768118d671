// k_frontend_stream.hip — the streaming front-end behind the fbank on the device: ONE launch takes the fbank rows
// of the 9600-sample chunks of B streams (launch_fbank's, made by the launch in front of this one on the same stream) to the
// encoder's input [B, 20, 560] and updates each stream's block (decode_blocks.h FrontendStreamBlock).  The host statement is
// online_frontend_step (online.cpp).  Compiled with -ffp-contract=off; every product and sum the host rounds separately goes
// through exact.h.
//
// Split.  Grid (10, B), 256 threads: workgroup (i, b) owns LFR frame i of stream b, i.e. rows pad[6 i .. 6 i + 6] of the 61-row
// splice pad = [carry0 ; carry1 ; fb[0 .. 58]] — the chunk's fbank rows fb[6 i - 2 .. 6 i + 4], read straight from the rows
// (seven consecutive rows are one run of 560 floats, so a thread's column j is one coalesced load).  Per column: CMVN (two
// roundings), the sqrt(512) scale through a double, the position term with fp64 sin / cos of the float argument, into speech row
// 10 + i (sentinel applied) and cache row i.  The thread that writes cache cell (i, j) has read the OLD cell (i, j) just before
// and sent it to speech row i: the ten cached rows move to the front of the chunk without a second copy, and no workgroup touches
// another's cache row or start_idx copy.
//
// The carried rows.  Only workgroup 0 needs pad[0] and pad[1], and only workgroup 0 touches the block's carry and flags: thread j
// < 160 reads carry cell j, then writes fb[58 .. 59] cell j over it — read-before-write in the program order of one thread, so
// the carry needs no second copy and no ordering between workgroups.  The old cells go through LDS to the threads that need them
// (one barrier, in workgroup 0 alone).  On a stream's first step (flags bit 0 clear) both carried rows are fb[0].
#include "exact.h"
#include "kdev.h"
#include "kernels.h"
#include "decode_blocks.h"

#include <cmath>

namespace pf {

namespace {
constexpr int kThreads = 256, kMels = 80, kW = 560, kRows = 60, kLfrN = 6;

struct FeDev {
  OnlineFrontendLaunch a;
  int64_t off_carry, off_cache, off_start, off_flags;      // FrontendStreamBlock, bytes
};
}  // namespace

__global__ __launch_bounds__(kThreads) void online_frontend_kernel(FeDev p) {
  __shared__ float carry_s[2 * kMels];
  const OnlineFrontendLaunch& a = p.a;
  const int tid = threadIdx.x, i = blockIdx.x, b = blockIdx.y;
  const int slot = a.slot ? a.slot[b] : b;
  char* blk = a.states + (int64_t)slot * a.state_stride;
  float* s_cache = (float*)(blk + p.off_cache) + (int64_t)i * kW;
  int32_t* s_start = (int32_t*)(blk + p.off_start) + i;
  const float* fb = a.fbank + (int64_t)b * kRows * kMels;
  const bool fresh = a.reset && a.reset[b] != 0;
  const int start_idx = fresh ? 0 : *s_start;
  if (i == 0) {                                            // (uniform over the workgroup)
    float* s_carry = (float*)(blk + p.off_carry);
    int32_t* s_flags = (int32_t*)(blk + p.off_flags);
    const int flags = s_flags[0];
    if (tid < 2 * kMels) {
      const float old = (flags & 1) ? s_carry[tid] : fb[tid % kMels];
      s_carry[tid] = fb[(kRows - 2) * kMels + tid];
      carry_s[tid] = old;
    }
    __syncthreads();
    if (tid == 0) s_flags[0] = flags | 1;
  }
  const float S = -23.025850929940457f;
  const float pos = (float)(start_idx + i + 1);
  float* sp_old = a.speech + ((int64_t)b * 20 + i) * kW;
  float* sp_new = a.speech + ((int64_t)b * 20 + 10 + i) * kW;
  for (int j = tid; j < kW; j += kThreads) {
    const int r = kLfrN * i * kMels + j - 2 * kMels;       // cell of fb; < 0: a carried row (workgroup 0, j < 160)
    float v = r < 0 ? carry_s[j] : fb[r];
    if (a.shift) v = mul_rn(add_rn(v, a.shift[j]), a.scale[j]);
    v = (float)((double)v * a.root);
    const int k = j < kW / 2 ? j : j - kW / 2;
    const double arg = (double)mul_rn(a.inv[k], pos);
    v = add_rn(v, j < kW / 2 ? (float)sin(arg) : (float)cos(arg));
    const float old = fresh ? 0.f : s_cache[j];
    s_cache[j] = v;
    sp_old[j] = old == 0.f ? S : old;
    sp_new[j] = v == 0.f ? S : v;
  }
  if (tid == 0) *s_start = start_idx + 10;
}

void launch_online_frontend(hipStream_t s, const OnlineFrontendLaunch& a) {
  PF_CHECK(a.fbank && a.states && a.inv && a.speech && a.B > 0, PF_ERR_INVALID_ARG, "online_frontend: bad arguments");
  PF_CHECK((a.shift == nullptr) == (a.scale == nullptr), PF_ERR_INVALID_ARG, "online_frontend: shift and scale come together");
  const FrontendStreamBlock blk = block_at_zero<FrontendStreamBlock>(kMels, kW);
  PF_CHECK(a.state_stride >= (int64_t)blk.bytes() && a.state_stride % 16 == 0, PF_ERR_INVALID_ARG,
           "online_frontend: the state stride does not hold a block");
  FeDev p;
  p.a = a;
  p.off_carry = (int64_t)blk.carry.off; p.off_cache = (int64_t)blk.cache.off; p.off_start = (int64_t)blk.start_idx.off;
  p.off_flags = (int64_t)blk.flags.off;
  hipLaunchKernelGGL(online_frontend_kernel, dim3((unsigned)kFrontendStreamFrames, (unsigned)a.B), dim3(kThreads), 0, s, p);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
