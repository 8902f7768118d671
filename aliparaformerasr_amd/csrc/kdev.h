// kdev.h — device-side primitives shared by the .hip files (included by them only): vector types, LDS-DMA, counted
// waits, the DPP wave sum and the result-store variants.  Everything is __forceinline__: a kernel's code does not
// depend on which file spells the helper.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace pf {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
typedef float f2v __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f16x __attribute__((ext_vector_type(16)));
// LDS scratch is written with one vector width and read back with another: these accesses must
// not be reordered by type-based alias analysis
typedef h8 __attribute__((may_alias)) h8a;
typedef h4 __attribute__((may_alias)) h4a;
typedef float4 __attribute__((may_alias)) float4a;

// LDS-DMA: 16 / 4 bytes per lane from global memory straight into LDS (lane i lands at l + i * size)
__device__ __forceinline__ void glds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}
__device__ __forceinline__ void glds4(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 4, 0, 0);
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  // gfx9 s_waitcnt simm16: vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt[5:4] << 14
  __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | ((N >> 4) << 14));
}
__device__ __forceinline__ void wait_lgkm0() { __builtin_amdgcn_s_waitcnt(0xC07F); }   // vmcnt 63, expcnt 7, lgkmcnt 0

// wave-wide sum, broadcast to every lane: four DPP steps give every lane its 16-lane row total (VALU only; a
// ds_bpermute-based butterfly is a chain of six LDS-crossbar round trips of ~120 cycles each, most of a small launch's
// run time), the four row totals are read through SGPRs
__device__ __forceinline__ float wave_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false));  // row_half_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false));  // row_mirror
  const float a = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
  const float b = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16));
  const float c = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32));
  const float d = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
  return (a + b) + (c + d);
}

// ---- the 64-bit-ballot window of the voice-activity walks (k_vad.hip, k_endpoint.hip): h[0 .. 3] hold one bit per frame for
// the 256 frames before a 64-frame chunk, h[4] the chunk's own ballot.  The set bits among positions [lo, hi] (inclusive; lo
// may be negative) of that 320-bit array.
__device__ __forceinline__ int vad_count_bits(const unsigned long long (&h)[5], int lo, int hi) {
  int c = 0;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int a = max(lo - 64 * j, 0), b = min(hi - 64 * j, 63);
    if (a <= b) {
      const unsigned long long m = (b == 63 ? ~0ull : ((1ull << (b + 1)) - 1ull)) & ~((1ull << a) - 1ull);
      c += __popcll(h[j] & m);
    }
  }
  return c;
}
// "the last event at or before the lane wins" (hysteresis): evm = the lanes with an event, onm = those whose event switches
// on, le = the mask of the lanes at or below this one, carry = the state in front of the chunk
__device__ __forceinline__ bool vad_last_event_state(unsigned long long evm, unsigned long long onm, unsigned long long le, bool carry) {
  const unsigned long long ev_le = evm & le;
  return ev_le ? ((onm >> (63 - __clzll((long long)ev_le))) & 1ull) != 0 : carry;
}

// ---- result stores.  The variants differ in cache policy and in what follows the store; each keeps its own name.

// gemm_f16_pp3's deferred f16 result stores (k_gemm.hip).  Cache policy: 0 plain, 1 nt, 2 sc1 (write-through, line
// dropped from the XCD's L2).  66 MB of results per launch otherwise churn the 8 x 4 MB L2s that hold the A panels and
// W tiles.  A/B in one session (tools/gemm_st.sh): plain 14.88-14.96 ms/step, nt 14.96-14.99 (the consumers then miss),
// sc1 14.81 (QKV -5 %, FFN-up -3 %, attention / FSMN / FFN-down unchanged).
#ifndef PF_GEMM_ST
#define PF_GEMM_ST 2
#endif
__device__ __forceinline__ void st16(void* p, h8 v) {
#if PF_GEMM_ST == 1
  asm volatile("global_store_dwordx4 %0, %1, off nt" ::"v"(p), "v"(v) : "memory");
#elif PF_GEMM_ST == 2
  asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
#else
  *reinterpret_cast<h8*>(p) = v;
#endif
}
__device__ __forceinline__ void st8(void* p, h4 v) {
#if PF_GEMM_ST == 1
  asm volatile("global_store_dwordx2 %0, %1, off nt" ::"v"(p), "v"(v) : "memory");
#elif PF_GEMM_ST == 2
  asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
#else
  *reinterpret_cast<h4*>(p) = v;
#endif
}
// the persistent kernels' blocked-layout stores (k_gemm_big.hip, k_gemm_qkv.hip): write-through and dropped from the
// XCD's L2 (sc1): 66 MB of results per launch would otherwise evict the W panel and the A panels the other tiles of
// this XCD are re-reading; the consumers run after the launch (store16_sc1 has no caller at present)
__device__ __forceinline__ void store16_sc1(void* p, h8 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void store8_sc1(void* p, h4 v) {
  asm volatile("global_store_dwordx2 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
// V pieces of the Q | K | V kernel: 16 bytes of a 64-byte row segment; write-back, so that the L2 merges the four
// pieces of a line
__device__ __forceinline__ void store16_wb(void* p, h8 v) {
  asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
// the LSTM recurrence's h exchange between workgroups (k_bicif.hip): write-through, read back with sc1 loads
// (L2-served, never a CU's stale L1)
__device__ __forceinline__ void st16_sc1(half_t* p, h8 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}

}  // namespace pf
