// k_gemm_panel.hip — panel-resident GEMM for K = 512 (the decoder's K | V projection of all layers, the vocabulary layer).
//
//   C[M,N] = A[M,512] * W[N,512]^T + bias     f16 operands, fp32 accumulate (v_mfma_f32_32x32x16_f16, D^T = W X^T)
//
// gemm_f16_pp3 (k_gemm.hip) walks 256 x 128 tiles; at K = 512 a tile is 8 k-steps, every tile restarts the LDS ring and
// reloads an A panel the previous tile of the same rows just had.  Here one 512-thread workgroup owns a
// PANEL of 128 consecutive A rows and a contiguous share of N:
//  * the panel [128 x 512] f16 (128 KiB) goes to LDS ONCE by LDS-DMA, in the swizzled k-block layout of k_ffn.hip's operand
//    tile (8 k-blocks of [128 rows][128 B], 16-byte chunks XOR-swizzled by row: conflict-free ds_read_b128 fragments);
//    rows at or beyond M re-read row M - 1 (nothing behind the operand is read);
//  * the weights come straight from a fragment-ordered image (launch_gemm_panel_retile, built once at load) into a register
//    ring, 1 KiB per wave per fragment, SGPR base + the lane's 32-bit offset; the ring never restarts: while a wave finishes
//    one 64-column block it already loads the fragments of its next one;
//  * wave (rh, cg) = (wave >> 2, wave & 3) multiplies rows 64 rh .. 64 rh + 63 of the panel with the 64-column blocks
//    cg, cg + 4, .. of the share (2 x 2 MFMAs per k-step of 16, the shape of k_ffn.hip's P1), each accumulator over k
//    ascending — the order of gemm_f16_pp3, so the results are bit-identical to that kernel's;
//  * a finished block is packed (f16 results: cvt_pk, 32 registers) or copied (fp32 results) and leaves through a per-wave
//    LDS scratch as whole row segments, one piece every few k-steps of the NEXT block (gfx950 retires stores through vmcnt in
//    order with the loads: a burst of stores in front of the ring's waits would stall the weight stream);
//  * one barrier (after the panel has landed), none in the steady state; nothing is shared between workgroups.
// Rounding points are those of gemm_f16_pp3: f16 results into a padded buffer start the accumulators as the bias (kind 1);
// every other case adds the bias to the finished sum (kind 2 and the edge tiles of kind 1).
#include "kernels.h"
#include "kdev.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace pf {

struct PanelDev {
  const half_t* A; const half_t* Wp; const float* bias;
  float* out_f32; half_t* out_f16;
  int lda, ldc32, ldc16;
  int M, N, nblk, S;           // nblk = cdiv(N, 64) column blocks, S shares of them per panel
  int bias_first;              // f16 results: whole blocks start their accumulators as the bias
  int al16;                    // f16 results: every row of the result is 16-byte aligned
};

constexpr int GP_ROWS = 128, GP_PANEL = GP_ROWS * 512 * 2, GP_KB = GP_ROWS * 128, GP_SCR = 2048;
constexpr int GP_LDS = GP_PANEL + 8 * GP_SCR;                  // 144 KiB
constexpr int GP_BLK_BYTES = 64 * 512 * 2;                     // one 64-column block of the weight image
constexpr int GP_LINE = 1152;                                  // the two bias lines inside a wave's scratch

// result stores: ST 0 = plain, 2 = sc1 (write-through, the line is dropped from the XCD's L2)
template <int ST>
__device__ __forceinline__ void gp_st16(void* p, h8 v) {
  if constexpr (ST == 2) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
  else *reinterpret_cast<h8*>(p) = v;
}
template <int ST>
__device__ __forceinline__ void gp_st16(void* p, float4 v) {
  if constexpr (ST == 2) {
    const f4v x = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(x) : "memory");
  } else *reinterpret_cast<float4*>(p) = v;
}

// KIND 1: f16 result, KIND 2: fp32 result.  PF: weight fragments in flight per wave (divides 64).  XD: k-steps the LDS fragment
// reads run ahead of their MFMAs (XD + 1 divides 32).  ST: cache policy of the result stores.
template <int KIND, int PF, int XD, int ST>
__global__ __launch_bounds__(512, 1) void gemm_panel_kernel(PanelDev p) {
  static_assert(64 % PF == 0 && 32 % (XD + 1) == 0, "the rings run on across blocks");
  constexpr int XR = XD + 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lh = lane >> 5, l31 = lane & 31;
  const int rh = wave >> 2, cg = wave & 3;
  const int bid = blockIdx.x;
  const int panel = bid / p.S, share = bid - panel * p.S;
  const int m0 = panel * GP_ROWS;
  const int b0 = (int)((long long)share * p.nblk / p.S), nb = (int)((long long)(share + 1) * p.nblk / p.S) - b0;
  // workgroups of one XCD walk the same weights: they start at rotated positions of the share (lockstep cold misses)
  const int rot = (((bid >> 3) & 3) * nb) >> 2;
  const int steps = nb > cg ? (nb - cg + 3) >> 2 : 0;
  auto blk_of = [&](int st) __attribute__((always_inline)) -> int {
    const int q = cg + 4 * st + rot;
    return b0 + (q >= nb ? q - nb : q);
  };
  auto swz = [](int row) __attribute__((always_inline)) -> int { return (row >> 1) & 7; };

  // ---- weight stream (uniform base in SGPRs + the lane's 32-bit byte offset)
  const unsigned lane16 = (unsigned)lane * 16u;
  auto wbase = [&](int blk) __attribute__((always_inline)) -> const char* {
    return reinterpret_cast<const char*>(p.Wp) + (size_t)blk * GP_BLK_BYTES;
  };
  auto wld = [&](const char* base, int pos) __attribute__((always_inline)) -> h8 {
    return *reinterpret_cast<const h8*>(base + pos * 1024 + lane16);
  };
  auto bias_ld = [&](int blk) __attribute__((always_inline)) -> float {
    int n = blk * 64 + lane;
    n = n < p.N ? n : p.N - 1;
    return p.bias ? p.bias[n] : 0.f;
  };
  char* const scr = smem + GP_PANEL + wave * GP_SCR;
  const char* cur = wbase(steps ? blk_of(0) : b0);
  h8 ring[PF];
  float bnx = 0.f;
  if (steps) {                                       // primed before the panel is waited for
#pragma unroll
    for (int i = 0; i < PF; ++i) ring[i] = wld(cur, i);
    bnx = bias_ld(blk_of(0));
  }

  // ---- the panel -> LDS: wave w brings rows 16 w .. 16 w + 15 of every k-block (1 KiB = 8 rows per piece)
  {
    const int srow = lane >> 3, schunk = lane & 7;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = (wave * 2 + h) * 8 + srow;
      int m = m0 + row;
      m = m < p.M ? m : p.M - 1;
      const char* src = reinterpret_cast<const char*>(p.A + (size_t)m * p.lda) + ((schunk ^ swz(row)) << 4);
#pragma unroll
      for (int kb = 0; kb < 8; ++kb) glds16(src + kb * 128, smem + kb * GP_KB + (wave * 2 + h) * 1024);
    }
  }
  wait_vmcnt<0>();                                   // (the builtin: the compiler's own wait counting then knows the panel has landed)
  reinterpret_cast<float*>(scr + GP_LINE)[lane] = bnx;            // bias line of the first block
  wait_lgkm0();
  __builtin_amdgcn_s_barrier();
  if (steps == 0) return;

  // fragment read offsets of the panel: row half i, 16-byte k-group (2 ss + lh) of a k-block
  unsigned xo[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int ss = 0; ss < 4; ++ss) {
      const int ra = rh * 64 + i * 32 + l31;
      xo[i][ss] = (unsigned)(ra * 128 + (((2 * ss + lh) ^ swz(ra)) << 4));
    }
  auto xld = [&](int s, int i) __attribute__((always_inline)) -> h8 {
    return *reinterpret_cast<const h8*>(smem + (s >> 2) * GP_KB + xo[i][s & 3]);
  };
  h8 xf[XR][2];
#pragma unroll
  for (int s0 = 0; s0 < XD; ++s0)
#pragma unroll
    for (int i = 0; i < 2; ++i) xf[s0][i] = xld(s0, i);

  f16x acc[2][2];
  const int mrow = m0 + rh * 64;                     // first row of this wave's blocks
  // ---- the finished block awaiting its stores
  int pn0 = 0;
  h4 hq[2][2][4];                                    // KIND 1: packed f16
  f16x pq[2][2];                                     // KIND 2: the fp32 sums
  const float* pl = reinterpret_cast<const float*>(scr + GP_LINE);   // KIND 2: its bias line (rewritten only behind the last chunk)

  // KIND 1: pass idx = rows 8 idx .. 8 idx + 7 of the wave's 64: the 16 owner lanes write them to the scratch, every lane reads
  // one 16-byte piece of a row back and stores it (whole 128-byte lines)
  char* const wp16 = scr + (lane & 7) * 144 + lh * 8;
  const char* const rp16 = scr + (lane >> 3) * 144 + (lane & 7) * 16;
  h8 rowv;
  auto pass_write = [&](auto IC, int q) __attribute__((always_inline)) {
    constexpr int i = decltype(IC)::value;
    if ((l31 >> 3) == q) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) *reinterpret_cast<h4a*>(wp16 + (j * 32 + 8 * g) * 2) = hq[i][j][g];
    }
  };
  // (the scratch and the bias lines carry values from lane to lane: the compiler, which reasons per lane, must not keep an
  //  earlier read of an address this lane has not written itself — hence the barriers around every such read)
  auto pass_read = [&]() __attribute__((always_inline)) {
    asm volatile("" ::: "memory");
    rowv = *reinterpret_cast<const h8a*>(rp16);
    asm volatile("" ::: "memory");
  };
  auto pass_store = [&](int idx) __attribute__((always_inline)) {
    const int m = mrow + idx * 8 + (lane >> 3), n = pn0 + (lane & 7) * 8;
    if (m >= p.M) return;
    half_t* o = p.out_f16 + (size_t)m * p.ldc16 + n;
    if (p.al16 && n + 8 <= p.N) gp_st16<ST>(o, rowv);
    else if (n + 8 <= p.N) {
      *reinterpret_cast<h4*>(o) = h4{rowv[0], rowv[1], rowv[2], rowv[3]};
      *reinterpret_cast<h4*>(o + 4) = h4{rowv[4], rowv[5], rowv[6], rowv[7]};
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (n + e < p.N) o[e] = rowv[e];
    }
  };
  // KIND 2: chunk c = rows 4 c .. 4 c + 3 of the wave's 64: 8 owner lanes write them, 16 lanes x 16 B read one row segment back
  char* const wp32 = scr + (l31 & 3) * 272 + lh * 16;
  const char* const rp32 = scr + (lane >> 4) * 272 + (lane & 15) * 16;
  float4 segv;
  auto chunk_write = [&](auto IC, int c8) __attribute__((always_inline)) {
    constexpr int i = decltype(IC)::value;
    if ((l31 >> 2) == c8) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<float4a*>(wp32 + (j * 32 + 8 * g) * 4) =
              make_float4(pq[i][j][4 * g + 0], pq[i][j][4 * g + 1], pq[i][j][4 * g + 2], pq[i][j][4 * g + 3]);
    }
  };
  auto chunk_read = [&]() __attribute__((always_inline)) {
    asm volatile("" ::: "memory");
    segv = *reinterpret_cast<const float4a*>(rp32);
    asm volatile("" ::: "memory");
  };
  auto chunk_store = [&](int c) __attribute__((always_inline)) {
    const int m = mrow + c * 4 + (lane >> 4), n = pn0 + (lane & 15) * 4;
    if (m >= p.M) return;
    float4 v = segv;
    const float4 pb4 = *reinterpret_cast<const float4a*>(pl + (lane & 15) * 4);
    v.x = fmaxf(v.x + pb4.x, -INFINITY); v.y = fmaxf(v.y + pb4.y, -INFINITY);
    v.z = fmaxf(v.z + pb4.z, -INFINITY); v.w = fmaxf(v.w + pb4.w, -INFINITY);
    float* o = p.out_f32 + (size_t)m * p.ldc32 + n;
    if (n + 4 <= p.N) gp_st16<ST>(o, v);
    else {
      if (n < p.N) o[0] = v.x;
      if (n + 1 < p.N) o[1] = v.y;
      if (n + 2 < p.N) o[2] = v.z;
    }
  };
  // the part of the pending block's stores that rides on k-step s of the following block
  auto drain = [&](int s) __attribute__((always_inline)) {
    if constexpr (KIND == 1) {
      const int idx = s >> 2;                        // 8 passes, one per 4 k-steps
      if ((s & 3) == 0) { if (idx < 4) pass_write(std::integral_constant<int, 0>{}, idx & 3); else pass_write(std::integral_constant<int, 1>{}, idx & 3); }
      if ((s & 3) == 1) pass_read();
      if ((s & 3) == 2) pass_store(idx);
    } else {
      const int c = s >> 1;                          // 16 chunks, one per 2 k-steps
      if ((s & 1) == 0) { if (c < 8) chunk_write(std::integral_constant<int, 0>{}, c & 7); else chunk_write(std::integral_constant<int, 1>{}, c & 7); }
      else { chunk_read(); chunk_store(c); }
    }
  };

  for (int st = 0; st < steps; ++st) {
    const int blk = blk_of(st);
    const bool last = st + 1 == steps;
    const int blk_n = last ? blk : blk_of(st + 1);
    const char* nxt = wbase(blk_n);
    const int n0 = blk * 64;
    const bool bf = KIND == 1 && p.bias_first && n0 + 64 <= p.N;
    const float* bl = reinterpret_cast<const float*>(scr + GP_LINE + (st & 1) * 256);
    asm volatile("" ::: "memory");
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bf) b4 = *reinterpret_cast<const float4a*>(bl + j * 32 + 8 * g + 4 * lh);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          acc[i][j][4 * g + 0] = b4.x; acc[i][j][4 * g + 1] = b4.y; acc[i][j][4 * g + 2] = b4.z; acc[i][j][4 * g + 3] = b4.w;
        }
      }
    bnx = bias_ld(blk_n);                            // consumed 31 k-steps from here: its wait never drains the ring
#pragma unroll
    for (int s = 0; s < 32; ++s) {
#pragma unroll
      for (int i = 0; i < 2; ++i) xf[(s + XD) % XR][i] = xld((s + XD) & 31, i);      // (runs on into the next block: same panel)
      h8 wf[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int pos = 2 * s + j;
        wf[j] = ring[pos % PF];
        ring[pos % PF] = pos + PF < 64 ? wld(cur, pos + PF) : wld(nxt, pos + PF - 64);
      }
      if (st > 0) drain(s);
      if (s == 31) {                                 // (behind the pending block's last chunk, which still reads this line)
        reinterpret_cast<float*>(scr + GP_LINE + ((st + 1) & 1) * 256)[lane] = bnx;
        asm volatile("" ::: "memory");
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[j], xf[s % XR][i], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- block end: the sums leave the accumulators
    asm volatile("" ::: "memory");
    if constexpr (KIND == 1) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
          if (!bf) b4 = *reinterpret_cast<const float4a*>(bl + j * 32 + 8 * g + 4 * lh);
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            float v0 = acc[i][j][4 * g + 0], v1 = acc[i][j][4 * g + 1], v2 = acc[i][j][4 * g + 2], v3 = acc[i][j][4 * g + 3];
            if (!bf) { v0 += b4.x; v1 += b4.y; v2 += b4.z; v3 += b4.w; }
            hq[i][j][g] = h4{(half_t)fmaxf(v0, -INFINITY), (half_t)fmaxf(v1, -INFINITY), (half_t)fmaxf(v2, -INFINITY),
                             (half_t)fmaxf(v3, -INFINITY)};
          }
        }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) pq[i][j] = acc[i][j];
      pl = bl;
    }
    pn0 = n0;
    cur = nxt;
  }
  // ---- the last block's stores
#pragma unroll
  for (int s = 0; s < 32; ++s) drain(s);
}

// W [N, ldw] (f16, K-contiguous, 512 columns) -> the fragment-ordered image the kernel streams (k_ffn.hip's out-projection
// image with the 64-row group index running over N):
//   img[((b * 32 + t) * 2 + j) * 512 + l * 8 + e] = W[b * 64 + j * 32 + (l & 31)][16 t + 8 (l >> 5) + e],  rows >= N: zeros
// one thread per 16-byte piece
__global__ void gemm_panel_retile_kernel(const half_t* __restrict__ W, int ldw, int N, int nblk, half_t* __restrict__ img) {
  const int64_t pc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pc >= (int64_t)nblk * 4096) return;
  const int l = (int)(pc & 63), j = (int)(pc >> 6) & 1, t = (int)(pc >> 7) & 31, b = (int)(pc >> 12);
  const int row = b * 64 + j * 32 + (l & 31);
  h8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (_Float16)0.f;
  if (row < N) {
    const half_t* src = W + (size_t)row * ldw + 16 * t + 8 * (l >> 5);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = src[e];
  }
  *reinterpret_cast<h8*>(img + (size_t)pc * 8) = v;
}

size_t gemm_panel_image_bytes(int N) { return (size_t)cdiv(N, 64) * GP_BLK_BYTES; }
void launch_gemm_panel_retile(hipStream_t s, const half_t* W, int ldw, int N, half_t* img) {
  const int nblk = cdiv(N, 64);
  if (nblk == 0) return;
  hipLaunchKernelGGL(gemm_panel_retile_kernel, dim3(nblk * 16), dim3(256), 0, s, W, ldw, N, nblk, img);
  PF_HIP(hipGetLastError());
}

// rows above which launch_gemm prefers this form where it applies (PF_PANEL_M overrides).  Below the short-input threshold
// k_gemm_small.hip keeps the problem; between it and the decoder's M = 5344 the form was measured at the small test
// configuration only.
int gemm_panel_min_rows() {
  static const int v = [] { const char* e = getenv("PF_PANEL_M"); return e && e[0] ? atoi(e) : 512; }();
  return v;
}

bool gemm_panel_applicable(const GemmArgs& a) {
  return a.K == 512 && a.W_panel && a.M > 0 && a.N > 0 && ((a.out_f16 != nullptr) != (a.out_f32 != nullptr)) && !a.resid && !a.add2 &&
         !a.relu && a.scale_cols == 0 && !a.out_blocked && !a.a_blocked && a.f16_lo_off == 0 && a.k_wrap == 0 && a.lda % 8 == 0 &&
         (a.out_f16 ? a.ldc16 % 4 == 0 : a.ldc32 % 4 == 0);
}

// shares of N per panel: the smallest S whose panels * S workgroups cover 0.9 of the CUs (one round, no second), no share
// below 512 columns.  PF_PANEL_S overrides (tools/: the rule's alternatives).
int gemm_panel_shares(int panels, int N, int cus) {
  static const int forced = [] { const char* e = getenv("PF_PANEL_S"); return e && e[0] ? atoi(e) : 0; }();
  const int cap = std::max(1, N / 512);
  if (forced > 0) return std::min(forced, std::max(1, cdiv(N, 64)));
  int S = 1;
  while (S < cap && (double)panels * S < 0.9 * cus) ++S;
  return S;
}

void launch_gemm_panel(hipStream_t s, const GemmArgs& a, int cus) {
  PF_CHECK(gemm_panel_applicable(a), PF_ERR_INVALID_ARG, "gemm: the panel-resident kernel does not apply to this problem");
  PanelDev d{};
  d.A = a.A; d.Wp = a.W_panel; d.bias = a.bias; d.out_f32 = a.out_f32; d.out_f16 = a.out_f16;
  d.lda = a.lda; d.ldc32 = a.ldc32; d.ldc16 = a.ldc16;
  d.M = a.M; d.N = a.N; d.nblk = cdiv(a.N, 64);
  const int panels = cdiv(a.M, GP_ROWS);
  d.S = gemm_panel_shares(panels, a.N, cus);
  // the rounding of gemm_f16_pp3 for the same arguments: its kind 1 (bias first) takes f16-only results into padded rows
  d.bias_first = a.out_f16 && a.out_padded && (a.ldc16 & 7) == 0;
  d.al16 = a.out_f16 && (a.ldc16 & 7) == 0 && (reinterpret_cast<uintptr_t>(a.out_f16) & 15) == 0;
  // result stores: f16 sc1, fp32 plain (measured both ways: DESIGN.md §4.1l)
  static const int st = [] { const char* e = getenv("PF_PANEL_ST"); return e && e[0] ? atoi(e) : -1; }();
  static DeviceOnce once;
  once.run([] {
    set_max_lds((const void*)gemm_panel_kernel<1, 16, 1, 2>, GP_LDS);
    set_max_lds((const void*)gemm_panel_kernel<1, 16, 1, 0>, GP_LDS);
    set_max_lds((const void*)gemm_panel_kernel<2, 8, 1, 2>, GP_LDS);
    set_max_lds((const void*)gemm_panel_kernel<2, 8, 1, 0>, GP_LDS);
  });
  const dim3 grid(panels * d.S), block(512);
  if (a.out_f16) {
    const bool sc1 = st < 0 ? true : st == 2;
    note_gemm_kernel(sc1 ? "gemm_panel_kernel<1, 16, 1, 2>" : "gemm_panel_kernel<1, 16, 1, 0>");
    if (sc1) hipLaunchKernelGGL((gemm_panel_kernel<1, 16, 1, 2>), grid, block, GP_LDS, s, d);
    else hipLaunchKernelGGL((gemm_panel_kernel<1, 16, 1, 0>), grid, block, GP_LDS, s, d);
  } else {
    const bool sc1 = st < 0 ? false : st == 2;
    note_gemm_kernel(sc1 ? "gemm_panel_kernel<2, 8, 1, 2>" : "gemm_panel_kernel<2, 8, 1, 0>");
    if (sc1) hipLaunchKernelGGL((gemm_panel_kernel<2, 8, 1, 2>), grid, block, GP_LDS, s, d);
    else hipLaunchKernelGGL((gemm_panel_kernel<2, 8, 1, 0>), grid, block, GP_LDS, s, d);
  }
  PF_HIP(hipGetLastError());
}

}  // namespace pf
