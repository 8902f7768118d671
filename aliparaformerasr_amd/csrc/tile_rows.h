// tile_rows.h — the device pieces the row-tile kernels share (k_vadnet.hip, k_punc.hip punc_rows_kernel).
//
// Rows are the concatenation of B members (utterances, windows) with row offsets off [B + 1]; a workgroup of four waves owns
// a tile of 64 consecutive rows, which may straddle members: every row looks up its own member (tr_row_info).
//
// A product is Y^T [N, 64] = W [N, K] X^T [K, 64] on v_mfma_f32_32x32x16_f16.  W is the A operand: fragments tiled once at
// attach time (tile_image.h TileGemm), streamed from L2 16 bytes per lane, the next fragment fetched one k-step ahead.  The
// activation tile X [64, K] f16 row-major in LDS (row stride ld halves) is the B operand, so a tile row is an output COLUMN:
// its result depends on that row of X and on W alone, in a fixed k order, whatever the other 63 rows hold.  A wave takes the
// 32-row blocks nt = wave, wave + 4, ... of W and both 32-row halves of the tile, half 0 before half 1 in every k-step; the
// accumulator starts as the bias.  Lane (r, h) then holds row 32 i + r of the tile and the 16 channels
// 32 nt + 8 q + 4 h + (0 .. 3), q = 0 .. 3.  Padded rows and columns of W are zeros, so padding never changes a sum.
//
// ld is a plain argument: k_punc.hip passes the constant 264, which the inlined code folds into its addresses; k_vadnet.hip
// passes the model's run-time stride.  Everything here is __forceinline__.
#pragma once
#include "kdev.h"
#include "tile_image.h"

namespace pf {

constexpr int TR_ROWS = 64;

// threads 0 .. 63: the member of tile row tid — the last b with off[b] <= row (members of no row share their offset with the
// next one and are stepped over, because the search looks for the LAST such b below B): its first row and its length.
// T = 0: no such row (at or beyond the total).  The caller synchronises before it reads start / T.
__device__ __forceinline__ void tr_row_info(const int64_t* off, int B, long long total, long long g0, int tid, long long* start, int* T) {
  if (tid < TR_ROWS) {
    const long long g = g0 + tid;
    long long s = 0;
    int t = 0;
    if (g < total) {
      int lo = 0, hi = B - 1;                            // off[0] = 0 <= g < off[B] = total
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid - 1;
      }
      s = off[lo];
      t = (int)(off[lo + 1] - s);
    }
    start[tid] = s;
    T[tid] = t;
  }
}

// the bias of the 32-row block nt of W into an accumulator.  tr_product below writes these four lines out in place instead of
// calling this: seeded through the call, the compiler builds both tile halves of vadnet_kernel as one 32-wide vector (82
// VGPRs for 66) and a forward measured 0.7 % longer; punc_rows_kernel's FFN seeds, which are no whole product, come here
__device__ __forceinline__ void tr_bias(const float* bias, int nt, int h, f16x& acc) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 b4 = *reinterpret_cast<const float4*>(bias + 32 * nt + 8 * q + 4 * h);
    acc[4 * q + 0] = b4.x; acc[4 * q + 1] = b4.y; acc[4 * q + 2] = b4.z; acc[4 * q + 3] = b4.w;
  }
}

// nks k-steps of one 32-row block of W (wp: the block's first fragment of the range, already offset by the lane) times the
// two 32-row halves of the tile (x0 / x1: the lane's row, already offset by the range's first column and the lane half)
__device__ __forceinline__ void tr_mma(const h8* wp, int nks, const half_t* x0, const half_t* x1, f16x& c0, f16x& c1) {
  h8 wn = wp[0];
  for (int ks = 0; ks < nks; ++ks) {
    const h8 wf = wn;
    if (ks + 1 < nks) wn = wp[(size_t)(ks + 1) * 64];
    const h8 b0 = *reinterpret_cast<const h8a*>(x0 + 16 * ks);
    const h8 b1 = *reinterpret_cast<const h8a*>(x1 + 16 * ks);
    c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, b0, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, b1, c1, 0, 0, 0);
  }
}

// X [64, g.Kpad] (LDS, row stride ld halves) times W^T over the whole K: epi(nt, i, acc) per 32-row block nt of W and tile half i
template <class Epi>
__device__ __forceinline__ void tr_product(const char* __restrict__ img, const TileGemm& g, const half_t* __restrict__ x, int ld, int wave,
                                           int lane, Epi&& epi) {
  const int r = lane & 31, h = lane >> 5, KS = g.Kpad >> 4;
  const h8* __restrict__ wt = reinterpret_cast<const h8*>(img + g.w_off);
  const float* __restrict__ bias = reinterpret_cast<const float*>(img + g.b_off);
  const half_t* x0 = x + r * ld + 8 * h;
  const half_t* x1 = x0 + 32 * ld;
  for (int nt = wave; nt < (g.Npad >> 5); nt += 4) {
    f16x acc[2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {                        // tr_bias in place: see there
      const float4 b4 = *reinterpret_cast<const float4*>(bias + 32 * nt + 8 * q + 4 * h);
      acc[0][4 * q + 0] = b4.x; acc[0][4 * q + 1] = b4.y; acc[0][4 * q + 2] = b4.z; acc[0][4 * q + 3] = b4.w;
    }
    acc[1] = acc[0];
    tr_mma(wt + ((size_t)nt * KS) * 64 + lane, KS, x0, x1, acc[0], acc[1]);
    epi(nt, 0, acc[0]);
    epi(nt, 1, acc[1]);
  }
}

// one accumulator (tile half i) into the f16 tile y at the columns of block nb, optional ReLU: x < 0 ? 0 : x, which keeps a NaN
__device__ __forceinline__ void tr_put_f16(const f16x& acc, bool relu, half_t* y, int ld, int i, int nb, int r, int h) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    h4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float f = acc[4 * q + e];
      if (relu) f = f < 0.f ? 0.f : f;
      v[e] = (half_t)f;
    }
    *reinterpret_cast<h4a*>(y + (32 * i + r) * ld + 32 * nb + 8 * q + 4 * h) = v;
  }
}

}  // namespace pf
