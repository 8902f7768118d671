// k_spk.hip — the CAM++ speaker embedding on the device (paraformer_hip.h "Speaker labels").  The definition
// in numpy float64 is tests/spk_ref.py.
//
// B windows of T[w] fbank rows each.  No tile straddles two windows: the grid's y (or x) is the window, so a window's bits
// depend on its own rows and on the weights alone.  15 launches per forward, whatever B and T:
//   10  spk_conv_kernel   one per head convolution: an implicit GEMM over the output positions (f, t) of a window, 64 positions
//                         per one-wave workgroup, K = 9 cin gathered into an LDS tile [64, Kpad + 8]; the 1x1 shortcut of a
//                         residual block is cin more columns of its second convolution's K; an identity shortcut is added to the
//                         accumulator.  The first launch subtracts the window's column means, which it sums itself in a fixed
//                         order.  The 3x3 halo is covered by the launch boundaries.  Activations are f16 in global memory,
//                         channels last; the last convolution writes the TDNN's frames [t][c F/8 + f].
//    1  spk_tdnn_kernel   64 output frames per workgroup: the 131 input frames they reach in LDS once, five shifted products
//    3  spk_block_kernel  ONE WORKGROUP PER WINDOW walks a dense block's layers and the transit behind it: the concatenated X
//                         lives in global memory (L2), each layer appends `growth` channels; the bottleneck tile [T', bn + 8]
//                         stays in LDS with `dilation` zero rows on either side; its column and segment means are summed by
//                         one thread per column in frame order; the two mask products, the three shifted taps and the mask
//                         multiply run on it.  Only __syncthreads orders the layers: no grid barrier, nothing persistent.
//                         A single window therefore uses one CU; the workload is thousands of windows.
//    1  spk_pool_kernel   one workgroup per window: ReLU(BN), mean and unbiased standard deviation per channel in frame order,
//                         the embedding product on the statistics (all 64 tile rows alias the one vector: row stride 0)
// and one launch of spk_affinity_kernel for the cosines of a call's streams (fp32, one thread per pair, k ascending).
//
// Every product is tile_rows.h's: W fragments from the image as the A operand, an f16 LDS tile as the B operand, fp32
// accumulation in ascending k.  Padded rows and columns of W are zeros and every padded column of a tile is WRITTEN as zero
// (0 * NaN is NaN), so padding never changes a sum.  Rounding points: R0 .. R10 of tests/spk_ref.py; everything else is fp32.
// ReLU is x < 0 ? 0 : x, which keeps a NaN.  Nothing at or beyond a window's T is read.
#include "kdev.h"
#include "kernels.h"
#include "tile_rows.h"

namespace pf {

namespace {

constexpr int SB_ROWS = PF_SPK_MAX_FRAMES / 2;     // the most frames behind the TDNN
constexpr int SB_PAD = kSpkMaxDilation;            // zero rows on either side of the bottleneck tile
constexpr int SB_CHUNK = 256;                      // columns of X staged per step of a rows product
constexpr int SB_LDS = SB_CHUNK + 8;
constexpr int SPK_MAX_LDS = 150 * 1024;

__device__ __forceinline__ void zero_acc(f16x& a) {
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = 0.f;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- the head's convolutions
__global__ __launch_bounds__(64) void spk_conv_kernel(SpkConvLaunch a) {
  extern __shared__ __attribute__((aligned(16))) char spk_lds[];
  __shared__ float mean[kSpkMaxMels];
  half_t* xt = reinterpret_cast<half_t*>(spk_lds);
  const int w = blockIdx.y, lane = threadIdx.x;
  const int T = a.w.T[w];
  const long long P = (long long)a.Fout * T, p0 = (long long)blockIdx.x * 64;
  if (p0 >= P) return;
  const int K = a.d.g.K, Kpad = a.d.g.Kpad, ld = Kpad + 8, m = a.m;
  const long long row0 = a.w.toff[w];
  if (a.d.cin == 1) {
    // conv1 on x - mean_t x (R1): the means of the columns this tile touches, summed over t ascending
    const long long x0r = a.w.xoff[w];
    const int f_lo = (int)(p0 / T), f_hi = (int)((p0 + 63 < P ? p0 + 63 : P - 1) / T);
    const int c_lo = f_lo > 0 ? f_lo - 1 : 0, c_hi = f_hi + 1 < a.Fin ? f_hi + 1 : a.Fin - 1;
    for (int c = c_lo + lane; c <= c_hi; c += 64) {
      float s = 0.f;
      for (int t = 0; t < T; ++t) s += a.x[(x0r + t) * a.n_mels + c];
      mean[c] = s / (float)T;
    }
    __syncthreads();
    for (int idx = lane; idx < 64 * 16; idx += 64) {
      const int row = idx >> 4, k = idx & 15;
      const long long p = p0 + row;
      float v = 0.f;
      if (p < P && k < 9) {
        const int f = (int)(p / T), t = (int)(p - (long long)f * T);
        const int fi = f + k / 3 - 1, ti = t + k % 3 - 1;
        if (fi >= 0 && fi < a.Fin && ti >= 0 && ti < T) v = a.x[(x0r + ti) * a.n_mels + fi] - mean[fi];
      }
      xt[row * ld + k] = (half_t)v;
    }
  } else {
    const int cin = a.d.cin, cpr = Kpad >> 3;
    for (int idx = lane; idx < 64 * cpr; idx += 64) {
      const int row = idx / cpr, k0 = (idx - row * cpr) << 3;
      const long long p = p0 + row;
      h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (p < P && k0 < K) {
        const int f = (int)(p / T), t = (int)(p - (long long)f * T);
        const int tap = k0 / cin, c = k0 - tap * cin;
        if (tap < 9) {
          const int fi = f * a.d.sf + tap / 3 - 1, ti = t + tap % 3 - 1;
          if (fi >= 0 && fi < a.Fin && ti >= 0 && ti < T)
            v = *reinterpret_cast<const h8a*>(a.in + ((row0 * a.Fin + (long long)fi * T + ti) * m + c));
        } else {                                           // the 1x1 shortcut over the block's input, stride 2 in frequency
          v = *reinterpret_cast<const h8a*>(a.aux + ((row0 * (2 * a.Fout) + (long long)(2 * f) * T + t) * m + c));
        }
      }
      *reinterpret_cast<h8a*>(xt + row * ld + k0) = v;
    }
  }
  __syncthreads();

  const int r = lane & 31, h = lane >> 5, KS = Kpad >> 4;
  const h8* __restrict__ wt = reinterpret_cast<const h8*>(a.w.img + a.d.g.w_off);
  const float* __restrict__ bias = reinterpret_cast<const float*>(a.w.img + a.d.g.b_off);
  const half_t* x0 = xt + r * ld + 8 * h;
  const half_t* x1 = x0 + 32 * ld;
  for (int nt = 0; nt < (a.d.g.Npad >> 5); ++nt) {
    f16x acc[2];
    tr_bias(bias, nt, h, acc[0]);
    acc[1] = acc[0];
    tr_mma(wt + ((size_t)nt * KS) * 64 + lane, KS, x0, x1, acc[0], acc[1]);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long long p = p0 + 32 * i + r;
      if (p >= P) continue;
      const int f = (int)(p / T), t = (int)(p - (long long)f * T);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ch = 32 * nt + 8 * q + 4 * h;
        if (ch >= m) continue;
        float v[4] = {acc[i][4 * q + 0], acc[i][4 * q + 1], acc[i][4 * q + 2], acc[i][4 * q + 3]};
        if (a.d.residual) {
          const h4 rs = *reinterpret_cast<const h4a*>(a.aux + ((row0 * a.Fout + p) * m + ch));
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += (float)rs[e];
        }
        h4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (half_t)(v[e] < 0.f ? 0.f : v[e]);                     // R2
        if (!a.d.to_frames) {
          *reinterpret_cast<h4a*>(a.out + ((row0 * a.Fout + p) * m + ch)) = o;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) a.out[(row0 + t) * a.frame_ld + (long long)(ch + e) * a.Fout + f] = o[e];
        }
      }
    }
  }
}

void launch_spk_conv(hipStream_t s, const SpkConvLaunch& a) {
  if (a.w.B <= 0 || a.w.Tmax <= 0) return;
  const size_t lds = (size_t)64 * (a.d.g.Kpad + 8) * sizeof(half_t);
  PF_CHECK(a.w.img && a.w.T && a.w.toff && a.out && (a.d.cin == 1 ? (a.x != nullptr && a.w.xoff != nullptr) : a.in != nullptr) &&
               (!(a.d.shortcut || a.d.residual) || a.aux != nullptr) && a.m % 8 == 0 && a.m <= kSpkMaxM && a.n_mels <= kSpkMaxMels &&
               (a.d.cin == 1 || a.d.cin == a.m) && a.d.g.Npad <= 64 && a.d.g.K == (a.d.cin == 1 ? 9 : (9 + a.d.shortcut) * a.d.cin) &&
               a.Fout >= 1 && a.Fin == a.Fout * a.d.sf && lds <= (size_t)SPK_MAX_LDS && a.w.Tmax <= PF_SPK_MAX_FRAMES,
           PF_ERR_INVALID_ARG, "spk conv: bad operand");
  static DeviceOnce once;
  once.run([] { set_max_lds((const void*)spk_conv_kernel, SPK_MAX_LDS); });
  const unsigned tiles = (unsigned)(((long long)a.Fout * a.w.Tmax + 63) / 64);
  hipLaunchKernelGGL(spk_conv_kernel, dim3(tiles, (unsigned)a.w.B), dim3(64), lds, s, a);
  PF_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------- the TDNN
__global__ __launch_bounds__(256) void spk_tdnn_kernel(SpkTdnnLaunch a) {
  extern __shared__ __attribute__((aligned(16))) char spk_lds[];
  half_t* xt = reinterpret_cast<half_t*>(spk_lds);          // [131, ld]: tile row j is input frame 2 t0 - 2 + j
  const int w = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int T = a.w.T[w], Tp = (T + 1) >> 1, t0 = (int)blockIdx.x * 64;
  if (t0 >= Tp) return;
  const int ld = a.frame_ld + 8, cpr = a.frame_ld >> 3;
  const long long row0 = a.w.toff[w];
  for (int idx = tid; idx < 131 * cpr; idx += 256) {
    const int j = idx / cpr, c0 = (idx - j * cpr) << 3;
    const int ti = 2 * t0 - 2 + j;
    h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ti >= 0 && ti < T && c0 < a.frame_w) v = *reinterpret_cast<const h8a*>(a.frames + (row0 + ti) * a.frame_ld + c0);
    *reinterpret_cast<h8a*>(xt + j * ld + c0) = v;
  }
  __syncthreads();
  const int nt = wave;
  if (nt >= (a.g.Npad >> 5)) return;
  const int r = lane & 31, h = lane >> 5, KS = a.g.Kpad >> 4, KSc = a.frame_ld >> 4;
  const h8* __restrict__ wt = reinterpret_cast<const h8*>(a.w.img + a.g.w_off);
  const float* __restrict__ bias = reinterpret_cast<const float*>(a.w.img + a.g.b_off);
  f16x acc[2];
  tr_bias(bias, nt, h, acc[0]);
  acc[1] = acc[0];
  for (int k = 0; k < 5; ++k) {
    const half_t* x0 = xt + (2 * r + k) * ld + 8 * h;
    tr_mma(wt + ((size_t)nt * KS + (size_t)k * KSc) * 64 + lane, KSc, x0, x0 + 64 * ld, acc[0], acc[1]);
  }
  half_t* X = a.X + a.w.tpoff[w] * a.ldx;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int t = t0 + 32 * i + r;
    if (t >= Tp) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ch = 32 * nt + 8 * q + 4 * h + e;
        const float v = acc[i][4 * q + e];
        if (ch < a.N) X[(long long)t * a.ldx + ch] = (half_t)(v < 0.f ? 0.f : v);                 // R3
      }
  }
}

void launch_spk_tdnn(hipStream_t s, const SpkTdnnLaunch& a) {
  if (a.w.B <= 0 || a.w.Tmax <= 0) return;
  const size_t lds = (size_t)131 * (a.frame_ld + 8) * sizeof(half_t);
  PF_CHECK(a.w.img && a.w.T && a.w.toff && a.w.tpoff && a.frames && a.X && a.frame_ld % 16 == 0 && a.frame_w % 8 == 0 && a.frame_w <= a.frame_ld &&
               a.g.Kpad == 5 * a.frame_ld && a.g.Npad <= 128 && a.N <= a.g.Npad && a.ldx >= a.N && lds <= (size_t)SPK_MAX_LDS &&
               a.w.Tmax <= PF_SPK_MAX_FRAMES,
           PF_ERR_INVALID_ARG, "spk tdnn: bad operand");
  static DeviceOnce once;
  once.run([] { set_max_lds((const void*)spk_tdnn_kernel, SPK_MAX_LDS); });
  const unsigned tiles = (unsigned)(((a.w.Tmax + 1) / 2 + 63) / 64);
  hipLaunchKernelGGL(spk_tdnn_kernel, dim3(tiles, (unsigned)a.w.B), dim3(256), lds, s, a);
  PF_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------- a dense block and its transit
namespace {

// Y = W ReLU(scale X + shift) over the window's frames: X [Tp, C] f16 in global memory (row stride ldx, a multiple of 8), staged
// SB_CHUNK columns at a time into st [64, SB_LDS] (R4); wave `wave` takes the 32-row blocks nt = wave, wave + 4, .. of W, four
// blocks per pass over the columns.  epi(rt, nt, i, acc): tile rt's half i.  Every thread of the workgroup calls this.
template <class Epi>
__device__ __forceinline__ void sb_rows_product(const char* __restrict__ img, const half_t* __restrict__ X, int ldx, int Tp, int ntiles, int C,
                                                const float* __restrict__ scale, const float* __restrict__ shift, const TileGemm& g, half_t* st,
                                                int tid, Epi&& epi) {
  const int wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5, KS = g.Kpad >> 4, NT = g.Npad >> 5;
  const h8* __restrict__ wt = reinterpret_cast<const h8*>(img + g.w_off);
  const float* __restrict__ bias = reinterpret_cast<const float*>(img + g.b_off);
  for (int rt = 0; rt < ntiles; ++rt)
    for (int ntg = 0; ntg < NT; ntg += 4) {
      const int nt = ntg + wave;
      const bool active = nt < NT;
      f16x acc[2];
      if (active) tr_bias(bias, nt, h, acc[0]); else zero_acc(acc[0]);
      acc[1] = acc[0];
      for (int k0 = 0; k0 < g.Kpad; k0 += SB_CHUNK) {
        const int kw = g.Kpad - k0 < SB_CHUNK ? g.Kpad - k0 : SB_CHUNK, cpr = kw >> 3;
        for (int idx = tid; idx < 64 * cpr; idx += 256) {
          const int row = idx / cpr, cc = (idx - row * cpr) << 3, c0 = k0 + cc, t = rt * 64 + row;
          h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
          if (t < Tp && c0 < C) {
            const h8 x = *reinterpret_cast<const h8a*>(X + (long long)t * ldx + c0);
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (c0 + e < C) {
                const float f = (float)x[e] * scale[c0 + e] + shift[c0 + e];
                v[e] = (half_t)(f < 0.f ? 0.f : f);
              }
          }
          *reinterpret_cast<h8a*>(st + row * SB_LDS + cc) = v;
        }
        __syncthreads();
        if (active)
          tr_mma(wt + ((size_t)nt * KS + (size_t)(k0 >> 4)) * 64 + lane, kw >> 4, st + r * SB_LDS + 8 * h, st + (32 + r) * SB_LDS + 8 * h, acc[0],
                 acc[1]);
        __syncthreads();
      }
      if (active) {
        epi(rt, nt, 0, acc[0]);
        epi(rt, nt, 1, acc[1]);
      }
    }
}

}  // namespace

__global__ __launch_bounds__(256) void spk_block_kernel(SpkBlockLaunch a) {
  extern __shared__ __attribute__((aligned(16))) char spk_lds[];
  const int w = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int T = a.w.T[w], Tp = (T + 1) >> 1;
  if (Tp == 0) return;
  const int ntiles = (Tp + 63) >> 6;
  const char* __restrict__ img = a.w.img;
  const SpkLayerDev* __restrict__ layers = reinterpret_cast<const SpkLayerDev*>(img + a.layers_off);
  const int ldb = layers[0].lin1.Npad + 8, ldh = layers[0].cam1.Npad + 8, gp = layers[0].cam2.Npad;
  half_t* bt = reinterpret_cast<half_t*>(spk_lds);                     // [SB_PAD + SB_ROWS + SB_PAD, ldb]: the bottleneck tile
  half_t* st = bt + (size_t)(SB_ROWS + 2 * SB_PAD) * ldb;              // [64, SB_LDS]: the staged columns of X; behind a layer's
  half_t* ctx = st;                                                    // bottleneck product: the context rows [64, ldb] and the
  half_t* hid = st + 64 * ldb;                                         // mask's hidden rows [64, ldh]
  float* mask = reinterpret_cast<float*>(st + 64 * SB_LDS);            // [64, gp]
  const long long base = a.w.tpoff[w];
  half_t* X = a.X + base * a.ldx;
  const int S = a.seg_len, d = a.dilation, bn = a.bn;

  for (int idx = tid; idx < 2 * SB_PAD * ldb; idx += 256) {            // the zero rows in front of and behind the tiles in use
    const int rr = idx / ldb, cc = idx - rr * ldb;
    const int row = rr < SB_PAD ? rr : 64 * ntiles + rr;
    bt[row * ldb + cc] = (half_t)0.f;
  }

  for (int l = 0; l < a.n_layers; ++l) {
    const SpkLayerDev L = layers[l];
    // ---- b = ReLU(W1 ReLU(s X + sh) + c1) into the tile (R5); rows at or beyond Tp are zeros: the taps below read them
    sb_rows_product(img, X, a.ldx, Tp, ntiles, L.C, reinterpret_cast<const float*>(img + L.scale_off),
                    reinterpret_cast<const float*>(img + L.shift_off), L.lin1, st, tid, [&](int rt, int nt, int i, const f16x& acc) {
                      const int t = rt * 64 + 32 * i + r;
#pragma unroll
                      for (int q = 0; q < 4; ++q) {
                        h4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                          const float f = acc[4 * q + e];
                          v[e] = t < Tp ? (half_t)(f < 0.f ? 0.f : f) : (half_t)0.f;
                        }
                        *reinterpret_cast<h4a*>(bt + (SB_PAD + t) * ldb + 32 * nt + 8 * q + 4 * h) = v;
                      }
                    });
    __syncthreads();
    // ---- the context rows: mean_t b + the mean of b over the segment, one thread per column, frames ascending (R6)
    for (int c = tid; c < L.cam1.Kpad; c += 256) {
      float tot = 0.f;
      if (c < bn) {
        for (int t = 0; t < Tp; ++t) tot += (float)bt[(SB_PAD + t) * ldb + c];
        tot /= (float)Tp;
      }
      for (int s0 = 0, seg = 0; s0 < Tp; s0 += S, ++seg) {
        float v = 0.f;
        if (c < bn) {
          const int s1 = s0 + S < Tp ? s0 + S : Tp;
          float sm = 0.f;
          for (int t = s0; t < s1; ++t) sm += (float)bt[(SB_PAD + t) * ldb + c];
          v = tot + sm / (float)(s1 - s0);
        }
        ctx[seg * ldb + c] = (half_t)v;
      }
    }
    __syncthreads();
    // ---- the mask of every segment: sigmoid(W3 ReLU(W2 c + b2) + b3) (R7 between the two)
    tr_product(img, L.cam1, ctx, ldb, wave, lane, [&](int nt, int i, const f16x& acc) { tr_put_f16(acc, true, hid, ldh, i, nt, r, h); });
    __syncthreads();
    tr_product(img, L.cam2, hid, ldh, wave, lane, [&](int nt, int i, const f16x& acc) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) mask[(32 * i + r) * gp + 32 * nt + 8 * q + 4 * h + e] = 1.f / (1.f + expf(-acc[4 * q + e]));
    });
    __syncthreads();
    // ---- the three dilated taps over the tile, times the mask of the frame's segment, appended to X (R8)
    {
      const int NT = L.local.Npad >> 5, KS = L.local.Kpad >> 4, KSb = KS / 3;
      const h8* __restrict__ wl = reinterpret_cast<const h8*>(img + L.local.w_off);
      for (int idx = wave; idx < ntiles * NT; idx += 4) {
        const int rt = idx / NT, nt = idx - rt * NT;
        f16x acc[2];
        zero_acc(acc[0]);
        acc[1] = acc[0];
        for (int k = 0; k < 3; ++k) {
          const half_t* x0 = bt + (SB_PAD + rt * 64 + r + (k - 1) * d) * ldb + 8 * h;
          tr_mma(wl + ((size_t)nt * KS + (size_t)k * KSb) * 64 + lane, KSb, x0, x0 + 32 * ldb, acc[0], acc[1]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int t = rt * 64 + 32 * i + r;
          if (t >= Tp) continue;
          const float* mk = mask + (t / S) * gp;
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int ch = 32 * nt + 8 * q + 4 * h + e;
              if (ch < a.growth) X[(long long)t * a.ldx + L.C + ch] = (half_t)(acc[i][4 * q + e] * mk[ch]);
            }
        }
      }
    }
    __syncthreads();                                                    // the appended channels are the next layer's input
  }

  // ---- the transit: W ReLU(s X + sh), no bias, into the next block's X (R9)
  half_t* Xn = a.Xn + base * a.ldxn;
  sb_rows_product(img, X, a.ldx, Tp, ntiles, a.C1, reinterpret_cast<const float*>(img + a.tr_scale_off),
                  reinterpret_cast<const float*>(img + a.tr_shift_off), a.transit, st, tid, [&](int rt, int nt, int i, const f16x& acc) {
                    const int t = rt * 64 + 32 * i + r;
                    if (t >= Tp) return;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                      for (int e = 0; e < 4; ++e) {
                        const int ch = 32 * nt + 8 * q + 4 * h + e;
                        if (ch < a.transit.N) Xn[(long long)t * a.ldxn + ch] = (half_t)acc[4 * q + e];
                      }
                  });
}

static void launch_spk_block_sized(hipStream_t s, const SpkBlockLaunch& a, int npb, int nph, int gp) {
  const size_t lds = ((size_t)(SB_ROWS + 2 * SB_PAD) * (npb + 8) + (size_t)64 * SB_LDS) * sizeof(half_t) + (size_t)64 * gp * sizeof(float);
  PF_CHECK(a.w.img && a.w.T && a.w.tpoff && a.X && a.Xn && a.n_layers >= 1 && a.ldx % 8 == 0 && a.ldx >= a.C1 && a.ldxn >= a.transit.N &&
               a.dilation >= 1 && a.dilation <= SB_PAD && a.seg_len >= 1 && (SB_ROWS + a.seg_len - 1) / a.seg_len <= 64 && a.bn <= npb &&
               npb + 8 + nph + 8 <= SB_LDS && a.growth <= gp && gp <= 64 && a.transit.K == a.C1 && lds <= (size_t)SPK_MAX_LDS &&
               a.w.Tmax <= PF_SPK_MAX_FRAMES,
           PF_ERR_INVALID_ARG, "spk block: bad operand");
  static DeviceOnce once;
  once.run([] { set_max_lds((const void*)spk_block_kernel, SPK_MAX_LDS); });
  hipLaunchKernelGGL(spk_block_kernel, dim3((unsigned)a.w.B), dim3(256), lds, s, a);
  PF_HIP(hipGetLastError());
}

void launch_spk_block(hipStream_t s, const SpkBlockLaunch& a) {
  if (a.w.B <= 0 || a.w.Tmax <= 0) return;
  // the tile widths are the same for every layer of a block: (bn padded to 32), (bn / 2 padded to 32), (growth padded to 32)
  launch_spk_block_sized(s, a, (int)round_up(a.bn, 32), (int)round_up(a.bn / 2, 32), (int)round_up(a.growth, 32));
}

// ---------------------------------------------------------------------------------------------- pooling and the embedding
__global__ __launch_bounds__(256) void spk_pool_kernel(SpkPoolLaunch a) {
  extern __shared__ __attribute__((aligned(16))) char spk_lds[];
  half_t* st = reinterpret_cast<half_t*>(spk_lds);          // [dense.Kpad]: mean || std (R10), zeros behind them
  const int w = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int T = a.w.T[w], Tp = (T + 1) >> 1, C = a.C;
  if (Tp == 0) {
    for (int e = tid; e < a.E; e += 256) a.emb[(long long)w * a.E + e] = 0.f;
    return;
  }
  const long long base = a.w.tpoff[w];
  const half_t* __restrict__ X = a.X + base * a.ldx;
  const float* __restrict__ scale = reinterpret_cast<const float*>(a.w.img + a.scale_off);
  const float* __restrict__ shift = reinterpret_cast<const float*>(a.w.img + a.shift_off);
  for (int c = tid; c < C; c += 256) {
    const float sc = scale[c], sh = shift[c];
    float sum = 0.f;
    for (int t = 0; t < Tp; ++t) {
      float v = (float)X[(long long)t * a.ldx + c] * sc + sh;
      v = v < 0.f ? 0.f : v;
      if (a.frames) a.frames[(base + t) * C + c] = v;
      sum += v;
    }
    const float mean = sum / (float)Tp;
    float ss = 0.f;
    for (int t = 0; t < Tp; ++t) {
      float v = (float)X[(long long)t * a.ldx + c] * sc + sh;
      v = v < 0.f ? 0.f : v;
      ss += (v - mean) * (v - mean);
    }
    st[c] = (half_t)mean;
    st[C + c] = (half_t)(Tp > 1 ? sqrtf(ss / (float)(Tp - 1)) : 0.f);
  }
  for (int c = 2 * C + tid; c < a.dense.Kpad; c += 256) st[c] = (half_t)0.f;
  __syncthreads();
  const int r = lane & 31, h = lane >> 5;
  tr_product(a.w.img, a.dense, st, 0, wave, lane, [&](int nt, int i, const f16x& acc) {
    if (r != 0 || i != 0) return;                          // every tile row is the same vector
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ch = 32 * nt + 8 * q + 4 * h + e;
        if (ch < a.E) a.emb[(long long)w * a.E + ch] = acc[4 * q + e];
      }
  });
}

void launch_spk_pool(hipStream_t s, const SpkPoolLaunch& a) {
  if (a.w.B <= 0) return;
  PF_CHECK(a.w.img && a.w.T && a.w.tpoff && a.X && a.emb && a.dense.K == 2 * a.C && a.E <= a.dense.Npad && a.ldx >= a.C, PF_ERR_INVALID_ARG,
           "spk pool: bad operand");
  hipLaunchKernelGGL(spk_pool_kernel, dim3((unsigned)a.w.B), dim3(256), (size_t)(a.dense.Kpad + 8) * sizeof(half_t), s, a);
  PF_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------- the cosines of a stream
__global__ __launch_bounds__(256) void spk_affinity_kernel(SpkAffinityLaunch a) {
  const int s = blockIdx.y;
  const long long n = a.eoff[s + 1] - a.eoff[s];
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * n) return;
  const long long i = idx / n, j = idx - i * n;
  const float* __restrict__ u = a.emb + (a.eoff[s] + i) * a.E;
  const float* __restrict__ v = a.emb + (a.eoff[s] + j) * a.E;
  float uv = 0.f, uu = 0.f, vv = 0.f;
  for (int k = 0; k < a.E; ++k) {
    uv += u[k] * v[k];
    uu += u[k] * u[k];
    vv += v[k] * v[k];
  }
  const float den = sqrtf(uu) * sqrtf(vv);
  a.out[a.ooff[s] + idx] = den > 0.f ? uv / den : 0.f;
}

void launch_spk_affinity(hipStream_t s, const SpkAffinityLaunch& a) {
  if (a.S <= 0 || a.nmax <= 0) return;
  PF_CHECK(a.emb && a.eoff && a.ooff && a.out && a.E >= 1 && a.nmax <= PF_SPK_MAX_WINDOWS, PF_ERR_INVALID_ARG, "spk affinity: bad operand");
  const unsigned tiles = (unsigned)(((long long)a.nmax * a.nmax + 255) / 256);
  hipLaunchKernelGGL(spk_affinity_kernel, dim3(tiles, (unsigned)a.S), dim3(256), 0, s, a);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
