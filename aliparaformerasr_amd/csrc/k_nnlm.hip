// k_nnlm.hip — a causal Transformer LM that scores token sequences on the device (paraformer_hip.h "Neural LM rescoring",
// DESIGN.md §4.6y).  The definition in numpy float64 is tests/nnlm_ref.py, the host twin host_nnlm_logp (nnlm.cpp).
//
// Rows are the concatenated input ids [sos, y_1 .. y_n] of B sequences (row offsets off [B + 1], 1 <= T[b] <= 256), each row
// with its target id ([y_1 .. y_n, eos]).  A forward is 2 + 2 n_layers launches:
//   1                 nnlm_rows (head 0, tail 0): embedding gather -> input Linear -> LayerNorm -> ReLU -> x; norm1_0 -> qkv_0
//   per layer l       nnlm_attn: causal softmax(q k^T) v per (64-query tile, head, sequence) -> ctx
//                     nnlm_rows (head 1): out(ctx) + x -> x; norm2 -> w2(relu(w1)) + x -> x; then
//                       tail 0 (l < n - 1): norm1_{l+1} -> qkv_{l+1}      tail 1 (l = n - 1): after_norm -> decoder -> logp[target]
//   1                 nnlm_sum: the sequential fp32 sum of a sequence's logp, with or without its eos row (one thread each)
// The dependences between workgroups (a sequence's keys) are covered by launch boundaries: no grid barrier, nothing persistent,
// no atomics.  Only x (fp32), q | k | v (f16), ctx (f16) and logp (fp32, one per row) go to global memory; the [rows, V] logits
// are never stored.
//
// nnlm_rows: a workgroup of four waves owns 32 consecutive rows, which may straddle sequences.  At d_model 512 a 64-row tile
// with the residual beside two activation tiles would need 265 KB of LDS; 32 rows need x fp32 [32, 516] + two f16 [32, 520]
// tiles = 130 KB, and twice as many workgroups work on the short sequences an n-best list holds.  A product is the one-half
// form of tile_rows.h (tr_product1 / tr_mma1): a tile row is an output column, so its result depends on that row and on W
// alone, in a fixed k order.  LayerNorm is one wave per row, eight channels per lane, in a fixed reduction order.  That, and an
// attention launch that sees one sequence per workgroup, is why a sequence's bits do not depend on its batch mates or on where
// its rows start.  The FFN hidden is walked in slices of 256 channels (w1 slice -> ReLU -> f16 tile -> w2 partial sums in four
// accumulators per wave).
//
// The vocabulary head (tail 1): a wave walks the decoder's 32-row blocks nt = wave, wave + 4, ...; lane (r, h) keeps an online
// (max, sum) of row r over the channels it owns and the target's logit when its block passes; channels at or beyond V (the
// zero padding of the last block, logit 0) take no part.  The 8 partials of a row (4 waves x 2 lane halves) are combined by
// one thread in the fixed order k = 2 wave + h = 0 .. 7: M = max m_k, S = sum s_k exp(m_k - M), logp = logit - (M + log S).
//
// nnlm_attn: one wave per (64-query tile, head of 64 channels, sequence).  V_h^T [64, keys] is staged in LDS; S^T = K Q^T in
// four k-steps (keys on the accumulator's rows, the query on the lane), so exp(S - max) converts in place into the B operand
// of O^T = V^T P^T for both 32-channel blocks of the head.  Only the key blocks at or below the query tile are visited, the
// blocks on the diagonal are masked per element (key <= query): a masked score takes no part in the maximum and is an exact
// zero in the sum and in O.  Two passes over the keys (row maximum, then exp / sum / PV): no rescaling.  Rows at or beyond T
// are clamped on load and never stored.
//
// Rounding points (everything else is fp32): R0 the weights and R0e the embedding table, once, at attach time; R1 the outputs
// of norm1, norm2 and after_norm (the input layer's LayerNorm + ReLU IS the residual and stays fp32); R2 q * dh^-0.5 (1 / 8,
// exact), k and v; R3 the softmax numerators exp(s - max) as the PV operand (their sum is taken from the fp32 values); R4 ctx;
// R5 the FFN hidden after ReLU.  ReLU is x < 0 ? 0 : x, which keeps a NaN.
#include "kdev.h"
#include "kernels.h"
#include "punc_dev.h"
#include "tile_rows.h"

namespace pf {

namespace {

constexpr int NR_ROWS = 32, NR_D = 512, NR_XLD = 516, NR_LD = 520;
constexpr size_t NR_X_BYTES = (size_t)NR_ROWS * NR_XLD * 4, NR_BUF_BYTES = (size_t)NR_ROWS * NR_LD * 2;
constexpr size_t NR_LDS_BYTES = NR_X_BYTES + 2 * NR_BUF_BYTES + TR_ROWS * 8 + TR_ROWS * 4;       // tr_row_info fills 64 entries

// the lane's eight channels of a row: 4 lane + (0 .. 3) and 256 + 4 lane + (0 .. 3); mean and variance in a fixed order
struct NrStat { float d[8], inv; };
__device__ __forceinline__ NrStat nr_stat(const float* __restrict__ xrow, int lane) {
  const float4 u = *reinterpret_cast<const float4a*>(xrow + 4 * lane), v = *reinterpret_cast<const float4a*>(xrow + 256 + 4 * lane);
  const float mu = wave_sum(((u.x + u.y) + (u.z + u.w)) + ((v.x + v.y) + (v.z + v.w))) * (1.f / NR_D);
  NrStat s;
  s.d[0] = u.x - mu; s.d[1] = u.y - mu; s.d[2] = u.z - mu; s.d[3] = u.w - mu;
  s.d[4] = v.x - mu; s.d[5] = v.y - mu; s.d[6] = v.z - mu; s.d[7] = v.w - mu;
  const float var = wave_sum(((s.d[0] * s.d[0] + s.d[1] * s.d[1]) + (s.d[2] * s.d[2] + s.d[3] * s.d[3])) +
                             ((s.d[4] * s.d[4] + s.d[5] * s.d[5]) + (s.d[6] * s.d[6] + s.d[7] * s.d[7]))) * (1.f / NR_D);
  s.inv = 1.f / sqrtf(var + 1e-12f);
  return s;
}

// LayerNorm of the fp32 tile into an f16 tile: one wave per row                                                   (R1)
__device__ __forceinline__ void nr_norm(const float* __restrict__ xs, const float* __restrict__ gam, const float* __restrict__ bet,
                                        half_t* __restrict__ y, int wave, int lane) {
  const float4 g0 = *reinterpret_cast<const float4*>(gam + 4 * lane), g1 = *reinterpret_cast<const float4*>(gam + 256 + 4 * lane);
  const float4 b0 = *reinterpret_cast<const float4*>(bet + 4 * lane), b1 = *reinterpret_cast<const float4*>(bet + 256 + 4 * lane);
  for (int row = wave; row < NR_ROWS; row += 4) {
    const NrStat s = nr_stat(xs + row * NR_XLD, lane);
    h4 o0, o1;
    o0[0] = (half_t)(s.d[0] * s.inv * g0.x + b0.x); o0[1] = (half_t)(s.d[1] * s.inv * g0.y + b0.y);
    o0[2] = (half_t)(s.d[2] * s.inv * g0.z + b0.z); o0[3] = (half_t)(s.d[3] * s.inv * g0.w + b0.w);
    o1[0] = (half_t)(s.d[4] * s.inv * g1.x + b1.x); o1[1] = (half_t)(s.d[5] * s.inv * g1.y + b1.y);
    o1[2] = (half_t)(s.d[6] * s.inv * g1.z + b1.z); o1[3] = (half_t)(s.d[7] * s.inv * g1.w + b1.w);
    *reinterpret_cast<h4a*>(y + row * NR_LD + 4 * lane) = o0;
    *reinterpret_cast<h4a*>(y + row * NR_LD + 256 + 4 * lane) = o1;
  }
}

__device__ __forceinline__ float nr_relu(float f) { return f < 0.f ? 0.f : f; }

}  // namespace

__global__ __launch_bounds__(256) void nnlm_rows_kernel(NnlmRowsLaunch a) {
  extern __shared__ __attribute__((aligned(16))) char nr_lds[];
  float* xs = reinterpret_cast<float*>(nr_lds);
  half_t* bufA = reinterpret_cast<half_t*>(nr_lds + NR_X_BYTES);
  half_t* bufB = reinterpret_cast<half_t*>(nr_lds + NR_X_BYTES + NR_BUF_BYTES);
  long long* row_start = reinterpret_cast<long long*>(nr_lds + NR_X_BYTES + 2 * NR_BUF_BYTES);
  int* row_T = reinterpret_cast<int*>(nr_lds + NR_X_BYTES + 2 * NR_BUF_BYTES + TR_ROWS * 8);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const long long g0 = (long long)blockIdx.x * NR_ROWS;

  tr_row_info(a.off, a.B, a.total, g0, tid, row_start, row_T);         // every row's sequence (entries 32 .. 63 are not used)
  __syncthreads();

  if (a.head == 0) {
    // ---- the embedding rows (f16, as the image holds them) into bufA [32, E]
    const half_t* __restrict__ emb = reinterpret_cast<const half_t*>(a.img + a.embed_off);
    for (int row = wave; row < NR_ROWS; row += 4)
      if (8 * lane < a.E) {
        h8 e = {0, 0, 0, 0, 0, 0, 0, 0};
        if (row_T[row] > 0) e = *reinterpret_cast<const h8*>(emb + (size_t)a.ids[g0 + row] * a.E + 8 * lane);
        *reinterpret_cast<h8a*>(bufA + row * NR_LD + 8 * lane) = e;
      }
    __syncthreads();
    // ---- the input Linear -> xs, then LayerNorm and ReLU in place: x, fp32
    tr_product1(a.img, a.in, bufA, NR_LD, wave, lane, [&](int nt, const f16x& acc) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4a*>(xs + r * NR_XLD + 32 * nt + 8 * q + 4 * h) =
            make_float4(acc[4 * q + 0], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
    });
    __syncthreads();
    {
      const float* gam = reinterpret_cast<const float*>(a.img + a.in_g);
      const float* bet = reinterpret_cast<const float*>(a.img + a.in_b);
      const float4 p0 = *reinterpret_cast<const float4*>(gam + 4 * lane), p1 = *reinterpret_cast<const float4*>(gam + 256 + 4 * lane);
      const float4 c0 = *reinterpret_cast<const float4*>(bet + 4 * lane), c1 = *reinterpret_cast<const float4*>(bet + 256 + 4 * lane);
      for (int row = wave; row < NR_ROWS; row += 4) {
        const NrStat s = nr_stat(xs + row * NR_XLD, lane);
        const float4 u = make_float4(nr_relu(s.d[0] * s.inv * p0.x + c0.x), nr_relu(s.d[1] * s.inv * p0.y + c0.y),
                                     nr_relu(s.d[2] * s.inv * p0.z + c0.z), nr_relu(s.d[3] * s.inv * p0.w + c0.w));
        const float4 v = make_float4(nr_relu(s.d[4] * s.inv * p1.x + c1.x), nr_relu(s.d[5] * s.inv * p1.y + c1.y),
                                     nr_relu(s.d[6] * s.inv * p1.z + c1.z), nr_relu(s.d[7] * s.inv * p1.w + c1.w));
        *reinterpret_cast<float4a*>(xs + row * NR_XLD + 4 * lane) = u;
        *reinterpret_cast<float4a*>(xs + row * NR_XLD + 256 + 4 * lane) = v;
        if (row_T[row] > 0) {
          *reinterpret_cast<float4*>(a.x + (g0 + row) * NR_D + 4 * lane) = u;
          *reinterpret_cast<float4*>(a.x + (g0 + row) * NR_D + 256 + 4 * lane) = v;
        }
      }
    }
    __syncthreads();
  } else {
    // ---- the ctx tile (f16, as stored) into bufA and the residual rows into xs: one wave per row
    for (int row = wave; row < NR_ROWS; row += 4) {
      h8 c = {0, 0, 0, 0, 0, 0, 0, 0};
      float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
      if (row_T[row] > 0) {
        c = *reinterpret_cast<const h8*>(a.ctx + (g0 + row) * NR_D + 8 * lane);
        u = *reinterpret_cast<const float4*>(a.x + (g0 + row) * NR_D + 4 * lane);
        v = *reinterpret_cast<const float4*>(a.x + (g0 + row) * NR_D + 256 + 4 * lane);
      }
      *reinterpret_cast<h8a*>(bufA + row * NR_LD + 8 * lane) = c;
      *reinterpret_cast<float4a*>(xs + row * NR_XLD + 4 * lane) = u;
      *reinterpret_cast<float4a*>(xs + row * NR_XLD + 256 + 4 * lane) = v;
    }
    __syncthreads();
    // ---- x + out(ctx) -> xs
    tr_product1(a.img, a.out, bufA, NR_LD, wave, lane, [&](int nt, const f16x& acc) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float* p = xs + r * NR_XLD + 32 * nt + 8 * q + 4 * h;
        float4 f = *reinterpret_cast<const float4a*>(p);
        f.x += acc[4 * q + 0]; f.y += acc[4 * q + 1]; f.z += acc[4 * q + 2]; f.w += acc[4 * q + 3];
        *reinterpret_cast<float4a*>(p) = f;
      }
    });
    __syncthreads();
    // ---- norm2 -> bufA; the FFN in slices of 256 hidden channels: w1 slice -> ReLU -> bufB (R5) -> w2 partial sums
    nr_norm(xs, reinterpret_cast<const float*>(a.img + a.n2_g), reinterpret_cast<const float*>(a.img + a.n2_b), bufA, wave, lane);
    __syncthreads();
    const h8* __restrict__ w1t = reinterpret_cast<const h8*>(a.img + a.w1.w_off);
    const h8* __restrict__ w2t = reinterpret_cast<const h8*>(a.img + a.w2.w_off);
    const float* __restrict__ b1 = reinterpret_cast<const float*>(a.img + a.w1.b_off);
    const int KS1 = a.w1.Kpad >> 4, KS2 = a.w2.Kpad >> 4;
    f16x y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) tr_bias(reinterpret_cast<const float*>(a.img + a.w2.b_off), wave + 4 * j, h, y[j]);
    const half_t* xa = bufA + r * NR_LD + 8 * h;
    const half_t* xb = bufB + r * NR_LD + 8 * h;
    for (int c = 0; c < (a.w1.Npad >> 8); ++c) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int nb = wave + 4 * j, nt = 8 * c + nb;
        f16x acc;
        tr_bias(b1, nt, h, acc);
        tr_mma1(w1t + ((size_t)nt * KS1) * 64 + lane, KS1, xa, acc);
        tr_put_f16(acc, true, bufB, NR_LD, 0, nb, r, h);                                                  // R5
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 4; ++j) tr_mma1(w2t + ((size_t)(wave + 4 * j) * KS2 + 16 * c) * 64 + lane, 16, xb, y[j]);
      __syncthreads();
    }
    // ---- x + ffn -> xs, and to memory where a later launch reads it
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = 32 * (wave + 4 * j) + 8 * q + 4 * h;
        float4 f = *reinterpret_cast<const float4a*>(xs + r * NR_XLD + n);
        f.x += y[j][4 * q + 0]; f.y += y[j][4 * q + 1]; f.z += y[j][4 * q + 2]; f.w += y[j][4 * q + 3];
        *reinterpret_cast<float4a*>(xs + r * NR_XLD + n) = f;
        if (a.tail == 0 && row_T[r] > 0) *reinterpret_cast<float4*>(a.x + (g0 + r) * NR_D + n) = f;
      }
    __syncthreads();
  }

  // ---- the tail: a LayerNorm of xs into bufA, then one product
  nr_norm(xs, reinterpret_cast<const float*>(a.img + a.n_g), reinterpret_cast<const float*>(a.img + a.n_b), bufA, wave, lane);
  __syncthreads();
  if (a.tail == 0) {
    // q * dh^-0.5 | k | v of the next layer, f16                                                            (R2)
    tr_product1(a.img, a.last, bufA, NR_LD, wave, lane, [&](int nt, const f16x& acc) {
      if (row_T[r] <= 0) return;
      const float sc = nt < (NR_D >> 5) ? 0.125f : 1.f;
      half_t* dst = a.qkv_out + (g0 + r) * (3 * NR_D) + 32 * nt + 4 * h;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        h4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (half_t)(acc[4 * q + e] * sc);
        *reinterpret_cast<h4*>(dst + 8 * q) = v;
      }
    });
    return;
  }
  // ---- the vocabulary head: online (max, sum) per lane over the decoder's blocks, the target's logit as its block passes
  const bool valid = row_T[r] > 0;
  const int tg = valid ? a.tgt[g0 + r] : -1;
  float m = -INFINITY, s = 0.f, tl = 0.f;
  tr_product1(a.img, a.last, bufA, NR_LD, wave, lane, [&](int nt, const f16x& acc) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = 32 * nt + 8 * q + 4 * h + e;
        if (n < a.V) {                                               // a padded decoder row holds logit 0, not -inf: left out
          const float v = acc[4 * q + e];
          if (v > m) { s = s * expf(m - v) + 1.f; m = v; }
          else s += expf(v - m);
          if (n == tg) tl = v;
        }
      }
  });
  float* part = reinterpret_cast<float*>(bufB);                      // [3][8][32]: m, s, the target's logit (0 where it did not pass)
  const int k = 2 * wave + h;
  part[(0 * 8 + k) * 32 + r] = m;
  part[(1 * 8 + k) * 32 + r] = s;
  part[(2 * 8 + k) * 32 + r] = tl;
  __syncthreads();
  if (tid < NR_ROWS && row_T[tid] > 0) {
    float M = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) M = fmaxf(M, part[(0 * 8 + j) * 32 + tid]);
    float S = 0.f, L = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      S += part[(1 * 8 + j) * 32 + tid] * expf(part[(0 * 8 + j) * 32 + tid] - M);      // a lane without channels: 0 * exp(-inf) = 0
      L += part[(2 * 8 + j) * 32 + tid];
    }
    a.logp[g0 + tid] = L - (M + logf(S));
  }
}

// ---------------------------------------------------------------- attention: one wave per (64-query tile, head, sequence)
constexpr int NA_VLD = 264;                 // V^T row stride in halves: 256 keys + 8
constexpr int NA_MAX_T = 256;

__global__ __launch_bounds__(64) void nnlm_attn_kernel(NnlmAttnLaunch a) {
  __shared__ __attribute__((aligned(16))) half_t vt[64 * NA_VLD];
  const int b = blockIdx.z, hd = blockIdx.y, q0 = blockIdx.x * 64;
  const long long start = a.off[b];
  const int T = (int)(a.off[b + 1] - start);
  if (q0 >= T) return;
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int nkb = min((T + 31) >> 5, (q0 >> 5) + 2);          // the key blocks at or below the query tile
  const half_t* __restrict__ base = a.qkv + start * (3 * NR_D) + hd * 64;

  // V_h^T: vt[d][key], zeros at keys in [T, 32 nkb)
  for (int key = lane; key < 32 * nkb; key += 64) {
    h8 v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      v[c] = h8{0, 0, 0, 0, 0, 0, 0, 0};
      if (key < T) v[c] = *reinterpret_cast<const h8*>(base + (size_t)key * (3 * NR_D) + 2 * NR_D + 8 * c);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
      for (int e = 0; e < 8; ++e) vt[(8 * c + e) * NA_VLD + key] = v[c][e];
  }
  __syncthreads();

  // Q: the B operand, lane (r, h) holds Q[query r][16 s + 8 h + j]; rows at or beyond T are clamped (never stored).
  // lim: one past the last key the lane's query may see
  h8 qf[2][4];
  int lim[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int qr = min(q0 + 32 * i + r, T - 1);
    lim[i] = qr + 1;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[i][s] = *reinterpret_cast<const h8*>(base + (size_t)qr * (3 * NR_D) + 16 * s + 8 * h);
  }
  auto keys = [&](int kb, h8 (&kf)[4]) {
    const int kr = min(32 * kb + r, T - 1);
    const half_t* kp = base + (size_t)kr * (3 * NR_D) + NR_D + 8 * h;
#pragma unroll
    for (int s = 0; s < 4; ++s) kf[s] = *reinterpret_cast<const h8*>(kp + 16 * s);
  };
  auto scores = [&](const h8 (&kf)[4], const h8 (&q)[4]) {
    f16x z;
#pragma unroll
    for (int e = 0; e < 16; ++e) z[e] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) z = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[s], q[s], z, 0, 0, 0);
    return z;
  };
  // pass 1: the row maximum over the keys at or below the query
  float mx[2] = {-INFINITY, -INFINITY};
  for (int kb = 0; kb < nkb; ++kb) {
    h8 kf[4];
    keys(kb, kf);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (32 * kb <= q0 + 32 * i + 31) pa_max(scores(kf, qf[i]), 32 * kb + 4 * h, lim[i], mx[i]);     // (a block above the half's diagonal: skipped)
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) mx[i] = fmaxf(mx[i], __shfl_xor(mx[i], 32, 64));
  // pass 2: exp (R3 as the PV operand; the sum takes the fp32 values), the sum and O^T = V^T P^T for both channel blocks
  float sum[2] = {0.f, 0.f};
  f16x O[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) O[i][c][e] = 0.f;
  for (int kb = 0; kb < nkb; ++kb) {
    h8 kf[4];
    keys(kb, kf);
    h8 vf[2][2];
#pragma unroll
    for (int c = 0; c < 2; ++c) pa_vfrag(vt + (32 * c + r) * NA_VLD + 32 * kb + 4 * h, vf[c]);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (32 * kb > q0 + 32 * i + 31) continue;
      const f16x S = scores(kf, qf[i]);
      const int key0 = 32 * kb + 4 * h;
      h8 pf[2];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float p = 0.f;
        if (key0 + (e & 3) + 8 * (e >> 2) < lim[i]) p = expf(S[e] - mx[i]);
        sum[i] += p;
        pf[e >> 3][e & 7] = (half_t)p;                                                         // R3
      }
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        O[i][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[c][0], pf[0], O[i][c], 0, 0, 0);
        O[i][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[c][1], pf[1], O[i][c], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float l = sum[i] + __shfl_xor(sum[i], 32, 64);
    const int qr = q0 + 32 * i + r;
    if (qr >= T) continue;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      half_t* dst = a.ctx + (start + qr) * NR_D + hd * 64 + 32 * c + 4 * h;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        h4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (half_t)(O[i][c][4 * q + e] / l);                   // R4
        *reinterpret_cast<h4*>(dst + 8 * q) = v;
      }
    }
  }
}

// ---------------------------------------------------------------- the sum: one thread per sequence, sequential fp32
__global__ __launch_bounds__(64) void nnlm_sum_kernel(NnlmSumLaunch a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  const long long start = a.off[b];
  const int n = (int)(a.off[b + 1] - start) - 1;                 // the hypothesis's tokens; row n is the eos row
  float s = 0.f;
  for (int t = 0; t < n; ++t) s = __fadd_rn(s, a.logp[start + t]);
  if (a.eos && n >= 0) s = __fadd_rn(s, a.logp[start + n]);
  a.lm_sum[b] = s;
}

void launch_nnlm_rows(hipStream_t s, const NnlmRowsLaunch& a) {
  if (a.total <= 0 || a.B <= 0) return;
  PF_CHECK(a.img && a.off && a.x && (a.head == 0 ? a.ids != nullptr : a.ctx != nullptr) &&
               (a.tail == 0 ? a.qkv_out != nullptr : (a.tgt != nullptr && a.logp != nullptr)),
           PF_ERR_INVALID_ARG, "nnlm: missing operand");
  PF_CHECK(a.last.Kpad == NR_D &&
               (a.head == 0 ? (a.in.Npad == NR_D && a.in.Kpad == a.E && a.E >= 16 && a.E <= NR_D && a.E % 16 == 0)
                            : (a.out.Kpad == NR_D && a.out.Npad == NR_D && a.w1.Kpad == NR_D && a.w1.Npad % 256 == 0 && a.w1.Npad >= 256 &&
                               a.w2.Npad == NR_D && a.w2.Kpad == a.w1.Npad)) &&
               (a.tail == 0 ? a.last.Npad == 3 * NR_D : (a.V >= 2 && a.last.Npad == (a.V + 31) / 32 * 32)),
           PF_ERR_UNSUPPORTED, "nnlm: the kernel is built for d_model 512, an embedding and an FFN width inside its tiles");
  static DeviceOnce once;
  once.run([] { set_max_lds((const void*)nnlm_rows_kernel, (int)NR_LDS_BYTES); });
  hipLaunchKernelGGL(nnlm_rows_kernel, dim3((unsigned)((a.total + NR_ROWS - 1) / NR_ROWS)), dim3(256), NR_LDS_BYTES, s, a);
  PF_HIP(hipGetLastError());
}

void launch_nnlm_attn(hipStream_t s, const NnlmAttnLaunch& a) {
  if (a.B <= 0) return;
  PF_CHECK(a.qkv && a.off && a.ctx && a.B <= 65535, PF_ERR_INVALID_ARG, "nnlm: missing operand or more than 65535 sequences");
  hipLaunchKernelGGL(nnlm_attn_kernel, dim3(NA_MAX_T / 64, 8, (unsigned)a.B), dim3(64), 0, s, a);
  PF_HIP(hipGetLastError());
}

void launch_nnlm_sum(hipStream_t s, const NnlmSumLaunch& a) {
  if (a.B <= 0) return;
  PF_CHECK(a.logp && a.off && a.lm_sum, PF_ERR_INVALID_ARG, "nnlm: missing operand");
  hipLaunchKernelGGL(nnlm_sum_kernel, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, s, a);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
