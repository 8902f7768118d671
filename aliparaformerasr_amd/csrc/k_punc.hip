// k_punc.hip — the CT-Transformer punctuation model on the device (paraformer_hip.h "Punctuation").  The
// definition in numpy float64 is tests/punc_ref.py, the host twin host_punc_* (punc.cpp).
//
// Rows are the concatenated ids of B windows (row offsets off [B + 1], 0 <= T[b] <= 512).  A forward is 2 + 2 n_layers launches:
//   1                 punc_rows (head 0, tail 0): embedding gather * 16 + pe -> x; norm1_0 -> qkv_0
//   per layer l       punc_attn: softmax(q k^T) v per (64-query tile, head, window) -> ctx
//                     punc_rows (head 1): out(ctx) + fsmn(v) + x -> x; norm2 -> w2(relu(w1)) + x -> x; then
//                       tail 0 (l < n - 1): norm1_{l+1} -> qkv_{l+1}        tail 1 (l = n - 1): after_norm -> decoder -> arg-max
//   1                 punc_cut: the cut rule and the last-window edits per window
// The dependences between workgroups (a window's keys, the FSMN halo) are covered by launch boundaries: no grid barrier,
// nothing persistent.  Only x (fp32), q | k | v (f16, two buffers that alternate: a row tile reads the v halo of its
// neighbours while it writes the next layer's rows) and ctx (f16) go to global memory; LayerNorm outputs, the FFN hidden and
// the FSMN sum stay in LDS and registers.
//
// punc_rows: a workgroup of four waves owns 64 consecutive rows, which may straddle windows (every row looks up its own
// window).  A product is the one of tile_rows.h, on an activation tile X [64, 256] f16 in LDS with a row stride of 264
// halves: a tile row's result depends on that row of X and on W alone, whatever the other 63 rows hold.  LayerNorm is one
// wave per row in a fixed reduction order.  That, and an
// attention launch that sees one window per workgroup, is why a window's bits do not depend on its batch mates or on where
// its rows start.  The FFN hidden is walked in slices of 256 channels (w1 slice -> ReLU -> f16 tile -> w2 partial sums in
// registers), which is what lets a 64-row tile fit: x fp32 [64, 260] + two f16 [64, 264] tiles = 132 KB of LDS.
//
// punc_attn: one wave per (64-query tile, head, window).  V_h^T [32, T] of the window is staged in LDS; S^T = K Q^T (keys on
// the accumulator's rows, the query on the lane), so exp(S - max) converts in place into the B operand of O^T = V^T P^T
// (k order inside a step permuted as the accumulator lays it out; the V^T fragment is read in that same order).  Two passes
// over the keys (row maximum, then exp / sum / PV): no rescaling.  Rows at or beyond T are clamped on load and never stored.
//
// Rounding points (everything else is fp32): R0 the weights and R0e the embedding table, once, at attach time; R1 every
// LayerNorm output; R2 q * dh^-0.5, k and v; R3 the softmax numerators exp(s - max) as the PV operand (their sum is taken
// from the fp32 values); R4 ctx; R5 the FFN hidden after ReLU.  ReLU is x < 0 ? 0 : x, which keeps a NaN.
// The tile geometry, the LayerNorm and the steps of the attention passes are punc_dev.h's, shared with k_punc_stream.hip.
#include "kdev.h"
#include "kernels.h"
#include "punc_dev.h"
#include "tile_rows.h"

namespace pf {

namespace {

constexpr size_t PR_LDS_BYTES = PR_X_BYTES + 2 * PR_BUF_BYTES + PR_ROWS * 8 + PR_ROWS * 4;

}  // namespace

__global__ __launch_bounds__(256) void punc_rows_kernel(PuncRowsLaunch a) {
  extern __shared__ __attribute__((aligned(16))) char pr_lds[];
  float* xs = reinterpret_cast<float*>(pr_lds);
  half_t* bufA = reinterpret_cast<half_t*>(pr_lds + PR_X_BYTES);
  half_t* bufB = reinterpret_cast<half_t*>(pr_lds + PR_X_BYTES + PR_BUF_BYTES);
  long long* row_start = reinterpret_cast<long long*>(pr_lds + PR_X_BYTES + 2 * PR_BUF_BYTES);
  int* row_T = reinterpret_cast<int*>(pr_lds + PR_X_BYTES + 2 * PR_BUF_BYTES + PR_ROWS * 8);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const long long g0 = (long long)blockIdx.x * PR_ROWS;

  tr_row_info(a.off, a.B, a.total, g0, tid, row_start, row_T);         // every row's window
  __syncthreads();

  if (a.head == 0) {
    // ---- x = fp32(embed[id]) * 16 + pe[t]: two roundings (the product is exact short of overflow)
    const half_t* __restrict__ emb = reinterpret_cast<const half_t*>(a.img + a.embed_off);
    const float* __restrict__ pe = reinterpret_cast<const float*>(a.img + a.pe_off);
    for (int row = wave; row < PR_ROWS; row += 4) {
      const long long g = g0 + row;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row_T[row] > 0) {
        const long long t = g - row_start[row];
        const h4 e = *reinterpret_cast<const h4*>(emb + (size_t)a.ids[g] * PR_D + 4 * lane);
        const float4 p4 = *reinterpret_cast<const float4*>(pe + t * PR_D + 4 * lane);
        v.x = __fadd_rn(__fmul_rn((float)e[0], 16.f), p4.x); v.y = __fadd_rn(__fmul_rn((float)e[1], 16.f), p4.y);
        v.z = __fadd_rn(__fmul_rn((float)e[2], 16.f), p4.z); v.w = __fadd_rn(__fmul_rn((float)e[3], 16.f), p4.w);
        *reinterpret_cast<float4*>(a.x + g * PR_D + 4 * lane) = v;
      }
      *reinterpret_cast<float4a*>(xs + row * PR_XLD + 4 * lane) = v;
    }
    __syncthreads();
  } else {
    // ---- the ctx tile (f16, as stored) into bufA: two rows per wave and step, 16 bytes per lane
    for (int row = 2 * wave + h; row < PR_ROWS; row += 8) {
      h8 c = {0, 0, 0, 0, 0, 0, 0, 0};
      if (row_T[row] > 0) c = *reinterpret_cast<const h8*>(a.ctx + (g0 + row) * PR_D + 8 * r);
      *reinterpret_cast<h8a*>(bufA + row * PR_LD + 8 * r) = c;
    }
    // ---- the FSMN sum over v (fp32 from the f16 rows, taps inside the window only) into xs
    const float* __restrict__ taps = reinterpret_cast<const float*>(a.img + a.taps_off);
    const int left = (a.kernel - 1) >> 1;
    for (int row = wave; row < PR_ROWS; row += 4) {
      const int T = row_T[row];
      const long long g = g0 + row, t = g - row_start[row];
      float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
      if (T > 0) {
        const h4 v0 = *reinterpret_cast<const h4*>(a.qkv_in + g * (3 * PR_D) + 2 * PR_D + 4 * lane);
        f = make_float4((float)v0[0], (float)v0[1], (float)v0[2], (float)v0[3]);
        for (int j = 0; j < a.kernel; ++j) {
          const long long u = t + j - left;
          if (u >= 0 && u < T) {
            const h4 vj = *reinterpret_cast<const h4*>(a.qkv_in + (g + j - left) * (3 * PR_D) + 2 * PR_D + 4 * lane);
            const float4 w4 = *reinterpret_cast<const float4*>(taps + j * PR_D + 4 * lane);
            f.x += w4.x * (float)vj[0]; f.y += w4.y * (float)vj[1]; f.z += w4.z * (float)vj[2]; f.w += w4.w * (float)vj[3];
          }
        }
      }
      *reinterpret_cast<float4a*>(xs + row * PR_XLD + 4 * lane) = f;
    }
    __syncthreads();
    // ---- x + (out(ctx) + fsmn) -> xs
    tr_product(a.img, a.out, bufA, PR_LD, wave, lane, [&](int nt, int i, const f16x& acc) {
      const int row = 32 * i + r;
      const long long g = g0 + row;
      const bool valid = row_T[row] > 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = 32 * nt + 8 * q + 4 * h;
        float4 xg = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid) xg = *reinterpret_cast<const float4*>(a.x + g * PR_D + n);
        float4 f = *reinterpret_cast<const float4a*>(xs + row * PR_XLD + n);
        f.x = xg.x + (acc[4 * q + 0] + f.x); f.y = xg.y + (acc[4 * q + 1] + f.y);
        f.z = xg.z + (acc[4 * q + 2] + f.z); f.w = xg.w + (acc[4 * q + 3] + f.w);
        *reinterpret_cast<float4a*>(xs + row * PR_XLD + n) = f;
      }
    });
    __syncthreads();
    // ---- norm2 -> bufA; the FFN in slices of 256 hidden channels: w1 slice -> ReLU -> bufB (R5) -> w2 partial sums
    pr_norm(xs, reinterpret_cast<const float*>(a.img + a.n2_g), reinterpret_cast<const float*>(a.img + a.n2_b), bufA, wave, lane);
    __syncthreads();
    const h8* __restrict__ w1t = reinterpret_cast<const h8*>(a.img + a.w1.w_off);
    const h8* __restrict__ w2t = reinterpret_cast<const h8*>(a.img + a.w2.w_off);
    const float* __restrict__ b1 = reinterpret_cast<const float*>(a.img + a.w1.b_off);
    const int KS1 = a.w1.Kpad >> 4, KS2 = a.w2.Kpad >> 4;
    f16x y[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      tr_bias(reinterpret_cast<const float*>(a.img + a.w2.b_off), wave + 4 * j, h, y[j][0]);
      y[j][1] = y[j][0];
    }
    const half_t* xa = bufA + r * PR_LD + 8 * h;
    const half_t* xb = bufB + r * PR_LD + 8 * h;
    for (int c = 0; c < (a.w1.Npad >> 8); ++c) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int nb = wave + 4 * j, nt = 8 * c + nb;
        f16x acc[2];
        tr_bias(b1, nt, h, acc[0]);
        acc[1] = acc[0];
        tr_mma(w1t + ((size_t)nt * KS1) * 64 + lane, KS1, xa, xa + 32 * PR_LD, acc[0], acc[1]);
#pragma unroll
        for (int i = 0; i < 2; ++i) tr_put_f16(acc[i], true, bufB, PR_LD, i, nb, r, h);                  // R5
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 2; ++j)
        tr_mma(w2t + ((size_t)(wave + 4 * j) * KS2 + 16 * c) * 64 + lane, 16, xb, xb + 32 * PR_LD, y[j][0], y[j][1]);
      __syncthreads();
    }
    // ---- x + ffn -> xs, and to memory where a later launch reads it
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = 32 * i + r;
        const long long g = g0 + row;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = 32 * (wave + 4 * j) + 8 * q + 4 * h;
          float4 f = *reinterpret_cast<const float4a*>(xs + row * PR_XLD + n);
          f.x += y[j][i][4 * q + 0]; f.y += y[j][i][4 * q + 1]; f.z += y[j][i][4 * q + 2]; f.w += y[j][i][4 * q + 3];
          *reinterpret_cast<float4a*>(xs + row * PR_XLD + n) = f;
          if (a.tail == 0 && row_T[row] > 0) *reinterpret_cast<float4*>(a.x + g * PR_D + n) = f;
        }
      }
    __syncthreads();
  }

  // ---- the tail: a LayerNorm of xs into bufA, then one product
  pr_norm(xs, reinterpret_cast<const float*>(a.img + a.n_g), reinterpret_cast<const float*>(a.img + a.n_b), bufA, wave, lane);
  __syncthreads();
  if (a.tail == 0) {
    // q * dh^-0.5 | k | v of the next layer, f16                                                            (R2)
    tr_product(a.img, a.last, bufA, PR_LD, wave, lane, [&](int nt, int i, const f16x& acc) {
      const int row = 32 * i + r;
      if (row_T[row] <= 0) return;
      const float sc = nt < (PR_D >> 5) ? 0.17677669529663687f : 1.f;
      half_t* dst = a.qkv_out + (g0 + row) * (3 * PR_D) + 32 * nt + 4 * h;
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
  // the decoder (one 32-row block of W: wave 0), the logits and the arg-max, ties to the larger index
  tr_product(a.img, a.last, bufA, PR_LD, wave, lane, [&](int nt, int i, const f16x& acc) {
    const int row = 32 * i + r;
    const long long g = g0 + row;
    const bool valid = row_T[row] > 0;
    float best = -INFINITY;
    int at = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = 32 * nt + 8 * q + 4 * h + e;
        if (n < a.n_punc) {
          const float v = acc[4 * q + e];
          if (v >= best) { best = v; at = n; }
          if (a.logits && valid) a.logits[g * a.n_punc + n] = v;
        }
      }
    const float ob = __shfl_xor(best, 32, 64);
    const int oat = __shfl_xor(at, 32, 64);
    if (ob > best || (ob == best && oat > at)) at = oat;
    if (h == 0 && valid && a.p) a.p[g] = at;
  });
}

// ---------------------------------------------------------------- attention: one wave per (64-query tile, head, window)
constexpr int PA_VLD = 520;                 // V^T row stride in halves: 512 keys + 8

__global__ __launch_bounds__(64) void punc_attn_kernel(PuncAttnLaunch a) {
  __shared__ __attribute__((aligned(16))) half_t vt[32 * PA_VLD];
  const int b = blockIdx.z, hd = blockIdx.y, q0 = blockIdx.x * 64;
  const long long start = a.off[b];
  const int T = (int)(a.off[b + 1] - start);
  if (q0 >= T) return;
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int nkb = (T + 31) >> 5;
  const half_t* __restrict__ base = a.qkv + start * (3 * PR_D) + hd * 32;

  // V_h^T: vt[d][key], zeros at keys in [T, 32 nkb)
  for (int key = lane; key < 32 * nkb; key += 64) {
    h8 v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[c] = h8{0, 0, 0, 0, 0, 0, 0, 0};
      if (key < T) v[c] = *reinterpret_cast<const h8*>(base + (size_t)key * (3 * PR_D) + 2 * PR_D + 8 * c);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int e = 0; e < 8; ++e) vt[(8 * c + e) * PA_VLD + key] = v[c][e];
  }
  __syncthreads();

  // Q: the B operand, lane (r, h) holds Q[query r][16 s + 8 h + j]; rows at or beyond T are clamped (never stored)
  h8 qf[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int qr = min(q0 + 32 * i + r, T - 1);
#pragma unroll
    for (int s = 0; s < 2; ++s) qf[i][s] = *reinterpret_cast<const h8*>(base + (size_t)qr * (3 * PR_D) + 16 * s + 8 * h);
  }
  auto scores = [&](int kb, f16x* S) {
    const int kr = min(32 * kb + r, T - 1);
    const half_t* kp = base + (size_t)kr * (3 * PR_D) + PR_D + 8 * h;
#pragma unroll
    for (int i = 0; i < 2; ++i) S[i] = pa_scores(kp, qf[i]);
  };
  // pass 1: the row maximum over the window's keys
  float mx[2] = {-INFINITY, -INFINITY};
  for (int kb = 0; kb < nkb; ++kb) {
    f16x S[2];
    scores(kb, S);
#pragma unroll
    for (int i = 0; i < 2; ++i) pa_max(S[i], 32 * kb + 4 * h, T, mx[i]);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) mx[i] = fmaxf(mx[i], __shfl_xor(mx[i], 32, 64));
  // pass 2: exp, the sum and O^T = V^T P^T
  float sum[2] = {0.f, 0.f};
  f16x O[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) O[i][e] = 0.f;
  for (int kb = 0; kb < nkb; ++kb) {
    f16x S[2];
    scores(kb, S);
    h8 vf[2];
    pa_vfrag(vt + r * PA_VLD + 32 * kb + 4 * h, vf);
#pragma unroll
    for (int i = 0; i < 2; ++i) pa_pv(S[i], mx[i], 32 * kb + 4 * h, T, vf, sum[i], O[i]);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float l = sum[i] + __shfl_xor(sum[i], 32, 64);
    const int qr = q0 + 32 * i + r;
    if (qr >= T) continue;
    half_t* dst = a.ctx + (start + qr) * PR_D + hd * 32 + 4 * h;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      h4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (half_t)(O[i][4 * q + e] / l);                      // R4
      *reinterpret_cast<h4*>(dst + 8 * q) = v;
    }
  }
}

// ---------------------------------------------------------------- the cut rule: one wave per window
__global__ __launch_bounds__(64) void punc_cut_kernel(PuncCutLaunch a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long start = a.off[b];
  const int n = (int)(a.off[b + 1] - start);
  int32_t* p = a.p + start;
  if (n == 0) {
    if (lane == 0) a.cut[b] = -1;
    return;
  }
  if (a.last[b]) {
    if (lane == 0) {
      const int v = p[n - 1];
      if (v == a.id_none || (a.id_comma >= 0 && v == a.id_comma) || (a.id_pause >= 0 && v == a.id_pause)) p[n - 1] = a.sentence_end_id;
      a.cut[b] = n - 1;
    }
    return;
  }
  int end = -1, comma = -1;                      // the largest index in [2, n - 2] that holds a full stop / a comma
  for (int i = 2 + lane; i <= n - 2; i += 64) {
    const int v = p[i];
    if ((a.id_period >= 0 && v == a.id_period) || (a.id_question >= 0 && v == a.id_question)) end = i;
    if (a.id_comma >= 0 && v == a.id_comma) comma = i;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    end = max(end, __shfl_xor(end, d, 64));
    comma = max(comma, __shfl_xor(comma, d, 64));
  }
  if (lane == 0) {
    int cut = end;
    const bool by_comma = cut < 0 && n > a.comma_window && comma >= 0;
    if (by_comma) cut = comma;
    if (n > a.hard_window && (cut < 0 || n - 1 - cut > a.hard_window)) cut = n - 1;      // no cut, or too long a tail behind it
    else if (by_comma) p[cut] = a.sentence_end_id;
    a.cut[b] = cut;
  }
}

void launch_punc_rows(hipStream_t s, const PuncRowsLaunch& a) {
  if (a.total <= 0 || a.B <= 0) return;
  PF_CHECK(a.img && a.off && a.x && (a.head == 0 ? a.ids != nullptr : (a.ctx != nullptr && a.qkv_in != nullptr)) &&
               (a.tail == 0 ? a.qkv_out != nullptr : (a.p != nullptr || a.logits != nullptr)),
           PF_ERR_INVALID_ARG, "punc: missing operand");
  PF_CHECK(a.last.Kpad == PR_D && (a.head == 0 || (a.out.Kpad == PR_D && a.out.Npad == PR_D && a.w1.Kpad == PR_D && a.w1.Npad % 256 == 0 &&
                                                   a.w2.Npad == PR_D && a.w2.Kpad == a.w1.Npad && a.kernel >= 1 && a.kernel % 2 == 1)) &&
               (a.tail == 0 ? a.last.Npad == 3 * PR_D : (a.last.Npad == 32 && a.n_punc >= 1 && a.n_punc <= 32)),
           PF_ERR_UNSUPPORTED, "punc: the kernel is built for d_model 256 and an FFN width that is a multiple of 256");
  static DeviceOnce once;
  once.run([] { set_max_lds((const void*)punc_rows_kernel, (int)PR_LDS_BYTES); });
  hipLaunchKernelGGL(punc_rows_kernel, dim3((unsigned)((a.total + PR_ROWS - 1) / PR_ROWS)), dim3(256), PR_LDS_BYTES, s, a);
  PF_HIP(hipGetLastError());
}

void launch_punc_attn(hipStream_t s, const PuncAttnLaunch& a) {
  if (a.B <= 0) return;
  PF_CHECK(a.qkv && a.off && a.ctx && a.B <= 65535, PF_ERR_INVALID_ARG, "punc: missing operand or more than 65535 windows");
  hipLaunchKernelGGL(punc_attn_kernel, dim3(PF_PUNC_MAX_WINDOW / 64, 8, (unsigned)a.B), dim3(64), 0, s, a);
  PF_HIP(hipGetLastError());
}

void launch_punc_cut(hipStream_t s, const PuncCutLaunch& a) {
  if (a.B <= 0) return;
  PF_CHECK(a.p && a.off && a.last && a.cut, PF_ERR_INVALID_ARG, "punc: missing operand");
  hipLaunchKernelGGL(punc_cut_kernel, dim3((unsigned)a.B), dim3(64), 0, s, a);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
