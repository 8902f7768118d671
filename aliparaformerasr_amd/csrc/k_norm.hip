// k_norm.hip — LayerNorm family (HBM-bound row kernels, one wavefront per row).
//
// Restates the LayerNormalization nodes of the FunASR ONNX graphs run by
// InferenceSession.Run (AliParaformerAsr/OfflineProjOfParaformer.cs:68): eps = 1e-12,
// statistics in fp32, two-pass (mean, then mean of squared deviations) so that the
// sentinel-padded rows (PadHelper.cs:63, |x| ~ 1.7e7 after the sqrt(512) scale) do not
// suffer E[x^2]-E[x]^2 cancellation.
//
// posenc_ln fuses the encoder prologue (x*sqrt(d_model) + sinusoidal PE, positions 1..T)
// into the first layer's norm1; the multiply and the add are kept as two separately
// rounded fp32 operations (no FMA contraction) to match a Mul node followed by an Add node.
#include "kernels.h"
#include "kdev.h"

#include <cstdlib>
#include "exact.h"

namespace pf {

#define LN_EPS 1e-12f

// NV = float4 slots per lane; row width D (multiple of 4, D/4 <= 64*NV)
template <int NV, bool POSENC>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, int64_t rows, int D,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta,
                                                        half_t* __restrict__ out16, int ld16,
                                                        float* __restrict__ out32, int ld32,
                                                        const float* __restrict__ pe, int T, float xscale) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nq = D >> 2;
  const float4* xr = reinterpret_cast<const float4*>(x + row * (int64_t)D);
  const float4* per = nullptr;
  if (POSENC) per = reinterpret_cast<const float4*>(pe + (row % T) * (int64_t)D);
  float4 v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int qd = lane + 64 * i;
    if (qd < nq) {
      float4 t = xr[qd];
      if (POSENC) {
        const float4 p = per[qd];
        t.x = add_rn(mul_rn(t.x, xscale), p.x);
        t.y = add_rn(mul_rn(t.y, xscale), p.y);
        t.z = add_rn(mul_rn(t.z, xscale), p.z);
        t.w = add_rn(mul_rn(t.w, xscale), p.w);
      }
      v[i] = t;
    } else {
      v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  // Shifted statistics: d = x - x0 (x0 = first element of the row).  For the sentinel rows
  // (|x| ~ 1.7e7, spread of a few ulps) x - x0 is exact, so the mean and the deviations keep
  // full precision where sum(x)/D would not.
  const float x0 = __shfl(v[0].x, 0, 64);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int qd = lane + 64 * i;
    if (qd < nq) {
      v[i].x = sub_rn(v[i].x, x0); v[i].y = sub_rn(v[i].y, x0);
      v[i].z = sub_rn(v[i].z, x0); v[i].w = sub_rn(v[i].w, x0);
      s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
  }
  const float mean = wave_sum(s) / (float)D;       // mean of (x - x0)
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int qd = lane + 64 * i;
    if (qd < nq) {
      const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
      ss += (a * a + b * b) + (c * c + d * d);
    }
  }
  const float var = wave_sum(ss) / (float)D;
  const float rstd = 1.0f / sqrtf(var + LN_EPS);
  const float4* g4 = reinterpret_cast<const float4*>(gamma);
  const float4* b4 = reinterpret_cast<const float4*>(beta);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int qd = lane + 64 * i;
    if (qd < nq) {
      const float4 g = g4[qd], b = b4[qd];
      float4 y;
      y.x = (v[i].x - mean) * rstd * g.x + b.x;
      y.y = (v[i].y - mean) * rstd * g.y + b.y;
      y.z = (v[i].z - mean) * rstd * g.z + b.z;
      y.w = (v[i].w - mean) * rstd * g.w + b.w;
      if (out32) reinterpret_cast<float4*>(out32 + row * (int64_t)ld32)[qd] = y;
      if (out16) {
        h4 h = {(half_t)y.x, (half_t)y.y, (half_t)y.z, (half_t)y.w};
        reinterpret_cast<h4*>(out16 + row * (int64_t)ld16)[qd] = h;
      }
    }
  }
  // zero the K-padding columns D..ld16-1 of the f16 operand (layer 0: 560 -> 576)
  if (out16 && ld16 > D) {
    for (int c = D + lane; c < ld16; c += 64) out16[row * (int64_t)ld16 + c] = (half_t)0.f;
  }
}

// D = 512, many rows (the encoder's post-FFN LayerNorm, 16 000 rows): one wave normalises R consecutive rows with all of
// their loads requested up front (R = 2: 4 KB in flight per wave instead of 2 KB, half the wave launches: 11.0 -> 9.0 us at
// 16 000 rows; R = 4 gives nothing more).  Same shifted two-pass form and reduction as layernorm_kernel; the compiler's
// FMA contraction differs between the two kernels, so results agree to the last bit or two, not bitwise.
template <int R>
__global__ __launch_bounds__(256) void layernorm512_kernel(const float* __restrict__ x, int64_t rows,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           half_t* __restrict__ out16, int ld16, float* __restrict__ out32, int ld32,
                                                           int lo_off = 0) {
  constexpr int D = 512;
  const int lane = threadIdx.x & 63;
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * R;
  if (row0 >= rows) return;
  float4 va[R], vb[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + r < rows ? row0 + r : rows - 1;
    const float4* xr = reinterpret_cast<const float4*>(x + row * (int64_t)D);
    va[r] = xr[lane];
    vb[r] = xr[lane + 64];
  }
  const float4* g4 = reinterpret_cast<const float4*>(gamma);
  const float4* b4 = reinterpret_cast<const float4*>(beta);
  const float4 ga = g4[lane], gb = g4[lane + 64], ba = b4[lane], bb = b4[lane + 64];
  float mean[R], rstd[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const float x0 = __shfl(va[r].x, 0, 64);
    va[r].x = sub_rn(va[r].x, x0); va[r].y = sub_rn(va[r].y, x0); va[r].z = sub_rn(va[r].z, x0); va[r].w = sub_rn(va[r].w, x0);
    vb[r].x = sub_rn(vb[r].x, x0); vb[r].y = sub_rn(vb[r].y, x0); vb[r].z = sub_rn(vb[r].z, x0); vb[r].w = sub_rn(vb[r].w, x0);
    float s = 0.f;
    s += (va[r].x + va[r].y) + (va[r].z + va[r].w);
    s += (vb[r].x + vb[r].y) + (vb[r].z + vb[r].w);
    mean[r] = wave_sum(s) / (float)D;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float ss = 0.f;
    {
      const float a = va[r].x - mean[r], b = va[r].y - mean[r], c = va[r].z - mean[r], d = va[r].w - mean[r];
      ss += (a * a + b * b) + (c * c + d * d);
    }
    {
      const float a = vb[r].x - mean[r], b = vb[r].y - mean[r], c = vb[r].z - mean[r], d = vb[r].w - mean[r];
      ss += (a * a + b * b) + (c * c + d * d);
    }
    rstd[r] = 1.0f / sqrtf(wave_sum(ss) / (float)D + LN_EPS);
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + r;
    if (row >= rows) break;
    float4 ya, yb;
    ya.x = (va[r].x - mean[r]) * rstd[r] * ga.x + ba.x; ya.y = (va[r].y - mean[r]) * rstd[r] * ga.y + ba.y;
    ya.z = (va[r].z - mean[r]) * rstd[r] * ga.z + ba.z; ya.w = (va[r].w - mean[r]) * rstd[r] * ga.w + ba.w;
    yb.x = (vb[r].x - mean[r]) * rstd[r] * gb.x + bb.x; yb.y = (vb[r].y - mean[r]) * rstd[r] * gb.y + bb.y;
    yb.z = (vb[r].z - mean[r]) * rstd[r] * gb.z + bb.z; yb.w = (vb[r].w - mean[r]) * rstd[r] * gb.w + bb.w;
    if (out32) {
      reinterpret_cast<float4*>(out32 + row * (int64_t)ld32)[lane] = ya;
      reinterpret_cast<float4*>(out32 + row * (int64_t)ld32)[lane + 64] = yb;
    }
    if (out16) {
      const h4 ha = h4{(half_t)ya.x, (half_t)ya.y, (half_t)ya.z, (half_t)ya.w}, hb = h4{(half_t)yb.x, (half_t)yb.y, (half_t)yb.z, (half_t)yb.w};
      reinterpret_cast<h4*>(out16 + row * (int64_t)ld16)[lane] = ha;
      reinterpret_cast<h4*>(out16 + row * (int64_t)ld16)[lane + 64] = hb;
      if (lo_off > 0) {                     // math_mode 3: the normalised row leaves as the (hi, lo') operand pair of an x3 product
        reinterpret_cast<h4*>(out16 + row * (int64_t)ld16 + lo_off)[lane] =
            h4{(half_t)((ya.x - (float)ha[0]) * 2048.f), (half_t)((ya.y - (float)ha[1]) * 2048.f), (half_t)((ya.z - (float)ha[2]) * 2048.f),
               (half_t)((ya.w - (float)ha[3]) * 2048.f)};
        reinterpret_cast<h4*>(out16 + row * (int64_t)ld16 + lo_off)[lane + 64] =
            h4{(half_t)((yb.x - (float)hb[0]) * 2048.f), (half_t)((yb.y - (float)hb[1]) * 2048.f), (half_t)((yb.z - (float)hb[2]) * 2048.f),
               (half_t)((yb.w - (float)hb[3]) * 2048.f)};
      }
    }
  }
}

template <bool POSENC>
static void ln_dispatch(hipStream_t s, const float* x, int64_t rows, int D, const float* gamma, const float* beta,
                        half_t* out16, int ld16, float* out32, int ld32, const float* pe, int T, float xscale) {
  PF_CHECK(D % 4 == 0 && D <= 64 * 4 * 8, PF_ERR_INVALID_ARG, "layernorm: unsupported width");
  if (rows == 0) return;
  if (!POSENC && D == 512 && rows >= 4096 && (!out16 || ld16 == D)) {
    hipLaunchKernelGGL(layernorm512_kernel<2>, dim3((unsigned)((rows + 7) / 8)), dim3(256), 0, s, x, rows, gamma, beta, out16, ld16, out32, ld32);
    PF_HIP(hipGetLastError());
    return;
  }
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  const int nv = (D / 4 + 63) / 64;
#define LN_CASE(N)                                                                                         \
  case N:                                                                                                  \
    hipLaunchKernelGGL((layernorm_kernel<N, POSENC>), grid, block, 0, s, x, rows, D, gamma, beta, out16,   \
                       ld16, out32, ld32, pe, T, xscale);                                                  \
    break;
  switch (nv) {
    LN_CASE(1) LN_CASE(2) LN_CASE(3) LN_CASE(4) LN_CASE(5) LN_CASE(6) LN_CASE(7) LN_CASE(8)
    default: throw Error(PF_ERR_INVALID_ARG, "layernorm: width too large");
  }
#undef LN_CASE
  PF_HIP(hipGetLastError());
}

// LayerNorm(512) whose result leaves ONLY as the operand pair of an x3 product (math_mode 3): hi = f16(y) at out[row, 0:512],
// lo' = f16((y - hi) 2^11) at out[row, lo_off : lo_off + 512] — what launch_layernorm + launch_split_x3 produce, one pass
void launch_layernorm_pair(hipStream_t s, const float* x, int64_t rows, const float* gamma, const float* beta, half_t* out, int ldo, int lo_off) {
  PF_CHECK(ldo % 4 == 0 && lo_off % 4 == 0 && lo_off >= 512, PF_ERR_INVALID_ARG, "layernorm_pair: bad layout");
  if (rows == 0) return;
  hipLaunchKernelGGL(layernorm512_kernel<2>, dim3((unsigned)((rows + 7) / 8)), dim3(256), 0, s, x, rows, gamma, beta, out, ldo, (float*)nullptr, 0,
                     lo_off);
  PF_HIP(hipGetLastError());
}

void launch_layernorm(hipStream_t s, const float* x, int64_t rows, int D, const float* gamma, const float* beta,
                      half_t* out16, int ld16, float* out32, int ld32) {
  ln_dispatch<false>(s, x, rows, D, gamma, beta, out16, ld16, out32, ld32, nullptr, 1, 1.f);
}

// pe: device table [>=T, F] built by the engine (SinusoidalPositionEncoder, positions 1..T)
void launch_posenc_ln_tab(hipStream_t s, const float* speech, int B, int T, int F, float xscale, const float* pe,
                          const float* gamma, const float* beta, half_t* out, int ldo) {
  ln_dispatch<true>(s, speech, (int64_t)B * T, F, gamma, beta, out, ldo, nullptr, 0, pe, T, xscale);
}

// LayerNorm of an f16 row (the decoder's FFN hidden, D = 2048: written by FFN-up as f16, normalised in place) -> f16.
// NV = 8-element slots per lane; statistics in fp32, shifted two-pass as above.
template <int NV>
__global__ __launch_bounds__(256) void layernorm_f16_kernel(const half_t* __restrict__ x, int64_t rows, int D,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            half_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int no = D >> 3;
  const h8* xr = reinterpret_cast<const h8*>(x + row * (int64_t)D);
  float v[NV][8];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int o = lane + 64 * i;
    h8 t = {};
    if (o < no) t = xr[o];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[i][e] = (float)t[e];
  }
  const float x0 = __shfl(v[0][0], 0, 64);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (lane + 64 * i < no) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[i][e] -= x0;       // exact: both operands are f16 values
      s += ((v[i][0] + v[i][1]) + (v[i][2] + v[i][3])) + ((v[i][4] + v[i][5]) + (v[i][6] + v[i][7]));
    }
  }
  const float mean = wave_sum(s) / (float)D;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (lane + 64 * i < no) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { v[i][e] -= mean; ss += v[i][e] * v[i][e]; }
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)D + LN_EPS);
  h8* orow = reinterpret_cast<h8*>(out + row * (int64_t)D);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int o = lane + 64 * i;
    if (o < no) {
      const float4 ga = *reinterpret_cast<const float4*>(gamma + 8 * o), gb = *reinterpret_cast<const float4*>(gamma + 8 * o + 4);
      const float4 ba = *reinterpret_cast<const float4*>(beta + 8 * o), bb = *reinterpret_cast<const float4*>(beta + 8 * o + 4);
      h8 y;
      y[0] = (half_t)(v[i][0] * rstd * ga.x + ba.x); y[1] = (half_t)(v[i][1] * rstd * ga.y + ba.y);
      y[2] = (half_t)(v[i][2] * rstd * ga.z + ba.z); y[3] = (half_t)(v[i][3] * rstd * ga.w + ba.w);
      y[4] = (half_t)(v[i][4] * rstd * gb.x + bb.x); y[5] = (half_t)(v[i][5] * rstd * gb.y + bb.y);
      y[6] = (half_t)(v[i][6] * rstd * gb.z + bb.z); y[7] = (half_t)(v[i][7] * rstd * gb.w + bb.w);
      orow[o] = y;
    }
  }
}

void launch_layernorm_f16(hipStream_t s, const half_t* x, int64_t rows, int D, const float* gamma, const float* beta, half_t* out) {
  PF_CHECK(D % 8 == 0 && D <= 64 * 8 * 4, PF_ERR_INVALID_ARG, "layernorm_f16: unsupported width");
  if (rows == 0) return;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  const int nv = (D / 8 + 63) / 64;
  switch (nv) {
    case 1: hipLaunchKernelGGL(layernorm_f16_kernel<1>, grid, block, 0, s, x, rows, D, gamma, beta, out); break;
    case 2: hipLaunchKernelGGL(layernorm_f16_kernel<2>, grid, block, 0, s, x, rows, D, gamma, beta, out); break;
    case 3: hipLaunchKernelGGL(layernorm_f16_kernel<3>, grid, block, 0, s, x, rows, D, gamma, beta, out); break;
    default: hipLaunchKernelGGL(layernorm_f16_kernel<4>, grid, block, 0, s, x, rows, D, gamma, beta, out); break;
  }
  PF_HIP(hipGetLastError());
}

// Decoder FSMN memory + the LayerNorm that follows it (decoder layer: norm2 -> FSMN -> +x -> norm3), D = 512:
//   x[b,l,:] += (sum_j w_j * tn[l+j-left] * m + tn[l] * m) * m_l,  m = (l < token_num[b]);   xn16 = LN(x)  (every row)
// One wave per FDL_ROWS consecutive positions of one utterance; a lane owns columns 4*lane..+3 and 256+4*lane..+3, the
// K-1 halo rows are read once per FDL_ROWS outputs (register sliding window, as fsmn_dec_kernel), and the row
// statistics are the shifted two-pass form of layernorm_kernel.  Saves one launch and one fp32 read of x per layer.
#ifndef PF_FDL_ROWS
#define PF_FDL_ROWS 2
#endif
constexpr int FDL_ROWS = PF_FDL_ROWS;   // measured at M = 5344: 2 rows 14.4 us, 4 rows 16.2 us, 8 rows 18.5 us per launch
template <int K>
__global__ __launch_bounds__(256) void fsmn_dec_ln_kernel(const float* __restrict__ tn, const float* __restrict__ wT,
                                                          const int32_t* __restrict__ token_num, int B, int L,
                                                          float* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, half_t* __restrict__ out16) {
  constexpr int D = 512, left = (K - 1) / 2;
  const int lane = threadIdx.x & 63;
  const int tb = (L + FDL_ROWS - 1) / FDL_ROWS;
  const int64_t wv = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wv >= (int64_t)B * tb) return;
  const int b = (int)(wv / tb), t0 = (int)(wv - (int64_t)b * tb) * FDL_ROWS;
  const int nvalid = token_num[b];
  const int c0 = 4 * lane, c1 = 256 + 4 * lane;
  const float* vb = tn + (int64_t)b * L * D;
  float4 acc[FDL_ROWS][2];
#pragma unroll
  for (int q = 0; q < FDL_ROWS; ++q) acc[q][0] = acc[q][1] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (t0 < nvalid) {                                  // a block of masked outputs adds nothing
    float4 w[K][2];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      w[j][0] = *reinterpret_cast<const float4*>(wT + (int64_t)j * D + c0);
      w[j][1] = *reinterpret_cast<const float4*>(wT + (int64_t)j * D + c1);
    }
#pragma unroll
    for (int s = 0; s < FDL_ROWS + K - 1; ++s) {
      const int tt = t0 - left + s;
      if (tt < 0 || tt >= L || tt >= nvalid) continue;
      const float4 xa = *reinterpret_cast<const float4*>(vb + (int64_t)tt * D + c0);
      const float4 xb = *reinterpret_cast<const float4*>(vb + (int64_t)tt * D + c1);
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const int q = s - j;
        if (q >= 0 && q < FDL_ROWS) {
          acc[q][0].x += w[j][0].x * xa.x; acc[q][0].y += w[j][0].y * xa.y; acc[q][0].z += w[j][0].z * xa.z; acc[q][0].w += w[j][0].w * xa.w;
          acc[q][1].x += w[j][1].x * xb.x; acc[q][1].y += w[j][1].y * xb.y; acc[q][1].z += w[j][1].z * xb.z; acc[q][1].w += w[j][1].w * xb.w;
        }
      }
      const int q0 = s - left;
      if (q0 >= 0 && q0 < FDL_ROWS) {
        acc[q0][0].x += xa.x; acc[q0][0].y += xa.y; acc[q0][0].z += xa.z; acc[q0][0].w += xa.w;
        acc[q0][1].x += xb.x; acc[q0][1].y += xb.y; acc[q0][1].z += xb.z; acc[q0][1].w += xb.w;
      }
    }
  }
  const float4 g0 = *reinterpret_cast<const float4*>(gamma + c0), g1 = *reinterpret_cast<const float4*>(gamma + c1);
  const float4 e0 = *reinterpret_cast<const float4*>(beta + c0), e1 = *reinterpret_cast<const float4*>(beta + c1);
#pragma unroll
  for (int q = 0; q < FDL_ROWS; ++q) {
    const int l = t0 + q;
    if (l >= L) break;
    float* xr = x + ((int64_t)b * L + l) * D;
    float4 a = *reinterpret_cast<const float4*>(xr + c0), c = *reinterpret_cast<const float4*>(xr + c1);
    if (l < nvalid) {
      a = make_float4(a.x + acc[q][0].x, a.y + acc[q][0].y, a.z + acc[q][0].z, a.w + acc[q][0].w);
      c = make_float4(c.x + acc[q][1].x, c.y + acc[q][1].y, c.z + acc[q][1].z, c.w + acc[q][1].w);
      *reinterpret_cast<float4*>(xr + c0) = a;
      *reinterpret_cast<float4*>(xr + c1) = c;
    }
    const float x0 = __shfl(a.x, 0, 64);
    a.x = sub_rn(a.x, x0); a.y = sub_rn(a.y, x0); a.z = sub_rn(a.z, x0); a.w = sub_rn(a.w, x0);
    c.x = sub_rn(c.x, x0); c.y = sub_rn(c.y, x0); c.z = sub_rn(c.z, x0); c.w = sub_rn(c.w, x0);
    const float mean = wave_sum(((a.x + a.y) + (a.z + a.w)) + ((c.x + c.y) + (c.z + c.w))) / (float)D;
    a.x -= mean; a.y -= mean; a.z -= mean; a.w -= mean; c.x -= mean; c.y -= mean; c.z -= mean; c.w -= mean;
    const float var = wave_sum(((a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w)) + ((c.x * c.x + c.y * c.y) + (c.z * c.z + c.w * c.w))) / (float)D;
    const float rstd = 1.0f / sqrtf(var + LN_EPS);
    half_t* orow = out16 + ((int64_t)b * L + l) * D;
    *reinterpret_cast<h4*>(orow + c0) = h4{(half_t)(a.x * rstd * g0.x + e0.x), (half_t)(a.y * rstd * g0.y + e0.y),
                                           (half_t)(a.z * rstd * g0.z + e0.z), (half_t)(a.w * rstd * g0.w + e0.w)};
    *reinterpret_cast<h4*>(orow + c1) = h4{(half_t)(c.x * rstd * g1.x + e1.x), (half_t)(c.y * rstd * g1.y + e1.y),
                                           (half_t)(c.z * rstd * g1.z + e1.z), (half_t)(c.w * rstd * g1.w + e1.w)};
  }
}

bool launch_fsmn_dec_ln(hipStream_t s, const float* tn, const float* wT, const int32_t* token_num, int B, int L, int D, int k,
                        float* x, const float* gamma, const float* beta, half_t* out16) {
  if (D != 512 || (k != 11 && k != 21)) return false;          // other geometries: the two separate kernels
  const int64_t waves = (int64_t)B * ((L + FDL_ROWS - 1) / FDL_ROWS);
  if (waves == 0) return true;
  const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
  note_gemm_kernel(k == 11 ? "fsmn_dec_ln_kernel<11>" : "fsmn_dec_ln_kernel<21>");
  if (k == 11) hipLaunchKernelGGL(fsmn_dec_ln_kernel<11>, grid, block, 0, s, tn, wT, token_num, B, L, x, gamma, beta, out16);
  else hipLaunchKernelGGL(fsmn_dec_ln_kernel<21>, grid, block, 0, s, tn, wT, token_num, B, L, x, gamma, beta, out16);
  PF_HIP(hipGetLastError());
  return true;
}

// fp32 -> f16 row copy (used for operands that arrive as fp32: stand-alone ops, CIF embeds)
__global__ void f32_to_f16_kernel(const float* __restrict__ x, int64_t rows, int cols, int ldx,
                                  half_t* __restrict__ y, int ldy) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = rows * (int64_t)ldy;
  if (i >= total) return;
  const int64_t r = i / ldy;
  const int c = (int)(i - r * ldy);
  y[i] = c < cols ? (half_t)x[r * (int64_t)ldx + c] : (half_t)0.f;
}

void launch_f32_to_f16(hipStream_t s, const float* x, int64_t rows, int cols, int ldx, half_t* y, int ldy) {
  const int64_t total = rows * (int64_t)ldy;
  if (total == 0) return;
  hipLaunchKernelGGL(f32_to_f16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, rows, cols,
                     ldx, y, ldy);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
