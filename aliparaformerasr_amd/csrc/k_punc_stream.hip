// k_punc_stream.hip — the CT-Transformer punctuation model in causal, stateful form (paraformer_hip.h "Punctuation, streaming",
// DESIGN.md §4.6s).  The definition in numpy float64 is tests/punc_stream_ref.py, the host twin host_punc_stream_step (punc.cpp).
//
// ONE launch per call, one workgroup of four waves per stream.  A stream whose context holds n words and now gets n_new walks
// them in tiles of at most 64 rows (and never past the context's end: max_context, or 256 without restarts) and runs every
// stage of a tile back to back:
//   head      x = fp32(embed[id]) * 16 + pe[context index] into the fp32 tile xs
//   per layer norm1 -> q | k | v (tile_rows.h): q * dh^-0.5 stays in LDS, k and v are appended to the stream's state block
//             x += v_t + sum_j taps[j] v_{t - (K - 1) + j} from the state's V rows (a tap before index 0 is skipped)
//             causal attention over the state's rows [0, n + row] (below); ctx takes q's place in LDS
//             x += out(ctx); norm2; the FFN in slices of 256 hidden channels; x += ffn          (as punc_rows_kernel, but for
//             the association of the residual: here (x + fsmn) + out(ctx), there x + (out(ctx) + fsmn); the FSMN sum has no
//             tile buffer left to wait in)
//   tail      after_norm -> decoder -> logits, arg-max (ties to the larger index)
//   the rule  the first row of the tile marked "。" / "？" ends the sentence: rows up to it are accepted, the context is emptied
//             and the rows behind it are computed again in the fresh context by the next pass (they depend on the mark).
//             Otherwise all rows are accepted and a context that now holds max_context words is emptied (forced restart).
// The state block: f16 [n_layers, 256, 2, 256] (row t of layer l: k, then v) | int32 {count, the newest word's mark, 0, 0}.
// This workgroup alone reads and writes it; a barrier lies between every store and the loads that need it.
//
// Attention: 4 rounds of two heads; V^T of the round's heads [64, 256 keys] is staged in the tile buffer norm1 left free, and
// wave w takes head 2 round + (w >> 1) and the 32-query half w & 1.  The keys are blocked from CONTEXT index 0, 32 to a block
// (punc_dev.h: two passes, a key behind the query contributes an exact zero), so a query's sums see the same blocks in the
// same order however the stream was cut into calls and tiles.  With tile_rows.h's products (a tile row's result depends on
// that row and on W alone) and a LayerNorm and FSMN sum of one row each, a word's logits, mark, k and v are bit-identical for
// every cut and for every set of streams that share the launch.  ONE EXCEPTION, for values no finite network produces: the
// exact zero of a masked key is 0 * V in the MFMA, and V of the tile's later words is staged as it is (only keys beyond the
// context are zeros).  A v that overflowed f16 (inf, or a NaN) therefore reaches the EARLIER queries of its own tile as a NaN,
// which it does not when it arrives in a later call; the float64 twin never propagates it backwards.
//
// Rounding points R0 .. R5 are k_punc.hip's.  LDS: xs fp32 [64, 260] + two f16 [64, 264] tiles + 64 marks = 134 400 bytes.
// Rows of a tile at or beyond its count are computed from a zero head and never stored.  Nothing at or beyond a stream's
// n_new is read or written; no state row beyond 255 is addressed (a tile ends where the context ends).
#include "kdev.h"
#include "kernels.h"
#include "punc_dev.h"
#include "tile_rows.h"

namespace pf {

namespace {
constexpr int PS_CTX = 256;                         // rows of a state block per layer
constexpr int PS_ROW = 2 * PR_D;                    // halves per state row: k | v
constexpr int PS_VLD = PS_CTX + 8;                  // V^T row stride in halves: 2 heads x 32 channels x 264 = one tile buffer
constexpr size_t PS_LDS_BYTES = PR_X_BYTES + 2 * PR_BUF_BYTES + PR_ROWS * 4;
static_assert((size_t)64 * PS_VLD * 2 <= PR_BUF_BYTES, "V^T of two heads fits a tile buffer");
}  // namespace

__global__ __launch_bounds__(256) void punc_stream_kernel(PuncStreamLaunch a) {
  extern __shared__ __attribute__((aligned(16))) char ps_lds[];
  float* xs = reinterpret_cast<float*>(ps_lds);
  half_t* bufA = reinterpret_cast<half_t*>(ps_lds + PR_X_BYTES);
  half_t* bufB = reinterpret_cast<half_t*>(ps_lds + PR_X_BYTES + PR_BUF_BYTES);
  int* pm = reinterpret_cast<int*>(ps_lds + PR_X_BYTES + 2 * PR_BUF_BYTES);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int b = blockIdx.x;

  char* sb = a.states + (int64_t)(a.slot ? a.slot[b] : b) * a.state_bytes;
  half_t* kv = reinterpret_cast<half_t*>(sb);
  int32_t* words = reinterpret_cast<int32_t*>(sb + a.words_off);
  int n = words[0], last = words[1];
  __syncthreads();                                                 // (thread 0 rewrites the words at the end)
  const int nn = a.n_new[b];
  const int cap_ctx = a.no_restart ? PS_CTX : a.max_context;
  const int32_t* __restrict__ ids = a.ids + (int64_t)b * a.ld;
  int32_t* marks = a.marks + (int64_t)b * a.ld;
  int32_t* mflags = a.mark_flags + (int64_t)b * a.ld;
  float* lg = a.logits ? a.logits + (int64_t)b * a.ld * a.n_punc : nullptr;
  const half_t* __restrict__ emb = reinterpret_cast<const half_t*>(a.img + a.embed_off);
  const float* __restrict__ pe = reinterpret_cast<const float*>(a.img + a.pe_off);

  int pos = 0;
  while (pos < nn) {
    int nr = nn - pos < PR_ROWS ? nn - pos : PR_ROWS;
    if (n < 0) break;                                              // (never with a state this kernel wrote: the host admits the count)
    if (nr > cap_ctx - n) nr = cap_ctx - n;
    if (nr <= 0) break;
    const int nctx = n + nr;                                       // the context's rows once the tile is appended: <= 256
    // ---- the head
    for (int row = wave; row < PR_ROWS; row += 4) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < nr) {
        const h4 e = *reinterpret_cast<const h4*>(emb + (size_t)ids[pos + row] * PR_D + 4 * lane);
        const float4 p4 = *reinterpret_cast<const float4*>(pe + (size_t)(n + row) * PR_D + 4 * lane);
        v.x = __fadd_rn(__fmul_rn((float)e[0], 16.f), p4.x); v.y = __fadd_rn(__fmul_rn((float)e[1], 16.f), p4.y);
        v.z = __fadd_rn(__fmul_rn((float)e[2], 16.f), p4.z); v.w = __fadd_rn(__fmul_rn((float)e[3], 16.f), p4.w);
      }
      *reinterpret_cast<float4a*>(xs + row * PR_XLD + 4 * lane) = v;
    }
    __syncthreads();

    for (int l = 0; l < a.n_layers; ++l) {
      half_t* kl = kv + (size_t)l * PS_CTX * PS_ROW;
      // ---- norm1 -> q * dh^-0.5 into bufB, k | v into the state rows n .. n + nr - 1                            (R1, R2)
      pr_norm(xs, reinterpret_cast<const float*>(a.img + a.n1_g[l]), reinterpret_cast<const float*>(a.img + a.n1_b[l]), bufA, wave, lane);
      __syncthreads();
      tr_product(a.img, a.qkv[l], bufA, PR_LD, wave, lane, [&](int nt, int i, const f16x& acc) {
        const int row = 32 * i + r;
        if (nt < (PR_D >> 5)) {
          half_t* dst = bufB + row * PR_LD + 32 * nt + 4 * h;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            h4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (half_t)(acc[4 * q + e] * 0.17677669529663687f);
            *reinterpret_cast<h4a*>(dst + 8 * q) = v;
          }
        } else if (row < nr) {
          half_t* dst = kl + (size_t)(n + row) * PS_ROW + (nt >= 2 * (PR_D >> 5) ? PR_D : 0) + 32 * (nt & 7) + 4 * h;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            h4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (half_t)acc[4 * q + e];
            *reinterpret_cast<h4*>(dst + 8 * q) = v;
          }
        }
      });
      __syncthreads();
      // ---- x += v_t + the FSMN sum over the state's V rows (fp32 from the f16 rows; all taps lie at or before the word)
      {
        const float* __restrict__ taps = reinterpret_cast<const float*>(a.img + a.taps[l]);
        for (int row = wave; row < nr; row += 4) {
          const int t = n + row;
          const half_t* vr = kl + (size_t)t * PS_ROW + PR_D + 4 * lane;
          const h4 v0 = *reinterpret_cast<const h4*>(vr);
          float4 f = make_float4((float)v0[0], (float)v0[1], (float)v0[2], (float)v0[3]);
          for (int j = 0; j < a.kernel; ++j) {
            const int u = t - (a.kernel - 1) + j;
            if (u >= 0) {
              const h4 vj = *reinterpret_cast<const h4*>(kl + (size_t)u * PS_ROW + PR_D + 4 * lane);
              const float4 w4 = *reinterpret_cast<const float4*>(taps + j * PR_D + 4 * lane);
              f.x += w4.x * (float)vj[0]; f.y += w4.y * (float)vj[1]; f.z += w4.z * (float)vj[2]; f.w += w4.w * (float)vj[3];
            }
          }
          float4 x4 = *reinterpret_cast<const float4a*>(xs + row * PR_XLD + 4 * lane);
          x4.x += f.x; x4.y += f.y; x4.z += f.z; x4.w += f.w;
          *reinterpret_cast<float4a*>(xs + row * PR_XLD + 4 * lane) = x4;
        }
      }
      // ---- causal attention, two heads per round; ctx replaces q in bufB                                      (R3, R4)
      const int nkb = (nctx + 31) >> 5;
      for (int rd = 0; rd < 4; ++rd) {
        if (tid < 32 * nkb) {                                      // V^T of heads 2 rd, 2 rd + 1: bufA[c][key], zeros at keys >= nctx
          const half_t* vr = kl + (size_t)tid * PS_ROW + PR_D + 64 * rd;
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (tid < nctx) v = *reinterpret_cast<const h8*>(vr + 8 * c);
#pragma unroll
            for (int e = 0; e < 8; ++e) bufA[(8 * c + e) * PS_VLD + tid] = v[e];
          }
        }
        __syncthreads();
        const int hs = wave >> 1, i = wave & 1, hd = 2 * rd + hs;
        if (32 * i < nr) {
          half_t* qrow = bufB + (32 * i + r) * PR_LD + hd * 32;
          h8 qf[2];
#pragma unroll
          for (int s = 0; s < 2; ++s) qf[s] = *reinterpret_cast<const h8a*>(qrow + 16 * s + 8 * h);
          const int t1 = n + 32 * i + r + 1, lim = t1 < nctx ? t1 : nctx;            // the keys of this lane's query: [0, lim)
          const int w1 = n + 32 * i + 32, nkw = ((w1 < nctx ? w1 : nctx) + 31) >> 5; // the blocks that hold a key of this wave
          const half_t* vtl = bufA + (hs * 32 + r) * PS_VLD + 4 * h;
          float mx = -INFINITY;
          for (int kb = 0; kb < nkw; ++kb) {
            const int kr = 32 * kb + r < nctx ? 32 * kb + r : nctx - 1;
            const f16x S = pa_scores(kl + (size_t)kr * PS_ROW + hd * 32 + 8 * h, qf);
            pa_max(S, 32 * kb + 4 * h, lim, mx);
          }
          mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
          float sum = 0.f;
          f16x O;
#pragma unroll
          for (int e = 0; e < 16; ++e) O[e] = 0.f;
          for (int kb = 0; kb < nkw; ++kb) {
            const int kr = 32 * kb + r < nctx ? 32 * kb + r : nctx - 1;
            const f16x S = pa_scores(kl + (size_t)kr * PS_ROW + hd * 32 + 8 * h, qf);
            h8 vf[2];
            pa_vfrag(vtl + 32 * kb, vf);
            pa_pv(S, mx, 32 * kb + 4 * h, lim, vf, sum, O);
          }
          const float den = sum + __shfl_xor(sum, 32, 64);
          half_t* dst = qrow + 4 * h;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            h4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (half_t)(O[4 * q + e] / den);                                 // R4
            *reinterpret_cast<h4a*>(dst + 8 * q) = v;
          }
        }
        __syncthreads();
      }
      // ---- x += out(ctx)
      tr_product(a.img, a.out[l], bufB, PR_LD, wave, lane, [&](int nt, int i, const f16x& acc) {
        const int row = 32 * i + r;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c = 32 * nt + 8 * q + 4 * h;
          float4 f = *reinterpret_cast<const float4a*>(xs + row * PR_XLD + c);
          f.x += acc[4 * q + 0]; f.y += acc[4 * q + 1]; f.z += acc[4 * q + 2]; f.w += acc[4 * q + 3];
          *reinterpret_cast<float4a*>(xs + row * PR_XLD + c) = f;
        }
      });
      __syncthreads();
      // ---- norm2 -> bufA; the FFN in slices of 256 hidden channels: w1 slice -> ReLU -> bufB (R5) -> w2 partial sums
      pr_norm(xs, reinterpret_cast<const float*>(a.img + a.n2_g[l]), reinterpret_cast<const float*>(a.img + a.n2_b[l]), bufA, wave, lane);
      __syncthreads();
      const TileGemm g1 = a.w1[l], g2 = a.w2[l];
      const h8* __restrict__ w1t = reinterpret_cast<const h8*>(a.img + g1.w_off);
      const h8* __restrict__ w2t = reinterpret_cast<const h8*>(a.img + g2.w_off);
      const float* __restrict__ b1 = reinterpret_cast<const float*>(a.img + g1.b_off);
      const int KS1 = g1.Kpad >> 4, KS2 = g2.Kpad >> 4;
      f16x y[2][2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        tr_bias(reinterpret_cast<const float*>(a.img + g2.b_off), wave + 4 * j, h, y[j][0]);
        y[j][1] = y[j][0];
      }
      const half_t* xa = bufA + r * PR_LD + 8 * h;
      const half_t* xb = bufB + r * PR_LD + 8 * h;
      for (int c = 0; c < (g1.Npad >> 8); ++c) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int nb = wave + 4 * j, nt = 8 * c + nb;
          f16x acc[2];
          tr_bias(b1, nt, h, acc[0]);
          acc[1] = acc[0];
          tr_mma(w1t + ((size_t)nt * KS1) * 64 + lane, KS1, xa, xa + 32 * PR_LD, acc[0], acc[1]);
#pragma unroll
          for (int i = 0; i < 2; ++i) tr_put_f16(acc[i], true, bufB, PR_LD, i, nb, r, h);                    // R5
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j)
          tr_mma(w2t + ((size_t)(wave + 4 * j) * KS2 + 16 * c) * 64 + lane, 16, xb, xb + 32 * PR_LD, y[j][0], y[j][1]);
        __syncthreads();
      }
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int row = 32 * i + r;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int c = 32 * (wave + 4 * j) + 8 * q + 4 * h;
            float4 f = *reinterpret_cast<const float4a*>(xs + row * PR_XLD + c);
            f.x += y[j][i][4 * q + 0]; f.y += y[j][i][4 * q + 1]; f.z += y[j][i][4 * q + 2]; f.w += y[j][i][4 * q + 3];
            *reinterpret_cast<float4a*>(xs + row * PR_XLD + c) = f;
          }
        }
      __syncthreads();
    }

    // ---- the tail: after_norm -> decoder (one 32-row block of W: wave 0) -> logits and the arg-max, ties to the larger index
    pr_norm(xs, reinterpret_cast<const float*>(a.img + a.after_g), reinterpret_cast<const float*>(a.img + a.after_b), bufA, wave, lane);
    __syncthreads();
    tr_product(a.img, a.dec, bufA, PR_LD, wave, lane, [&](int nt, int i, const f16x& acc) {
      const int row = 32 * i + r;
      const bool valid = row < nr;
      float best = -INFINITY;
      int at = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = 32 * nt + 8 * q + 4 * h + e;
          if (c < a.n_punc) {
            const float v = acc[4 * q + e];
            if (v >= best) { best = v; at = c; }
            if (lg && valid) lg[(int64_t)(pos + row) * a.n_punc + c] = v;   // (a row behind a sentence end is written again by its own pass)
          }
        }
      const float ob = __shfl_xor(best, 32, 64);
      const int oat = __shfl_xor(at, 32, 64);
      if (ob > best || (ob == best && oat > at)) at = oat;
      if (h == 0) pm[row] = at;
    });
    __syncthreads();

    // ---- the rule (every thread takes the same decisions from the marks in LDS)
    int take = nr, flag = 0;
    if (!a.no_restart) {
      for (int q = 0; q < nr; ++q) {
        const int p = pm[q];
        if (p == a.id_period || p == a.id_question) { take = q + 1; flag = 1; break; }
      }
      if (!flag && nctx == a.max_context) flag = 2;
    }
    if (tid < take) {
      marks[pos + tid] = pm[tid];
      mflags[pos + tid] = tid == take - 1 ? flag : 0;
    }
    last = pm[take - 1];
    n = flag ? 0 : n + take;
    pos += take;
    __syncthreads();
  }

  if (tid == 0) {
    int fm = -1;
    if (a.flush && a.flush[b] != 0) {                              // the offline last-window edit on the newest word, reported apart
      if (n > 0) fm = (last == a.id_none || last == a.id_comma || last == a.id_pause) ? a.sentence_end_id : last;
      n = 0;
    }
    a.flush_mark[b] = fm;
    words[0] = n;
    words[1] = n > 0 ? last : 0;
  }
}

void launch_punc_stream(hipStream_t s, const PuncStreamLaunch& a, int B) {
  if (B <= 0) return;
  PF_CHECK(a.img && a.states && a.ids && a.n_new && a.marks && a.mark_flags && a.flush_mark && a.ld >= 0, PF_ERR_INVALID_ARG,
           "punc_stream: missing operand");
  PF_CHECK(a.n_layers >= 1 && a.n_layers <= 8 && a.kernel >= 1 && a.kernel <= 31 && a.n_punc >= 1 && a.n_punc <= 32 &&
               a.max_context >= 2 && a.max_context <= PS_CTX && a.dec.Kpad == PR_D && a.dec.Npad == 32 &&
               a.words_off == (int64_t)a.n_layers * PS_CTX * PS_ROW * 2 && a.state_bytes >= a.words_off + 16 && a.state_bytes % 16 == 0,
           PF_ERR_UNSUPPORTED, "punc_stream: the kernel is built for d_model 256, up to 8 layers and a context of at most 256 words");
  for (int l = 0; l < a.n_layers; ++l)
    PF_CHECK(a.qkv[l].Kpad == PR_D && a.qkv[l].Npad == 3 * PR_D && a.out[l].Kpad == PR_D && a.out[l].Npad == PR_D && a.w1[l].Kpad == PR_D &&
                 a.w1[l].Npad % 256 == 0 && a.w2[l].Npad == PR_D && a.w2[l].Kpad == a.w1[l].Npad,
             PF_ERR_UNSUPPORTED, "punc_stream: the kernel is built for d_model 256 and an FFN width that is a multiple of 256");
  static DeviceOnce once;
  once.run([] { set_max_lds((const void*)punc_stream_kernel, (int)PS_LDS_BYTES); });
  hipLaunchKernelGGL(punc_stream_kernel, dim3((unsigned)B), dim3(256), PS_LDS_BYTES, s, a);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
