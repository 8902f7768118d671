// kernels.h — launchers of the gfx950 kernels (implemented in k_*.hip)
#pragma once
#include "common.h"
#include "tile_image.h"
#include "spk.h"

namespace pf {

// ---------------------------------------------------------------- GEMM ------
// C[M,N] = A[M,K] * W[N,K]^T (+ bias) ; f16 operands, f32 accumulate (MFMA 32x32x16).
// A rows must be readable up to round_up(M,128), W rows up to round_up(N,128); K is the
// padded depth (multiple of 64; pad columns of A and W hold zeros).
struct GemmArgs {
  const half_t* A; int lda;
  const half_t* W; int ldw;
  const float* bias;          // [N] or null
  int M, N, K;
  // epilogue
  float* out_f32; int ldc32;  // optional fp32 result
  half_t* out_f16; int ldc16; // optional f16 result
  const float* resid; int ldr;   // += resid[m,n] (fp32), may alias out_f32
  const float* add2; int ld2;    // += add2[m,n]  (fp32), e.g. the FSMN memory
  int relu;                      // max(v,0) after bias/resid
  int scale_cols; float scale;   // columns n < scale_cols are multiplied by scale (after bias); multiple of 64
  int out_padded;                // out_f16 has >= round_up(M,256) writable rows (enables whole-tile stores)
  // "blocked" f16 activation layout, element (m, n) of an [M, N] matrix at
  //   ((m/32 * N/8 + n/8) * 32 + m%32) * 8 + n%8      (32 rows x 8 columns = 512 contiguous bytes)
  // It is what a D^T MFMA fragment stores as whole lines WITHOUT a transposition and what the A-operand
  // LDS-DMA reads as 1 KiB contiguous pieces that land conflict-free (no swizzle).  Used for the FFN hidden:
  // FFN-up writes it (out_blocked, f16-only results, N % 64 == 0), FFN-down reads it (a_blocked, lda ignored).
  int out_blocked;
  int a_blocked;
  float* small_ws;               // scratch of the short-input kernel (k_gemm_small.hip, gemm_small_ws_bytes() bytes, one per
                                 // stream); null = never dispatch to it
  int f16_lo_off;                // > 0 (selects the fp32-kind epilogue): out_f16 receives the result as the operand pair of an
                                 // "x3" product (math_mode 3): hi = f16(v) at column n, lo' = f16((v - hi) * 2^11) at n + f16_lo_off
  // K-loop wrap (math_mode 3: the three partial products of an x3 Linear in ONE accumulation).  k_wrap > 0: after k_wrap
  // k-steps (of 64 columns) the accumulators are multiplied by wrap_scale and the operand cursors step BACK by a_wrap / w_wrap
  // columns, then the loop runs on to K / 64 steps in total:  A = [hi_x | lo'_x], W = [lo'_W | hi_W] (both 2 Kp wide),
  // K = 3 Kp, k_wrap = 2 Kp / 64, a_wrap = 2 Kp, w_wrap = Kp, wrap_scale = 2^-11  gives
  //   (hi_x lo'_W^T + lo'_x hi_W^T) 2^-11 + hi_x hi_W^T   — the small terms first, one fp32 accumulator, no intermediate in HBM.
  int k_wrap, a_wrap, w_wrap; float wrap_scale;
  int force_mi;                  // 0 = choose by shape; 1 / 2 = 128- / 256-row tiles of gemm_f16_pp3, 4 = the short-input kernel, 5 = the persistent 256 x 256 kernel (blocked result)
                                 // (stand-alone op tests; 4 / 5 fail when that kernel does not apply)
                                 // 7 = the panel-resident kernel (k_gemm_panel.hip; fails where gemm_panel_applicable is false)
  const half_t* W_panel;         // optional: launch_gemm_panel_retile image of W (K = 512): the panel-resident kernel may take the problem
};
void launch_gemm(hipStream_t s, const GemmArgs& a);
// panel-resident kernel for K = 512 (k_gemm_panel.hip): a workgroup keeps 128 rows of A in LDS and streams the weights of its
// share of N from a fragment-ordered image; bias + f16 (ldc16) or fp32 (ldc32) row-major result, rows >= M and columns >= N
// are never written; results bit-identical to gemm_f16_pp3's for the same arguments
size_t gemm_panel_image_bytes(int N);
void launch_gemm_panel_retile(hipStream_t s, const half_t* W, int ldw, int N, half_t* img);   // W [N, ldw >= 512]; pad rows of the image are zeros
bool gemm_panel_applicable(const GemmArgs& a);
int gemm_panel_min_rows();                       // rows above which launch_gemm chooses it (PF_PANEL_M)
int gemm_panel_shares(int panels, int N, int cus);
void launch_gemm_panel(hipStream_t s, const GemmArgs& a, int cus);
// name of the kernel the calling thread's most recent GEMM launcher chose (bench.py prints it next to the class it
// reports as `roofline`; the same name appears in the rocprofv3 kernel trace)
const char* last_gemm_kernel();
void note_gemm_kernel(const char* name);
// persistent 256 x 192 tile kernel for the encoder's fused Q | K | V projection (k_gemm_qkv.hip): Q (scaled) and K leave in
// the blocked layout as one [Mpad, 1024] matrix, V row-major [Mpad, ldv].  Wp / bias_p: the weight rows and bias in tile order
// (launch_qkv_permute: [1536, ldw] f16 from the [Q | K | V] weight, bias may be null -> zeros); out rows up to round_up(M, 256).
bool gemm_qkvp_applicable(int M, int K, int lda, int ldw, int ldv);
void launch_qkv_permute(hipStream_t s, const half_t* w, int ldw, const float* bias, half_t* wp, float* bp);
void launch_gemm_qkvp(hipStream_t s, const half_t* A, int lda, const half_t* Wp, int ldw, const float* bias_p, int M, int K,
                      float qscale, half_t* out_qk, half_t* out_v, int ldv);
// persistent 256 x 256 tile kernel for the blocked-layout result (FFN-up; k_gemm_big.hip)
bool gemm_bigp_applicable(const GemmArgs& a);
void launch_gemm_bigp(hipStream_t s, const GemmArgs& a, int cus);

// ---- int8 (u8 x u8 dynamic quantisation as onnxruntime's quantize_dynamic emits it; k_gemm.hip gemm_i8_pp3 + k_quant.hip)
//   y[m,n] = float( sum_k (a_q[m,k] - a_zp)(w_q[n,k] - w_zp[n]) ) * (a_scale * w_scale[n]) + bias[n]  [+ add2 + resid] [ReLU]
// The device keeps SIGNED bytes a' = a_q - 128, w' = w_q - 128 (the matrix cores multiply signed int8) plus the row /
// column sums that turn sum a' w' back into the exact integer above.
// Epilogue order: dequantise, + bias, x scale (columns n < scale_cols), + add2, + resid, ReLU, f16 round-to-nearest-even.
// Rows and columns read and written (tiles are 128 or 256 rows by 128 columns, Mpad = round_up(M, 256), Npad = round_up(N, 128)):
//   read     A rows [0, Mpad) and W rows [0, Npad), columns [0, Kpad) of both: the rows behind M - 1 / N - 1 may hold any bytes
//            (their products reach no cell of [M, N] and not the range); the columns [K, Kpad) of both hold 0;
//            aparams [0, 2); wscale, bias, colsum, wzp, dz: elements [0, N) only; resid, add2: rows [0, M), columns [0, N) only;
//            rowsum: rows [0, M) only — except the f16-result kernel (below), which reads rows [0, Mpad): what the rows behind
//            M - 1 hold reaches no cell of [M, N] and not the range;
//   written  fp32 result (out_f32, with or without out_f16 beside it) and an f16 result without dz or with out_padded = 0
//            (gemm_i8_pp3): rows [0, M), columns [0, N) of each result, nothing else;
//            f16-only result with dz and out_padded = 1 (gemm_i8f_pp3, needs ldc16 % 8 == 0, no resid / add2): rows [0, Mpad),
//            columns [0, N) — the rows behind M - 1 hold the products of the pad rows, i.e. garbage — never a column in
//            [N, ldc16) or a row at or beyond Mpad;
//            range_out (f16 results only; refused together with out_f32): all 256 {min, max} pairs, each including 0, over the
//            f16 values of rows [0, M), columns [0, N); nothing behind quant_scratch_bytes().
struct GemmI8Args {
  const int8_t* A; int lda;            // [M, Kpad] a', rows readable up to round_up(M, 256); lda (bytes) % 16 == 0
  const int8_t* W; int ldw;            // [round_up(N,128), Kpad] w', K-contiguous; pad columns of A and W hold 0
  const int32_t* rowsum;               // [M] sum_k a'
  const int32_t* colsum;               // [N] sum_k w'
  const int32_t* wzp;                  // [N] w_zp - 128
  const float* wscale;                 // [N]
  const float* aparams;                // device [2]: a_scale, a_zp (written by launch_quantize_rows)
  const float* bias;                   // [N] or null
  int M, N, K, Kpad;                   // K = true depth, Kpad = multiple of 128
  float* out_f32; int ldc32; half_t* out_f16; int ldc16;
  const float* resid; int ldr; const float* add2; int ld2;
  int relu; int scale_cols; float scale;
  // f16-only results (out_f16, nothing else) into a buffer whose rows are padded to the tile height take the deferred
  // packed epilogue when dz is given: dz[n] = (colsum[n] - K wzp[n]) * 256 + (wzp[n] & 255)  (launch_pack_dz)
  const int32_t* dz; int out_padded;
  float* range_out;                    // null, or quant_scratch_bytes(): {min, max} of the results per workgroup (pass 1 of the consumer's quantiser)
  int force_mi;                        // 0 = choose the tile height by shape; 1 / 2 = 128- / 256-row tiles (stand-alone op tests)
};
void launch_pack_dz(hipStream_t s, const int32_t* colsum, const int32_t* wzp, int N, int K, int32_t* dz);
void launch_gemm_i8(hipStream_t s, const GemmI8Args& a);
// DynamicQuantizeLinear over the WHOLE tensor x [rows, cols] (fp32, or f16 when x16 is given): min / max (including 0)
// -> a_scale = (max - min) / 255, a_zp = rne(clamp(-min / a_scale, 0, 255)); q = clamp(rne(x / a_scale) + a_zp, 0, 255);
// writes a' = q - 128 into out [rows, ld] (pad columns 0), the row sums of a', and {a_scale, a_zp} into params[2].
// scratch: quant_scratch_bytes() of device memory (one {min, max} pair per workgroup of the min / max pass).
void launch_quantize_rows(hipStream_t s, const float* x32, const half_t* x16, int64_t rows, int cols, int ldx, int8_t* out, int ld,
                          int32_t* rowsum, float* params, unsigned* scratch);
// the two passes as separate launches; part: quant_scratch_bytes() of scratch ({min, max} per workgroup of pass 1)
size_t quant_scratch_bytes();
void launch_minmax(hipStream_t s, const float* x32, const half_t* x16, int64_t rows, int cols, int ldx, float* part);
void launch_quantize(hipStream_t s, const float* x32, const half_t* x16, int64_t rows, int cols, int ldx, int8_t* out, int ld,
                     int32_t* rowsum, float* params, const float* part);
// LayerNorm(x) quantised without ever storing LayerNorm(x): pass 1 min / max, pass 2 quantise (both normalise in registers)
void launch_ln_minmax(hipStream_t s, const float* x, int64_t rows, int D, const float* gamma, const float* beta, float* part);
void launch_ln_quantize(hipStream_t s, const float* x, int64_t rows, int D, const float* gamma, const float* beta, int8_t* out, int ld,
                        int32_t* rowsum, float* params, const float* part);
// per-output-channel weight quantisation as onnxruntime.quantization quantize_dynamic(per_channel=True, weight_type=QUInt8)
// does it: row n of W [N, K] (fp32): rmin = min(0, min), rmax = max(0, max), scale = (rmax - rmin) / 255,
// zp = rne(-rmin / scale) clamped to [0, 255], q = clamp(rne(w / scale) + zp, 0, 255) -> w' = q - 128 [N, ld], colsum, wzp = zp - 128, wscale
void launch_quantize_weight(hipStream_t s, const float* W, int N, int K, int8_t* out, int ld, int32_t* colsum, int32_t* wzp, float* wscale);
void launch_import_weight(hipStream_t s, const uint8_t* Q, const uint8_t* zp, const float* scale, int N, int K, int8_t* out, int ld,
                          int32_t* colsum, int32_t* wzp, float* wscale);

// Row-complete GEMM for N = 512 (k_gemm_rc.hip): x = resid + A W^T + bias + FSMN(V); n = LayerNorm(x).
// One workgroup = 64 complete rows, so the residual add, the FSMN memory and the following LayerNorm are its epilogue.
struct GemmRcArgs {
  const half_t* A; int lda; int a_blocked;       // [M,K] f16 (row-major, or the blocked activation layout)
  const half_t* W; int ldw;                      // [512, K] f16, K-contiguous
  const float* bias;                             // [512] or null
  int M, K;
  const float* resid; int ldr;                   // fp32 [M,512] or null; may alias out_x
  float* out_x; int ldx;                         // fp32 [M,512] result x, or null when only LayerNorm(x) is kept
  const half_t* fsmn_v; int ldv;                 // f16 V slice [M, ldv] (null = no FSMN term)
  const float* fsmn_wT; int fsmn_k; int T;       // taps [k][512]; utterances are runs of T rows
  const float* ln_g; const float* ln_b; float eps;   // LayerNorm over the 512 columns (null = none)
  half_t* out_n16; int ldn16;                    // f16 LayerNorm result (next GEMM's operand) or null
  float* out_n32; int ldn32;                     // fp32 LayerNorm result or null
};
// short inputs (k_gemm_small.hip): one-shot bricks, K > 576 as split partials + a row-wise reduction that also takes
// the LayerNorm behind the GEMM; optional FSMN-memory epilogue (attention out-projection)
struct GemmSmallArgs {
  const half_t* A; int lda;                      // f16 operand [M,K]
  const half_t* W; int ldw; const float* bias;   // [N,K] f16, K-contiguous
  int M, N, K;
  float* out_f32; int ldc32; half_t* out_f16; int ldc16;
  const float* resid; int ldr; const float* add2; int ld2;           // fp32 [M,N]; resid may alias out_f32
  int relu; int scale_cols; float scale;
  const half_t* fsmn_v; int ldv; const float* fsmn_wT; int fsmn_k; int T;   // + FSMN memory of the V slice (k = 11, N = 512, K <= 576)
  const float* post_ln_g; const float* post_ln_b;                    // K > 576 only: LayerNorm of the result ->
  half_t* post_n16; int ldn16; float* post_n32; int ldn32;           //   f16 / fp32 (out_f32 / out_f16 stay optional)
  float* ws;                                     // gemm_small_ws_bytes() of scratch (K > 576), one per stream
};
size_t gemm_small_ws_bytes();
int gemm_small_max_rows();                       // rows up to which the pipeline uses this kernel (PF_SMALL_M)
bool gemm_small_applicable(const GemmSmallArgs& a);
void launch_gemm_small(hipStream_t s, const GemmSmallArgs& a);
void launch_gemm_rc(hipStream_t s, const GemmRcArgs& a);
// The encoder's whole feed-forward block in one launch (k_ffn.hip): x = resid + relu(A W1^T + b1) W2^T + b2;
// n = LayerNorm(x).  d_model 512, hidden 2048; 64-row tiles, the hidden stays in LDS, W1 / W2 are streamed from their
// fragment-ordered images (launch_ffn_retile, once per layer at load) straight into registers.
// Rows read and written (tiles are 64 rows, Mpad = round_up(M, 64)):
//   read     A and ctx rows [0, Mpad) (the rows behind M - 1 may hold anything finite or not: nothing of them reaches a row < M);
//            resid rows [0, M) only; fsmn_v rows [0, M) only (the window is clamped to them and masked at the edges of each run
//            of T rows);
//   written  out_x, out_n16, out_n32: rows [0, M), columns [0, 512), nothing else;  with the tail out_qk (blocked, 1024 columns)
//            and out_v (columns [0, 512) of row stride ldvo): rows [0, Mpad) — the rows behind M - 1 hold the projection of the
//            pad rows, i.e. garbage — never a row at or beyond Mpad.
struct FfnFusedArgs {
  const half_t* A; int lda;                      // [M,512] f16 (LayerNorm norm2 of the residual stream), rows readable up to round_up(M,64)
  const half_t* Wt;                              // ffn_fused_weight_bytes(): W1t | W2t
  const float* b1; const float* b2;              // [2048], [512]
  int M;
  const float* resid; int ldr;                   // fp32 [M,512] or null; may alias out_x
  float* out_x; int ldx;                         // fp32 [M,512] or null
  const float* ln_g; const float* ln_b; float eps;
  half_t* out_n16; int ldn16; float* out_n32; int ldn32;
  // ctx != null: the attention out-projection runs in front of the block in the same launch (A is ignored):
  //   x_mid = resid + ctx Wo^T + bo + FSMN(V) (kept on chip);  the block's operand = LayerNorm(x_mid; ln2) stays in LDS;  x = x_mid + FFN(.)
  const half_t* ctx; int lda_c;                  // attention context [M,512] f16
  const half_t* Wot; const float* bo;            // launch_ffn_retile_out image of Wo [512,512]; bias [512]
  const half_t* fsmn_v; int ldv; const float* fsmn_wT; int T;   // V slice (f16, row stride ldv), taps [11][512], utterances = runs of T rows (T >= 8)
  const float* ln2_g; const float* ln2_b;        // norm2
  // (resid may be null: the first layer)
  // Wqt != null (needs ctx and ln_g): the NEXT layer's fused Q | K | V projection of LayerNorm(x; ln_g, ln_b) behind the block,
  // same launch: Wqt = three launch_ffn_retile_out images ([Q | K | V] weight rows 0-511, 512-1023, 1024-1535), bq [1536];
  // Q (x qscale) and K -> blocked [Mpad, 1024] out_qk, V -> row-major out_v (row stride ldvo); out_n16 / out_n32 stay optional
  const half_t* Wqt; const float* bq; half_t* out_qk; half_t* out_v; int ldvo; float qscale;
};
bool ffn_fused_applicable(int D, int F);
size_t ffn_outproj_weight_bytes();
void launch_ffn_retile_out(hipStream_t s, const half_t* Wo, int ldw, half_t* Wot);
size_t ffn_fused_weight_bytes();
void launch_ffn_retile(hipStream_t s, const half_t* W1, int ldw1, const half_t* W2, int ldw2, half_t* Wt);
void launch_ffn_fused(hipStream_t s, const FfnFusedArgs& a);

// The decoder's position-wise block  t = LN_F(relu(A W1^T + b1)) W2^T  [, n = LayerNorm(t; ln_g, ln_b)]  (k_ffn.hip, split form):
// the same chunked kernel, the hidden range of a 64-row tile shared by 1 | 2 | 3 | 4 | 8 workgroups (ffn_dec_splits: the decoder
// has few rows), LN_F applied afterwards from row statistics collected on the way.  D = 512, F = 2048 only.
// Rows read and written (tiles are 64 rows, Mpad = round_up(M, 64)):
//   read     A / ctx rows [0, Mpad) (what the rows behind M - 1 hold reaches no row < M); resid rows [0, M) only;
//   written  out_x, t32, n32, n16: rows [0, M), columns [0, 512), nothing else;
//            ws: share s owns the rows [s Mpad, (s + 1) Mpad) of the partial-row block [S Mpad, 512] and of the statistics block
//            [S Mpad, 2] behind it (ffn_dec_workspace_bytes); of these the rows [0, M) of every share are written, the others
//            are the launch's to use; nothing at or beyond ffn_dec_workspace_bytes(M, splits).
struct FfnDecArgs {
  const half_t* A; int lda;                      // norm1(x) as f16 [M,512] (ignored when ctx != null)
  // ctx != null: the PREVIOUS layer's cross-attention out-projection in front of the block, same launch:
  //   x = resid + ctx Wo^T + bo -> out_x (fp32, must NOT alias resid);  the block's operand = LayerNorm(x; ln1_g, ln1_b), kept in LDS
  const half_t* ctx; int lda_c; const half_t* Wot; const float* bo;      // Wot: launch_ffn_retile_out image of Wo [512,512]
  const float* resid; int ldr; float* out_x; int ldx;
  const float* ln1_g; const float* ln1_b; float eps1;
  const half_t* img;                             // launch_ffn_dec_retile image of (W1, gamma_F (.) W2, b1, colsum, W2 beta_F)
  void* ws;                                      // ffn_dec_workspace_bytes(M)
  int M;
  int splits;                                    // 0 = ffn_dec_splits(M); 1 | 2 | 3 | 4 | 8 forces the form (ws must then hold that many)
  float eps_hidden;                              // epsilon of LN_F
  float* t32; int ldt;                           // t, fp32 [M,512] or null
  const float* ln_g; const float* ln_b; float eps;
  float* n32; int ldn32; half_t* n16; int ldn16; // LayerNorm(t) or null
  bool no_finish = false;                        // the shares stay in ws: launch_dec_mid (k_decmid.hip) finishes them
};
const float* ffn_dec_image_cd(const half_t* img);  // the (c | d) vectors of the finishing pass inside the image

// the middle of a decoder layer in one launch (k_decmid.hip, round 6): finishing pass of the split FFN + norm2 + FSMN memory +
// residual + norm3 + q-projection, on the workspace a launch_ffn_dec(no_finish) left behind
// Rows read and written (M = B L):
//   read     ws: of every share the partial rows and statistics of the positions l < min(token_num[b], L) only (a masked
//            position is a zero row of norm2's result, whatever the workspace holds there); x rows [0, M);
//   written  x: the rows with l < token_num[b], in place; every other cell keeps its bits;  q16: rows [0, M), columns [0, 512) —
//            all of them, masked positions too (norm3 and the projection run on every row) — never a column in [512, ldq) or a
//            row at or beyond M.
struct DecMidArgs {
  const void* ws; const half_t* img; int splits; float eps_hidden;   // as the FfnDecArgs of the split launch in front
  const float* n2_g; const float* n2_b; float eps2;                   // norm2
  const float* fsmn_wT; int k; const int32_t* token_num; int B, L;    // taps [k][512], token_num [B]
  float* x;                                                           // residual stream [B L, 512] fp32, updated in place
  const float* n3_g; const float* n3_b;                               // norm3
  const half_t* Wqt; const float* bq; float qscale; half_t* q16; int ldq;   // launch_ffn_retile_out image of Wq; q out f16 [B L, ldq]
};
bool launch_dec_mid(hipStream_t s, const DecMidArgs& a);              // false: geometry not covered (caller runs the three launches)
size_t ffn_dec_image_bytes();
size_t ffn_dec_workspace_bytes(int M, int splits = 0);
int ffn_dec_splits(int M);
void launch_ffn_dec_retile(hipStream_t s, const half_t* W1, int ldw1, const float* W2_f32, const float* gamma, const float* beta,
                           const float* b1, half_t* img);
void launch_ffn_dec(hipStream_t s, const FfnDecArgs& a);

// ---------------------------------------------------------------- fp32 parity mode (k_fp32.hip) ----
// C[M,N] = A[M,K] W[N,K]^T on v_mfma_f32_32x32x2_f32 (gemm_f32_kernel): fp32 operands, none truncated (a one-term product comes
// back as fl32(a w), the float64 product rounded once), fp32 accumulation in k order.  Epilogue order: + bias, x scale (columns
// n < scale_cols, any value: no multiple of 64 needed), + resid, ReLU.  Any M, N, K >= 1 and any lda, ldw >= K, ldc, ldr >= N.
//   read     A rows [0, M) and W rows [0, N), columns [0, K) of both, nothing else (no pad row, no pad column: rows behind M - 1 / N - 1
//            and the columns [K, ld) may hold anything); bias elements [0, N); resid rows [0, M), columns [0, N); resid may
//            alias out (each cell is read and written by the same lane);
//   written  out rows [0, M), columns [0, N), nothing else.
void launch_gemm_f32(hipStream_t s, const float* A, int lda, const float* W, int ldw, const float* bias, int M, int N, int K,
                     float* out, int ldc, const float* resid, int ldr, bool relu, int scale_cols, float scale);
void launch_attention_f32(hipStream_t s, const float* q, int64_t q_bs, int q_rs, const float* k, int64_t k_bs, int k_rs,
                          const float* v, int64_t v_bs, int v_rs, float* o, int64_t o_bs, int o_rs, int B, int H, int Lq, int Lk);
bool launch_attention_f32_pair(hipStream_t s, const float* q, int64_t q_bs, int q_rs, const float* k, int64_t k_bs, int k_rs,
                               const float* v, int64_t v_bs, int v_rs, half_t* pair, int64_t p_bs, int p_rs, int p_lo, int B, int H, int Lq, int Lk);
// x [rows, K] fp32 -> out [rows, 2 Kp] f16 = hi | lo' (swap: lo' | hi), hi = f16(x) (round to nearest even), lo' = f16((x - hi) * 2^11):
// x - hi and its 2^11-fold are exact in fp32, so the pair is a function of x alone, bit for bit.  Kp % 4 == 0, Kp >= K, ldo % 4 == 0,
// ldo >= 2 Kp.  Domain: finite |x| < 65520 (beyond, hi is infinite and lo' a NaN).  hi + lo'/2048 is x up to 2^-22 (1 + 2^-11) |x| for
// |x| >= 2^-14; below, hi is an f16 subnormal and lo' one as well: up to 2^-36 absolute (fp32 subnormals split into (+-0, +-0)).
//   read     x rows [0, rows), columns [0, K), nothing else;
//   written  out rows [0, rows), columns [0, 2 Kp): both halves' pad columns [K, Kp) as zeros; never a column in [2 Kp, ldo) or a row
//            at or beyond `rows`.
void launch_split_x3(hipStream_t s, const float* x, int64_t rows, int K, int ldx, half_t* out, int ldo, int Kp, int swap);
void launch_im2col_f32(hipStream_t s, const float* H, int B, int T, int D, int l_order, int r_order, float* out);
void launch_add_f32(hipStream_t s, float* x, const float* y, int64_t n);     // x += y
void launch_spin(hipStream_t s, unsigned long long cycles);                  // one wave spinning ~cycles shader clocks (queue probe)
void launch_nop(hipStream_t s);
void launch_export_plan(hipStream_t s, const int32_t* max_count, const int32_t* fire_count, const int32_t* token_num, int B, int32_t* dst_dev);
void launch_posenc_f32(hipStream_t s, const float* x, const float* pe, int B, int T, int F, float xscale, float* out);
// one LSTM time step on fp32 gate pre-activations [B, 4D] (i, f, g, o): c / h [B, D] updated in place, h also to hout
void launch_lstm_cell_f32(hipStream_t s, const float* gates, int ldg, float* c, float* h, float* hout, int64_t hout_bs, int B, int D);

// ------------------------------------------------------------- frontend -----
struct FbankTables;   // device tables (window, twiddles, mel weights)
FbankTables* fbank_tables_create(int n_mels, int fs, const char* window);
void fbank_tables_destroy(FbankTables*);
// audio: B device pointers are expressed as base + offsets; out [sum T80, n_mels]
void launch_fbank(hipStream_t s, const FbankTables* tb, const float* audio, const int64_t* audio_off,
                  const int64_t* n_samples, const int64_t* frame_off, int B, int64_t total_frames,
                  int snip_edges, float* fbank, float dither = 0.f, uint32_t dither_seed = 0);
// LFR (m,n) + CMVN + right pad + sentinel: fbank rows (per-utt offsets) -> [B,Tmax,m*80]
void launch_lfr_cmvn_pad(hipStream_t s, const float* fbank, const int64_t* frame_off, const int32_t* t80,
                         int B, int Tmax, int lfr_m, int lfr_n, int n_mels, const float* shift,
                         const float* scale, int apply_cmvn, int apply_sentinel, float* out, const float* prompt = nullptr, int P = 0);
// ragged features -> padded + sentinel (PadSequence)
void launch_pad_sentinel(hipStream_t s, const float* feats, const int64_t* feat_off, const int32_t* n_floats,
                         int B, int row_floats, float* out);

// ----------------------------------------------------------------- norms ----
// x*sqrt(d_model) + PE(pos 1..T) then LayerNorm(width F) -> f16 [M, ldo] (cols F..ldo-1 zeroed)
void launch_posenc_ln_tab(hipStream_t s, const float* speech, int B, int T, int F, float xscale, const float* pe,
                      const float* gamma, const float* beta, half_t* out, int ldo);
// LayerNorm rows of width D (512 or 2048, or generic) : fp32 in -> f16 and/or fp32 out
// D = 512; the result leaves ONLY as the (hi | lo') operand pair of an x3 product: the pair is launch_split_x3's of the fp32
// value the kernel formed (hi = f16(y), lo' = f16((y - hi) * 2^11)); ldo % 4 == 0, lo_off % 4 == 0, lo_off >= 512.
//   read     x rows [0, rows), columns [0, 512) (row stride 512); gamma, beta [0, 512);
//   written  out rows [0, rows), columns [0, 512) and [lo_off, lo_off + 512), nothing else — the columns between the halves and
//            behind them keep what they held, so a consumer with Kp > 512 pad columns must have zeroed them itself.
void launch_layernorm_pair(hipStream_t s, const float* x, int64_t rows, const float* gamma, const float* beta, half_t* out, int ldo,
                           int lo_off);
void launch_layernorm(hipStream_t s, const float* x, int64_t rows, int D, const float* gamma,
                      const float* beta, half_t* out16, int ld16, float* out32, int ld32);

// -------------------------------------------------------------- attention ---
struct AttnArgs {
  const half_t* q; int64_t q_bstride; int q_rstride;   // element strides (batch, row)
  const half_t* k; int64_t k_bstride; int k_rstride;
  const half_t* v; int64_t v_bstride; int v_rstride;
  half_t* o; int64_t o_bstride; int o_rstride;
  int B, H, Lq, Lk;                                   // head dim fixed at 128
  float* range;                                       // null, or quant_scratch_bytes(): {min, max} of the stored context per workgroup
                                                      // (pass 1 of the quantiser that consumes it, k_quant.hip); see attention_reports_range
  // Q and K handed over in ONE blocked matrix (the result of launch_gemm_qkvp): q == k == its base, `blk_groups` 8-column
  // groups per row (128), utterance b starts at row b * blk_brows, head h's Q columns are groups 16 h .., its K columns
  // groups blk_kgrp + 16 h ..; the q / k strides are ignored, V and the output stay row-major
  int qk_blocked, blk_groups, blk_brows, blk_kgrp;
  int force_nw;                                       // 0 = choose by shape; 4 / 8 = the 128- / 256-query workgroup (stand-alone op tests)
};
void launch_attention(hipStream_t s, const AttnArgs& a);
bool attention_reports_range(const AttnArgs& a);      // the launch has at most 256 workgroups (one {min, max} pair each)

// ------------------------------------------------------------------ misc ----
void launch_f32_to_f16(hipStream_t s, const float* x, int64_t rows, int cols, int ldx, half_t* y, int ldy);
// encoder FSMN: v f16 [B*T, ldv] (cols 0..D-1 used), w taps [k][D] -> f fp32 [B*T, D]: dwconv + identity; k = 3 | 5 | 7 | 9 | 11
// (PF_ERR_UNSUPPORTED otherwise, and for a D that is no multiple of 4 and of the channels per thread, or a v / ldv off the
// width of one thread's load)
// read: v rows [0, B T) x columns [0, D) only (the columns beside them and the rows behind row B T - 1 may hold anything; a
// window stops at the edges of its utterance);  written: f rows [0, B T) x [0, D), all of them; nothing behind row B T - 1
void launch_fsmn_enc(hipStream_t s, const half_t* v, int ldv, const float* w, int B, int T, int D, int k, float* f);
// decoder FSMN: x[B*L,D] += (dwconv(tn*m) + tn*m)*m ; tn fp32 [B*L,D]; valid l < token_num[b]; any k (11 and 21: the register
// window kernel, otherwise fsmn_f32_kernel<0> under the same contract)
// read: tn rows with l < min(token_num[b], L) only (a masked row may hold anything), x rows with l < min(token_num[b], L);
// written: x rows with l < min(token_num[b], L) (every other cell keeps its bits); nothing behind row B L - 1
void launch_fsmn_dec(hipStream_t s, const float* tn, const float* w, const int32_t* token_num, int B, int L,
                     int D, int k, float* x);
// LayerNorm of f16 rows -> f16 (may run in place); D % 8 == 0, D <= 2048
void launch_layernorm_f16(hipStream_t s, const half_t* x, int64_t rows, int D, const float* gamma, const float* beta, half_t* out);
// the same followed by LayerNorm(x) -> f16 (norm3): one launch; false = geometry not covered (D != 512 or k not 11/21)
// read: tn rows with l < min(token_num[b], L) only (a masked row may hold anything), x rows [0, B L);  written: x rows with
// l < token_num[b] (every other cell keeps its bits), out16 rows [0, B L) x [0, 512), all of them; nothing behind row B L - 1
bool launch_fsmn_dec_ln(hipStream_t s, const float* tn, const float* w, const int32_t* token_num, int B, int L, int D, int k,
                        float* x, const float* gamma, const float* beta, half_t* out16);
// streaming decoder FSMN (FunASR MultiHeadedAttentionSANMDecoder export with a cache): xc = cat(cache_in [B,D,K-1],
// (tn*m)^T); x[b,l,:] += (sum_j w_j * xc[l+j] + tn[l]*m) * m, m = (l < len[b]); cache_out = last K-1 columns of xc
// read: tn rows with l < min(len[b], L) only (a masked row may hold anything; it enters xc and cache_out as +0, where the
// graph's tn * 0 is -0 for a negative tn);  written: x rows with l < len[b] (every other cell keeps its bits), cache_out
// [B, D, K-1], all of it, a bitwise copy of its source columns; cache_out must not alias cache_in
void launch_fsmn_dec_stream(hipStream_t s, const float* tn, const float* wT, const int32_t* len, const float* cache_in,
                            int B, int L, int D, int k, float* x, float* cache_out);
// fp32 encoder FSMN of the V third of a fused [B T, ldv] Q | K | V result (fsmn_f32_win_kernel<11>): no mask, k = 11, ldv and D
// multiples of 4, v 16-byte aligned; y = dwconv(v) + v, fp32 [B*T, D]
// read: v rows [0, B T) x columns [0, D) only (Q and K beside them and the rows behind row B T - 1 may hold anything; the rows
// of a window beyond its utterance's edge are re-reads of the edge row, never used);  written: y rows [0, B T) x [0, D), all of
// them; nothing behind row B T - 1; v and y must not overlap
void launch_fsmn_f32_ld(hipStream_t s, const float* v, int ldv, const float* wT, int B, int T, int D, int k, float* y);
// generic fp32 FSMN (mask [B,T] floats or null, any k): y = (dwconv(v m) + v m) m over dense rows (ldv = D).  No mask and k = 11:
// launch_fsmn_f32_ld (unless force_generic: the stand-alone op comparing the two kernels); otherwise fsmn_f32_kernel<0>
// read: v rows [0, B T) x [0, D), all of them, and mask [B, T]: the mask MULTIPLIES (fractional values are allowed), so a NaN or
// Inf under a zero mask value reaches y;  written: y rows [0, B T) x [0, D), all of them; nothing behind row B T - 1;
// v == y is refused (PF_ERR_INVALID_ARG): every thread reads its neighbours' rows
void launch_fsmn_f32(hipStream_t s, const float* v, const float* w, const float* mask, int B, int T, int D,
                     int k, float* y, bool force_generic = false);
// CIF: im2col of H (f16) for the k=3 conv: [B*T, 3*D]
void launch_cif_im2col(hipStream_t s, const half_t* H, int B, int T, int D, int l_order, int r_order, half_t* out);
// alphas[b,t] = relu(sigmoid(dot(y[b,t,:], w) + b0)*smooth - noise), alphas[b,T] = tail
void launch_cif_alpha(hipStream_t s, const float* y, int B, int T, int D, const float* w, const float* b0,
                      float smooth, float noise, float tail, float* alphas);
// sequential integrate-and-fire per utterance -> fire table; then weighted gather
struct CifPlan {           // device arrays sized for B utterances
  int32_t* fire_count;     // [B]
  int32_t* token_num;      // [B]
  int32_t* fire_frame;     // [B, T1]  frame index of the l-th fire
  float* w_cur;            // [B, T1]  weight applied to frame t in the token open at t
  float* w_rem;            // [B, T1]  remainder carried into the next token when t fires
  int32_t* max_count;      // [1]
};
void launch_cif_scan(hipStream_t s, const float* alphas, int B, int T1, float threshold, CifPlan plan);
void launch_cif_gather(hipStream_t s, const float* H, int B, int T, int D, int T1, CifPlan plan, int L,
                       float* E);
// the prefix-sum CIF formulation (FunASR cif_v1_export): fire table + carried remainders, then the embeddings
void launch_cif_scan_cumsum(hipStream_t s, const float* alphas, int B, int T1, CifPlan plan);
void launch_cif_gather_cumsum(hipStream_t s, const float* H, const float* alphas, int B, int T, int D, int T1, CifPlan plan,
                              int L, float* E);
// ---------------------------------------------------- BiCIF timestamp head ----
struct LstmArgs {
  const half_t* whh;   // [2 dir][4D][D] f16, PyTorch gate order i,f,g,o
  const float* xg;     // [B*T3][2 dir * 4D] input-side gate pre-activations (+ both biases)
  half_t* hstate;      // [ndir][2 ping-pong][B][D]; the persistent launcher needs room for [ndir][4][B][D] (ring form) and initialises it
  float* cstate;       // [2 dir][B][D]
  float* hout;         // [B*T3][2D]  forward | reverse hidden states
  int B, T3, D, step;  // step s handles t = s (forward) and t = T3-1-s (reverse)
  int ndir;            // 2 = bidirectional (BiCIF head), 1 = forward only (SeACo hotword embedder)
};
void launch_lstm_step(hipStream_t s, const LstmArgs& a);
// all T3 steps in one launch (a.step ignored; hstate / cstate zeroed by the caller; cstate is not used: the cell
// state lives in registers).  sync_words: >= 64 device words ([63] = time-out flag, zeroed here).
// false = not applicable (more workgroups than CUs): use launch_lstm_step per step.
bool launch_lstm_persistent(hipStream_t s, const LstmArgs& a, unsigned* sync_words);
// the same recurrence with (hi, lo') pair operands (math_mode 3): whh = [ndir][4D][2D] pair rows, hstate [ndir][4][B][2D]
bool launch_lstm_persistent_x3(hipStream_t s, const LstmArgs& a, unsigned* sync_words);
void launch_us_alpha(hipStream_t s, const float* hout, int64_t rows, int W, const float* w, const float* b0,
                     float smooth, float noise, float* out);
void launch_us_peak(hipStream_t s, float* alphas, const int32_t* token_num, int B, int T3, float thr, float* peak);
// ------------------------------------------------------------------ SeACo ----
// rows[r, :] = table[ids[r], :]  (fp32) and its f16 copy
void launch_embed_gather(hipStream_t s, const float* table, const int32_t* ids, int rows, int D, int vocab,
                         float* out32, half_t* out16);
// out16[r, :] = f16(a[r, :] + b[r, :])
void launch_add_to_f16(hipStream_t s, const float* a, const float* b, int64_t rows, int D, half_t* out16);
// per row: keep = (first-index arg-max of dha[row, 0:V] == nobias); if !keep: ids[row] = dha_ids[row] and
// (copy_logits) logits[row, 0:V] = dha[row, 0:V]
void launch_seaco_merge(hipStream_t s, const float* dha, int ld_dha, const int64_t* dha_ids, int64_t rows, int V,
                        int nobias, int copy_logits, float* logits, int ld_logits, int64_t* ids);
// last-index arg-max over rows of width V.  mode 0: over the values as given; 1: over the log-probs
// y = (x - max) - log(sum exp(x - max)) (what the reference scans), y not stored; 2: same, y stored in place
// best_out (optional, [rows]): the value at the winning index, as mode 2 stores it (the position's confidence)
void launch_argmax(hipStream_t s, float* x, int64_t rows, int V, int ldx, int mode, int64_t* ids, float* best_out = nullptr);
// ------------------------------------------------------------------ CTC ------
// CTC collapse of per-frame ids [B, T] with their log-probs [B, T] over the first len[b] frames of each row (k_ctc.hip):
// n_out[b] tokens, and per token (arrays [B, cap], frame order) id, first / last frame and the run's largest log-prob;
// slots past n_out[b] hold -1 / -1 / -1 / 0.  A token whose slot is >= cap is counted but not stored.
void launch_ctc_collapse(hipStream_t s, const int64_t* ids, const float* score, const int32_t* len, int B, int T, int blank,
                         int cap, int32_t* n_out, int64_t* ids_out, int32_t* first_out, int32_t* last_out, float* score_out);
// ------------------------------------------------------------------ top-k ------
// The K (1 .. 8) best entries of each row of x [rows, V] (row stride ldx >= V) in the arg-max's order (k_topk.hip): larger
// value first, of equal values the larger index; NaN never ranked.  ids [rows, K] / val [rows, K]: slots past
// n[row] = min(K, non-NaN entries) hold -1 / -inf.  Every output slot is written.
void launch_topk(hipStream_t s, const float* x, int64_t rows, int V, int ldx, int K, int64_t* ids, float* val, int32_t* n);
// ------------------------------------------------------------------ CTC prefix beam search ------
// Per utterance b the N best labelings of a prefix beam search of width W over the frames t < min(max(len[b], 0), T), from
// the frames' top-k lists ids / val [B * T, K], n [B * T] (as launch_topk leaves them) and the blank log-prob
// blank_lp[(b * T + t) * blank_stride] (k_ctcbeam.hip; the definition is tests/ctcbeam_ref.py).  1 <= N <= W <= 64,
// 1 <= K <= PF_TOPK_MAX.  node_par / node_tok: workspaces of B * (T * W + 1) int32 each.  out_ids [B, N, cap] (int32; -1 past
// a hypothesis' length; a token at or beyond cap is counted but not stored), out_len [B, N] (0), out_score [B, N] float64
// (-inf), n_hyp [B]: every slot is written.  Nothing at or beyond len[b] or n[row] is read.
void launch_ctc_beam(hipStream_t s, const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val,
                     const int32_t* n, const int32_t* len, int B, int T, int K, int blank, int W, int N, int cap, int32_t* node_par,
                     int32_t* node_tok, int32_t* out_ids, int32_t* out_len, double* out_score, int32_t* n_hyp);
// The biased form (hot words; the definition is tests/ctcbeam_bias_ref.py): tok_col [V] / table [S, A] as build_hotword_graph
// leaves them (device copies), boost finite and > 0.  The hypotheses come in the biased order with score = total + boost *
// matched; out_matched [B, N] (0) and out_loglik [B, N] float64 (-inf) hold m and the unbiased total: every slot is written.
void launch_ctc_beam_hot(hipStream_t s, const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val,
                         const int32_t* n, const int32_t* len, int B, int T, int K, int blank, int W, int N, int cap,
                         int32_t* node_par, int32_t* node_tok, const int32_t* tok_col, int V, const int32_t* table, int A, float boost,
                         int32_t* out_ids, int32_t* out_len, double* out_score, int32_t* out_matched, double* out_loglik,
                         int32_t* n_hyp);
// The fused forms (language model; the definition is tests/ctcbeam_lm_ref.py): lm_image as lm_build leaves it (a device copy),
// alpha finite and >= 0, beta finite, lm_flags PF_LM_EOS or 0.  tok_col == nullptr: the model alone (table / boost / out_matched
// unused), else together with the hot-word set.  score = (total + boost * matched) + lm_sum in the re-ordered list; out_loglik
// [B, N] (-inf) the unfused total, out_lm [B, N] (0) the weighted LM score of the hypothesis: every slot is written.
void launch_ctc_beam_lm(hipStream_t s, const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val,
                        const int32_t* n, const int32_t* len, int B, int T, int K, int blank, int W, int N, int cap, int32_t* node_par,
                        int32_t* node_tok, const int32_t* tok_col, int V, const int32_t* table, int A, float boost,
                        const int32_t* lm_image, float alpha, float beta, int lm_flags, int32_t* out_ids, int32_t* out_len,
                        double* out_score, int32_t* out_matched, double* out_loglik, double* out_lm, int32_t* n_hyp);
// the model's walk on its own (k_lm.hip): ids [B, L], lens [B] -> g [B, L] float64 and state [B, L] after every token
// p < lens[b] from the start state; later positions are not written
void launch_lm_walk(hipStream_t s, const int32_t* image, const int32_t* ids, const int32_t* lens, int B, int L, float alpha, float beta,
                    double* g, int32_t* state);
// ------------------------------------------------------------------ n-best search (paraformer) ------
// Per utterance b the N best rank vectors of a position-synchronous beam search of width W over the top-k lists ids / val
// [B * L, K], n [B * L] (as launch_topk leaves them), free positions l < min(L, max(token_num[b], 0)), rank 0 behind them
// (k_nbestsearch.hip; the definition is tests/nbest_search_ref.py).  1 <= N <= W <= 64, 1 <= K <= PF_TOPK_MAX.  tok_col != nullptr:
// a hot-word set biases (tok_col [V] / table [S, A] as build_hotword_graph leaves them, boost finite and > 0); lm_image !=
// nullptr: a language model is fused (alpha finite and >= 0, beta finite, lm_eos: the end-of-sentence step at finish).  All
// device pointers.  bp: workspace of B * L * W int32.  out_ranks [B, N, L] (-1), out_score / out_loglik [B, N] float64 (-inf),
// out_lm [B, N] float64 (0), out_matched [B, N] (0), n_hyp [B]: every slot is written in every form.  Nothing at or beyond
// n[row] is read.
struct NbestSearchArgs {
  const int64_t* ids; const float* val; const int32_t* n; const int32_t* token_num;
  int L, K, W, N;
  int32_t* bp;
  const int32_t* tok_col; const int32_t* table; int V, A; double boost;
  const int32_t* lm_image; double alpha, beta; int lm_eos;
  int32_t* out_ranks; double* out_score; double* out_loglik; double* out_lm; int32_t* out_matched; int32_t* n_hyp;
};
void launch_nbest_search(hipStream_t s, const NbestSearchArgs& a, int B);
// ------------------------------------------------------------------ CTC forced alignment -------
// Per job (b, h) the best CTC alignment of the target tgt[b, h, 0 .. tlen[b, h]) to the log-prob rows lp[(b * T + t) * ld + v],
// t < min(max(len[b], 0), T), v < V, and the float64 log of the sum over all of its alignments (k_ctcalign.hip; the definition
// is tests/ctcalign_ref.py).  tlen = -1 skips the job; tlen above cap or PF_ALIGN_MAX_TOKENS and an id outside [0, V) make it
// not ok.  bp: workspace of B * H * bp_stride words, bp_stride >= ctc_align_bp_words(T, cap).  path_score / loglik / ok [B, H],
// first / last / tok_score [B, H, cap]: every slot is written (-inf / -inf / 0 and -1 / -1 / 0 for a skipped job).  Nothing at
// or beyond len[b], V or tlen is read.  B <= 65535.
size_t ctc_align_bp_words(int T, int cap);
void launch_ctc_align(hipStream_t s, const float* lp, int64_t ld, int V, const int32_t* tgt, const int32_t* tlen, const int32_t* len,
                      int B, int T, int H, int cap, uint32_t* bp, int64_t bp_stride, float* path_score, double* loglik, int32_t* ok,
                      int32_t* first, int32_t* last, float* tok_score);
// The jobs of a forward, assembled on the device: job 0 from the caller's targets c_tgt [B, c_cap] / c_len [B] (when c_len is
// given), then N jobs from the beam search's result block (b_ids [B, N, b_cap], b_len [B, N], b_nhyp [B]; hypotheses past
// b_nhyp[b] get tlen -1).  H = (c_len ? 1 : 0) + N.  tgt [B, H, cap] (-1 past a target), tlen [B, H]: every slot is written.
void launch_ctc_align_jobs(hipStream_t s, const int32_t* c_tgt, const int32_t* c_len, int c_cap, const int32_t* b_ids,
                           const int32_t* b_len, const int32_t* b_nhyp, int N, int b_cap, int B, int H, int cap, int32_t* tgt,
                           int32_t* tlen);

// ---------------------------------------------------------------- PCM intake (k_pcm.hip) ------
// One utterance of a pcm_to_samples launch: n raw values of `format` (pf_pcm_format) at raw + in_off (bytes, 16-byte aligned)
// -> n_out float samples at samples + out_off (floats, a multiple of 4).  n_mono = values after the optional down-mix;
// resample: out[i] interpolates the mono sequence at i * ratio (hostutil.h PcmPlan).
struct PcmJob { int64_t in_off, out_off, n_mono, n_out; double ratio; int32_t format, downmix, resample, reserved; };
void launch_pcm_to_samples(hipStream_t s, const PcmJob* jobs_dev, int B, int64_t max_n_out, const void* raw, float* samples);
// the same kernel for ONE utterance, its job passed in the kernel arguments (no table in device memory)
void launch_pcm_to_samples_one(hipStream_t s, const PcmJob& job, const void* raw, float* samples);

// ---------------------------------------------------------------- voice-activity segmentation (k_vad.hip) ------
// The detector of paraformer_hip.h "Voice-activity segmentation"; the definition in numpy is tests/vad_ref.py.
// Step 1: rows [T, n_mels] fp32 (row stride n_mels) -> levels [T] int32.
void launch_vad_levels(hipStream_t s, const float* rows, int64_t T, int n_mels, int32_t* levels);
// Steps 2-6 for B utterances in one launch: utterance b = T[b] levels at levels + off[b].  seg [B, cap, 2] frame pairs (only
// the first min(n[b], cap) rows are written), n [B] = the segments that exist.  cfg: validated by vad_check (hostutil.h).
struct VadParams { int32_t floor_pct, margin_q, abs_level, window, on_count, off_count, pad_begin, pad_end, min_speech, max_len,
                   split_search, n_mels; };
void launch_vad_segments(hipStream_t s, const int32_t* levels, const int64_t* off, const int32_t* T, int B, const VadParams& p,
                         int32_t* seg, int cap, int32_t* n);

// ---------------------------------------------------------------- streaming endpointing (k_endpoint.hip) ------
// The detector of paraformer_hip.h "Voice-activity endpointing, streaming"; the definition in numpy is tests/endpoint_ref.py.
// Steps 2' - 7 for B streams in one launch: stream b = its state block states [slot[b], PF_ENDPOINT_STATE_INTS] (read, then
// written; slot null: block b; the slots of a launch are distinct) and n_new[b] new levels at levels + off[b] (off null: levels
// + b * ld; nothing at or beyond n_new[b] is read), then its flush when flush[b] != 0 (flush may be null).  events [B, cap, 3] = (b, e, kind), cap >= 1: only the first min(n_events[b], cap) rows of a stream are written;
// n_events / in_speech / open_begin [B] are always written.  cfg: validated by endpoint_check (hostutil.h).
struct EndpointParams { int32_t rise, margin_q, abs_level, window, on_count, off_count, pad_begin, pad_end, end_silence, min_speech,
                        max_len, n_mels; };
void launch_endpoint_update(hipStream_t s, int32_t* states, const int32_t* slot, const int32_t* levels, const int32_t* off, int64_t ld,
                            const int32_t* n_new, const int32_t* flush, int B, const EndpointParams& p, int32_t* events, int cap, int32_t* n_events, int32_t* in_speech,
                            int32_t* open_begin);

// ---------------------------------------------------------------- the carried CIF of the streaming path (k_cif_stream.hip) ------
// The reference's streaming integrate-and-fire with the carried pair (OnlineRecognizer.cs:146-220); the host statement is
// online_cif_step (online.cpp), the definition in numpy tests/cif_stream_ref.py.  ONE launch for B streams: stream b = its state
// block at states + slot[b] * state_stride (slot null: block b; the slots of a launch are distinct; decode_blocks.h
// CifStreamBlock; read, then written) and Tc rows of enc [B, Tc, D] (dense) with alphas + b * lda.  DynamicMask happens inside:
// chunk positions < lo and >= hi walk with alpha 0.  reset[b] != 0 (reset may be null): the walk starts from a zero block.
// Written: fired [B, cap, D], ALL of it (rows at and beyond counts[b] zero), fire_entry [B, cap] (-1 at and beyond counts[b]),
// counts [B], the state block.  D % 4 == 0, cap >= Tc + 1 (a walk of Tc + 1 entries fires at most that often).
struct CifStreamLaunch {
  char* states; int64_t state_stride; const int32_t* slot;
  const float* enc; const float* alphas; int lda; const int32_t* reset;
  int B, Tc, D; float threshold; int lo, hi;
  float* fired; int32_t* fire_entry; int cap; int32_t* counts;
};
void launch_cif_stream(hipStream_t s, const CifStreamLaunch& a);
// The FSMN caches of the streaming decoder between a stream's slot and the decoder's batch.  A slot holds nd caches of DC =
// D * (k - 1) floats from byte cache_off on.  gather: cin [nd, B, DC], EVERY layer from the slot's LAYER-0 cache (stack_states,
// OnlineModel.cs:199-220), zeros where reset[b] != 0.  scatter: layer l of slot[b] = cout [l, b, :].  DC % 4 == 0.
void launch_cif_cache_gather(hipStream_t s, const char* states, int64_t state_stride, int64_t cache_off, const int32_t* slot,
                             const int32_t* reset, int B, int nd, int DC, float* cin);
void launch_cif_cache_scatter(hipStream_t s, char* states, int64_t state_stride, int64_t cache_off, const int32_t* slot, int B, int nd,
                              int DC, const float* cout);
// rows [0, L) of every stream of fired [B, cap, D] as dst [B, L, D]
void launch_cif_pack(hipStream_t s, const float* fired, int B, int cap, int L, int D, float* dst);
// `n` int32 words into pinned host memory through its device alias (as export_plan_kernel): the counts and fire entries of a step
void launch_export_words(hipStream_t s, const int32_t* src, int n, int32_t* dst_dev);

// ---------------------------------------------------------------- the FSMN-VAD model score (k_vadnet.hip) ------
// The second form of step 1 of the voice-activity segmentation; the definition in numpy is tests/vadnet_ref.py.  One launch
// of the 1 + n_layers that make a forward (the plan is at the head of k_vadnet.hip; Engine::run_vadnet fills these in).
// img: the model's device image (vadnet.h); every *_off is a byte offset into it.
struct VadNetLaunch {
  const char* img; const int64_t* off; int B; int64_t total;    // rows: `total` frames, utterance b at rows [off[b], off[b + 1])
  int ld;                                                       // LDS row stride in halves (VadModel::lds_ld)
  int head, head_w;                                             // head 0: LFR + CMVN over x; 1: the FSMN taps over p_in.  head_w: the tile's width
  const float* x; int n_mels, lfr_m, in_dim; int64_t shift_off, scale_off;
  const float* p_in; int64_t taps_off; int lorder, lstride, ldp;
  int n_mid; TileGemm mid[2]; int mid_relu[2];                   // the products whose result stays in LDS as f16
  int tail; TileGemm last;                                       // tail 0: `last` = linear_l -> p_out fp32 [total, ldp]; 1: out_linear2 -> softmax
  float* p_out;
  int64_t sil_off; int out_dim; float* logits; int32_t* levels; // logits [total, out_dim] / levels [total]: either may be null
};
size_t vadnet_lds_bytes(int ld);
void launch_vadnet(hipStream_t s, const VadNetLaunch& a);

// ---------------------------------------------------------------- the FSMN-VAD model score, streaming (k_vadnet_stream.hip) ------
// paraformer_hip.h "Voice-activity endpointing, streaming, model score"; the release schedule in Python is
// tests/vadnet_stream_ref.py.  ONE launch for B streams, one workgroup of four waves per stream: stream b = its state block
// states + slot[b] * state_bytes (read, then written; slot null: block b; the slots of a launch are distinct; the layout is
// vadnet.h VadStreamLayout) and n_new[b] new fbank rows at x + off[b] * n_mels (off null: x + b * ldx * n_mels; nothing at or
// beyond n_new[b] is read), then its flush when flush[b] != 0 (flush may be null).  levels [B, cap] int32 / logits
// [B, cap, out_dim] fp32 (either may be null): only the released ones of a stream are written, n_out[b] of them, and the
// caller has made sure that cap holds them (vad_stream_released); n_out [B] is always written.
struct VadNetStreamLaunch {
  const char* img; int ld, ldp, ldw;                            // ld: f16 tile stride (halves); ldw: stride of the fp32 p window (floats)
  int n_layers, lorder, lstride, reach;                         // reach = (lorder - 1) * lstride history rows per layer
  char* states; int64_t state_bytes, words_off; const int32_t* slot;
  const float* x; const int32_t* off; int64_t ldx; int n_mels, lfr_m, in_dim; int64_t shift_off, scale_off;
  const int32_t* n_new; const int32_t* flush;
  TileGemm in1, in2, out1, out2, lin[8], aff[8]; int64_t taps_off[8];
  int64_t sil_off; int out_dim; float* logits; int32_t* levels; int64_t cap; int32_t* n_out;
};
// the dynamic LDS of a launch: two f16 tiles and the fp32 window of (reach + 64) rows; at most kVadStreamMaxLds
constexpr size_t kVadStreamMaxLds = 156 * 1024;
size_t vadnet_stream_lds_bytes(int ld, int ldp, int reach);
void launch_vadnet_stream(hipStream_t s, const VadNetStreamLaunch& a, int B);

// ---------------------------------------------------------------- the CT-Transformer punctuation model (k_punc.hip) ------
// The definition in numpy is tests/punc_ref.py; the launch plan (2 + 2 n_layers launches per forward) is at the head of
// k_punc.hip and Engine::run_punc fills these in.  img: the model's device image (punc.h); every *_off and TileGemm offset is a
// byte offset into it.  Rows: `total` ids, window b at rows [off[b], off[b + 1]), at most PF_PUNC_MAX_WINDOW each.
struct PuncRowsLaunch {
  const char* img; const int64_t* off; int B; int64_t total;
  int head;                                                     // 0: embedding * 16 + pe -> x; 1: the layer behind its attention
  int tail;                                                     // 0: LayerNorm (n_g, n_b) + `last` = qkv -> qkv_out; 1: + `last` = decoder -> logits / p
  float* x;                                                     // the residual stream fp32 [total, 256], updated in place
  const int32_t* ids; int64_t pe_off, embed_off;                // head 0
  const half_t* ctx; const half_t* qkv_in; int64_t taps_off; int kernel; TileGemm out; int64_t n2_g, n2_b; TileGemm w1, w2;   // head 1
  int64_t n_g, n_b; TileGemm last;
  half_t* qkv_out;                                              // tail 0: f16 [total, 768], q pre-scaled by dh^-0.5
  int n_punc; float* logits; int32_t* p;                        // tail 1: logits [total, n_punc] / p [total]: either may be null
};
void launch_punc_rows(hipStream_t s, const PuncRowsLaunch& a);
struct PuncAttnLaunch { const half_t* qkv; const int64_t* off; int B; half_t* ctx; };      // ctx f16 [total, 256]
void launch_punc_attn(hipStream_t s, const PuncAttnLaunch& a);
// the cut rule of the text loop on p (edited in place): last [B] != 0 marks a text's last window; cut [B]
struct PuncCutLaunch {
  int32_t* p; const int64_t* off; const int32_t* last; int B; int32_t* cut;
  int id_none, id_comma, id_period, id_question, id_pause, sentence_end_id, comma_window, hard_window;
};
void launch_punc_cut(hipStream_t s, const PuncCutLaunch& a);

// ---------------------------------------------------------------- the punctuation model, streaming (k_punc_stream.hip) ------
// paraformer_hip.h "Punctuation, streaming"; the definition in numpy is tests/punc_stream_ref.py.  ONE launch for B streams, one
// workgroup of four waves per stream: stream b = its state block states + slot[b] * state_bytes (read, then written; slot null:
// block b; the slots of a launch are distinct; the layout is punc.h PuncStreamLayout) and n_new[b] new word ids at ids + b * ld
// (nothing at or beyond n_new[b] is read), then its flush when flush[b] != 0 (flush may be null).  marks / mark_flags [B, ld]
// int32 and logits [B, ld, n_punc] fp32 (logits may be null): only a stream's first n_new[b] are written; flush_mark [B] is
// always written.  The caller has admitted every stream (punc.h punc_stream_admit): ids inside the vocabulary, a count inside its
// context and, with no_restart, count + n_new <= 256.
struct PuncStreamLaunch {
  const char* img; int n_layers, kernel, n_punc, max_context, no_restart;
  int64_t pe_off, embed_off, n1_g[8], n1_b[8], taps[8], n2_g[8], n2_b[8], after_g, after_b;
  TileGemm qkv[8], out[8], w1[8], w2[8], dec;
  char* states; int64_t state_bytes, words_off; const int32_t* slot;
  const int32_t* ids; int64_t ld; const int32_t* n_new; const int32_t* flush;
  int id_none, id_comma, id_period, id_question, id_pause, sentence_end_id;
  int32_t* marks; int32_t* mark_flags; float* logits; int32_t* flush_mark;
};
void launch_punc_stream(hipStream_t s, const PuncStreamLaunch& a, int B);

// ---------------------------------------------------------------- the CAM++ speaker model (k_spk.hip) ------
// The definition in numpy is tests/spk_ref.py; the launch plan (15 launches per forward) is at the head of k_spk.hip and
// Engine::run_spk fills these in.  img: the model's device image (spk.h); every *_off and TileGemm offset is a byte offset into
// it.  Windows: T [B] rows each (at most PF_SPK_MAX_FRAMES), window w at input rows [toff[w], toff[w + 1]) and at output
// frames [tpoff[w], tpoff[w + 1]) (ceil(T / 2) each).  A head activation of F frequencies is f16 [(toff[w] F + f T + t) m + c].
// xoff[w]: the window's first row in the rows conv1 reads (windows may overlap there: the recogniser's windows lie in its staged fbank).
struct SpkWin { const char* img; const int32_t* T; const int64_t* toff; const int64_t* tpoff; const int64_t* xoff; int B; int Tmax; };
struct SpkConvLaunch {
  SpkWin w; SpkConvDesc d; int m, Fin, Fout, n_mels, frame_ld;
  const float* x;                                                // conv1: the fbank rows [sum T, n_mels]
  const half_t* in; const half_t* aux; half_t* out;              // aux: the shortcut's input (2 Fout frequencies) or the residual (Fout)
};
void launch_spk_conv(hipStream_t s, const SpkConvLaunch& a);
struct SpkTdnnLaunch { SpkWin w; TileGemm g; int frame_w, frame_ld, N; const half_t* frames; half_t* X; int ldx; };
void launch_spk_tdnn(hipStream_t s, const SpkTdnnLaunch& a);
struct SpkBlockLaunch {
  SpkWin w; int64_t layers_off; int n_layers, growth, bn, dilation, seg_len;
  half_t* X; int ldx;                                            // the block's concatenated activations f16 [sum T', ldx]
  int C1; int64_t tr_scale_off, tr_shift_off; TileGemm transit; half_t* Xn; int ldxn;     // the transit behind it -> the next block's X
};
void launch_spk_block(hipStream_t s, const SpkBlockLaunch& a);
struct SpkPoolLaunch {
  SpkWin w; const half_t* X; int ldx, C; int64_t scale_off, shift_off; TileGemm dense; int E;
  float* emb; float* frames;                                     // emb [B, E]; frames [sum T', C] or null
};
void launch_spk_pool(hipStream_t s, const SpkPoolLaunch& a);
// the cosine blocks of S streams: stream s holds n[s] = eoff[s + 1] - eoff[s] embeddings, its block starts at out + ooff[s]
struct SpkAffinityLaunch { const float* emb; const int64_t* eoff; const int64_t* ooff; int S, E, nmax; float* out; };
void launch_spk_affinity(hipStream_t s, const SpkAffinityLaunch& a);

}  // namespace pf
