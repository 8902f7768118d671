// engine_int8.cpp — pf_engine_config.math_mode = 2: the graph as the reference's DEFAULT model files compute it.
//
// `-accuracy int8` is the reference CLI's default (AliParaformerAsr.Examples/Program.cs:98-101 -> model.int8.onnx,
// Examples/OfflineAliParaformerAsrRecognizer.cs:17-22): FunASR exports passed through onnxruntime's quantize_dynamic,
// in which every MatMul with a constant weight runs as DynamicQuantizeLinear (per-tensor uint8 activations, computed at
// run time) + MatMulInteger (uint8 weights, per output channel) + a float rescale (k_quant.hip restates the operator
// arithmetic; oracle/int8.py is its numpy twin).  Here those products run on v_mfma_i32_32x32x32_i8 with exact int32
// accumulation (k_gemm.hip gemm_i8_pp3); everything else — LayerNorm, FSMN, attention (f16 MFMA), CIF, soft-max, arg-max
// — is the f16 path's kernels.  What is NOT quantised, as in the export: the depthwise FSMN convolutions, the CIF
// Conv1d (Conv nodes) and the N = 1 predictor output (kept fp32 here).
// Weights: a container converted from an int8 export carries the stored bytes (`<linear>.weight_q` u8, `.weight_zp` u8,
// `.weight_scale` f32, aliparaformerasr_amd/convert.py) and those are what is multiplied; a container with fp32 tensors
// only (the synthetic models) is quantised at first use on the device with quantize_dynamic's per-channel algorithm.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "engine.h"
#include "op_stage.h"

namespace pf {

static const size_t kAlignQ = 256;

void Engine::ensure_q(int64_t rows, int kpad) {
  const int64_t rp = round_up(rows, 256) + 256;
  const size_t need = (size_t)rp * kpad + (size_t)rp * 4 + 1024;
  if (!ws_q_.p || ws_q_.bytes < need || q_kpad_ < kpad || q_rows_ < rp) {
    const int64_t r2 = std::max(rp, q_rows_);
    const int k2 = std::max(kpad, q_kpad_);
    ensure(ws_q_, (size_t)r2 * k2 + (size_t)r2 * 4 + 1024);
    q_rows_ = r2; q_kpad_ = k2;
    char* b = (char*)ws_q_.p;
    q_a_ = (int8_t*)b;
    q_rowsum_ = (int32_t*)(b + round_up((int64_t)r2 * k2, (int64_t)kAlignQ));
    q_params_ = (float*)((char*)q_rowsum_ + (size_t)r2 * 4);
    q_scratch_ = (unsigned*)(q_params_ + 8);
  }
}

const QLin& Engine::qlin_raw(const float* w32, const float* bias, int N, int K) {
  auto it = qlins_.find(w32);
  if (it != qlins_.end()) return it->second;
  QLin q;
  q.N = N; q.K = K; q.Kpad = (int)round_up(K, 128);
  const size_t npad = (size_t)round_up(N, 128);
  q.w = (int8_t*)dalloc(npad * q.Kpad);
  PF_HIP(hipMemsetAsync(q.w, 0, npad * q.Kpad, stream_));
  q.colsum = (int32_t*)dalloc((size_t)(N + 8) * 4);
  q.wzp = (int32_t*)dalloc((size_t)(N + 8) * 4);
  q.wscale = (float*)dalloc((size_t)(N + 8) * 4);
  PF_HIP(hipMemsetAsync(q.colsum, 0, (size_t)(N + 8) * 4, stream_));
  PF_HIP(hipMemsetAsync(q.wzp, 0, (size_t)(N + 8) * 4, stream_));
  PF_HIP(hipMemsetAsync(q.wscale, 0, (size_t)(N + 8) * 4, stream_));
  // an int8 export's container carries the stored bytes beside the float image: multiply THOSE (no re-quantisation)
  const auto nm = lin_names_.find(w32);
  const Tensor* sq = nm == lin_names_.end() ? nullptr : tensor_u8(nm->second + ".weight_q");
  if (sq) {
    const Tensor* sz = tensor_u8(nm->second + ".weight_zp");
    const Tensor& ss = tensor(nm->second + ".weight_scale");
    PF_CHECK(sz && sq->shape.size() == 2 && sq->shape[0] == N && sq->shape[1] == K && sz->numel == N && ss.numel == N, PF_ERR_FORMAT,
             "weights: '" + nm->second + "' weight_q / weight_zp / weight_scale do not match the Linear's [N, K]");
    launch_import_weight(stream_, (const uint8_t*)sq->dev, (const uint8_t*)sz->dev, ss.dev, N, K, q.w, q.Kpad, q.colsum, q.wzp, q.wscale);
  } else {
    launch_quantize_weight(stream_, w32, N, K, q.w, q.Kpad, q.colsum, q.wzp, q.wscale);
  }
  q.dz = (int32_t*)dalloc((size_t)(N + 8) * 4);
  PF_HIP(hipMemsetAsync(q.dz, 0, (size_t)(N + 8) * 4, stream_));
  launch_pack_dz(stream_, q.colsum, q.wzp, N, K, q.dz);
  q.bias = bias;
  return qlins_.emplace(w32, q).first->second;
}

const QLin& Engine::qlin(const Lin& l, bool bias) {
  PF_CHECK(l.w32, PF_ERR_UNSUPPORTED, "int8 mode: a Linear without its fp32 tensor");
  return qlin_raw(l.w32, bias ? l.bias : nullptr, l.N, l.K);
}

void Engine::quantize_act(const QAct& dst, int kpad, const float* x32, const half_t* x16, int ldx, int64_t M, int K, const LNp* ln,
                          bool have_range) {
  if (!q_part_) q_part_ = (float*)dalloc(quant_scratch_bytes());
  prof_begin("quantize", 0);
  if (have_range) {                                    // pass 1 was the producing GEMM's epilogue
    PF_CHECK(!ln, PF_ERR_INVALID_ARG, "quantize_act: a LayerNorm input has no producer range");
    launch_quantize(stream_, x32, x16, M, K, ldx, dst.a, kpad, dst.rowsum, dst.params, q_part_);
    prof_end("quantize");
    return;
  }
  if (ln) {                                            // LayerNorm(x32) is never stored: normalised in registers by both passes
    PF_CHECK(x32 && ln->D == K && ldx == K, PF_ERR_INVALID_ARG, "quantize_act: LayerNorm rows must be dense fp32");
    launch_ln_minmax(stream_, x32, M, K, ln->g, ln->b, q_part_);
    launch_ln_quantize(stream_, x32, M, K, ln->g, ln->b, dst.a, kpad, dst.rowsum, dst.params, q_part_);
  } else {
    launch_minmax(stream_, x32, x16, M, K, ldx, q_part_);
    launch_quantize(stream_, x32, x16, M, K, ldx, dst.a, kpad, dst.rowsum, dst.params, q_part_);
  }
  prof_end("quantize");
}

// Is this Linear a DynamicQuantizeLinear + MatMulInteger pair in the model file?  A container made from an int8 export
// answers by what it carries: stored bytes (`<linear>.weight_q`) = quantised, none = the export left that MatMul in
// float (FunASR passes nodes_to_exclude to quantize_dynamic: the vocabulary projections and the N = 1 predictor outputs).
// A container with fp32 tensors only (the synthetic models) quantises everything except the names listed in its
// `int8_exclude` config key.
bool Engine::lin_quantised(const Lin& l) const {
  const auto nm = lin_names_.find(l.w32);
  if (nm == lin_names_.end()) return !any_stored_q_;
  if (any_stored_q_) return tensors_.count(nm->second + ".weight_q") != 0;
  for (const std::string& e : int8_exclude_)
    if (nm->second.compare(0, e.size(), e) == 0) return false;
  return true;
}

// a Linear the export did not quantise, inside math_mode 2: the f16 path's GEMM (A rounded to f16 as everywhere in mode 0)
void Engine::fgemm_in_int8(const char* cls, const Lin& l, bool bias, const float* x32, const half_t* x16, int ldx, int M, float* out32,
                           int ld32, half_t* out16, int ld16, const float* resid, int ldr, const float* add2, int ld2, bool relu,
                           int scale_cols, float scale, const LNp* ln, int range) {
  PF_CHECK(l.w, PF_ERR_UNSUPPORTED, "int8 mode: an un-quantised Linear without its f16 operand");
  const half_t* A = x16;
  int lda = ldx;
  if (!A) {
    PF_CHECK(x32, PF_ERR_INVALID_ARG, "int8 mode: an un-quantised Linear needs its input");
    const int64_t Mp = round_up(M, 256) + 256;
    ensure(ws_qf_, (size_t)Mp * l.Kpad * 2);
    half_t* a16 = (half_t*)ws_qf_.p;
    // the conversion writes K of Kpad columns per row: the pad columns meet zero weight columns in the GEMM, but the
    // arena is re-carved per call and a stale Inf / NaN bit pattern times zero is NaN — clear them
    if (l.K != l.Kpad) PF_HIP(hipMemsetAsync(a16, 0, (size_t)Mp * l.Kpad * 2, stream_));
    prof_begin("layernorm", 0);
    if (ln) launch_layernorm(stream_, x32, M, ln->D, ln->g, ln->b, a16, l.Kpad, nullptr, 0);
    else launch_f32_to_f16(stream_, x32, M, l.K, ldx, a16, l.Kpad);
    prof_end("layernorm");
    A = a16; lda = l.Kpad;
  }
  gemm(cls, l, A, lda, M, out32, ld32, out16, ld16, resid, ldr, add2, ld2, relu, scale_cols, scale, bias);
  if (range & kRangeOut) {                             // the consumer's quantiser expects pass 1 done
    if (!q_part_) q_part_ = (float*)dalloc(quant_scratch_bytes());
    launch_minmax(stream_, out16 ? nullptr : out32, out16, M, l.N, out16 ? ld16 : ld32, q_part_);
  }
}

void Engine::qgemm(const char* cls, const Lin& lw, bool use_bias, const float* x32, const half_t* x16, int ldx, int M, float* out32, int ld32,
                   half_t* out16, int ld16, const float* resid, int ldr, const float* add2, int ld2, bool relu, int scale_cols,
                   float scale, const LNp* ln, const QAct* pre, int range) {
  if (M == 0) return;
  if (!lin_quantised(lw)) {
    PF_CHECK(!pre, PF_ERR_UNSUPPORTED, "int8 mode: a pre-quantised input for an un-quantised Linear");
    fgemm_in_int8(cls, lw, use_bias, x32, x16, ldx, M, out32, ld32, out16, ld16, resid, ldr, add2, ld2, relu, scale_cols, scale, ln, range);
    return;
  }
  const QLin& w = qlin(lw, use_bias);
  QAct act;
  if (pre) {
    act = *pre;                                        // quantised earlier (the encoder memory: one tensor, sixteen K / V projections)
  } else {
    ensure_q(M, w.Kpad);
    act.a = q_a_; act.rowsum = q_rowsum_; act.params = q_params_;
    if (x32 || x16) quantize_act(act, w.Kpad, x32, x16, ldx, M, w.K, ln, (range & kRangeIn) != 0);   // null / null: the previous call's tensor is reused
  }
  prof_begin(cls, 2.0 * M * (double)w.N * w.K);
  GemmI8Args g{};
  g.A = act.a; g.lda = w.Kpad; g.W = w.w; g.ldw = w.Kpad;
  g.rowsum = act.rowsum; g.colsum = w.colsum; g.wzp = w.wzp; g.wscale = w.wscale; g.aparams = act.params;
  g.bias = w.bias; g.M = M; g.N = w.N; g.K = w.K; g.Kpad = w.Kpad;
  g.out_f32 = out32; g.ldc32 = ld32; g.out_f16 = out16; g.ldc16 = ld16;
  g.resid = resid; g.ldr = ldr; g.add2 = add2; g.ld2 = ld2;
  g.relu = relu ? 1 : 0; g.scale_cols = scale_cols; g.scale = scale;
  g.dz = w.dz; g.out_padded = 1;                       // every f16 result of this path lands in a buffer padded to whole tiles
  if (range & kRangeOut) {
    if (!q_part_) q_part_ = (float*)dalloc(quant_scratch_bytes());
    g.range_out = q_part_;
  }
  launch_gemm_i8(stream_, g);
  prof_end(cls);
}

void Engine::encoder_int8(const float* speech_dev, int B, int T) {
  const int D = mc_.d_model, F = mc_.ffn, Fd = mc_.feat_dim;
  const int64_t M = (int64_t)B * T, Mp = round_up(M, 128) + 128;
  const int taps = mc_.cif_l_order + mc_.cif_r_order + 1;
  const float qscale = 1.0f / std::sqrt((float)(D / mc_.heads));
  size_t off = 0;
  const Carve carve{off, kAlignQ};
  const size_t o_x = carve(Mp * D * 4), o_t = carve(Mp * std::max(Fd, D) * 4);
  const size_t o_qkv = carve(Mp * 3 * D * 2), o_ctx = carve(Mp * D * 2), o_fsm = carve(Mp * D * 4);
  const size_t o_h = carve(Mp * std::max(F, taps * D) * 2), o_H32 = carve(Mp * D * 4), o_H16 = carve(Mp * D * 2);
  const CifCarve o_cif(carve, B, T + 1);
  ensure(ws_enc_, off);
  char* base = (char*)ws_enc_.p;
  x_ = (float*)(base + o_x);
  float* t32e = (float*)(base + o_t);
  qkv16_ = (half_t*)(base + o_qkv); ctx16_ = (half_t*)(base + o_ctx); fsm_ = (float*)(base + o_fsm); h16_ = (half_t*)(base + o_h);
  H32_ = (float*)(base + o_H32); H16_ = (half_t*)(base + o_H16);
  alphas_ = (float*)(base + o_cif.al); plan_ = o_cif.plan(base);

  // ---- encoder: LayerNorm (fp32) -> quantise -> QKV (f16 out, q scaled) -> attention (f16) | FSMN(V) -> quantise(ctx) ->
  //      out-projection (+ FSMN memory + residual, fp32) -> LayerNorm -> quantise -> FFN-up + ReLU (f16) -> quantise -> FFN-down + residual
  auto layer = [&](const EncLayer& L, bool first) {
    const int din = first ? Fd : D;
    if (first) launch_posenc_f32(stream_, speech_dev, (const float*)ws_pe_.p, B, T, Fd, std::sqrt((float)D), t32e);
    qgemm("gemm_qkv", L.qkv, true, first ? t32e : x_, nullptr, din, (int)M, nullptr, 0, qkv16_, 3 * D, nullptr, 0, nullptr, 0, false, D, qscale,
          &L.norm1);
    AttnArgs a{};
    a.q = qkv16_; a.k = qkv16_ + D; a.v = qkv16_ + 2 * D; a.o = ctx16_;
    a.q_bstride = a.k_bstride = a.v_bstride = (int64_t)T * 3 * D;
    a.q_rstride = a.k_rstride = a.v_rstride = 3 * D;
    a.o_bstride = (int64_t)T * D; a.o_rstride = D;
    a.B = B; a.H = mc_.heads; a.Lq = T; a.Lk = T;
    if (!q_part_) q_part_ = (float*)dalloc(quant_scratch_bytes());
    const bool ctx_range = attention_reports_range(a);   // the context's {min, max} from the attention epilogue: no min / max pass
    a.range = ctx_range ? q_part_ : nullptr;
    prof_begin("attn_self", 4.0 * B * (double)T * T * D);
    launch_attention(stream_, a);
    prof_end("attn_self");
    prof_begin("fsmn", 0);
    launch_fsmn_enc(stream_, qkv16_ + 2 * D, 3 * D, L.fsmn_wT, B, T, D, mc_.kernel, fsm_);
    prof_end("fsmn");
    qgemm("gemm_out", L.out, true, nullptr, ctx16_, D, (int)M, x_, D, nullptr, 0, first ? nullptr : x_, D, fsm_, D, false, 0, 1.f, nullptr,
          nullptr, ctx_range ? kRangeIn : 0);
    qgemm("gemm_ffn1", L.w1, true, x_, nullptr, D, (int)M, nullptr, 0, h16_, F, nullptr, 0, nullptr, 0, true, 0, 1.f, &L.norm2, nullptr, kRangeOut);
    qgemm("gemm_ffn2", L.w2, true, nullptr, h16_, F, (int)M, x_, D, nullptr, 0, x_, D, nullptr, 0, false, 0, 1.f, nullptr, nullptr, kRangeIn);
  };
  for (size_t i = 0; i < enc_.size(); ++i) layer(enc_[i], i == 0);
  prof_begin("layernorm", 0);
  if (tp_.empty()) {
    launch_layernorm(stream_, x_, M, D, enc_after_.g, enc_after_.b, H16_, D, H32_, D);
  } else {
    launch_layernorm(stream_, x_, M, D, enc_after_.g, enc_after_.b, nullptr, 0, x_, D);
  }
  prof_end("layernorm");
  if (!tp_.empty()) {
    for (size_t i = 0; i < tp_.size(); ++i) layer(tp_[i], false);
    prof_begin("layernorm", 0);
    launch_layernorm(stream_, x_, M, D, tp_norm_.g, tp_norm_.b, H16_, D, H32_, D);
    prof_end("layernorm");
  }
}

DecStage Engine::dec_arena_int8(int B, int T, int L) {
  const int D = mc_.d_model, Md = B * L;
  const int64_t Mp = round_up((int64_t)B * T, 128) + 128;
  DecStage d;
  d.rows = round_up(Md, 128) + 128;
  d.b = carve_into(ws_dec_, kAlignQ, [&](Arena& a) {
    const DecBufs b = carve_dec8(a, d.rows, mc_.ffn);
    d.kv = a.take<half_t>((size_t)Mp * 2 * D * 2); logits_ = a.take<float>((size_t)d.rows * round_up(mc_.vocab, 4) * 4);
    ids_dev_ = a.take<int64_t>((size_t)Md * 8);
    d.qH.a = a.take<int8_t>((size_t)(Mp + 256) * round_up(D, 128)); d.qH.rowsum = a.take<int32_t>((size_t)(Mp + 256) * 4);
    d.qH.params = a.take<float>(64);
    return b;
  });
  return d;
}

void Engine::asr_decoder_int8(DecStage& d, int B, int T, int L) {
  const int D = mc_.d_model, M = B * T, Md = B * L;
  half_t* kv16 = (half_t*)d.kv;
  const QAct& qH = d.qH;
  float* t32 = d.b.t32;
  logits_ld_ = (int)round_up(mc_.vocab, 4);
  // K / V of the encoder memory: every layer's MatMul quantises the SAME tensor — one DynamicQuantizeLinear result here
  quantize_act(qH, (int)round_up(D, 128), H32_, nullptr, D, M, D, nullptr);
  DecRun r;
  r.b = d.b;
  r.B = B; r.L = L; r.token_num = plan_.token_num;
  r.kv_rs = 2 * D; r.kv_bs = (int64_t)T * 2 * D; r.Lk = T;
  r.kv_layer = [&](int i) -> const void* {
    const Lin& kv = dec_.layers[i].kv32;
    if (lin_quantised(kv))
      qgemm("gemm_dec_kv", kv, true, nullptr, nullptr, D, M, nullptr, 0, kv16, 2 * D, nullptr, 0, nullptr, 0, false, 0, 1.f, nullptr, &qH);
    else
      gemm("gemm_dec_kv", kv, H16_, D, M, nullptr, 0, kv16, 2 * D, nullptr, 0, nullptr, 0, false, 0, 1.f);
    return kv16;
  };
  decoder_int8(dec_, r);
  if (d.hid) {                                         // the bias decoder's second input: the after_norm hidden itself
    prof_begin("layernorm", 0);
    launch_layernorm(stream_, t32, Md, D, dec_.after.g, dec_.after.b, nullptr, 0, d.hid, D);
    prof_end("layernorm");
    qgemm("gemm_vocab", dec_.out, true, d.hid, nullptr, D, Md, logits_, logits_ld_, nullptr, 0, nullptr, 0, nullptr, 0, false, 0, 1.f);
  } else {
    qgemm("gemm_vocab", dec_.out, true, t32, nullptr, D, Md, logits_, logits_ld_, nullptr, 0, nullptr, 0, nullptr, 0, false, 0, 1.f, &dec_.after);
  }
}

// ---- SeACo bias branch in math_mode 2 (reference default for the flagship model: model.int8.onnx + model_eb.int8.onnx,
// Examples/OfflineAliParaformerAsrRecognizer.cs:17-21).  The hot-word embedder (Embedding + LSTM) holds no MatMul with a
// constant operand outside the LSTM nodes and stays on the f16 path; the bias decoder is the ASR decoder's structure.
// K / V rows of bias_embed [NJ, D]: every layer's MatMul quantises the same tensor (the per-tensor range of the tiled
// [B, NJ, D] input equals that of one copy), so it is quantised once.
void Engine::seaco_kv_int8(const float* hw32, const half_t* hw16, int NJ, half_t* kv16, int ldkv) {
  const int D = mc_.d_model, kp = (int)round_up(D, 128);
  const int64_t rp = round_up(NJ, 256) + 256;
  ensure(ws_seaco_q_, (size_t)rp * kp + (size_t)rp * 4 + 1024);
  QAct q;
  char* b = (char*)ws_seaco_q_.p;
  q.a = (int8_t*)b; q.rowsum = (int32_t*)(b + (size_t)rp * kp); q.params = (float*)(b + (size_t)rp * kp + (size_t)rp * 4);
  quantize_act(q, kp, hw32, nullptr, D, NJ, D, nullptr);
  for (size_t i = 0; i < bias_dec_.layers.size(); ++i) {
    const Lin& kv = bias_dec_.layers[i].kv32;
    // a [NJ, 2D] slice of the [NJ, ns * 2D] buffer: f16-only results with a row stride of ldkv
    if (lin_quantised(kv))
      qgemm("gemm_seaco", kv, true, nullptr, nullptr, D, NJ, nullptr, 0, kv16 + i * 2 * D, ldkv, nullptr, 0, nullptr, 0, false, 0, 1.f, nullptr, &q);
    else
      gemm("gemm_seaco", kv, hw16, D, NJ, nullptr, 0, kv16 + i * 2 * D, ldkv, nullptr, 0, nullptr, 0, false, 0, 1.f);
  }
}

DecBufs Engine::carve_dec8(Arena& a, int64_t rows, int F) {
  const int D = mc_.d_model;
  DecBufs d;
  d.x = a.take<float>((size_t)rows * D * 4); d.h32 = a.take<float>((size_t)rows * F * 4);
  d.t32 = a.take<float>((size_t)rows * D * 4); d.tn32 = a.take<float>((size_t)rows * D * 4);
  d.q16 = a.take<half_t>((size_t)rows * D * 2); d.ctx16 = a.take<half_t>((size_t)rows * D * 2);
  return d;
}

// The decoder stack in math_mode 2: every Linear a qgemm with the LayerNorm in front of it folded into its quantise pass;
// leaves the final block's FFN-down result in t32.
void Engine::decoder_int8(const DecStack& S, const DecRun& r) {
  const int D = mc_.d_model, F = S.ffn, R = r.B * r.L;
  const DecBufs& b = r.b;
  const float qscale = 1.0f / std::sqrt((float)(D / mc_.heads));
  if (!q_part_) q_part_ = (float*)dalloc(quant_scratch_bytes());
  auto ffn_dec = [&](const LNp& n1, const Lin& w1, const LNp& fn, const Lin& w2) {
    qgemm(r.cls_ffn1, w1, true, b.x, nullptr, D, R, b.h32, F, nullptr, 0, nullptr, 0, nullptr, 0, true, 0, 1.f, &n1);
    qgemm(r.cls_ffn2, w2, false, b.h32, nullptr, F, R, b.t32, D, nullptr, 0, nullptr, 0, nullptr, 0, false, 0, 1.f, &fn);
  };
  for (size_t i = 0; i < S.layers.size(); ++i) {
    const DecLayer& Lr = S.layers[i];
    ffn_dec(Lr.norm1, Lr.w1, Lr.ffn_norm, Lr.w2);
    prof_begin("layernorm", 0);
    launch_layernorm(stream_, b.t32, R, D, Lr.norm2.g, Lr.norm2.b, nullptr, 0, b.tn32, D);
    prof_end("layernorm");
    prof_begin("fsmn", 0);
    launch_fsmn_dec(stream_, b.tn32, Lr.fsmn_wT, r.token_num, r.B, r.L, D, S.fsmn_k, b.x);
    prof_end("fsmn");
    qgemm(r.cls_q, Lr.q, true, b.x, nullptr, D, R, nullptr, 0, b.q16, D, nullptr, 0, nullptr, 0, false, D, qscale, &Lr.norm3);
    const half_t* k16 = r.kv_layer ? (const half_t*)r.kv_layer((int)i) : (const half_t*)r.kv + i * 2 * D;
    AttnArgs a = cross_attn_args(b.q16, k16, k16 + D, r.kv_rs, r.kv_bs, b.ctx16, r.B, r.L, r.Lk);
    const bool cx_range = attention_reports_range(a);     // the context's {min, max} from the attention epilogue: no min / max pass
    a.range = cx_range ? q_part_ : nullptr;
    prof_begin(r.cls_attn, 4.0 * r.B * (double)r.L * r.Lk * D);
    launch_attention(stream_, a);
    prof_end(r.cls_attn);
    qgemm(r.cls_out, Lr.out, true, nullptr, b.ctx16, D, R, b.x, D, nullptr, 0, b.x, D, nullptr, 0, false, 0, 1.f, nullptr, nullptr,
          cx_range ? kRangeIn : 0);
  }
  ffn_dec(S.final_norm1, S.final_w1, S.final_ffn_norm, S.final_w2);
}

// stand-alone operator (parity tests): one dynamically quantised Linear, nothing cached
void Engine::op_qlinear(const float* x, const float* W, const float* bias, int M, int N, int K, int relu, int x_is_f16, float* y,
                        uint8_t* xq_out, float* aparams_out, uint8_t* wq_out, float* wscale_out, int32_t* wzp_out) {
  PF_HIP(hipSetDevice(device_));
  PF_CHECK(x && W && y && M > 0 && N > 0 && K > 0 && K % 4 == 0, PF_ERR_INVALID_ARG, "op_qlinear: bad arguments (K must be a multiple of 4)");
  const int Kp = (int)round_up(K, 128), ldy = (int)round_up(N, 4);
  const int64_t Mp = round_up(M, 256) + 256, Np = round_up(N, 128);
  // bit 1 of x_is_f16: the f16-result kernel (deferred packed epilogue + the result's range for the next quantiser)
  const bool f16_result = (x_is_f16 & 2) != 0;
  x_is_f16 &= 1;
  const int ld16 = (int)round_up(N, 8), Kq = (int)round_up(N, 128);
  const size_t scratch = quant_scratch_bytes() / 4;
  StageCarve st{0, kAlignQ};
  const auto dx = st.take<float>((size_t)M * K);
  const auto dx16 = st.take<half_t>((size_t)M * K);
  const auto dW = st.take<float>((size_t)N * K), db = st.take<float>((size_t)N + 8);
  const auto da = st.take<int8_t>((size_t)Mp * Kp);
  const auto drs = st.take<int32_t>(Mp);
  const auto dpar = st.take<float>(16);
  const auto dsc = st.take<unsigned>(scratch);
  const auto dw = st.take<int8_t>((size_t)Np * Kp);
  const auto dcs = st.take<int32_t>((size_t)N + 8), dzp = st.take<int32_t>((size_t)N + 8);
  const auto dws = st.take<float>((size_t)N + 8), dy = st.take<float>((size_t)Mp * ldy);
  const auto dy16 = st.take<half_t>((size_t)Mp * ld16);
  const auto ddz = st.take<int32_t>((size_t)N + 8);
  const auto drng = st.take<float>(scratch);
  const auto dsc2 = st.take<unsigned>(scratch);
  const auto dq2 = st.take<int8_t>((size_t)Mp * Kq);
  const auto drs2 = st.take<int32_t>(Mp);
  const auto dpa = st.take<float>(16), dpb = st.take<float>(16);
  void* ws = op_ws(st);
  upload(stream_, dx(ws), x, (size_t)M * K);
  upload(stream_, dW(ws), W, (size_t)N * K);
  if (bias) upload(stream_, db(ws), bias, N);
  PF_HIP(hipMemsetAsync(dw(ws), 0, (size_t)Np * Kp, stream_));
  PF_HIP(hipMemsetAsync(da(ws), 0, (size_t)Mp * Kp, stream_));
  launch_quantize_weight(stream_, dW(ws), N, K, dw(ws), Kp, dcs(ws), dzp(ws), dws(ws));
  if (x_is_f16) {                                      // the activation arrives as f16 (attention context, FFN hidden): exact widening
    launch_f32_to_f16(stream_, dx(ws), M, K, K, dx16(ws), K);
    launch_quantize_rows(stream_, nullptr, dx16(ws), M, K, K, da(ws), Kp, drs(ws), dpar(ws), dsc(ws));
  } else {
    launch_quantize_rows(stream_, dx(ws), nullptr, M, K, K, da(ws), Kp, drs(ws), dpar(ws), dsc(ws));
  }
  GemmI8Args g{};
  g.A = da(ws); g.lda = Kp; g.W = dw(ws); g.ldw = Kp;
  g.rowsum = drs(ws); g.colsum = dcs(ws); g.wzp = dzp(ws); g.wscale = dws(ws);
  g.aparams = dpar(ws); g.bias = bias ? db(ws) : nullptr;
  g.M = M; g.N = N; g.K = K; g.Kpad = Kp; g.relu = relu;
  float pa[2] = {0, 0}, pb[2] = {1, 1};
  if (f16_result) {
    launch_pack_dz(stream_, g.colsum, g.wzp, N, K, ddz(ws));
    g.out_f16 = dy16(ws); g.ldc16 = ld16; g.dz = ddz(ws); g.out_padded = 1; g.range_out = drng(ws);
    launch_gemm_i8(stream_, g);
    PF_CHECK(std::strncmp(last_gemm_kernel(), "gemm_i8f", 8) == 0, PF_ERR_DEVICE, "op_qlinear: the f16-result kernel was not selected");
    // the range the kernel reports must be the range a min / max pass over its output finds: quantise the output both ways
    launch_quantize(stream_, nullptr, dy16(ws), M, N, ld16, dq2(ws), Kq, drs2(ws), dpa(ws), drng(ws));
    launch_quantize_rows(stream_, nullptr, dy16(ws), M, N, ld16, dq2(ws), Kq, drs2(ws), dpb(ws), dsc2(ws));
    download(stream_, pa, (const float*)dpa(ws), 2);
    download(stream_, pb, (const float*)dpb(ws), 2);
    download_f16(stream_, y, dy16(ws), M, N, ld16);
  } else {
    g.out_f32 = dy(ws); g.ldc32 = ldy;
    launch_gemm_i8(stream_, g);
    download2d(stream_, y, N, (const float*)dy(ws), ldy, N, M);
  }
  std::vector<int8_t> aq, wq;
  std::vector<int32_t> zp((size_t)N);
  if (xq_out) { aq.resize((size_t)M * Kp); download(stream_, aq.data(), (const int8_t*)da(ws), aq.size()); }
  if (wq_out) { wq.resize((size_t)N * Kp); download(stream_, wq.data(), (const int8_t*)dw(ws), wq.size()); }
  if (aparams_out) download(stream_, aparams_out, (const float*)dpar(ws), 2);
  if (wscale_out) download(stream_, wscale_out, (const float*)dws(ws), N);
  if (wzp_out) download(stream_, zp.data(), (const int32_t*)dzp(ws), N);
  PF_HIP(hipStreamSynchronize(stream_));
  PF_CHECK(!f16_result || (pa[0] == pb[0] && pa[1] == pb[1]), PF_ERR_DEVICE,
           "op_qlinear: the range reported by the GEMM epilogue differs from a min / max pass over its output");
  if (xq_out)
    for (int m = 0; m < M; ++m)
      for (int k = 0; k < K; ++k) xq_out[(size_t)m * K + k] = (uint8_t)((int)aq[(size_t)m * Kp + k] + 128);
  if (wq_out)
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < K; ++k) wq_out[(size_t)n * K + k] = (uint8_t)((int)wq[(size_t)n * Kp + k] + 128);
  if (wzp_out)
    for (int n = 0; n < N; ++n) wzp_out[n] = zp[(size_t)n] + 128;
}

// ---- hostile hosts of the int8 path (as engine_ops.cpp's for the f16 kernels): whatever kernels.h only calls readable holds a
// pattern that shows in the result when it is used — large finite floats in pad rows, pad columns and behind a tensor, NaN
// behind the float vectors, large magnitudes behind the integer vectors, the codes +127 / -128 in the operand pad rows — and
// every output sits in a sentinel-filled buffer: a result cell must come back written, every other cell with its sentinel.
// A byte has no value a code cannot take, so the byte outputs run twice, on two sentinels: an unwritten cell holds both.
namespace {
constexpr int kTail = 136;                                    // hostile cells behind a vector (more than one wave tile of columns)
inline float quiet_nan() { return std::nanf(""); }
// `n` sentinel words of which the first `m` must come back written and the rest untouched
inline GuardGeom vector_geom(int64_t n, int64_t m) { return GuardGeom{n, 1, m, 1, m, false, true}; }
void check_bytes_written(const std::string& what, const std::vector<uint8_t>& a0, const std::vector<uint8_t>& a1, int64_t ld, int64_t M, int64_t N) {
  if (const GuardHit hit = bytes_written_scan(a0.data(), a1.data(), ld, M, N))
    throw Error(PF_ERR_DEVICE, guard_message(what, GuardGeom{M, ld, M, N, M, false, true}, hit));
}
}  // namespace

void Engine::op_quantize(const float* x, int rows, int cols, int ldx, int x_is_f16, int ld, const float* gamma, const float* beta,
                         int8_t* codes_out, int32_t* rowsum_out, float* params_out) {
  PF_HIP(hipSetDevice(device_));
  const bool ln = gamma || beta;
  PF_CHECK(x && codes_out && rowsum_out && params_out && rows > 0 && cols > 0 && cols % 4 == 0 && ldx % 4 == 0 && ldx >= cols && ld % 4 == 0 && ld >= cols,
           PF_ERR_INVALID_ARG, "op_quantize: cols, ldx and ld must be multiples of 4, ldx and ld at least cols");
  PF_CHECK(!ln || (gamma && beta && !x_is_f16 && ldx == cols), PF_ERR_INVALID_ARG, "op_quantize: LayerNorm rows are dense fp32 and need gamma and beta");
  const int64_t xr = rows + 8, orows = rows + 8;               // hostile rows behind x, guard rows behind the outputs
  const size_t part_words = quant_scratch_bytes() / 4;
  StageCarve st{0, kAlignQ};
  const auto dx = st.take<uint8_t>((size_t)xr * ldx * (x_is_f16 ? 2 : 4));     // (f16 or fp32)
  const auto dg = st.take<float>((size_t)cols + kTail), db = st.take<float>((size_t)cols + kTail);
  const auto dout = st.take<uint8_t>((size_t)orows * ld);
  const auto drs = st.take<uint32_t>(orows), dpar = st.take<uint32_t>(16), dpart = st.take<uint32_t>(part_words + 64);
  void* ws = op_ws(st);
  const float* x32 = x_is_f16 ? nullptr : (const float*)dx(ws);
  const half_t* x16 = x_is_f16 ? (const half_t*)dx(ws) : nullptr;
  // x: the tensor inside [rows, cols], the large finite pattern in the pad columns and in the rows behind it
  if (x_is_f16) {
    std::vector<half_t> h((size_t)xr * ldx);
    for (int64_t r = 0; r < xr; ++r)
      for (int c = 0; c < ldx; ++c) h[(size_t)r * ldx + c] = r < rows && c < cols ? (half_t)x[(size_t)r * cols + c] : hostile16((size_t)r * 131 + c);
    upload_sync(stream_, (half_t*)dx(ws), h);
  } else {
    std::vector<float> h((size_t)xr * ldx);
    for (int64_t r = 0; r < xr; ++r)
      for (int c = 0; c < ldx; ++c) h[(size_t)r * ldx + c] = r < rows && c < cols ? x[(size_t)r * cols + c] : hostile32((size_t)r * 131 + c);
    upload_sync(stream_, (float*)dx(ws), h);
  }
  if (ln) {
    std::vector<float> g((size_t)cols + kTail, quiet_nan()), b((size_t)cols + kTail, quiet_nan());
    std::copy(gamma, gamma + cols, g.begin());
    std::copy(beta, beta + cols, b.begin());
    upload_sync(stream_, dg(ws), g);
    upload_sync(stream_, db(ws), b);
  }
  const std::vector<uint32_t> rs0((size_t)orows, kSentinel32), par0(16, kSentinel32), part0(part_words + 64, kSentinel32);
  std::vector<uint32_t> rs1, par1;
  std::vector<uint8_t> out1[2];
  for (int run = 0; run < 2; ++run) {
    const std::vector<uint8_t> out0((size_t)orows * ld, kSentinel8[run]);
    upload_sync(stream_, dout(ws), out0);
    upload_sync(stream_, drs(ws), rs0);
    upload_sync(stream_, dpar(ws), par0);
    upload_sync(stream_, dpart(ws), part0);
    int8_t* codes = (int8_t*)dout(ws); int32_t* rowsum = (int32_t*)drs(ws);
    float* par = (float*)dpar(ws); float* part = (float*)dpart(ws);
    if (ln) {
      launch_ln_minmax(stream_, x32, rows, cols, dg(ws), db(ws), part);
      launch_ln_quantize(stream_, x32, rows, cols, dg(ws), db(ws), codes, ld, rowsum, par, part);
    } else {
      launch_minmax(stream_, x32, x16, rows, cols, ldx, part);
      launch_quantize(stream_, x32, x16, rows, cols, ldx, codes, ld, rowsum, par, part);
    }
    out1[run] = check_guard(stream_, "op_quantize: the codes", codes, kSentinel8[run], GuardGeom{orows, ld, rows, ld, rows, false, false}, &out0);
    rs1 = check_guard(stream_, "op_quantize: rowsum", rowsum, kSentinel32, vector_geom(orows, rows), &rs0);
    par1 = check_guard(stream_, "op_quantize: params", par, kSentinel32, vector_geom(16, 2), &par0);
    check_guard(stream_, "op_quantize: the {min, max} pairs", part, kSentinel32, vector_geom((int64_t)part_words + 64, (int64_t)part_words), &part0);
  }
  check_bytes_written("op_quantize: the codes", out1[0], out1[1], ld, rows, ld);
  std::memcpy(codes_out, out1[1].data(), (size_t)rows * ld);
  std::memcpy(rowsum_out, rs1.data(), (size_t)rows * 4);
  std::memcpy(params_out, par1.data(), 8);
}

void Engine::op_weight(const float* W, const uint8_t* Q, const uint8_t* zp, const float* scale, int N, int K, int ld, int8_t* w_out,
                       int32_t* colsum_out, int32_t* wzp_out, float* wscale_out, int32_t* dz_out) {
  PF_HIP(hipSetDevice(device_));
  PF_CHECK((W || (Q && zp && scale)) && w_out && colsum_out && wzp_out && wscale_out && dz_out && N > 0 && K > 0 && ld >= K, PF_ERR_INVALID_ARG,
           "op_quantize_weight / op_import_weight: bad arguments (ld >= K)");
  const std::string op = Q ? "op_import_weight" : "op_quantize_weight";
  const int64_t wr = N + 4, orows = N + 4, vn = N + kTail;
  StageCarve st{0, kAlignQ};
  const auto dW = st.take<float>((size_t)wr * K);
  const auto dQ = st.take<uint8_t>((size_t)wr * K), dzq = st.take<uint8_t>(vn);
  const auto dsq = st.take<float>(vn);
  const auto dout = st.take<uint8_t>((size_t)orows * ld);
  const Field<uint32_t> dvec[4] = {st.take<uint32_t>(vn), st.take<uint32_t>(vn), st.take<uint32_t>(vn), st.take<uint32_t>(vn)};   // colsum, wzp, wscale, dz
  static const char* const vec_name[4] = {": colsum", ": wzp", ": wscale", ": dz"};
  void* ws = op_ws(st);
  if (Q) {                                                     // the rows and vector cells behind N: the largest bytes, NaN scales
    std::vector<uint8_t> q((size_t)wr * K, 255), z((size_t)vn, 255);
    std::vector<float> sc((size_t)vn, quiet_nan());
    std::copy(Q, Q + (size_t)N * K, q.begin());
    std::copy(zp, zp + N, z.begin());
    std::copy(scale, scale + N, sc.begin());
    upload_sync(stream_, dQ(ws), q);
    upload_sync(stream_, dzq(ws), z);
    upload_sync(stream_, dsq(ws), sc);
  } else {
    std::vector<float> w((size_t)wr * K);
    for (size_t i = 0; i < w.size(); ++i) w[i] = i < (size_t)N * K ? W[i] : hostile32(i);
    upload_sync(stream_, dW(ws), w);
  }
  const std::vector<uint32_t> v0((size_t)vn, kSentinel32);
  std::vector<uint32_t> vec1[4];
  std::vector<uint8_t> out1[2];
  for (int run = 0; run < 2; ++run) {
    const std::vector<uint8_t> out0((size_t)orows * ld, kSentinel8[run]);
    upload_sync(stream_, dout(ws), out0);
    for (const Field<uint32_t>& f : dvec) upload_sync(stream_, f(ws), v0);
    int8_t* codes = (int8_t*)dout(ws);
    int32_t* cs = (int32_t*)dvec[0](ws);
    int32_t* wz = (int32_t*)dvec[1](ws);
    if (Q) launch_import_weight(stream_, dQ(ws), dzq(ws), dsq(ws), N, K, codes, ld, cs, wz, (float*)dvec[2](ws));
    else launch_quantize_weight(stream_, dW(ws), N, K, codes, ld, cs, wz, (float*)dvec[2](ws));
    launch_pack_dz(stream_, cs, wz, N, K, (int32_t*)dvec[3](ws));
    out1[run] = check_guard(stream_, op + ": w'", codes, kSentinel8[run], GuardGeom{orows, ld, N, ld, N, false, false}, &out0);
    for (int i = 0; i < 4; ++i) vec1[i] = check_guard(stream_, op + vec_name[i], dvec[i](ws), kSentinel32, vector_geom(vn, N), &v0);
  }
  check_bytes_written(op + ": w'", out1[0], out1[1], ld, N, ld);
  std::memcpy(w_out, out1[1].data(), (size_t)N * ld);
  std::memcpy(colsum_out, vec1[0].data(), (size_t)N * 4);
  std::memcpy(wzp_out, vec1[1].data(), (size_t)N * 4);
  std::memcpy(wscale_out, vec1[2].data(), (size_t)N * 4);
  std::memcpy(dz_out, vec1[3].data(), (size_t)N * 4);
}

void Engine::op_qgemm_ex(const pf_qgemm_desc& ds, const uint8_t* a_codes, const uint8_t* w_codes, float* y32, float* y16, float* range_out) {
  PF_HIP(hipSetDevice(device_));
  const int M = ds.M, N = ds.N, K = ds.K, kind = ds.out_kind;
  PF_CHECK(M > 0 && N > 0 && K > 0 && a_codes && w_codes && ds.w_zp && ds.w_scale, PF_ERR_INVALID_ARG, "qgemm_ex: empty problem");
  PF_CHECK(kind >= 0 && kind <= 3, PF_ERR_INVALID_ARG, "qgemm_ex: out_kind must be 0 .. 3");
  PF_CHECK(ds.tile_rows == 0 || ds.tile_rows == 128 || ds.tile_rows == 256, PF_ERR_INVALID_ARG, "qgemm_ex: tile_rows must be 0, 128 or 256");
  PF_CHECK(kind != 1 || (!ds.resid && !ds.add2), PF_ERR_INVALID_ARG, "qgemm_ex: the f16-result kernel takes no residual / addend");
  PF_CHECK(ds.a_zp >= 0 && ds.a_zp <= 255, PF_ERR_INVALID_ARG, "qgemm_ex: a_zp must be in 0 .. 255");
  const bool has32 = kind == 0 || kind == 3, has16 = kind != 0;
  PF_CHECK((!has32 || y32) && (!has16 || y16) && (!ds.want_range || range_out), PF_ERR_INVALID_ARG, "qgemm_ex: missing output");
  const int Kp = (int)round_up(K, 128);
  const int64_t Mp = round_up(M, 256), Np = round_up(N, 128), Mo = Mp + 128, vn = N + kTail;
  const int ld32 = (int)round_up(N, 4) + 4, ld16 = kind == 1 ? (int)round_up(N, 8) + 8 : (int)round_up(N, 4) + 4;
  const size_t part_words = quant_scratch_bytes() / 4;
  StageCarve st{0, kAlignQ};
  const auto da = st.take<int8_t>((size_t)Mp * Kp), dw = st.take<int8_t>((size_t)Np * Kp);
  const auto drs = st.take<int32_t>(Mp); const auto dpar = st.take<float>(16);
  const auto dcs = st.take<int32_t>(vn), dzp = st.take<int32_t>(vn), ddz = st.take<int32_t>(vn);
  const auto dwsc = st.take<float>(vn), db = st.take<float>(vn);
  const auto d32 = st.take<uint32_t>((size_t)Mo * ld32); const auto d16 = st.take<uint16_t>((size_t)Mo * ld16);
  const auto dR = st.take<float>((size_t)Mo * ld32), dD = st.take<float>((size_t)Mo * ld32);
  const auto dpart = st.take<uint32_t>(part_words + 64);
  void* ws = op_ws(st);
  // a', w' with their sums and dz, on the host; pad columns 0 (the contract), pad rows the largest codes of both signs
  std::vector<int8_t> a((size_t)Mp * Kp, 0), w((size_t)Np * Kp, 0);
  std::vector<int32_t> rs((size_t)Mp), cs((size_t)vn), wz((size_t)vn), dz((size_t)vn);
  std::vector<float> wsc((size_t)vn, quiet_nan()), bias((size_t)vn, quiet_nan());
  for (int64_t m = 0; m < Mp; ++m) {
    int sum = 0;
    for (int k = 0; k < K; ++k) {
      const int v = m < M ? (int)a_codes[(size_t)m * K + k] - 128 : (((m + k) & 1) ? 127 : -128);
      a[(size_t)m * Kp + k] = (int8_t)v;
      sum += v;
    }
    rs[(size_t)m] = m < M ? sum : hostile_i32((size_t)m);
  }
  for (int64_t n = 0; n < Np; ++n)
    for (int k = 0; k < K; ++k)
      w[(size_t)n * Kp + k] = (int8_t)(n < N ? (int)w_codes[(size_t)n * K + k] - 128 : (((n + k) & 1) ? -128 : 127));
  for (int64_t n = 0; n < vn; ++n) {
    if (n >= N) { cs[(size_t)n] = hostile_i32((size_t)n); wz[(size_t)n] = hostile_i32((size_t)n + 1); dz[(size_t)n] = hostile_i32((size_t)n + 2); continue; }
    PF_CHECK(ds.w_zp[n] >= 0 && ds.w_zp[n] <= 255, PF_ERR_INVALID_ARG, "qgemm_ex: w_zp must be in 0 .. 255");
    int sum = 0;
    for (int k = 0; k < K; ++k) sum += w[(size_t)n * Kp + k];
    cs[(size_t)n] = sum;
    wz[(size_t)n] = ds.w_zp[n] - 128;
    dz[(size_t)n] = (int32_t)((uint32_t)(sum - K * wz[(size_t)n]) * 256u + (uint32_t)(wz[(size_t)n] & 255));
    wsc[(size_t)n] = ds.w_scale[n];
    if (ds.bias) bias[(size_t)n] = ds.bias[n];
  }
  PF_CHECK(kind != 1 || K <= 16384, PF_ERR_UNSUPPORTED, "qgemm_ex: K too large for the packed column word");
  const float par[16] = {ds.a_scale, (float)ds.a_zp, quiet_nan(), quiet_nan()};
  upload_sync(stream_, da(ws), a);
  upload_sync(stream_, dw(ws), w);
  upload_sync(stream_, drs(ws), rs);
  upload_sync(stream_, dcs(ws), cs);
  upload_sync(stream_, dzp(ws), wz);
  upload_sync(stream_, ddz(ws), dz);
  upload_sync(stream_, dwsc(ws), wsc);
  upload_sync(stream_, db(ws), bias);
  upload(stream_, dpar(ws), par, 16);
  // results: sentinels; a residual aliases the fp32 result where there is one (its cells of [M, N] hold the residual)
  std::vector<uint32_t> c32((size_t)Mo * ld32, kSentinel32), after32;
  std::vector<uint16_t> c16((size_t)Mo * ld16, kSentinel16), after16;
  const std::vector<uint32_t> part0(part_words + 64, kSentinel32);
  auto pad32 = [&](const float* src, float* dst) {                       // [M, N] into [Mo, ld32], hostile around it
    std::vector<float> h((size_t)Mo * ld32);
    for (int64_t m = 0; m < Mo; ++m)
      for (int n = 0; n < ld32; ++n) h[(size_t)m * ld32 + n] = m < M && n < N ? src[(size_t)m * N + n] : hostile32((size_t)m * 131 + n);
    upload_sync(stream_, dst, h);
  };
  const bool alias = has32 && ds.resid;
  if (alias)
    for (int m = 0; m < M; ++m) std::memcpy(&c32[(size_t)m * ld32], ds.resid + (size_t)m * N, (size_t)N * 4);
  else if (ds.resid) pad32(ds.resid, dR(ws));
  if (ds.add2) pad32(ds.add2, dD(ws));
  if (has32) upload_sync(stream_, d32(ws), c32);
  if (has16) upload_sync(stream_, d16(ws), c16);
  upload_sync(stream_, dpart(ws), part0);
  GemmI8Args g{};
  g.A = da(ws); g.lda = Kp; g.W = dw(ws); g.ldw = Kp;
  g.rowsum = drs(ws); g.colsum = dcs(ws); g.wzp = dzp(ws); g.wscale = dwsc(ws);
  g.aparams = dpar(ws); g.bias = ds.bias ? db(ws) : nullptr;
  g.M = M; g.N = N; g.K = K; g.Kpad = Kp;
  g.relu = ds.relu ? 1 : 0; g.scale_cols = ds.scale_cols; g.scale = ds.scale;
  if (has32) { g.out_f32 = (float*)d32(ws); g.ldc32 = ld32; }
  if (has16) { g.out_f16 = (half_t*)d16(ws); g.ldc16 = ld16; }
  if (ds.resid) { g.resid = alias ? (const float*)d32(ws) : dR(ws); g.ldr = ld32; }
  if (ds.add2) { g.add2 = dD(ws); g.ld2 = ld32; }
  if (kind == 1) { g.dz = ddz(ws); g.out_padded = 1; }
  if (ds.want_range) g.range_out = (float*)dpart(ws);
  g.force_mi = ds.tile_rows == 128 ? 1 : (ds.tile_rows == 256 ? 2 : 0);
  prof_begin("gemm_op", 2.0 * M * (double)N * K);
  try {
    launch_gemm_i8(stream_, g);
  } catch (...) {                                              // a refusal of the launcher: close the profile's event pair
    prof_end("gemm_op");
    throw;
  }
  prof_end("gemm_op");
  PF_CHECK(std::strncmp(last_gemm_kernel(), kind == 1 ? "gemm_i8f_pp3" : "gemm_i8_pp3", kind == 1 ? 12 : 11) == 0, PF_ERR_DEVICE,
           "qgemm_ex: the result kind ran on another kernel than kernels.h names for it");
  const std::string tag = std::string("qgemm_ex [") + last_gemm_kernel() + "]: ";
  const int64_t pw = ds.want_range ? (int64_t)part_words : 0;
  if (has32) after32 = check_guard(stream_, tag + "the fp32 result", d32(ws), kSentinel32, GuardGeom{Mo, ld32, M, N, M, false, !alias}, &c32);
  if (has16) after16 = check_guard(stream_, tag + "the f16 result", d16(ws), kSentinel16, GuardGeom{Mo, ld16, M, N, kind == 1 ? Mp : M, false, true}, &c16);
  const std::vector<uint32_t> part1 = check_guard(stream_, tag + "the {min, max} pairs", dpart(ws), kSentinel32, vector_geom((int64_t)part_words + 64, pw), &part0);
  if (has32)
    for (int m = 0; m < M; ++m) std::memcpy(y32 + (size_t)m * N, &after32[(size_t)m * ld32], (size_t)N * 4);
  if (has16)
    for (int m = 0; m < M; ++m)
      for (int n = 0; n < N; ++n) {
        half_t h;
        std::memcpy(&h, &after16[(size_t)m * ld16 + n], 2);
        y16[(size_t)m * N + n] = (float)h;
      }
  if (ds.want_range) {                                         // the consumer's fold of the 256 pairs (k_quant.hip fold_minmax)
    float lo = 0.f, hi = 0.f;
    for (size_t i = 0; i < part_words / 2; ++i) {
      float l, h;
      std::memcpy(&l, &part1[2 * i], 4);
      std::memcpy(&h, &part1[2 * i + 1], 4);
      lo = std::fmin(lo, l);
      hi = std::fmax(hi, h);
    }
    range_out[0] = lo; range_out[1] = hi;
  }
}

}  // namespace pf

