// engine.h — device engine: weights, workspace and the forward pipeline.
// Replaces OfflineModel (ORT session, AliParaformerAsr/OfflineModel.cs:35-70) and the numeric
// body of IOfflineProj.ModelProj (AliParaformerAsr/IOfflineProj.cs:38).
#pragma once
#include <functional>
#include <map>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "lm.h"
#include "vadnet.h"
#include "spk.h"
#include "punc.h"
#include "json.h"
#include "kernels.h"
#include "shards.h"

namespace pf {

struct ModelCfg {
  std::string kind = "paraformer";
  int feat_dim = 560, d_model = 512, heads = 4, ffn = 2048, enc_layers = 50, tp_layers = 0, kernel = 11;
  int dec_layers = 16, vocab = 8404;
  float cif_threshold = 1.0f, cif_tail = 0.45f, cif_smooth = 1.0f, cif_noise = 0.0f;
  int cif_l_order = 1, cif_r_order = 1;
  bool cif_cumsum = false;           // cif_variant = "cumsum": the prefix-sum export (cif_v1_export) instead of the loop
  bool timestamp_head = false, seaco = false, use_itn = false;
  float cif_smooth2 = 0.25f, cif_noise2 = 0.01f;
  int upsample = 3;
  int seaco_layers = 4, seaco_ffn = 1024, seaco_kernel = 21, seaco_lstm_layers = 2, seaco_nobias = 8377;
  int kind_id() const { return kind == "sensevoicesmall" ? 1 : (kind == "seacoparaformer" ? 2 : 0); }
};

struct FrontendCfg {
  int fs = 16000, n_mels = 80, lfr_m = 7, lfr_n = 6;
  bool snip_edges = false;
  float dither = 0.f;
  uint32_t dither_seed = 0;
  std::string window = "hamming";
};

struct Lin {          // y = x W^T + b ; W stored f16 [Npad][Kpad]
  half_t* w = nullptr;
  const float* bias = nullptr;
  int N = 0, K = 0, Kpad = 0;
  const float* w32 = nullptr;         // the fp32 tensor [N][K] as stored in the container (fp32 parity mode)
  half_t* w_panel = nullptr;          // the weight in the fragment order of gemm_panel_kernel (k_gemm_panel.hip; null: not built)
};
struct LNp { const float* g = nullptr; const float* b = nullptr; int D = 0; };
// a Linear as onnxruntime's quantize_dynamic stores it (math_mode 2): w' = w_q - 128 as signed bytes [Npad][Kpad], K-contiguous
struct QLin {
  int8_t* w = nullptr;
  int32_t* colsum = nullptr;      // [N] sum_k w'
  int32_t* wzp = nullptr;         // [N] w_zp - 128
  float* wscale = nullptr;        // [N]
  int32_t* dz = nullptr;          // [N] packed column word of the f16-result kernel (kernels.h GemmI8Args::dz)
  const float* bias = nullptr;
  int N = 0, K = 0, Kpad = 0;
};
// a quantised activation tensor: a' = a_q - 128 [rows, Kpad], row sums of a', {scale, zero point}
struct QAct { int8_t* a = nullptr; int32_t* rowsum = nullptr; float* params = nullptr; };
struct EncLayer {
  LNp norm1, norm2; Lin qkv, out, w1, w2; float* fsmn_wT = nullptr; int d_in = 512;
  half_t* qkv_p = nullptr; float* qkv_bias_p = nullptr;   // qkv weight rows / bias in the tile order of gemm_qkvp_kernel (null: not built)
  half_t* ffn_wt = nullptr;                               // W1 | W2 in the fragment order of ffn_fused_kernel (k_ffn.hip; null: not built)
  half_t* qkv_t = nullptr;                                // the [Q | K | V] weight in that order too (three 512-row images): the PREVIOUS layer's launch runs this projection
  half_t* out_wt = nullptr;                               // the attention out-projection weight in the same kernel's fragment order
};
struct DecLayer {
  LNp norm1, ffn_norm, norm2, norm3; Lin w1, w2, q, out, kv32; float* fsmn_wT = nullptr;   // kv32: fp32 pointers only
  half_t* ffn_img = nullptr;   // (W1, gamma_F (.) W2, b1, colsum, W2 beta_F) in the fragment order of the split FFN form (k_ffn.hip; null: not built)
  half_t* out_wt = nullptr;    // the cross-attention out-projection weight in that kernel's fragment order: the NEXT block's launch runs it
  half_t* q_wt = nullptr;      // the cross-attention query projection in the same fragment order (k_decmid.hip; null: not built)
};
// the weights of one decoder stack (the ASR decoder, the SeACo bias decoder): layers, the final FFN block, after_norm, the
// output layer and the K | V projections of all layers as one Linear [layers * 2D, D] (Engine::load_dec_stack)
struct DecStack {
  std::vector<DecLayer> layers;
  LNp final_norm1, final_ffn_norm, after;
  Lin final_w1, final_w2, out, kv_all;
  half_t* final_img = nullptr;   // the final block's image for the split FFN form (DecLayer::ffn_img)
  int ffn = 0, fsmn_k = 0;
};
// the activation buffers of one decoder walk [rows, *]; every arithmetic carves the ones its walk uses (Engine::carve_dec*)
struct DecBufs {
  float* x = nullptr; float* t32 = nullptr; float* tn32 = nullptr;                                   // residual stream, FFN-down result, norm2 of it
  half_t* xn16 = nullptr; half_t* h16 = nullptr; half_t* q16 = nullptr; half_t* ctx16 = nullptr;     // f16 walks; int8: q16, ctx16
  float* xn32 = nullptr; float* h32 = nullptr; float* hn32 = nullptr; float* q32 = nullptr; float* ctx32 = nullptr;   // fp32 walk; int8: h32
};
// one run of a decoder walk (decoder16 / decoder32 / decoder_int8): layers + the final block's FFN, FFN-down result left in t32
struct DecRun {
  int B = 0, L = 0;                        // rows = B * L; B is also the batch count of token_num
  const int32_t* token_num = nullptr;
  // K | V of layer i: kv + i * 2D with the strides below (projected ahead for all layers), or what kv_layer(i) returns (it
  // enqueues that layer's projection; V = K + D either way).  kv_bs = 0: one set of rows for every utterance
  const void* kv = nullptr; int kv_rs = 0; int64_t kv_bs = 0; int Lk = 0;
  std::function<const void*(int)> kv_layer;
  DecBufs b;
  const char* cls_ffn1 = "gemm_dec_ffn1"; const char* cls_ffn2 = "gemm_dec_ffn2"; const char* cls_q = "gemm_dec_q";
  const char* cls_out = "gemm_dec_out"; const char* cls_attn = "attn_cross";
  bool operand_only = false;               // fp32: norm1 / norm3 / the context feed gemm32 alone (layernorm32, attention32 only_operand)
  const float* cache_in = nullptr; float* cache_out = nullptr;   // f16 plain walk: the streaming FSMN with its caches [layers, B, D, k - 1]
};
static const size_t kAlign = 256;   // of every buffer carved out of a workspace
// carves aligned buffers out of one allocation; with base == nullptr it only measures (Engine::carve_into)
struct Arena {
  char* base = nullptr; size_t align = kAlign; size_t off = 0;
  template <class T> T* take(size_t bytes) { const size_t o = off; off += (bytes + align - 1) / align * align; return base ? (T*)(base + o) : nullptr; }
};

// the same rounding as offsets: carve(bytes) gives where the buffer starts and moves the caller's `off` past it
struct Carve {
  size_t& off; size_t align = kAlign;
  size_t operator()(size_t bytes) const { const size_t o = off; off += (bytes + align - 1) / align * align; return o; }
};
// the CIF stage's arrays for (B, T1 = T + 1) in the order every arena keeps them: the alphas, then the plan's six
struct CifCarve {
  size_t al, fc, tn, ff, wc, wr, mx;
  CifCarve(const Carve& c, int B, int T1)
      : al(c((size_t)B * T1 * 4)), fc(c((size_t)B * 4)), tn(c((size_t)B * 4)), ff(c((size_t)B * T1 * 4)), wc(c((size_t)B * T1 * 4)),
        wr(c((size_t)B * T1 * 4)), mx(c(256)) {}
  CifPlan plan(char* base) const {
    return CifPlan{(int32_t*)(base + fc), (int32_t*)(base + tn), (int32_t*)(base + ff), (float*)(base + wc), (float*)(base + wr),
                   (int32_t*)(base + mx)};
  }
};
// the decoder stage of one forward (Engine::forward_device): the walk's arena, whose x receives the CIF embeds, and what the
// arithmetic keeps beside it
struct DecStage {
  DecBufs b; int64_t rows = 0;                 // rows: the arena's row count (f16 / int8: padded)
  void* kv = nullptr;                          // f16: every layer's K | V, projected ahead of the length; int8 / fp32: one layer's
  QAct qH;                                     // int8: the quantised encoder memory
  float* x_alt = nullptr;                      // f16: the residual stream's second buffer (out-projection chain)
  float* e0 = nullptr; float* hid = nullptr;   // SeACo with hot words: the CIF embeds set aside, the ASR decoder's after_norm hidden
};

struct DevBuf {       // grow-only device allocation
  void* p = nullptr;
  size_t bytes = 0;
};

class Engine {
 public:
  explicit Engine(const pf_engine_config& cfg);
  ~Engine();

  // ---- front-end ---------------------------------------------------------
  int num_lfr_frames(int64_t n_samples) const;
  int num_fbank_frames(int64_t n_samples) const;
  void fbank_host(const float* samples, int64_t n, std::vector<float>& out, int& t80);
  void frontend_host(const float* samples, int64_t n, std::vector<float>& feats, int& t_lfr);
  // the same on samples that already live on this device (OfflineStream keeps the audio of its AddSamples call there)
  void frontend_staged_one(std::vector<float>& feats, int& t_lfr);
  void frontend_from_device(const float* samples_dev, int64_t n, std::vector<float>& feats, int& t_lfr);
  // stage_audio without the copy: utterance b = n[b] floats at the DEVICE address samples_dev[b] (4-byte aligned, alive until
  // the run has been synchronised); the batched front-end of run_staged reads them where they are
  void stage_device_audio(const float* const* samples_dev, const int64_t* n, int B, int force_T = 0);

  // ---- forward -----------------------------------------------------------
  // speech_dev: [B,T,feat] fp32 already on device (padded + sentinel)
  void forward_device(const float* speech_dev, int B, int T, bool want_logits);
  void forward_feats_host(const float* speech, int B, int T, bool want_logits);
  void model_proj_host(const float* const* speech, const int32_t* n_floats, int B, bool want_logits);
  // force_T > 0: pad to at least force_T LFR frames (a shard of a larger batch pads to the GLOBAL maximum, PadHelper.cs:25)
  void stage_audio(const float* const* samples, const int64_t* n, int B, int force_T = 0);
  // stage_audio for raw PCM (paraformer_hip.h "PCM intake"): the raw bytes are uploaded and pcm_to_samples_kernel (k_pcm.hip)
  // writes the float samples into the layout stage_audio fills — everything behind it (frame counts, force_T, decode
  // lengths, the dither's per-sample counters) follows from the per-utterance n_out.  descs: n_descs == B, or 1 for all
  void stage_pcm(const void* const* data, const int64_t* n_values, const pf_pcm_desc* descs, int n_descs, int B, int force_T = 0);
  void run_staged(bool want_logits);
  void fetch(pf_batch_out* out);
  void fetch_ids_device(int64_t* ids_dev, int l_cap, int32_t* L_out);   // last forward's ids -> caller's device buffer [B, l_cap], -1 padded
  // Results are kept per CALLING THREAD: a forward entry point (pf_forward_feats / pf_model_proj / pf_recognize)
  // publishes its outcome into the caller's slot, and pf_fetch from the same thread reads that slot, so the
  // two-call protocol (learn L, then fetch into right-sized buffers) is safe with concurrent callers on one
  // engine.  The staged API (pf_stage_audio / pf_run_staged) is engine state and single-caller by contract.
  void publish_thread_result();
  void drop_thread_result();
  void sync();
  // multi-device groups (group.h): the decoder length becomes the maximum over all shards of the batch
  void set_l_hook(std::function<int(int)> h) { l_hook_ = std::move(h); }
  const HostBatchOut& last_result() const { return last_; }
  // the same for a reader that lets go of the engine before it is done reading (Recognizer::Forward, after sync()): a copy, so
  // the pf_fetch_* calls still serve this forward.  No logits: those are read from the device or live in a per-thread slot.
  HostBatchOut result_copy() const { return last_; }
  void copy_logits(HostBatchOut& r);                 // host copy of the last forward's log-probs into r.logits
  const int64_t* ids_device() const { return ids_dev_; }
  const int32_t* token_num_device() const { return plan_.token_num; }
  hipStream_t stream() const { return stream_; }
  // SeACo: hotword ids [n, 10] (PadList output, EmbedSeacoModel.cs:70-123) used by the following forwards;
  // n = 0 -> bias_embed [B,0,512]: the bias branch is skipped and the ASR log-probs are returned
  void set_hotwords(const int32_t* hw, int n);
  // Decoding extras of the forwards that follow (PF_DECODE_* of paraformer_hip.h; 0 = the reference behaviour, nothing
  // extra is launched).  SCORES: the log-prob of every arg-max position [B, L].  CTC (SenseVoice only, implies SCORES):
  // the collapse of k_ctc.hip over the first n_b frames of each utterance, right behind the arg-max on stream_.
  void set_decode(int flags);
  int decode_flags() const { return decode_flags_; }
  void fetch_scores(float* scores, int64_t cap, int32_t* L_out);
  void fetch_ctc(int64_t* ids, int32_t* first, int32_t* last, float* score, int32_t cap, int32_t* n, int32_t* n_max);
  // TOPK (implies SCORES): the K best (id, log-prob) of every position [B, L, K] by k_topk.hip, right behind the arg-max,
  // which then stores its log-probs in place (mode 2, the form a logits request already runs).  K: 1 .. PF_TOPK_MAX.
  void set_topk(int k);
  int topk() const { return topk_k_; }
  void fetch_topk(int64_t* ids, float* val, int32_t* n, int64_t cap_rows, int32_t* L_out, int32_t* K_out);
  void op_topk(const float* x, int64_t rows, int V, int ld, int K, int64_t* ids, float* val, int32_t* n);
  // CTC_BEAM (SenseVoice; implies TOPK and SCORES): behind the top-k launch one kernel (k_ctcbeam.hip) runs a prefix beam
  // search of width W over every utterance's frames and keeps the N best labelings.  1 <= N <= W <= 64, default 16 / 16.
  void set_ctc_beam(int W, int N);
  int ctc_beam_w() const { return beam_w_; }
  int ctc_beam_n() const { return beam_n_; }
  void fetch_ctc_beam(int64_t* ids, int32_t* len, double* score, int32_t cap, int32_t* n_hyp, int32_t* len_max, int32_t* N_out);
  void op_ctc_beam(const float* blank_lp, const int64_t* ids, const float* val, const int32_t* n, const int32_t* lens, int B, int T,
                   int K, int blank, int W, int N, int64_t* out_ids, int32_t* out_len, double* out_score, int cap, int32_t* n_hyp);
  // hot words inside the search (paraformer_hip.h "CTC hot words"): the set of the forwards that follow, compiled into the
  // automaton's table and uploaded here; n == 0 or boost == 0 clears it.  With a set installed CTC_BEAM launches the biased
  // form of the kernel and fetch_ctc_beam_hot gives matched / loglik_sum beside fetch_ctc_beam's (biased) scores.
  void set_ctc_hotwords(const int32_t* ids, const int32_t* lens, int n, float boost);
  bool ctc_hotwords_on() const { return hot_.boost > 0.f; }
  // Language model (SenseVoice; the definition is tests/ctcbeam_lm_ref.py): with a model installed a forward with CTC_BEAM runs
  // a fused form of the kernel and fetch_ctc_beam_lm gives lm_sum / loglik_sum beside fetch_ctc_beam's (fused) scores.  nullptr
  // clears; the image is uploaded once, the same model again only takes the new weights.
  void set_ctc_lm(const std::shared_ptr<const LmImage>& lm, float alpha, float beta, int flags);
  bool ctc_lm_on() const { return (bool)lm_; }
  void fetch_ctc_beam_lm(double* lm_sum, double* loglik);
  void fetch_ctc_beam_hot(int32_t* matched, double* loglik);
  void op_ctc_beam_hot(const float* blank_lp, const int64_t* ids, const float* val, const int32_t* n, const int32_t* lens, int B, int T,
                       int K, int blank, int W, int N, const int32_t* hw_ids, const int32_t* hw_lens, int n_hw, float boost,
                       int64_t* out_ids, int32_t* out_len, double* out_score, int32_t* out_matched, double* out_loglik, int cap,
                       int32_t* n_hyp);
  // the fused forms on caller data (language model, with or without a hot-word set), and the model's walk on its own
  void op_ctc_beam_lm(const float* blank_lp, const int64_t* ids, const float* val, const int32_t* n, const int32_t* lens, int B, int T,
                      int K, int blank, int W, int N, const int32_t* hw_ids, const int32_t* hw_lens, int n_hw, float boost,
                      int64_t* out_ids, int32_t* out_len, double* out_score, int32_t* out_matched, double* out_loglik, int cap,
                      int32_t* n_hyp, const std::shared_ptr<const LmImage>& lm, float alpha, float beta, int lm_flags, double* out_lm);
  void op_lm_score(const std::shared_ptr<const LmImage>& lm, const int32_t* ids, const int32_t* lens, int B, int L, float alpha,
                   float beta, double* g, int32_t* state);
  // N-best search (paraformer, not SeACo; the definition is tests/nbest_search_ref.py): with W > 0 installed a forward with TOPK
  // runs, behind the top-k launch, one kernel (k_nbestsearch.hip) that searches every utterance's lists with a beam of width W
  // and keeps the N best rank vectors; W == 0 turns it off (nothing is launched, allocated or uploaded).  A model and a hot-word
  // set of its own may be fused in; both are inert until a search is installed, and share rules and one-time upload with their
  // set_ctc_* siblings.
  void set_nbest_search(int W, int N);
  int nbest_search_w() const { return nbs_w_; }
  void set_nbest_lm(const std::shared_ptr<const LmImage>& lm, float alpha, float beta, int flags);
  void set_nbest_hotwords(const int32_t* ids, const int32_t* lens, int n, float boost);
  void fetch_nbest_search(int32_t* ranks, double* score, double* loglik, double* lm_sum, int32_t* matched, int32_t* n_hyp, int32_t* L_out,
                          int32_t* N_out);
  // the kernel alone on caller-supplied lists [B, L, K] with token_num [B]
  void op_nbest_search(const int64_t* ids, const float* val, const int32_t* n, const int32_t* token_num, int B, int L, int K, int W, int N,
                       const int32_t* hw_ids, const int32_t* hw_lens, int n_hw, float boost, const std::shared_ptr<const LmImage>& lm,
                       float alpha, float beta, int lm_flags, int32_t* out_ranks, double* out_score, double* out_loglik, double* out_lm,
                       int32_t* out_matched, int32_t* n_hyp);
  // ALIGN (SenseVoice; implies SCORES): behind the other decode launches one kernel (k_ctcalign.hip) aligns the caller's
  // targets of this forward (set_align_targets; consumed) and, with CTC_BEAM, the beam's hypotheses to the log-prob rows
  void set_align_targets(const int64_t* ids, const int32_t* len, int B, int cap);
  void fetch_align(float* path_score, double* loglik, int32_t* ok, int32_t* len, int32_t* first, int32_t* last, float* tok_score,
                   int32_t cap, int32_t* H_out, int32_t* len_max);
  void op_ctc_align(const float* lp, int B, int T, int V, int ld, const int32_t* tgt, const int32_t* tlen, const int32_t* lens, int H,
                    int cap, float* path_score, double* loglik, int32_t* ok, int32_t* first, int32_t* last, float* tok_score);
  void op_pcm_convert(const void* data, int64_t n_values, const pf_pcm_desc& desc, float* out, int64_t cap, int64_t* n_out);
  // voice-activity segmentation (k_vad.hip): stage_audio, run_staged's one fbank launch, then the two detector launches (profile
  // class "vad") over all B utterances; only n [B] and the segment lists come back.  seg [B, cap, 2].
  void vad_segment(const float* const* samples, const int64_t* n, int B, const pf_vad_config* cfg, int32_t* seg, int cap, int32_t* n_seg);
  // the same over audio that is already on the device (stage_device_audio: the recognizer's resident streams)
  void vad_segment_device(const float* const* samples_dev, const int64_t* n, int B, const pf_vad_config* cfg, int32_t* seg, int cap,
                          int32_t* n_seg);
  void vad_staged(const pf_vad_config* cfg, int32_t* seg, int cap, int32_t* n_seg);
  void op_vad_levels(const float* rows, int64_t T, int n_mels, int32_t* out);
  // The FSMN-VAD model score (k_vadnet.hip, vadnet.h): with a model attached vad_staged computes the levels with the network
  // (profile class "vadnet", 1 + n_layers launches) where it otherwise launches the energy level; everything behind the levels
  // is unchanged.  nullptr detaches and frees the image and the p rows (nothing of it is launched or allocated then; attaching the
  // same model to an engine that still has it costs no upload).  The engine keeps a reference and uploads the
  // image once.  PF_ERR_INVALID_ARG unless n_mels * lfr_m equals the model's input width; PF_ERR_UNSUPPORTED with snip_edges.
  void set_vad_model(const std::shared_ptr<const VadModel>& m);
  bool vad_model_on() const { return (bool)vadnet_; }
  const std::shared_ptr<const VadModel>& vad_model() const { return vadnet_; }
  // the network on caller rows: rows = the concatenated frames of B utterances of T[b] frames; logits [sum T, output_dim]
  // and / or levels [sum T] (either may be null).  Uses the attached model.
  void op_vad_model(const float* rows, const int32_t* T, int B, int n_mels, float* logits, int32_t* levels);
  // The CT-Transformer punctuation model (k_punc.hip, punc.h).  nullptr detaches and frees the image and the workspace (nothing
  // of it is launched or allocated then; attaching the model an engine still has costs no upload).  The engine keeps a
  // reference and uploads the image once.  A forward is profile class "punc": 1 + 2 n_layers launches, one more with the cut.
  void set_punc_model(const std::shared_ptr<const PuncModel>& m);
  const std::shared_ptr<const PuncModel>& punc_model() const { return punc_; }
  // the text loop over B texts given as ids (punc.h host_punc_ids is its host form): punc_ids [sum lens]; returns the rounds
  int punctuate(const int32_t* ids, const int32_t* lens, int B, int32_t* punc_ids);
  // the forward on caller windows: logits [sum T, n_punc], x0 [sum T, d_model] (layer 0's input), p [sum T] and cut [B] (the
  // cut launch runs when cut is asked for; it needs last [B]); every output may be null
  void op_punc(const int32_t* ids, const int32_t* T, const int32_t* last, int B, float* logits, float* x0, int32_t* p, int32_t* cut);
  // The attached model in streaming form (k_punc_stream.hip; causal models only, PF_ERR_UNSUPPORTED otherwise).
  // punc_stream_step: ONE launch of profile class "punc_stream" over B streams on device operands (kernels.h PuncStreamLaunch;
  // the caller has admitted every stream, punc.h punc_stream_admit).  op_punc_stream_step: the same over B caller streams through
  // op_stage.h (hostile ids behind n_new[b], sentinel-filled outputs, the guard rule): states [B, state bytes] in / out, ids
  // [B, ld], marks / mark_flags [B, ld], logits [B, ld, n_punc] (may be null), flush_mark [B]; flags bit 0: no restarts
  void punc_stream_step(char* states_dev, const int32_t* slot_dev, const int32_t* ids_dev, int64_t ld, const int32_t* n_new_dev,
                        const int32_t* flush_dev, int B, int max_context, int flags, int32_t* marks_dev, int32_t* mark_flags_dev,
                        float* logits_dev, int32_t* flush_mark_dev);
  void op_punc_stream_step(void* states, const int32_t* ids, const int32_t* n_new, const int32_t* flush, int B, int ld, int max_context,
                           int flags, int32_t* marks, int32_t* mark_flags, float* logits, int32_t* flush_mark);
  // The CAM++ speaker model (k_spk.hip, spk.h).  nullptr detaches and frees the image and the workspace (nothing of it is
  // launched or allocated then; attaching the model an engine still has costs no upload).  The engine keeps a reference and
  // uploads the image once.  PF_ERR_INVALID_ARG unless the model's n_mels is the front-end's.  A forward is profile class
  // "spk": kSpkLaunches launches whatever the windows.
  static constexpr int kSpkLaunches = 15;
  void set_spk_model(const std::shared_ptr<const SpkModel>& m);
  const std::shared_ptr<const SpkModel>& spk_model() const { return spk_; }
  // the forward on caller windows: rows = the concatenated rows of B windows of T[b] frames (0 .. PF_SPK_MAX_FRAMES);
  // emb [B, embedding]; frames [sum ceil(T / 2), c_out] or null
  void op_spk_embed(const float* rows, const int32_t* T, int B, int n_mels, float* emb, float* frames);
  // The recogniser's form, behind vad_staged on the SAME staged utterances (their fbank rows are still in ws_fbank_): win [N, 3]
  // = (staged utterance, first frame, end frame), grouped by utterance in order, n_utt [st_B] windows each.  Embeds the windows,
  // as many per forward as keep the activations within kSpkScratchBudget bytes whatever the windows' length (about 1000 windows of
  // 150 frames at the released dimensions, 300 of 512), and computes one cosine block per utterance in one launch:
  // emb [N, embedding], aff = the concatenated [n, n] blocks.
  static constexpr size_t kSpkScratchBudget = (size_t)2 << 30;
  void spk_staged(const int32_t* win, int N, const int32_t* n_utt, float* emb, float* aff);
  // the cosine blocks of S streams of n[s] embeddings (host arrays in and out; one launch of class "spk"; needs no model)
  void op_spk_affinity(const float* emb, const int32_t* n, int S, int E, float* out);
  void op_vad_segments(const int32_t* levels, const int32_t* T, int B, int ld, int n_mels, const pf_vad_config* cfg, int32_t* seg,
                       int cap, int32_t* n);
  // the streaming endpoint kernel (k_endpoint.hip) on caller state blocks and levels: ONE launch of class "endpoint" over B
  // streams, through op_stage.h (sentinel-filled outputs, hostile levels behind n_new[b], the guard rule on events)
  void op_endpoint_update(int32_t* states, const int32_t* levels, const int32_t* n_new, const int32_t* flush, int B, int ld, int n_mels,
                          const pf_endpoint_config* cfg, int32_t* events, int cap, int32_t* n_events, int32_t* in_speech,
                          int32_t* open_begin);
  // The streaming recognizer's form (OnlineRecognizerM::Forward): B streams whose state blocks are states_dev [*, PF_ENDPOINT_STATE_INTS]
  // at slot[b] (device memory the recognizer owns), rows = their new fbank rows concatenated [sum n_new, n_mels].  ONE upload
  // (n_new | flush | slot | offsets | rows), the level launch over all rows, the endpoint launch (both profile class "endpoint"),
  // ONE read-back: out = n_events [B] | in_speech [B] | open_begin [B] | events [B, cap, 3].  cap >= max n_new + 1 always suffices.
  // net_states_dev != null (the streaming model score): the attached FSMN-VAD model's stream launch (profile
  // class "vadnet_stream", ONE launch) takes the place of the level launch, on the state blocks net_states_dev
  // [*, vad_stream_layout().bytes] at the same slots, and hands its released counts to the endpoint launch as its n_new; a
  // flush releases the held-back levels in the same launch set.  cap >= max n_new + lfr_m then always suffices.
  void endpoint_streams(int32_t* states_dev, const int32_t* slot, const float* rows, const int32_t* n_new, const int32_t* flush, int B,
                        const pf_endpoint_config& c, int cap, std::vector<int32_t>& out, char* net_states_dev = nullptr);
  // The attached model in streaming form (k_vadnet_stream.hip).  vad_stream_check: PF_ERR_UNSUPPORTED for a model whose two
  // tiles and history window do not fit the LDS (kernels.h kVadStreamMaxLds).  op_vad_model_stream: ONE launch of class
  // "vadnet_stream" over B caller streams through op_stage.h (hostile rows behind n_new[b], sentinel-filled outputs, the guard
  // rule on levels and logits): states [B, state_bytes] in / out, rows [B, ld, n_mels], levels [B, cap] / logits
  // [B, cap, output_dim] (either may be null), n_out [B].  An argument error launches nothing and changes nothing.
  static void vad_stream_check(const VadModel& m);
  void op_vad_model_stream(void* states, const float* rows, const int32_t* n_new, const int32_t* flush, int B, int ld, int n_mels,
                           int32_t* levels, float* logits, int cap, int32_t* n_out);
  void op_ctc_collapse(const int64_t* ids, const float* scores, const int32_t* lens, int B, int T, int blank, int64_t* ids_out,
                       int32_t* first_out, int32_t* last_out, float* score_out, int cap, int32_t* n_out);
  // ---- streaming seams (OnlineRecognizer.cs EncoderProj / DecoderProj) ------
  void online_encoder(const float* speech, int B, int Tc, float* enc_out, float* alphas_out);
  void online_decoder(const float* enc, int B, int Tc, const float* embeds, int L, const int32_t* embeds_len,
                      const float* caches_in, float* logits_out, int64_t* ids_out, float* caches_out);
  int dec_layers() const { return (int)dec_.layers.size(); }
  // ---- the device-resident chunk step (OnlineRecognizerM with SetTokenInfo) ----
  // A stream's slot of the recognizer's device buffer: the carried CIF block (decode_blocks.h CifStreamBlock) at byte 0, the
  // dec_layers() FSMN caches [D, k - 1] fp32 from online_slot_cache_off() on; online_slot_bytes() apart.
  size_t online_slot_cache_off() const;
  size_t online_slot_bytes() const;
  // One chunk of B streams, from the upload of speech [B, Tc, feat_dim] to the ids, without the encoder output, the fired rows
  // or the caches leaving the device: encoder, cif_alpha_stage, cif_stream_kernel on H32_ / alphas_ and the streams' blocks
  // (slots_dev + slot[b] * online_slot_bytes(); cif_reset[b] != 0: from a zero block), counts and fire entries to the host
  // through pinned memory and an event, max_tok = max(counts); 0: return (the carry is updated, the caches are not).  Else the
  // pack, f32_to_f16 and the K | V product, the cache gather (every layer from the slot's layer-0 cache; cache_reset[b] != 0:
  // zeros), decoder16 with L = max_tok exactly, layer norm, vocabulary product, arg-max with its winners' log-probs, the cache
  // scatter, ids and scores back.  out: counts [B], fire_entry [B, Tc + 1], ids / scores [B, max_tok].
  struct OnlineStepOut { int max_tok = 0, cap = 0; std::vector<int32_t> counts, fire_entry; std::vector<int64_t> ids; std::vector<float> scores; };
  void online_step(const float* speech, int B, int Tc, char* slots_dev, const int32_t* slot, const int32_t* cif_reset,
                   const int32_t* cache_reset, int lo, int hi, OnlineStepOut& out);
  // exactly cif_stream_kernel's launch on caller data through op_stage.h: states [B, online_cif_state_bytes(D)] in / out
  void op_online_cif_step(void* states, const float* enc, const float* alphas, const int32_t* reset, int B, int Tc, int D, float threshold,
                          int lo, int hi, float* fired, int32_t* fire_entry, int cap, int32_t* counts);

  // ---- stand-alone ops (parity tests) -------------------------------------
  void op_lfr_cmvn_pad(const float* const* fbank, const int32_t* t80, int B, int sentinel, float* out,
                       int64_t cap, int32_t* tmax);
  // stage_audio + the ONE launch_fbank over all B utterances that run_staged makes; rows [sum t80, n_mels] and t80 [B] back
  void op_fbank_batch(const float* const* samples, const int64_t* n, int B, float* out, int64_t cap, int32_t* t80);
  void op_argmax(const float* x, int64_t rows, int V, int64_t* ids);
  void op_gemm(const float* A, const float* W, const float* bias, int M, int N, int K, int epi, float* C);
  void op_gemm_ex(const pf_gemm_desc& d, const float* A, const float* W, float* C);
  void op_gemm_panel(int M, int N, int out_kind, int form, int padded, const float* bias, const float* A, const float* W, float* C);
  void op_linear32(const float* x, const float* W, const float* bias, const float* resid, int M, int N, int K, bool relu, float* y);
  void op_ffn32(const float* x, const float* W1, const float* b1, const float* W2, const float* b2, int M, int D, int F, float* y);
  // the fp32 graph's Linear, split, LayerNorm, FFN chain and Q, K, V triple on hostile hosts (tests/test_gpu_fp32_conformance.py)
  void op_linear32_ex(const pf_linear32_desc& d, const float* A, const float* W, float* C);
  void op_split_x3(const float* x, int rows, int K, int ldx, int ldo, int Kp, int swap, uint16_t* out);
  void op_layernorm32(const float* x, const float* gamma, const float* beta, int M, int D, int direct_pair, float* out32, uint16_t* pair,
                      int32_t* wrote_pair, const float* W, const float* bias, int N, float* y);
  void op_ffn32_ex(const float* x, const float* W1, const float* b1, const float* W2, const float* b2, int M, int D, int F, float hidden_scale,
                   float* y, uint16_t* hidden_pair, int32_t* pair_written);
  void op_qkv32(const float* x, const float* W, const float* bias, int M, int D, int K, float qscale, float* out);
  void op_gemm_rc(const pf_gemm_rc_desc& d, const float* A, const float* W, float* x_out, float* n16_out, float* n32_out);
  // DynamicQuantizeLinear(x) + MatMulInteger + rescale (+ bias) (+ ReLU) on the int8 MFMA; optional outputs: the uint8
  // activations [M, K], {a_scale, a_zp}, the uint8 weights [N, K] and their per-channel scale / zero point
  void op_qlinear(const float* x, const float* W, const float* bias, int M, int N, int K, int relu, int x_is_f16, float* y,
                  uint8_t* xq_out, float* aparams_out, uint8_t* wq_out, float* wscale_out, int32_t* wzp_out);
  // the parts of the int8 path one at a time, each on a hostile host that enforces kernels.h's contracts (engine_int8.cpp)
  void op_quantize(const float* x, int rows, int cols, int ldx, int x_is_f16, int ld, const float* gamma, const float* beta,
                   int8_t* codes_out, int32_t* rowsum_out, float* params_out);
  // Q == null: quantize_weight_kernel on W; else import_weight_kernel on the stored bytes
  void op_weight(const float* W, const uint8_t* Q, const uint8_t* zp, const float* scale, int N, int K, int ld, int8_t* w_out,
                 int32_t* colsum_out, int32_t* wzp_out, float* wscale_out, int32_t* dz_out);
  void op_qgemm_ex(const pf_qgemm_desc& d, const uint8_t* a_codes, const uint8_t* w_codes, float* y32, float* y16, float* range_out);
  void op_dec_ffn_fused(const pf_dec_ffn_desc& ds, float* t_out, float* n_out, float* x_out);
  void op_dec_mid(const pf_dec_mid_desc& ds, float* x_out, float* q_out, float* tn_out, float* xn16_out, int32_t* ran);
  void op_fsmn_dec_ln(const float* tn, const float* taps, const int32_t* token_num, int B, int L, int k, const float* x, const float* gamma,
                      const float* beta, float* x_out, float* xn16_out);
  // the row kernels of k_norm.hip / k_misc.hip alone; every result comes back with its guard rows (include/paraformer_hip.h)
  void op_layernorm_ex(const float* x, const float* g, const float* b, int64_t rows, int D, int ld16, int ld32, int posenc_T, uint16_t* out16,
                       float* out32);
  void op_layernorm_f16(const uint16_t* x, const float* g, const float* b, int64_t rows, int D, int in_place, uint16_t* out);
  void op_fsmn_dec_stream(const float* tn, const float* taps, const int32_t* len, const float* cache_in, int B, int L, int D, int k,
                          const float* x, float* x_out, float* cache_out);
  // the stand-alone FSMN memory blocks (k_misc.hip) on a hostile host, results guarded (tests/fsmn_ref.py); taps [k, D]
  void op_fsmn_enc_ex(const uint16_t* v16, const float* taps, int B, int T, int D, int k, int ldv, int col, float* y_out);
  void op_fsmn_f32_ex(const float* v, const float* taps, const float* mask, int B, int T, int D, int k, int ldv, int col, int form,
                      float* y_out);
  void op_fsmn_dec_ex(const float* tn, const float* taps, const int32_t* token_num, int B, int L, int D, int k, int hostile,
                      const float* x, float* x_out);
  void op_embed_gather(const float* table, const int32_t* ids, int rows, int D, int vocab, float* out32, uint16_t* out16);
  void op_add_to_f16(const float* a, const float* b, int64_t rows, int D, uint16_t* out16);
  void op_seaco_merge(const float* dha, int ld_dha, const int64_t* dha_ids, int64_t rows, int V, int nobias, int copy_logits,
                      const float* logits_in, int ld_logits, const int64_t* ids_in, float* logits_out, int64_t* ids_out);
  int short_input_max_rows() const { return small_ws_ ? gemm_small_max_rows() : 0; }   // M up to which enc_layer() takes k_gemm_small.hip
  void op_ffn_fused(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* resid,
                    const float* g, const float* be, int M, float* x_out, float* n16_out, const pf_attn_ffn_desc* op = nullptr);
  void op_ffn(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* resid,
              int M, int D, int F, float* y);
  void op_fsmn_enc(const float* v, const float* w, int B, int T, int D, int k, float* y);
  void op_fsmn_dec(const float* tn, const float* w, const int32_t* token_num, int B, int L, int D, int k, float* x);
  // the (Bi)LSTM recurrence through the functions the heads call; form: 0 = as timestamp_head chooses (ring, else the cached graph of
  // step launches), 1 = plain step launches (seaco_head), 2 = f16 ring, 3 = pair-operand ring, 4 = fp32 GEMM + cell per step
  void op_lstm(const float* xg, const float* whh, int B, int T3, int D, int ndir, int form, float* hout);
  // launch_us_alpha + launch_us_peak as the timestamp heads run them
  void op_us_peak(const float* hout, const float* w, const float* b0, float smooth, float noise, const int32_t* token_num, float thr,
                  int B, int T3, int W, float* alphas_raw, float* alphas, float* peak);
  void op_logsoftmax_argmax(const float* x, int64_t rows, int V, float* y, int64_t* ids);
  void op_layernorm(const float* x, const float* g, const float* b, int64_t rows, int D, float* y);
  void op_attention(const float* q, const float* k, const float* v, int B, int Lq, int Lk, int H, float* o);
  void op_attention_ex(const float* q, const float* k, const float* v, int B, int Lq, int Lk, int H, const pf_attn_desc& ds, float* out,
                       void* raw, int64_t raw_bytes, float* range_out, int32_t* ran);
  void op_qkv_attention(const float* x, const float* w, const float* bias, int B, int T, int K, float* q_out, float* k_out,
                        float* v_out, float* ctx_out);
  void op_fsmn(const float* v, const float* w, const float* mask, int B, int T, int D, int k, float* y);
  void op_cif(const float* H, const float* alphas, int B, int T, int D, float thr, int Lcap, float* E,
              int32_t* fire_count, int32_t* token_num, int32_t* L_out);
  // the predictor's alpha stage on caller data with the loaded predictor weights: cif_alpha_stage (math_mode 0) or
  // cif_alpha_stage32 (math_mode 1 / 3), the bodies the pipelines run; alphas [B, T+1] incl. the tail weight
  void op_cif_alphas(const float* H, int B, int T, float* alphas);
  void op_encoder(const float* speech, int B, int T, float* H);

  // ---- profiling -----------------------------------------------------------
  void profile_enable(bool on) { prof_on_ = on; }
  void profile_reset();
  void profile_select(const std::string& cls) { prof_only_ = cls; }
  bool profile_get(const std::string& cls, double* ms, int64_t* launches, double* flops_per_launch);
  std::string profile_kernel(const std::string& cls) const;   // GEMM classes: the kernel the launcher chose ("" otherwise)
  double last_flops() const { return last_flops_; }

  const ModelCfg& model() const { return mc_; }
  const FrontendCfg& frontend() const { return fc_; }
  const std::vector<float>& embed_table() const { return embed_host_; }   // SenseVoice [16,560]
  std::mutex& mutex() { return mu_; }
  int device() const { return device_; }
  // the batched front-end of run_staged (LFR + CMVN + pad in one kernel) computes what frontend_host + PadSequence compute
  bool staged_frontend_matches_host() const { return fc_.lfr_m * fc_.n_mels == mc_.feat_dim && (!cmvn_shift_ || cmvn_dim_ == mc_.feat_dim); }
  bool has_device_prompt() const { return sv_prompt_ != nullptr; }

 private:
  struct Tensor { const float* dev = nullptr; std::vector<int64_t> shape; int64_t numel = 0; bool u8 = false; };   // u8: dev points at bytes
  struct ProfClass { std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; double flops = 0; int64_t n = 0; std::string kernel; };

  void load_weights(const pf_engine_config& cfg);
  const Tensor& tensor(const std::string& name) const;          // float32 tensors only (a u8 tensor here is a format error)
  const Tensor* tensor_u8(const std::string& name) const;       // nullptr when absent
  bool has_tensor(const std::string& name) const { return tensors_.count(name) != 0; }
  Lin make_lin(const std::string& prefix, bool bias);
  half_t* make_dec_ffn_image(const Lin& w1, const LNp& fn, const Lin& w2);
  // layers, final block and after_norm of `prefix` (".layers.N", ".final", ".after_norm"); the caller loads `out`.  fused_images:
  // also the weight images of the split FFN / fused middle forms (the ASR decoder alone takes those forms)
  DecStack load_dec_stack(const std::string& prefix, int n_layers, int ffn, int fsmn_k, bool fused_images);
  LNp make_ln(const std::string& prefix, int width);
  void release();
  float* make_fsmn_wT(const std::string& name, int K = 0);
  void* dalloc(size_t bytes);
  void ensure(DevBuf& b, size_t bytes);
  void build_pe(int T);
  void encoder(const float* speech_dev, int B, int T, bool pre_encoded = false);
  // the LayerNorm applied to the residual stream right after a layer's FFN-down, and where its results go
  struct EncNext { LNp ln; half_t* n16 = nullptr; float* n32 = nullptr; bool keep_x = true; const EncLayer* next = nullptr; };
  bool qkv_done_ = false;            // the previous layer's launch has already written this layer's Q | K (blocked) and V
  int v_pp_ = 0;                     // which of the two V buffers the current layer reads (the fused launch writes the other)
  // first: 0 = not the first layer, 1 = first (x sqrt(d) + position encoding fused into norm1), 2 = first, input already encoded
  void enc_layer(const EncLayer& L, int first, const float* speech_dev, int B, int T, const EncNext& nx);
  // im2col -> conv GEMM with ReLU -> launch_cif_alpha (scan: then the fire scan into *scan, as the offline pipeline has it)
  void cif_alpha_stage(const half_t* H16, int B, int T, half_t* col16, float* conv32, float* alphas, const CifPlan* scan);
  void cif_alpha_stage32(const float* H32, int B, int T, float* col32, float* conv32, float* alphas);
  // ---- the stages of forward_device, each written once.  An arithmetic (f16; int8 = math_mode 2, engine_int8.cpp: every Linear as
  // DynamicQuantizeLinear + MatMulInteger on v_mfma_i32_32x32x32_i8; fp32 = math_mode 1 / 3, engine_fp32.cpp) has of its own:
  // its encoder (leaves H32_, H16_ except fp32, alphas_ and plan_ bound), its decoder arena, and its walk + vocabulary product
  void encoder_int8(const float* speech_dev, int B, int T);
  void encoder_fp32(const float* speech_dev, int B, int T);
  void sensevoice_head(int B, int T, bool want_logits);
  void predictor(int B, int T);                      // alphas, fire scan, plan export; starts the timestamp head
  void dec_kv_ahead(int B, int T);                   // f16: all layers' K | V projections of the encoder memory -> ws_kv_
  int decoder_length(int B, int T);                  // the forward's one host round trip: L, and last_'s shape
  DecStage dec_arena_f16(int B, int T, int L);
  DecStage dec_arena_int8(int B, int T, int L);
  DecStage dec_arena_fp32(int B, int T, int L);
  void cif_embeds(DecStage& d, int B, int T, int L, const char* cls);   // cls: the launches' profile class, or null for no bracket
  void asr_decoder_f16(DecStage& d, int B, int T, int L);              // the walk, then logits_ = the vocabulary product
  void asr_decoder_int8(DecStage& d, int B, int T, int L);
  void asr_decoder_fp32(DecStage& d, int B, int T, int L);
  // arg-max | SeACo head (d with hot-word inputs) | timestamp join | ids copy | decoding extras, over B * L rows of logits_
  void finish(int B, int L, bool want_logits, const DecStage* d, const char* cls);
  const QLin& qlin(const Lin& l, bool bias = true);
  const QLin& qlin_raw(const float* w32, const float* bias, int N, int K);
  // y = dequant(quant(x) w_q^T) + bias [* scale on the first scale_cols columns] [+ add2] [+ resid] [ReLU]; x fp32 [M, ldx] or f16
  void qgemm(const char* cls, const Lin& w, bool bias, const float* x32, const half_t* x16, int ldx, int M, float* out32, int ld32,
             half_t* out16, int ld16, const float* resid, int ldr, const float* add2, int ld2, bool relu, int scale_cols, float scale,
             const LNp* ln = nullptr, const QAct* pre = nullptr, int range = 0);   // range: 1 = leave the result's {min, max} pairs
                                                                                    // in q_part_, 2 = the input's are there already
  bool lin_quantised(const Lin& l) const;            // is this Linear a DynamicQuantizeLinear + MatMulInteger pair in the model file?
  void fgemm_in_int8(const char* cls, const Lin& l, bool bias, const float* x32, const half_t* x16, int ldx, int M, float* out32, int ld32,
                     half_t* out16, int ld16, const float* resid, int ldr, const float* add2, int ld2, bool relu, int scale_cols,
                     float scale, const LNp* ln, int range);
  void seaco_kv_int8(const float* hw32, const half_t* hw16, int NJ, half_t* kv16, int ldkv);
  void decoder_int8(const DecStack& S, const DecRun& r);
  enum { kRangeOut = 1, kRangeIn = 2 };
  // quantise an activation tensor into `dst` (min / max pass, quantise pass); ln: of LayerNorm(x32), which is never stored
  void quantize_act(const QAct& dst, int kpad, const float* x32, const half_t* x16, int ldx, int64_t M, int K, const LNp* ln,
                    bool have_range = false);
  void timestamp_head_fp32(int B, int T);
  void seaco_head_fp32(int B, int L, const float* e0, const float* hid, bool want_logits);
  // fp32 LSTM over rows [Bn * Tn] of x (row b * Tn + t): hout[(b * Tn + t) * ldh + col0 .. + D); reverse = time runs backwards
  void lstm_fp32(const float* x, int Bn, int Tn, const float* w_ih, const float* w_hh, const float* bias, bool reverse,
                 float* xg, float* gates, float* hbuf, float* cbuf, float* hout, int ldh, int col0);
  // the recurrence of lstm_fp32 on prepared gate inputs xg [Bn * Tn, 4D]: one fp32 GEMM + one cell kernel per time step
  void lstm_fp32_steps(const float* xg, int Bn, int Tn, const float* w_hh, bool reverse, float* gates, float* hbuf, float* cbuf,
                       float* hout, int ldh, int col0);
  // the f16-operand recurrences on prepared LstmArgs (k_bicif.hip); the heads and op_lstm run the same functions
  void lstm_clear16(const LstmArgs& a);              // h_{-1} = c_{-1} = 0 of the per-step form: hstate [ndir][2][B][D], cstate [ndir][B][D]
  void lstm_steps16(LstmArgs a);                     // T3 launches of lstm_step_kernel
  // clears the state, then the ring (sw: 64 sync words) when every workgroup fits on the device, otherwise the T3 step launches as a
  // cached hipGraph; returns whether the ring ran.  ring_only: PF_ERR_UNSUPPORTED instead of the step launches
  bool lstm_recurrence16(LstmArgs a, unsigned* sw, bool ring_only = false);
  bool lstm_ring_x3(const LstmArgs& a, unsigned* sw);   // the pair-operand ring (math_mode 3); false = does not fit, nothing was launched
  void enc_layer_fp32(const EncLayer& L, bool first, const float* speech_dev, int B, int T, float** bufs);
  void timestamp_head(int B, int T);
  void start_timestamp_head(int B, int T);
  void seaco_head(int B, int L, const float* e0, const float* hid32, bool want_logits);
  void gemm(const char* cls, const Lin& w, const half_t* A, int lda, int M, float* out32, int ld32,
            half_t* out16, int ld16, const float* resid, int ldr, const float* add2, int ld2, bool relu,
            int scale_cols, float scale, bool bias = true, int blocked = 0);   // blocked: 1 = out_f16 blocked, 2 = A blocked
  void gemm_small_call(const char* cls, const Lin& w, GemmSmallArgs g, bool bias = true);
  void dec_ffn_hidden(const char* cls, const Lin& w1, const LNp& fn, const half_t* xn16, int lda, int rows, half_t* h16);
  void decoder16(const DecStack& S, const DecRun& r);      // f16: the plain nine-launch layer (bias decoder, streaming seam)
  void decoder32(const DecStack& S, const DecRun& r);      // math_mode 1 / 3
  AttnArgs cross_attn_args(const half_t* q, const half_t* k, const half_t* v, int kv_rs, int64_t kv_bs, half_t* o, int B, int L, int Lk) const;
  // the walk buffers in the order every arena keeps them; rows = the arena's padded row count
  DecBufs carve_dec16(Arena& a, int64_t rows, int F, bool with_h32);
  DecBufs carve_dec32(Arena& a, int64_t rows, int F);
  DecBufs carve_dec8(Arena& a, int64_t rows, int F);
  template <class Fn> auto carve_into(DevBuf& ws, size_t align, Fn fn) {   // fn(Arena&) lays the arena out: once to measure, once in place
    Arena m{nullptr, align}, a{nullptr, align};
    fn(m); ensure(ws, m.off); a.base = (char*)ws.p;
    return fn(a);
  }
  void prof_begin(const char* cls, double flops);
  void prof_end(const char* cls);
  // a stand-alone op's timed launch loop (engine_ops.cpp): PF_OP_REPEAT launches, class "gemm_op" then "gemm_op_warm"
  template <class Fn> void op_timed(double flops, Fn launch);
  template <class Fn> void fsmn_timed(Fn launch);
  void* op_ws(const struct StageCarve& st);                  // ws_tmp_ grown to the carve's size (op_stage.h)

  // dither stream: seed of call c = hash(dither_seed, c); an engine built with the same seed replays the same
  // features for the same sequence of front-end calls
  uint32_t dither_calls_ = 0;
  uint32_t next_dither_seed() { return fc_.dither_seed * 2654435761u + (dither_calls_++) * 40503u; }
  int device_ = 0;
  hipStream_t stream_ = nullptr;
  int32_t* step_host_ = nullptr; int32_t* step_host_dev_ = nullptr; int step_host_cap_ = 0; bool step_host_tried_ = false;   // online_step: counts | fire entries, pinned
  hipEvent_t ev_step_ = nullptr;
  DevBuf ws_step_;                    // online_step: speech-independent scratch that must survive the decoder arena's growth
  int32_t* plan_host_ = nullptr; int32_t* plan_host_dev_ = nullptr; int plan_host_cap_ = 0;   // CIF counts exported into pinned host memory
  void ensure_plan_host(int B);
  void export_plan(int B);
  int32_t read_back_plan(int B);
  hipStream_t aux_stream_ = nullptr;   // carries the decoder-length read-back, so stream_ keeps running (K/V projections) meanwhile
  hipEvent_t ev_scan_ = nullptr;       // CIF scan finished
  // the BiCIF timestamp head depends on the encoder output and token_num only: it runs on its own stream beside the
  // decoder (its recurrence is 1500 dependent steps on 128 workgroups — latency, not throughput) and is joined before
  // the call's last copy (PF_TS_STREAM=0 keeps it on the main stream)
  hipStream_t ts_stream_ = nullptr;
  hipEvent_t ev_ts_ = nullptr, ev_enc_ = nullptr;
  bool ts_pending_ = false, ts_defer_copy_ = false;
  size_t ts_copy_floats_ = 0;
  void join_ts();
  void own_hardware_queue_ts();
  void own_hardware_queue();         // round 6: the main stream must not share a hardware queue with another live engine's (see engine.cpp)
  bool dec_mid_ = true;              // PF_DEC_MID: finishing pass + norm2 + FSMN + residual + norm3 + q-projection in one launch (k_decmid.hip)
  bool gemm_panel_ = true;           // PF_GEMM_PANEL: the K | V and vocabulary products on the panel-resident kernel where its rule admits them (0: gemm_f16_pp3)
  int ffn_fused_min_rows_ = 1200;    // PF_FFN_MIN: below, 64-row tiles leave most CUs idle and the persistent kernels tie or win (tools/mid_rows.py)
  int qkv_split_min_tiles_ = 256;    // PF_QKV_MIN: least number of 256 x 192 tiles for which the split form is chosen
  int qkv_split_min_fill_ = 60;      // PF_QKV_FILL: ... and least fill (percent) of its rounds of tiles (85 was the break-even with ONE step in
                                     // flight; with two, the other engine's kernels run on the CUs a short last round leaves)
  int cus_ = 256;                    // compute units the persistent kernels size their grids for (cu_limit)
  unsigned* lstm_err_ = nullptr;     // device time-out word of the last persistent LSTM launch (checked at the next result sync)
  void check_async_errors();         // after a stream sync: raises what a kernel of the finished forward reported through a flag word
  void attention32(const float* q, int64_t q_bs, int q_rs, const float* k, int64_t k_bs, int k_rs, const float* v, int64_t v_bs, int v_rs,
                   float* o, int64_t o_bs, int o_rs, int B, int H, int Lq, int Lk, bool only_operand = false);
  // LayerNorm of the fp32 graph whose result is ONLY the A operand of gemm32 calls that follow (xn names it): in math_mode 3
  // (D = 512, above the short-input threshold) it is written as that operand pair and xn is not touched
  void layernorm32(const float* x, int M, int D, const LNp& ln, float* xn);
  bool x3a_pair_only_ = false;       // x3a_src_ exists ONLY as the pair in ws_x3a_ (its fp32 form was never written)
  bool x3_mode_ = false;             // math_mode 3: the fp32 graph with every large Linear as three f16 MFMA products of (hi, lo') operand pairs
  void x3_poison(int M, int N, int K);     // stand-alone ops: the three x3 arenas at the size an [M, K] x [N, K] product needs, filled with a large finite pattern
  void x3_forget(const float* W);          // drops W's cached pair image (stand-alone ops: their weights live in a scratch arena)
  std::map<std::pair<const float*, int>, half_t*> x3w_;   // (fp32 weight, rows N) -> its [lo' | hi] f16 pair image (built on first use; the fused
                                                          // Q | K | V product and the three separate ones name the same first row)
  DevBuf ws_x3a_, ws_x3t_, ws_x3h_;
  bool x3_pair_live_ = false; int x3_pair_M_ = 0, x3_pair_K_ = 0;   // ws_x3h_ holds the (hi | lo') pair the next gemm32 consumes
  enum { kX3OutPair = 1, kX3InPair = 2, kX3SameInput = 4 };
  const float* x3a_src_ = nullptr; int x3a_M_ = 0, x3a_K_ = 0, x3a_ld_ = 0; half_t* x3a_buf_ = nullptr;   // what ws_x3a_ holds the pair of
  // profile class of the gemm32 / attention32 calls that follow (bench.py's `exact` roofline; "gemm32_*" / "attn32_*")
  const char* cls32_ = "gemm32_misc";
  void gemm32_impl(const float* A, int lda, const float* W, int ldw, const float* bias, int M, int N, int K, float* out, int ldc,
                   const float* resid, int ldr, bool relu, int scale_cols, float scale, int flags, const float* resid2);
  void gemm32(const float* A, int lda, const float* W, int ldw, const float* bias, int M, int N, int K, float* out, int ldc,
              const float* resid, int ldr, bool relu, int scale_cols, float scale, int flags = 0, const float* resid2 = nullptr);
  bool fp32_mode_ = false;           // math_mode 1: every GEMM / attention product on the fp32 MFMA path (parity runs)
  bool int8_mode_ = false;           // math_mode 2: Linear layers dynamically quantised to uint8, products on the int8 MFMA
  std::map<const float*, QLin> qlins_;
  std::map<const float*, std::string> lin_names_;     // float32 `<linear>.weight` device pointer -> `<linear>` (stored int8 bytes lookup)
  std::vector<std::string> int8_exclude_;   // config key `int8_exclude`: Linear name prefixes a synthetic container keeps in float
  bool any_stored_q_ = false;        // the container carries stored bytes of an int8 export
  DevBuf ws_qf_, ws_seaco_q_;        // f16 operand of an un-quantised Linear; quantised bias_embed rows
  DevBuf ws_q_;                      // quantised activations: a' [Mp, Kpad], row sums, {scale, zp}, min / max scratch
  int8_t* q_a_ = nullptr; int32_t* q_rowsum_ = nullptr; float* q_params_ = nullptr; unsigned* q_scratch_ = nullptr;
  int64_t q_rows_ = 0; int q_kpad_ = 0;
  float* q_part_ = nullptr;          // {min, max} per workgroup of a min / max pass (k_quant.hip)
  void ensure_q(int64_t rows, int kpad);
  ModelCfg mc_;
  FrontendCfg fc_;
  std::mutex mu_;

  // weights
  void* blob_dev_ = nullptr;        // device copy of the PFW data section (owned unless external)
  bool blob_owned_ = false;
  std::map<std::string, Tensor> tensors_;
  std::vector<void*> owned_;        // every other device allocation
  std::vector<EncLayer> enc_, tp_;
  DecStack dec_, bias_dec_;         // ASR decoder, SeACo bias decoder
  LNp enc_after_, tp_norm_;
  Lin cif_conv_, ctc_;
  const float* cif_out_w_ = nullptr;
  const float* cif_out_b_ = nullptr;
  struct LstmLayer { Lin ih; half_t* whh = nullptr; };
  std::vector<LstmLayer> seaco_lstm_;
  const float* seaco_embed_w_ = nullptr;
  std::vector<int32_t> hotwords_;   // [n_hotwords_, 10]
  int n_hotwords_ = 0;
  Lin ts_up_, ts_ih_;               // BiCIF: ConvTranspose1d as [3D, D], W_ih of both directions [8D, D]
  half_t* ts_whh_ = nullptr;        // [2][4D][D]
  half_t* ts_whh_x3_ = nullptr;     // math_mode 3: [2][4D][hi (D) | lo' (D)] pair rows of the fp32 W_hh (built at first use)
  const float* ts_out_w_ = nullptr;
  const float* ts_out_b_ = nullptr;
  std::vector<float> embed_host_;
  float* sv_prompt_ = nullptr;      // SenseVoice: device [4, feat_dim] query rows (effective ids)

  // front-end
  FbankTables* fb_ = nullptr;
  float* cmvn_shift_ = nullptr;
  float* cmvn_scale_ = nullptr;
  int cmvn_dim_ = 0;

  // workspace
  DevBuf ws_f32_;
  float* small_ws_ = nullptr;        // short-input GEMM: split partials
  float* cif_conv_w32_ = nullptr;    // fp32 mode: the CIF conv as a [D][taps*D] GEMM operand
  float* ts_up_w32_ = nullptr;       // fp32 mode: the transposed conv as a [(j, out)][in] GEMM operand
  DevBuf ws_pcm_;                   // stage_pcm: the raw bytes of the batch | its PcmJob table
  DevBuf ws_audio_, ws_meta_, ws_fbank_, ws_speech_, ws_enc_, ws_dec_, ws_decffn_, ws_kv_, ws_pe_, ws_tmp_, ws_ts_, ws_seaco_, ws_seaco_in_, ws_seaco_hw_;
  bool seaco_hw_valid_ = false;     // ws_seaco_hw_ holds the embedder output / K,V rows of the CURRENT hot-word list (f16 path)
  int pe_T_ = 0;
  // encoder views (valid after the arithmetic's encoder)
  float* x_ = nullptr; half_t* xn16_ = nullptr; half_t* qkv16_ = nullptr; half_t* ctx16_ = nullptr;
  float* fsm_ = nullptr; half_t* h16_ = nullptr; float* H32_ = nullptr; half_t* H16_ = nullptr;
  float* alphas_ = nullptr; CifPlan plan_{};
  float* col32_ = nullptr;          // fp32: the predictor's im2col operand (fsm_ takes its conv result)
  float* us_peak_ = nullptr;
  struct { const float* xg = nullptr; int B = 0, T3 = 0; const void* rest[4] = {nullptr, nullptr, nullptr, nullptr}; int ndir = 0; } lstm_graph_key_;
  hipGraphExec_t lstm_graph_exec_ = nullptr;
  // decoder views
  float* logits_ = nullptr; int64_t* ids_dev_ = nullptr; int logits_ld_ = 0;
  // staged audio
  std::vector<int64_t> st_n_; std::vector<int32_t> st_t80_; int st_B_ = 0, st_T_ = 0;
  int64_t st_total_frames_ = 0;
  const float* st_audio_ext_ = nullptr;   // base of the externally staged audio (stage_device_audio); null: ws_audio_
  HostBatchOut last_;
  int decode_flags_ = 0;
  std::vector<int32_t> dec_len_;     // n_b of the forward being queued (valid rows per utterance); empty: every row of the batch
  std::vector<int32_t> ctc_len_;     // the lengths the queued collapse reads (clamped to [0, L]); alive until the next forward
  DevBuf ws_score_, ws_ctc_;         // arg-max log-probs [B * L]; the collapse's len [B] and result block (HostBatchOut::ctc)
  float* score_buf(int64_t rows);    // where the arg-max leaves its winners' values; null without decode flags
  int topk_k_ = 4;                   // K of PF_DECODE_TOPK
  DevBuf ws_topk_;                   // the top-k result block (HostBatchOut::topk); allocated with the flag only
  // the arg-max form of a pipeline head: the top-k kernel reads the log-probs the arg-max leaves in place
  int beam_w_ = 16, beam_n_ = 16;    // W / N of PF_DECODE_CTC_BEAM
  DevBuf ws_beam_;                   // the beam result block (HostBatchOut::beam) | len [B] | prefix nodes; allocated with the flag only
  // an installed hot-word set (set_ctc_hotwords for the CTC search, set_nbest_hotwords for the n-best search)
  struct HotDev {
    float boost = 0.f;               // > 0: a set is installed; its table lives in buf
    int A = 0;                       // columns of the table
    std::vector<int32_t> ids, lens;  // the installed set as given: a call with the same content keeps the table
    DevBuf buf;                      // tok_col [V] | table [S, A]; allocated by the setter only
    void clear() { boost = 0.f; A = 0; ids.clear(); lens.clear(); }
  };
  HotDev hot_, nbs_hot_;
  void install_hotwords(HotDev& d, const char* who, const int32_t* ids, const int32_t* lens, int n, float boost);
  // the language model's image in a buffer of its own: uploaded when a model is first used, kept (with a reference to the
  // model) while the same one is given
  struct LmDev { DevBuf buf; std::shared_ptr<const LmImage> src; };
  LmDev lm_inst_, lm_op_;            // the installed model's image (set_ctc_lm / set_nbest_lm: an engine is of one kind), and
                                     // the one pf_op_* last used
  const int32_t* lm_device_image(LmDev& d, const std::shared_ptr<const LmImage>& lm);
  std::shared_ptr<const LmImage> lm_;   // the installed model (nullptr: none), its weights and flags
  // an auxiliary network: the attached model, its image on the device (with the model it was uploaded from) and a workspace;
  // allocated by an attach / a run only, freed by a detach (attach_model with nullptr)
  template <class M> struct ModelDev { DevBuf buf; std::shared_ptr<const M> src; };
  template <class M> void attach_model(std::shared_ptr<const M>& on, ModelDev<M>& dev, DevBuf& ws, const std::shared_ptr<const M>& m);
  // the FSMN-VAD model (set_vad_model): ws_vadnet_ holds the two p buffers the launches alternate between
  std::shared_ptr<const VadModel> vadnet_;
  ModelDev<VadModel> vadnet_dev_;
  DevBuf ws_vadnet_;
  // the punctuation model (set_punc_model): as above; ws_punc_ holds ids, offsets, x, the two q | k | v buffers, ctx, logits, p, cut
  std::shared_ptr<const PuncModel> punc_;
  ModelDev<PuncModel> punc_dev_;
  DevBuf ws_punc_;
  // the speaker model (set_spk_model): as above; ws_spk_ holds the window table, the rows, the head's three activation buffers,
  // the TDNN's frames, the four X buffers, the embeddings and the frames asked for
  std::shared_ptr<const SpkModel> spk_;
  ModelDev<SpkModel> spk_dev_;
  DevBuf ws_spk_;
  // the 15 launches over rows that are on the device: T / toff / tpoff [B] / [B + 1] / [B + 1] device arrays, scratch from ws
  void run_spk(const float* rows_dev, const int32_t* T_dev, const int64_t* toff_dev, const int64_t* tpoff_dev, const int64_t* xoff_dev, int B,
               int Tmax, int64_t total, int64_t totalp, char* scratch, float* emb_dev, float* frames_dev);
  static size_t spk_scratch_bytes(const SpkModel& m, int64_t total, int64_t totalp);
  void run_punc(const int32_t* ids, const int64_t* off, const int32_t* last, int B, float* logits, float* x0, int32_t* p, int32_t* cut);
  void run_vadnet_stream(char* states_dev, const int32_t* slot_dev, const float* rows_dev, const int32_t* off_dev, int64_t ldx,
                         const int32_t* n_new_dev, const int32_t* flush_dev, int B, float* logits_dev, int32_t* levels_dev, int64_t cap,
                         int32_t* n_out_dev);
  void run_vadnet(const float* rows_dev, const int64_t* off_dev, int B, int64_t total, int n_mels, float* logits_dev, int32_t* levels_dev);
  float lm_alpha_ = 0.f, lm_beta_ = 0.f;
  int lm_flags_ = 0;
  // the n-best search (set_nbest_search; 0: off), its model with weights and flags (set_nbest_lm), its workspace
  int nbs_w_ = 0, nbs_n_ = 0;
  std::shared_ptr<const LmImage> nbs_lm_;
  float nbs_alpha_ = 0.f, nbs_beta_ = 0.f;
  int nbs_flags_ = 0;
  DevBuf ws_nbs_;                    // the result block (HostBatchOut::nbs) | back-pointers [B, L, W]; allocated by a search only
  void queue_nbest_search(int B, int L);
  // PF_DECODE_ALIGN: the targets of the next forward (int32, [B, align_cap_]; align_B_ = 0: none) and those of the forward
  // being queued (alive until the next forward: the host-to-device copies may read them after the call returns)
  std::vector<int32_t> align_tgt_, align_len_, align_tgt_q_, align_len_q_;
  int align_B_ = 0, align_cap_ = 0;
  DevBuf ws_align_;                  // the result block (HostBatchOut::align) | jobs | len [B] | targets | back-pointers; with the flag only
  int argmax_mode(bool want_logits) const { return (want_logits || (decode_flags_ & (PF_DECODE_TOPK | PF_DECODE_ALIGN))) ? 2 : 1; }
  // Behind the ids copy: the scores' copy, then one step per decoder flag.  A step lays out its ws_* buffer with the block
  // type of decode_blocks.h (the result block, its scratch behind it), launches, and queues the one copy of the block.
  void queue_decode_results(int B, int L);
  void queue_topk(int B, int L);
  void queue_ctc_beam(int B, int L);
  void queue_align(int B, int L);
  void queue_ctc_collapse(int B, int L);
  // What every fetch starts with: waits for the forward, raises what its kernels reported, and returns the calling thread's
  // published result (else the engine's last one) after checking that it was made with all of `flags` (else `refusal`)
  const HostBatchOut& fetch_result(int flags, const char* refusal);
  uint64_t uid_ = 0;                 // key of this engine in the per-thread result store
  static uint64_t register_uid();
  static void unregister_uid(uint64_t id);
  bool last_logits_ = false;
  double last_flops_ = 0;

  std::function<int(int)> l_hook_;
  bool prof_on_ = false;
  std::string prof_only_;
  std::map<std::string, ProfClass> prof_;
};

}  // namespace pf
