// online.h — C++ mirror of the reference's STREAMING classes above the device engine:
//   OnlineRecognizer  AliParaformerAsr/OnlineRecognizer.cs:14-542   (Forward :336-403, PredictorProj :126-231 =
//                     the C# CIF with the carried integrator, DecodeMulti :405-437)
//   OnlineStream      AliParaformerAsr/OnlineStream.cs:7-358        (AddSamples :79-105, InputSpeech :106-160,
//                     GetDecodeChunk :162-208: splice cache, LFR, CMVN, x sqrt(512), position encoding, 10-frame cache)
//   OnlineWavFrontend AliParaformerAsr/OnlineWavFrontend.cs:63-80 (LFR without left context), :152-188 (PE)
//   OnlineModel       AliParaformerAsr/OnlineModel.cs:141-165 (DynamicMask), :199-247 (stack / unstack of the FSMN caches)
// The two ONNX sessions (encoder, decoder) are replaced by Engine::online_encoder / online_decoder.
#pragma once
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "engine.h"
#include "hostutil.h"

namespace pf {

// ---- pure host pieces, exposed for parity tests ---------------------------------------------------------------
// OnlineWavFrontend.ApplyLfr (:63-80): windows of lfr_m frames every lfr_n, NO left context;
// t_lfr = t/lfr_n - 1 when t % lfr_n < lfr_m - lfr_n, else t/lfr_n
std::vector<float> online_apply_lfr(const std::vector<float>& fbank, int n_mels, int lfr_m, int lfr_n);
// OnlineWavFrontend.SinusoidalPositionEncoder (:152-188): adds rows start_idx .. of the table whose row p-1 is
// [sin(inv_i * p) | cos(inv_i * p)], inv_i = exp(-(i + 1) * ln(1e4) / (dim/2 - 1))   (note i + 1: differs from offline)
void online_position_encode(std::vector<float>& x, int timesteps, int dim, int start_idx);
// OnlineModel.DynamicMask (:141-165): alphas[0:5] = 0 and alphas[15:] = 0 (chunk_size 5, lfr 10)
void online_dynamic_mask(std::vector<float>& alphas, int chunk_size = 5, int lfr = 10);
// one stream's share of PredictorProj (:146-197): integrate-and-fire over [carried pair ; new frames].
// hiddens [n][D], alphas [n]; returns fired frames; carry_alpha / carry_hidden = the new cache
void online_cif(const std::vector<std::vector<float>>& hiddens, const std::vector<float>& alphas, float threshold,
                std::vector<std::vector<float>>& fired, float& carry_alpha, std::vector<float>& carry_hidden,
                std::vector<int32_t>* fire_entry = nullptr);   // fire_entry: the walked entry that completed each fired frame
// One chunk step of one stream on its carried state block (decode_blocks.h CifStreamBlock, online_cif_state_bytes(D) bytes; a
// zero-filled block is the constructor's state): DynamicMask with [lo, hi) inside, online_cif over [carry ; Tc frames], the new
// carry written back.  fired [cap, D] (rows at and beyond the count zero), fire_entry [cap] (entry 0 = the carry, entry j =
// chunk position j - 1; -1 at and beyond the count).  Returns the count.  cif_stream_kernel (k_cif_stream.hip) is its device
// twin, bit for bit.  PF_ERR_INVALID_ARG: null pointers, Tc <= 0, D % 4 != 0, cap < Tc + 1.
size_t online_cif_state_bytes(int D);
int online_cif_step(void* state, const float* hiddens, const float* alphas, int Tc, int D, float threshold, int lo, int hi, bool reset,
                    float* fired, int32_t* fire_entry, int cap);
// OnlineRecognizer.DecodeMulti (:405-437) for one stream
std::string online_decode_text(const std::vector<std::string>& tokens, const std::vector<int64_t>& ids);
// Streaming punctuation (paraformer_hip.h "Punctuation, streaming"; tests/punc_stream_ref.py committed_words): the words of
// online_decode_text(tokens, ids) as host_punc_words splits them.  While the last token that contributes text ends in "@@" the
// last word is held back (n_committed = words.size() - 1): the next piece changes it.
struct OnlineCommitted { std::string text; std::vector<PuncWord> words; size_t n_committed = 0; };
OnlineCommitted online_committed_words(const PuncModel& m, const std::vector<std::string>& tokens, const std::vector<int64_t>& ids);
std::string online_word(const OnlineCommitted& c, size_t i);
// the committed words of one call must be a prefix of the next call's: PF_ERR_RECOGNITION otherwise
void online_check_committed_prefix(const std::vector<std::string>& before, const OnlineCommitted& now);

class OnlineRecognizerM;
class Recognizer;
class Stream;

class OnlineStreamM {
 public:
  explicit OnlineStreamM(std::shared_ptr<OnlineRecognizerM> r);
  ~OnlineStreamM();
  void AddSamples(const float* samples, int64_t n);           // OnlineStream.cs:79-105
  // ---- endpointing (OnlineRecognizerM::SetEndpoint; paraformer_hip.h "Streaming endpointing"; no counterpart in the reference)
  // The input is complete: every cached chunk goes through InputSpeech, the samples short of a chunk zero-padded to one (the
  // online model then decodes the tail too); the GetResults that has decoded the last chunk flushes the detector.  A later
  // AddSamples throws PF_ERR_INVALID_ARG.
  void InputFinished();
  // a finished sentence: [begin_ms, end_ms) in the caller's audio, PF_ENDPOINT_* kind, the online model's text at the closing
  // chunk, the second pass's text (= first_pass without one) and the offline stream that produced it (null without one)
  struct SentenceM {
    int begin_ms = 0, end_ms = 0, kind = 0; std::string first_pass, text; std::shared_ptr<Stream> offline;
    std::vector<pf_online_token> tokens;                      // TokenInfo as of the closing call (empty without SetTokenInfo)
    std::string punctuated;                                   // SetPuncModel: first_pass under its marks, the flush's edit applied
    std::vector<int32_t> punc_ids;
  };
  // SetPuncModel: of the last GetResults, the open text under the marks of its committed words (a held-back word appended raw),
  // the mark and the restart flags (bit 0 sentence end, bit 1 forced restart) of every committed word
  std::string Punctuated;
  std::vector<int32_t> PuncIds, PuncFlags;
  std::vector<SentenceM> Sentences;
  bool InSpeech = false;                                      // a sentence is open (as of the last GetResults)
  int OpenBeginMs = -1;
  bool GetDecodeChunk(std::vector<float>& chunk);             // :162-208 (chunk = [10 cached ; 10 new] x 560), false = not enough frames
  std::vector<int64_t> Tokens{0, 0};                          // :52
  // SetTokenInfo: what is known about Tokens[i], index for index (paraformer_hip.h "Streaming token times and scores");
  // token_info() first brings it to Tokens' length (the constructor's zeros: no flags).  Empty with the mode off.
  std::vector<pf_online_token> TokenInfo;
  const std::vector<pf_online_token>& token_info();           // (the caller holds mu)
  std::vector<std::vector<float>> States;                     // 16 x [512*10]
  std::vector<std::vector<float>> CifHidden;                  // carried hidden(s)
  std::vector<float> CifAlpha;
  std::vector<float> Speech;                                  // OnlineInputEntity.Speech (fbank frames, 80-dim)
  bool disposed = false;
  std::shared_ptr<OnlineRecognizerM> owner;
  // The reference serialises AddSamples / InputSpeech / GetDecodeChunk with lock(obj) (OnlineStream.cs:30,86,116,174):
  // a capture thread may add samples while a decode thread runs GetResults on the same stream.  Here the lock is per
  // stream; it is never held while the engine mutex is taken (AddSamples releases it around the fbank call), so
  // Forward (engine mutex, then stream state) cannot dead-lock against it.
  std::mutex mu;

 private:
  friend class OnlineRecognizerM;
  // n_caller: how many of the chunk's leading samples are the caller's (0 for the chunk of silence the constructor queued)
  void InputSpeech(const std::vector<float>& samples, size_t n_caller);   // :106-160
  void ResetDecoder();                                        // the decoder context back to the constructor's, Tokens cleared
  std::vector<float> cache_samples_, cache_feats_, cache_lfr_splice_;
  bool first_input_ = true;                                   // _cacheInput.Length == 0
  int start_idx_ = 0;
  int64_t chunks_in_ = 0, caller_samples_ = 0;                // chunks / caller samples that went through InputSpeech
  bool finished_ = false;
  // endpointing: the detector's frame 0 is the caller's sample ep_origin_; ep_rows_ = fbank rows not yet sent to the detector;
  // ep_audio_ = the caller's samples from ep_audio_base_ (relative to ep_origin_) on; ep_fed_ = frames sent so far
  // slot_: the stream's slot in EVERY per-stream device buffer of the recognizer (detector state, network state, decoder state);
  // taken when the first of them is needed, released in the destructor
  int slot_ = -1;
  bool ep_joined_ = false, decoded_ = false;                  // has fed the detector / has decoded a chunk (SetEndpointModel, SetTokenInfo)
  // SetTokenInfo: the decoder context lives in the slot; these ask the next step to start the CIF block / the caches from zeros
  bool cif_reset_ = true, cache_reset_ = true;
  // provenance of the time rule: the caller-sample index (-1: none) of every row of Speech, of the splice row, of the ten cached
  // feature rows, of the rows of the chunk GetDecodeChunk built last, and of position hi - 1 of the chunk decoded last
  std::vector<int64_t> speech_idx_, cache_idx_ = std::vector<int64_t>(10, -1), chunk_idx_;
  int64_t splice_idx_ = -1, carry_idx_ = -1;
  int64_t ep_origin_ = -1, ep_audio_base_ = 0, ep_samples_ = 0;
  std::vector<float> ep_rows_, ep_audio_;
  int ep_fed_ = 0, ep_prev_end_ = 0;
  bool ep_flushed_ = false;
  // streaming punctuation: the committed words already marked (the next call's must begin with them), whether the slot's
  // punctuation state is in use, whether the end-of-input flush was made, and what an endpoint close left for this call's launch
  std::vector<std::string> pn_words_;
  bool pn_joined_ = false, pn_flushed_ = false;
  struct PuncPending { bool on = false; size_t sentence = 0; OnlineCommitted c; };
  PuncPending pn_close_;
};

class OnlineRecognizerM : public std::enable_shared_from_this<OnlineRecognizerM> {
 public:
  // (encoderFilePath, decoderFilePath, configFilePath, mvnFilePath, tokensFilePath, threadsNum) — OnlineRecognizer.cs:22;
  // here ONE .pfw container holds both graphs' tensors (model_path); decoder_path is accepted and unused
  OnlineRecognizerM(const std::string& model, const std::string& decoder_unused, const std::string& config,
                    const std::string& mvn, const std::string& tokens, int threads_num, int device);
  std::shared_ptr<OnlineStreamM> CreateOnlineStream();
  std::vector<std::string> GetResults(const std::vector<OnlineStreamM*>& streams);   // Forward + DecodeMulti
  void Dispose();
  bool disposed() const { return disposed_.load(); }
  std::shared_ptr<Engine> engine() { std::lock_guard<std::mutex> lk(mu_); return engine_; }
  const ConfEntity& conf() const { return conf_; }
  int chunk_length() const { return 10 * 5 + 10; }            // OnlineModel.cs:29: lfr * chunkSize + 10 = 60 fbank frames
  const std::vector<float>& shift() const { return shift_; }
  const std::vector<float>& scale() const { return scale_; }
  const std::vector<std::string>& tokens() const { return tokens_; }
  // ---- endpointing and the second pass (paraformer_hip.h "Streaming endpointing") ----
  // cfg != null: every GetResults that follows runs the streaming endpoint detector over the caller-audio fbank rows of its
  // streams (one launch set for all of them), closes sentences at its events and resets their decoder context.  null: off —
  // every path is then what it is without this call.  PF_ERR_INVALID_ARG as pf_endpoint_config; PF_ERR_UNSUPPORTED with snip_edges.
  void SetEndpoint(const pf_endpoint_config* cfg);
  // the offline recognizer that re-recognises every finished sentence (ONE GetResults per call over the sentences that closed
  // in it); null: none.  PF_ERR_UNSUPPORTED for a recognizer with SetVad on (one sentence stays one stream).
  void SetSecondPass(std::shared_ptr<Recognizer> offline);
  // The FSMN-VAD model score as the detector's level (paraformer_hip.h "Voice-activity endpointing, streaming, model score";
  // DESIGN.md 4.6q): loads a `.pfw` of kind "fsmnvad" and attaches it to the engine; "" detaches.  Every stream's network state
  // lives in a second device buffer, indexed by the detector's slot.  Inert until SetEndpoint.  Errors as vad_model_load and
  // Engine::set_vad_model; PF_ERR_UNSUPPORTED for a model whose window does not fit the LDS, and while a live stream has already
  // fed the detector (two kinds of level must not meet in one state block).
  void SetEndpointModel(const std::string& pfw_path);
  bool endpoint_on() const { return ep_on_.load(); }
  // Token times and scores (paraformer_hip.h "Streaming token times and scores"): with the mode on Forward runs
  // Engine::online_step — the carried CIF and the FSMN caches stay in the stream's slot of a device buffer — and fills
  // OnlineStreamM::TokenInfo.  PF_ERR_UNSUPPORTED once a live stream has decoded a chunk; the value it already has is a no-op.
  void SetTokenInfo(bool on);
  bool token_info_on() const { return ti_on_.load(); }
  // Streaming punctuation (paraformer_hip.h "Punctuation, streaming"): loads a causal `.pfw` of kind
  // "cttransformer" and attaches it to the engine; "" detaches and frees.  Every GetResults then marks the newly committed
  // words of all its streams in ONE punc_stream launch; a stream's keys and values live in one more slot-indexed device buffer.
  // max_context 0: the default of 200.  PF_ERR_UNSUPPORTED for a model that is not causal and while a live stream holds
  // punctuation state; PF_ERR_INVALID_ARG for max_context outside 2 .. 256.
  void SetPuncModel(const std::string& pfw_path, int max_context);
  bool punc_on() const { return pn_on_.load(); }
  void release_stream(int slot, bool ep_joined, bool decoded, bool punc_joined);   // ~OnlineStreamM

 private:
  void Forward(const std::vector<OnlineStreamM*>& streams);   // :336-403
  void ForwardEndpoint(const std::vector<OnlineStreamM*>& streams);
  void ForwardDevice(Engine* e, const std::vector<OnlineStreamM*>& work, const std::vector<float>& speech, int Tc);
  void ForwardPunc(const std::vector<OnlineStreamM*>& streams);
  // a slot for a stream that has none (the engine's mutex is held): every per-stream buffer grows together by reallocate-and-copy
  // on the device; the detector's and the network's blocks are zeroed where the stream joins the detector (ForwardEndpoint),
  // the decoder state by its reset flags
  void ensure_slot(OnlineStreamM* s, Engine* e);
  std::atomic<bool> ti_on_{false};
  std::atomic<bool> ep_on_{false};
  std::mutex ep_mu_;                                          // guards the eight below and the four behind them
  pf_endpoint_config ep_cfg_{};
  std::shared_ptr<Recognizer> second_;
  int32_t* ep_states_ = nullptr;                              // [ep_cap_, PF_ENDPOINT_STATE_INTS] on the device, a block per stream slot
  int ep_cap_ = 0;
  std::vector<int> ep_free_;
  std::shared_ptr<const VadModel> ep_model_;                  // the model score (SetEndpointModel); null: the energy level
  char* ep_net_states_ = nullptr;                             // [ep_cap_, ep_net_bytes_] on the device: the network's state per slot
  size_t ep_net_bytes_ = 0;
  char* ti_states_ = nullptr;                                 // [ep_cap_, ti_bytes_] on the device: CIF block | FSMN caches per slot (SetTokenInfo)
  size_t ti_bytes_ = 0;
  std::atomic<bool> pn_on_{false};
  std::shared_ptr<const PuncModel> pn_model_;                 // SetPuncModel
  char* pn_states_ = nullptr;                                 // [ep_cap_, pn_bytes_] on the device: k | v and the count per slot
  char* pn_ws_ = nullptr;                                     // the launch's staged operands and results
  size_t pn_bytes_ = 0, pn_ws_bytes_ = 0;
  int pn_max_context_ = 0, pn_live_ = 0;
  int ep_live_ = 0, decoded_live_ = 0;                        // live streams that have fed the detector / decoded a chunk
  std::mutex mu_;
  std::shared_ptr<Engine> engine_;
  ConfEntity conf_;
  std::vector<float> shift_, scale_;
  std::vector<std::string> tokens_;
  std::atomic<bool> disposed_{false};
};

}  // namespace pf
