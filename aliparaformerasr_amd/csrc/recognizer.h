// recognizer.h — C++ mirror of the reference's public classes OfflineRecognizer
// (AliParaformerAsr/OfflineRecognizer.cs:13-477) and OfflineStream
// (AliParaformerAsr/OfflineStream.cs:7-121) above the device engine.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <functional>
#include <initializer_list>
#include <map>
#include <array>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "lm.h"
#include "copycrew.h"
#include "engine.h"
#include "hostutil.h"
#include "stream_result.h"

namespace pf {

// DecodeMulti for one stream (OfflineRecognizer.cs:304-418)
ResultEntity decode_multi_one(const std::vector<std::string>& tokens, const std::vector<int64_t>& ids,
                              const TsList& timestamps);
// What DecodeMulti derives from a vocabulary entry every time it meets it (the text in front of a tab, whether it is one of the four
// markers, whether it is all Chinese), computed once per recognizer
struct TokenTable {
  TokenTable() = default;
  explicit TokenTable(const std::vector<std::string>& tokens);
  std::vector<std::string> cur;
  std::vector<uint8_t> kind;
};
ResultEntity decode_multi_one(const TokenTable& table, const std::vector<int64_t>& ids, const TsList& timestamps);
// GetHotwords (OfflineRecognizer.cs:72-90) over in-memory lines; appends [sos_eos_id]
std::vector<std::vector<int32_t>> hotword_ids(const std::vector<std::string>& tokens,
                                              const std::vector<std::string>& lines, int sos_eos_id);

class Recognizer;
struct FwdClock;               // PF_RECOGNIZER_TIMING's laps (recognizer.cpp)

// Ownership: a stream shares ownership of its recognizer OBJECT (so a stream handle that outlives
// pf_recognizer_free still reaches valid memory and answers PF_ERR_DISPOSED), the recognizer does not track
// its streams (the reference's CreateOfflineStream does not either, OfflineRecognizer.cs:92-100), and the
// device engine is released by Dispose() — never by the last stream going away.
//
// Where the features live (round 5).  The reference computes them inside AddSamples (OfflineStream.cs:40-41) and keeps them
// in OfflineInputEntity.Speech until Forward pads and uploads them.  Nothing of the C ABI reads Speech — only its length
// (pf_stream_num_feature_floats), a function of the sample count — so a stream that has received ONE AddSamples call
// keeps the SAMPLES of that call on the device (one host-to-device copy, no kernel, no read-back) and the batched
// front-end of GetResults (fbank -> LFR + CMVN + pad in two launches over the whole batch) computes the same features from
// them.  A second AddSamples before GetResults, a SenseVoice stream that survives GetResults with its prompt rows
// prepended (quirk Q8), or a front-end configuration the batched kernels do not cover turn the stream into the host form
// (Speech = the feature floats, exactly as before): materialize().
class Stream : public StreamResult {        // (the fields a GetResults writes: stream_result.h)
 public:
  explicit Stream(std::shared_ptr<Recognizer> r);
  // The reference's PUBLIC constructor, new OfflineStream(mvnFilePath, confEntity) (OfflineStream.cs:20-28): a stream that
  // belongs to no recognizer yet.  It owns no engine, so AddSamples keeps the samples on the host (SpeechLength is a function
  // of the sample counts) and the first GetResults that receives it adopts it (Recognizer::adopt): the pending calls are
  // replayed there.  Its front-end must be the adopting recognizer's (same am.mvn values, same frontend_conf) — the reference
  // would compute the features with the stream's own files; anything else answers PF_ERR_UNSUPPORTED instead of guessing.
  Stream(const std::string& mvn_path, const ConfEntity& conf);
  ~Stream();
  ConfEntity uconf; std::vector<float> ushift, uscale;        // unbound form only
  std::vector<std::vector<float>> pending;                    // AddSamples calls not yet replayed
  void AddSamples(const float* samples, int64_t n);          // OfflineStream.cs:36-57
  // AddSamples for raw PCM (paraformer_hip.h "PCM intake").  First call on an owned stream: the raw bytes go through the copy
  // lane, pcm_to_samples_kernel runs on the lane's stream behind the last DMA piece and dev_ev is recorded behind the kernel —
  // dev_audio / dev_n then hold what AddSamples of the converted floats would have left.  Every other case converts on the
  // host (pcm_to_samples, the same arithmetic) and continues through AddSamples.
  void AddPcm(const void* data, int64_t n_values, const pf_pcm_desc& d);
  void Dispose();                                             // OfflineStream.cs:81-121: drops the buffers
  std::vector<float> Speech;                                  // OfflineInputEntity.Speech (host form)
  bool has_speech = false;                                    // Speech != null
  int SpeechLength = 0;                                       // float count
  // device form: the samples of the single AddSamples call (dev_audio may be null when dev_n == 0)
  bool device_form = false;
  float* dev_audio = nullptr; size_t dev_bytes = 0; int64_t dev_n = 0;
  hipEvent_t dev_ev = nullptr; bool dev_ev_pending = false;   // recorded behind the last DMA piece of dev_audio (staged uploads)
  float* dev_raw = nullptr; size_t dev_raw_bytes = 0;         // AddPcm: the raw bytes the kernel behind dev_ev reads; back to the cache once it has completed
  void wait_device_audio();                                   // host-side wait for that event
  void materialize();                                         // device form -> host form (features computed and read back)
  void drop_device_audio();
  bool hotwords_null = false;
  std::vector<std::vector<int32_t>> Hotwords;
  // CTC forced alignment (Recognizer::SetAlign): the stream's target (token ids), kept until cleared
  std::vector<int64_t> AlignIds; bool has_align = false;
  // long-audio recognition (Recognizer::SetVad): the pieces the stream was cut into by the last GetResults, in time order —
  // [begin_ms, end_ms) on the stream's clock, where the piece ran (batch, row of the plan), its share [tok_begin, tok_end) of
  // Tokens / Scores / Timestamps, and its own text.  Empty without SetVad.
  struct Segment { int begin_ms = 0, end_ms = 0, batch = 0, row = 0, tok_begin = 0, tok_end = 0; std::string text; };
  std::vector<Segment> Segments;
  // punctuation (Recognizer::SetPuncModel): of the last GetResults, the punctuated form of its Text, the mark of every word and
  // the sentences: words [word_begin, word_end), their text, and [begin_ms, end_ms] when the result has exactly one Timestamps
  // entry per word (has_time).  Empty without a model.
  struct Sentence { int word_begin = 0, word_end = 0, begin_ms = 0, end_ms = 0; bool has_time = false; std::string text; };
  // speaker labels (Recognizer::SetSpkModel with SetVad): of the last long-audio GetResults, the windows that were embedded
  // with their labels, the label of every segment (aligned with Segments; -1: the stream has no window), the number of
  // speakers and their centroids [NumSpeakers, SpkE]; empty without a model
  struct SpkWindow { int begin_ms = 0, end_ms = 0, label = -1; };
  std::vector<SpkWindow> SpkWindows;
  std::vector<int32_t> SegSpeakers;
  std::vector<float> SpkCentroids;
  int NumSpeakers = 0, SpkE = 0;
  std::string Punctuated;
  std::vector<int32_t> PuncIds;
  std::vector<Sentence> Sentences;
  bool borrowed = false;                                      // dev_audio points INTO another stream's buffer (a piece): never freed here
  void RemoveChunk();                                         // OfflineStream.cs:69-79
  bool disposed = false;
  std::shared_ptr<Recognizer> owner;
};

class Recognizer : public std::enable_shared_from_this<Recognizer> {
 public:
  Recognizer(const std::string& model, const std::string& config, const std::string& mvn,
             const std::string& tokens, const std::string& modeleb, const std::string& hotword, int batch_size,
             int threads_num, int device);
  ~Recognizer();
  std::shared_ptr<Stream> CreateOfflineStream();              // OfflineRecognizer.cs:92-100
  void adopt(Stream* s);                                      // binds a stream built with the public constructor (see Stream)
  // GetResults (:110-116).  The result list belongs to the CALLING THREAD until its next GetResults on this
  // recognizer (the reference returns a fresh List per call; concurrent callers must not share one).
  void GetResults(const std::vector<Stream*>& streams);
  const std::vector<ResultEntity>& results_of_this_thread();
  void Dispose();                                             // waits for calls in flight, then frees the engines
  // Decoding extras (PF_DECODE_*) of every GetResults that follows, on every engine of the pool, present and future.  With
  // PF_DECODE_CTC (SenseVoice) Forward leaves the collapsed ids, [begin, end] milliseconds per token and the token scores
  // in the streams; DecodeMulti, RemoveChunk and the Q8 branch run unchanged on those Tokens.
  void SetDecode(int flags);
  // Alternatives (paraformer_hip.h "Top-k and n-best"): N = 0 off; N >= 1: PF_DECODE_TOPK with K (0 = 4) on every engine beside
  // the SetDecode flags — TokenAlternatives in every stream, and for paraformer with N > 1 the n-best list
  void SetNBest(int N, int K);
  // SenseVoice only (paraformer_hip.h "CTC beam search"): N = 0 off; N >= 1: PF_DECODE_CTC_BEAM with beam width W (0 = max(16, N))
  // and top-k K (0 = 4) on every engine — Alternatives holds up to N labelings by descending CTC score
  void SetCtcBeam(int N, int W, int K);
  // SenseVoice only (paraformer_hip.h "CTC forced alignment"): PF_DECODE_ALIGN on every engine — a stream's target (AlignIds)
  // is aligned to its audio, and with SetCtcBeam every Alternative gets its own times and log-likelihood
  void SetAlign(bool on);
  // SenseVoice only (paraformer_hip.h "CTC hot words"): boost per matched hot-word token inside the beam search of SetCtcBeam
  // (inert without it); 0 = off.  The hot words of a batch: the union of its streams' Hotwords, else the hot-word file's.
  void SetHotwordBoost(float s);
  // SenseVoice: an ARPA n-gram LM fused into the beam search of SetCtcBeam (inert without it).  Loaded once against the token
  // table; every engine of the pool uploads it on first use.  An empty path clears it.
  void SetLm(const std::string& arpa_path, float alpha, float beta, int flags);
  // Paraformer only (paraformer_hip.h "N-best search"): W = 0 off (always accepted); W in 1 .. 64: with SetNBest(N > 1, K) the
  // n-best list comes from the beam search on the device (width max(W, N)) instead of the host enumeration, in the fused order,
  // with score, loglik_sum, lm_sum and hot_tokens per Alternative.  Inert until SetNBest(N > 1, K).
  void SetNBestSearch(int W);
  // the model and the hot-word boost of that search (inert without it).  The ARPA file is read once against the token table,
  // every engine of the pool uploads it on first use; an empty path clears it.  The hot words come from where SetHotwordBoost
  // reads them: the union of the batch's streams' Hotwords, else the hot-word file's.  "Off" is always accepted.
  void SetNBestLm(const std::string& arpa_path, float alpha, float beta, int flags);
  void SetNBestHotwordBoost(float s);
  // Long-audio recognition (paraformer_hip.h "Voice-activity segmentation"): cfg != null: every GetResults that follows cuts
  // its streams into speech pieces on the device (Engine::vad_segment_device over the resident audio), plans batches of similar
  // length (host_long_plan), forwards each batch over pointers into the streams' audio and stitches one result per stream.
  // cfg == null: off.  PF_ERR_UNSUPPORTED beside SetNBest / SetCtcBeam / SetAlign (either order).
  void SetVad(const pf_vad_config* cfg, int batch_max, int64_t frame_budget, const char* sep);
  bool vad_on() { std::lock_guard<std::mutex> lk(vad_mu_); return vad_on_; }
  // The FSMN-VAD model score for SetVad's segmentation (paraformer_hip.h "Voice-activity segmentation, model score"): a `.pfw`
  // of kind "fsmnvad", loaded once and attached to every engine of the pool, present and future; "" clears.  Inert until SetVad.
  void SetVadModel(const std::string& pfw_path);
  // Punctuation of every GetResults that follows (paraformer_hip.h "Punctuation"): a `.pfw` of kind "cttransformer", loaded
  // once; "" clears.  GetResults then punctuates each stream's final Text (with SetVad: the stitched text), all streams of the
  // call in one pf_engine_punctuate on a leased engine, and keeps the result on the stream; Text / Tokens / Timestamps stay.
  void SetPuncModel(const std::string& pfw_path);
  // Speaker labels of every long-audio GetResults that follows (paraformer_hip.h "Speaker labels"): a `.pfw` of kind "campplus",
  // loaded once and attached to every engine of the pool, present and future; "" clears.  Inert until SetVad, and may be set
  // before or after it.  Behind the segmentation, on the fbank rows it staged, under the same lease: the windows of all of the
  // call's streams are planned, embedded and turned into one cosine block per stream on the device, each stream is clustered on
  // the host.  Text / Tokens / Timestamps / Scores / Segments / Punctuated / Sentences stay what they are without it.
  void SetSpkModel(const std::string& pfw_path, const pf_spk_config* cfg);
  bool disposed() const { return disposed_.load(); }
  // engine 0 (nullptr once disposed): what pf_recognizer_engine hands out; callers lock engine->mutex() themselves
  std::shared_ptr<Engine> engine() { std::lock_guard<std::mutex> lk(mu_); return engines_.empty() ? nullptr : engines_[0]; }
  const std::vector<std::string>& tokens() const { return tokens_; }

  // ---- engine pool (round 5; VERDICT r4 "missing" #1).  The reference's GetResults is unlocked — concurrent calls overlap
  // inside onnxruntime (OfflineRecognizer.cs:110-198; the only lock of the path is OfflineStream.cs:19).  Here a call
  // takes a free engine of the pool (engines on ONE device sharing the device weight image; each has its own stream, f16
  // operands and workspaces): two callers' batches are in flight together, one's host work (audio upload, text) under the
  // other's kernels.  Engines beyond the first are created when a call finds every engine busy (up to max_engines_).
  class Lease {
   public:
    Lease() = default;
    Lease(Lease&& o) noexcept { *this = std::move(o); }
    Lease& operator=(Lease&& o) noexcept;
    ~Lease() { release(); }
    Engine* operator->() const { return e_.get(); }
    Engine* get() const { return e_.get(); }
    void release();
   private:
    friend class Recognizer;
    Recognizer* r_ = nullptr; int idx_ = -1; std::shared_ptr<Engine> e_; std::unique_lock<std::mutex> lk_;
  };
  Lease acquire();                                            // throws PF_ERR_DISPOSED once disposed
  int engines_created() { std::lock_guard<std::mutex> lk(mu_); return (int)engines_.size(); }
  // device buffers for the streams' audio (size-class cache: a server creating one stream per utterance re-uses them)
  float* audio_alloc(size_t bytes, size_t* got);
  void audio_free(float* p, size_t bytes);
  // host -> device on a copy lane.  Returns when `src` may be reused; with `ev` (staged form) the bytes are on the device when
  // *ev has completed and *pending is set — without staging the call is synchronous and *pending stays false
  // `after` (AddPcm): launches that follow the bytes on the lane's stream, in front of *ev (which is then recorded on both paths)
  void upload(float* dst, const float* src, size_t bytes, hipEvent_t* ev = nullptr, bool* pending = nullptr,
              const std::function<void(hipStream_t)>* after = nullptr);
  int device() const { return device_; }
  bool device_streams() const { return device_streams_; }     // new streams keep their first AddSamples call's audio on the device
  int feature_floats(int64_t n_samples);                      // what GetFbank + LfrCmvn return for n samples (float count)

 private:
  void Forward(const std::vector<Stream*>& streams);          // :118-198
  // Forward's stages, in the order they run; behind them build_stream_result (stream_result.h) per stream
  bool prepare_streams(const std::vector<Stream*>& streams);                                  // -> every stream is in the device form
  ResultPlan configure_engine(Engine* e, const std::vector<Stream*>& streams);
  std::chrono::steady_clock::time_point run(Engine* e, const std::vector<Stream*>& streams, bool all_dev, FwdClock& fc);
  HostBatchOut read(Lease& lease, const std::vector<Stream*>& streams, std::chrono::steady_clock::time_point t_step, FwdClock& fc);
  std::vector<std::vector<int32_t>> batch_hotwords(const std::vector<Stream*>& streams, bool null_throws) const;
  void prepend_sv_prompt(Stream& s) const;
  struct LmSetting { std::shared_ptr<const LmImage> lm; float alpha = 0.f, beta = 0.f; int flags = 0; };
  LmSetting lm_snapshot(bool search);                         // SetLm's (beam search) or SetNBestLm's (n-best search), under lm_mu_
  void ForwardLong(const std::vector<Stream*>& streams, std::vector<ResultEntity>& out);   // GetResults with SetVad
  struct Piece { int stream, b, e; };                         // a speech piece of ForwardLong: frames [b, e) of streams[stream]
  void label_speakers(Lease& lease, const std::vector<Stream*>& streams, const std::vector<int32_t>& seg, const std::vector<int32_t>& nseg,
                      int cap);
  void stitch_pieces(const std::vector<Stream*>& streams, const std::vector<Piece>& pieces, const std::vector<std::unique_ptr<Stream>>& views,
                     const std::vector<int32_t>& batch, const std::vector<int32_t>& row, const std::string& sep,
                     std::vector<ResultEntity>& out);
  void Punctuate(const std::vector<Stream*>& streams, const std::vector<ResultEntity>& out);
  std::mutex spk_mu_;                                         // guards spk_model_ and spk_cfg_
  std::shared_ptr<const SpkModel> spk_model_;
  pf_spk_config spk_cfg_{};
  std::mutex punc_mu_;                                        // guards punc_model_
  std::shared_ptr<const PuncModel> punc_model_;
  std::mutex vad_mu_;                                         // guards the five below
  std::shared_ptr<const VadModel> vad_model_;
  bool vad_on_ = false; pf_vad_config vad_cfg_{}; int vad_batch_max_ = 32; int64_t vad_budget_ = 96000; std::string vad_sep_;
  std::shared_ptr<Engine> make_engine();
  std::mutex mu_;                                             // guards engines_, busy_, the audio cache
  std::condition_variable cv_;
  std::vector<std::shared_ptr<Engine>> engines_;
  std::vector<char> busy_;
  float stagger_frac_ = 0.35f; double step_ema_us_ = 0.0;      // PF_RECOGNIZER_STAGGER (Recognizer::stagger_start)
  std::chrono::steady_clock::time_point last_start_{};
  void stagger_start();
  void note_step(std::chrono::steady_clock::time_point t0);
  int max_engines_ = 2;                                       // PF_RECOGNIZER_ENGINES (1..8)
  bool device_streams_ = true;                                // PF_RECOGNIZER_DEVICE_STREAMS=0: always the host form
  int feat_m_ = 1;
  std::string engine_kind_; bool sv_device_prompt_ = false;
  bool plain_paraformer_ = false;                             // a paraformer without the SeACo bias decoder: what the n-best search serves
  int creating_ = 0;                                          // engines being built outside the lock
  int device_ = 0;
  pf_engine_config ec_{};                                     // template for further engines (strings owned below)
  std::string model_path_, mvn_path_, window_;
  std::vector<float> cmvn_shift_, cmvn_scale_;
  // the PFW image on the device, adopted in place by every engine of the pool.  Shared ownership: each engine's deleter holds
  // a reference, so a caller of pf_recognizer_engine that still holds its shared_ptr<Engine> across Dispose() keeps the
  // weights it points into alive (Dispose used to hipFree it under such a caller)
  std::shared_ptr<void> image_; int64_t image_bytes_ = 0;
  void free_device_side();                                    // audio cache + copy lanes + our image reference (Dispose, ~Recognizer)
  // SenseVoice prompt table, flag and row width: copies of engine 0's (every engine of the pool adopts the same image), so the
  // prompt prepend (quirk Q8) needs no engine lease
  std::vector<float> sv_embed_; bool sv_use_itn_ = false; int sv_width_ = 0;
  size_t audio_cache_cap_ = (size_t)1 << 30;                  // PF_RECOGNIZER_AUDIO_CACHE_MB
  std::map<size_t, std::vector<float*>> audio_cache_; size_t audio_cached_bytes_ = 0;
  // A copy lane = a stream + a ring of PINNED host memory.  AddSamples copies the caller's (pageable) samples into the ring piece by
  // piece and queues one DMA per piece: the call returns when the last piece has been COPIED OUT of the caller's array — the
  // reference's contract (the array belongs to the caller again) — not when the DMA has landed; the stream's `dev_ev` says when
  // it has, and whoever reads dev_audio waits for it (on the engine's stream in Forward).  The runtime's own pageable path
  // pins the caller's pages, copies and returns after both: 120 - 390 us per 1.9 MB for pages it has not seen, 50 us for pages it
  // still holds pinned from an earlier copy (tools/ubench/h2d.cpp, profiles/round6_staging_ab.txt) — hence the policy below.
  struct CopyLane {
    std::mutex mu; hipStream_t s = nullptr;          // the runtime's pageable path (synchronous)
    hipStream_t sp = nullptr;                        // the staged path: highest stream priority (its DMAs are copy kernels)
    char* pin = nullptr; size_t cap = 0, head = 0; bool tried = false;
    struct Piece { size_t off, bytes; hipEvent_t ev; };
    std::deque<Piece> inflight; std::vector<hipEvent_t> spare;
  };
  std::unique_ptr<CopyCrew> crew_; std::once_flag crew_once_; int crew_threads_ = 3;   // PF_RECOGNIZER_COPY_THREADS (helpers)
  // Which way an upload goes.  A (pointer, size) seen before is a buffer the caller re-uses: the runtime keeps such pages pinned
  // after their first copy and DMAs straight out of them (50 us per 1.9 MB) — no staged copy beats that.  An array not seen
  // before would be pinned first (120 - 390 us, tools/ubench/h2d.cpp): it goes through the ring (45 - 60 us).
  std::mutex seen_mu_; std::unordered_map<const void*, size_t> seen_; bool staging_always_ = false;   // PF_RECOGNIZER_STAGING_POLICY=always
  bool seen_before(const void* p, size_t bytes);
  size_t staging_bytes_ = (size_t)16 << 20;                   // PF_RECOGNIZER_STAGING_MB per lane (0: the runtime's pageable copy)
  size_t staging_piece_ = (size_t)2 << 20;                    // PF_RECOGNIZER_STAGING_PIECE_KB
  std::array<CopyLane, 4> lanes_;
  std::atomic<unsigned> next_lane_{0};
  std::vector<std::string> tokens_;
  TokenTable token_table_;
  ConfEntity conf_;
  std::vector<std::vector<int32_t>> hotwords_;
  uint64_t uid_ = 0;                                          // key of this recognizer in the per-thread result store
  std::atomic<bool> disposed_{false};
  std::atomic<int> decode_flags_{0};                          // what the engines run: user_flags_ | TOPK while nbest_n_ > 0
  std::atomic<int> user_flags_{0};                            // as given to SetDecode
  std::atomic<int> nbest_n_{0};
  std::atomic<int> topk_k_{4};
  std::atomic<int> beam_w_{16}, beam_n_{16};
  std::atomic<float> hot_boost_{0.f};   // SetHotwordBoost
  std::mutex lm_mu_;                    // SetLm: the model and its weights, read by every GetResults call
  std::shared_ptr<const LmImage> lm_;
  float lm_alpha_ = 0.f, lm_beta_ = 0.f;
  int lm_flags_ = 0;
  std::atomic<int> search_w_{0};        // SetNBestSearch
  std::atomic<float> search_boost_{0.f};   // SetNBestHotwordBoost
  std::shared_ptr<const LmImage> search_lm_;   // SetNBestLm (under lm_mu_), its weights and flags
  float search_alpha_ = 0.f, search_beta_ = 0.f;
  int search_flags_ = 0;
  std::atomic<bool> beam_on_{false};
  std::atomic<bool> align_on_{false};
  int extra_flags() const { return (nbest_n_ > 0 ? PF_DECODE_TOPK : 0) | (beam_on_ ? PF_DECODE_CTC_BEAM : 0) | (align_on_ ? PF_DECODE_ALIGN : 0); }
  void set_decode_all(int flags, int k);
  friend class Stream;
};

}  // namespace pf
