// online.cpp — see online.h.  Host-side logic of the reference's streaming API restated in C++ (the reference is
// compiled C#; no .NET toolchain exists in the build image); citations are relative to AliParaformerAsr/.
#include "online.h"
#include "recognizer.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace pf {

// ------------------------------------------------------------------ pure host pieces -------
std::vector<float> online_apply_lfr(const std::vector<float>& in, int n_mels, int lfr_m, int lfr_n) {
  // OnlineWavFrontend.cs:63-80
  const int t = (int)(in.size() / (size_t)n_mels);
  int t_lfr = 0;
  if (t % lfr_n < lfr_m - lfr_n) t_lfr = t / lfr_n - 1;
  if (t % lfr_n >= lfr_m - lfr_n) t_lfr = t / lfr_n;
  if (t_lfr < 0) throw Error(PF_ERR_RECOGNITION, "Arithmetic operation resulted in an overflow (negative LFR frame count)");
  std::vector<float> out((size_t)t_lfr * lfr_m * n_mels);
  for (int i = 0; i < t_lfr; ++i) {
    const size_t src = (size_t)i * lfr_n * n_mels, len = (size_t)lfr_m * n_mels;
    if (src + len > in.size()) throw Error(PF_ERR_RECOGNITION, "Source array was not long enough (ApplyLfr)");   // Array.Copy would throw
    std::memcpy(&out[(size_t)i * len], &in[src], len * sizeof(float));
  }
  return out;
}

void online_position_encode(std::vector<float>& x, int timesteps, int dim, int start_idx) {
  // OnlineWavFrontend.cs:152-188, float / double mix as written there
  const int half = dim / 2;
  const float inc = (float)std::log((double)10000.0f) / (float)(half - 1);
  std::vector<float> inv((size_t)half);
  for (int i = 0; i < half; ++i) {
    const float v = (float)(i + 1) * (-inc);
    inv[(size_t)i] = (float)std::exp((double)v);
  }
  for (int t = 0; t < timesteps; ++t) {
    const float p = (float)(start_idx + t + 1);
    float* row = &x[(size_t)t * dim];
    for (int i = 0; i < half; ++i) {
      const float arg = inv[(size_t)i] * p;                   // float product, then double sin / cos
      row[i] += (float)std::sin((double)arg);
      row[half + i] += (float)std::cos((double)arg);
    }
  }
}

void online_dynamic_mask(std::vector<float>& a, int chunk_size, int lfr) {
  // OnlineModel.cs:141-165
  const int n = (int)a.size();
  for (int i = 0; i < std::min(chunk_size, n); ++i) a[(size_t)i] = 0.f;
  const int decode_lfr = chunk_size + lfr;
  for (int i = decode_lfr; i < n; ++i) a[(size_t)i] = 0.f;
}

void online_cif(const std::vector<std::vector<float>>& hiddens, const std::vector<float>& alphas, float threshold,
                std::vector<std::vector<float>>& fired, float& carry_alpha, std::vector<float>& carry_hidden,
                std::vector<int32_t>* fire_entry) {
  // OnlineRecognizer.cs:152-197, float arithmetic, products and sums rounded separately
  const size_t D = hiddens.empty() ? 0 : hiddens[0].size();
  float integrate = 0.0f;
  std::vector<float> frames(D, 0.f);
  fired.clear();
  if (fire_entry) fire_entry->clear();
  const size_t n = std::min(hiddens.size(), alphas.size());
  for (size_t j = 0; j < n; ++j) {
    const float alpha = alphas[j];
    const std::vector<float>& h = hiddens[j];
    if (alpha + integrate < threshold) {
      integrate += alpha;
      for (size_t k = 0; k < D; ++k) { const volatile float prod = alpha * h[k]; frames[k] += prod; }
    } else {
      const float wgt = threshold - integrate;
      for (size_t k = 0; k < D; ++k) { const volatile float prod = wgt * h[k]; frames[k] += prod; }
      fired.push_back(frames);
      if (fire_entry) fire_entry->push_back((int32_t)j);
      integrate += alpha;
      integrate -= threshold;
      for (size_t k = 0; k < D; ++k) frames[k] = integrate * h[k];
    }
  }
  carry_alpha = integrate;
  carry_hidden = frames;
  if (integrate > 0.0f)
    for (size_t k = 0; k < D; ++k) carry_hidden[k] = frames[k] / integrate;
}

// ---- one chunk step of one stream on its state block (decode_blocks.h CifStreamBlock): what cif_stream_kernel computes
size_t online_cif_state_bytes(int D) { return block_at_zero<CifStreamBlock>(D).bytes(); }

int online_cif_step(void* state, const float* hiddens, const float* alphas, int Tc, int D, float threshold, int lo, int hi, bool reset,
                    float* fired, int32_t* fire_entry, int cap) {
  PF_CHECK(state && hiddens && alphas && fired && fire_entry, PF_ERR_INVALID_ARG, "online_cif_step: null pointer");
  PF_CHECK(Tc > 0 && D > 0 && D % 4 == 0 && cap >= Tc + 1, PF_ERR_INVALID_ARG, "online_cif_step: Tc > 0, D % 4 == 0 and cap >= Tc + 1 expected");
  const CifStreamBlock blk = block_at_zero<CifStreamBlock>(D);
  float* s_hidden = blk.hidden(state);
  float* s_integrate = blk.integrate(state);
  std::vector<std::vector<float>> h((size_t)Tc + 1);
  std::vector<float> a((size_t)Tc + 1, 0.f);
  h[0].assign((size_t)D, 0.f);                                  // entry 0: the carried pair (a reset: the constructor's)
  if (!reset) { h[0].assign(s_hidden, s_hidden + D); a[0] = s_integrate[0]; }
  for (int t = 0; t < Tc; ++t) {
    h[(size_t)t + 1].assign(hiddens + (size_t)t * D, hiddens + (size_t)(t + 1) * D);
    a[(size_t)t + 1] = (t >= lo && t < hi) ? alphas[t] : 0.f;   // DynamicMask
  }
  std::vector<std::vector<float>> f;
  std::vector<float> ch;
  std::vector<int32_t> ent;
  float ca = 0.f;
  online_cif(h, a, threshold, f, ca, ch, &ent);
  std::memcpy(s_hidden, ch.data(), (size_t)D * 4);
  for (size_t g = 0; g < blk.groups; ++g) s_integrate[g] = ca;  // one copy per channel group; the padding cells keep their bits
  const int count = (int)f.size();                              // <= Tc + 1 <= cap
  std::memset(fired, 0, (size_t)cap * D * 4);
  for (int l = 0; l < cap; ++l) fire_entry[l] = l < count ? ent[(size_t)l] : -1;
  for (int l = 0; l < count; ++l) std::memcpy(fired + (size_t)l * D, f[(size_t)l].data(), (size_t)D * 4);
  return count;
}

static bool is_chinese_all(const std::string& s) {             // ^[一-龥]+$  (OnlineRecognizer.cs:446-458)
  const std::vector<uint32_t> cps = utf8_decode(s);
  if (cps.empty()) return false;
  for (uint32_t c : cps)
    if (c < 0x4e00 || c > 0x9fa5) return false;
  return true;
}
static void replace_all(std::string& s, const std::string& from, const std::string& to) {
  size_t pos = 0;
  while ((pos = s.find(from, pos)) != std::string::npos) { s.replace(pos, from.size(), to); pos += to.size(); }
}

std::string online_decode_text(const std::vector<std::string>& tokens, const std::vector<int64_t>& ids) {
  // OnlineRecognizer.cs:405-437
  static const std::string bar = "\xE2\x96\x81";               // U+2581
  std::string text;
  for (int64_t id : ids) {
    if (id == 2) break;
    if (id < 0 || id >= (int64_t)tokens.size()) throw Error(PF_ERR_RECOGNITION, "Index was outside the bounds of the array (tokens)");
    const std::string& tk = tokens[(size_t)id];
    if (tk != "</s>" && tk != "<s>" && tk != "<blank>" && tk != "<unk>") {
      if (is_chinese_all(tk)) text += tk;
      else text += bar + tk + bar;
    }
  }
  replace_all(text, "@@" + bar + bar, "");
  replace_all(text, "@@" + bar, "");
  replace_all(text, bar + bar, " ");
  replace_all(text, bar, "");
  for (char& c : text)                                         // ToLower(): ASCII letters (the token tables are CJK + lower-case BPE)
    if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a');
  return text;
}

// ---- streaming punctuation: the committed words of a partial text (tests/punc_stream_ref.py committed_words)
OnlineCommitted online_committed_words(const PuncModel& m, const std::vector<std::string>& tokens, const std::vector<int64_t>& ids) {
  OnlineCommitted c;
  c.text = online_decode_text(tokens, ids);
  c.words = host_punc_words(m, c.text);
  const std::string* last = nullptr;                           // the last token that contributes text
  for (int64_t id : ids) {
    if (id == 2) break;
    const std::string& tk = tokens[(size_t)id];                // (online_decode_text has checked the range)
    if (tk != "</s>" && tk != "<s>" && tk != "<blank>" && tk != "<unk>") last = &tk;
  }
  const bool held = last && last->size() >= 2 && last->compare(last->size() - 2, 2, "@@") == 0 && !c.words.empty();
  c.n_committed = c.words.size() - (held ? 1 : 0);
  return c;
}

std::string online_word(const OnlineCommitted& c, size_t i) {
  return c.text.substr((size_t)c.words[i].begin, (size_t)(c.words[i].end - c.words[i].begin));
}

void online_check_committed_prefix(const std::vector<std::string>& before, const OnlineCommitted& now) {
  bool ok = before.size() <= now.n_committed;
  for (size_t i = 0; ok && i < before.size(); ++i) ok = online_word(now, i) == before[i];
  if (!ok) throw Error(PF_ERR_RECOGNITION, "streaming punctuation: the committed words of this call do not begin with the last call's");
}

// ------------------------------------------------------------------ OnlineStream -----------
OnlineStreamM::OnlineStreamM(std::shared_ptr<OnlineRecognizerM> r) : owner(std::move(r)) {
  std::shared_ptr<Engine> e = owner->engine();
  const int nd = e ? e->dec_layers() : 16, D = 512, lorder = 10;                    // OnlineStream.cs:44-46, 263-273
  States.assign((size_t)nd, std::vector<float>((size_t)D * lorder, 0.f));
  CifHidden.assign(1, std::vector<float>((size_t)D, 0.f));                          // InitHidden :241-250
  CifAlpha.assign(1, 0.f);                                                          // InitAlpha :251-260
  cache_feats_.assign((size_t)10 * 560, 0.f);                                       // InitCacheFeats :274-278
  cache_samples_.assign((size_t)160 * owner->chunk_length(), 0.f);                  // :63: a chunk of SILENCE is queued first
}

OnlineStreamM::~OnlineStreamM() {
  if (owner && (slot_ >= 0 || ep_joined_ || decoded_ || pn_joined_)) owner->release_stream(slot_, ep_joined_, decoded_, pn_joined_);
}

const std::vector<pf_online_token>& OnlineStreamM::token_info() {
  if (owner && owner->token_info_on())
    while (TokenInfo.size() < Tokens.size()) TokenInfo.push_back(pf_online_token{Tokens[TokenInfo.size()], -1, -1, 0.f, 0});
  return TokenInfo;
}

void OnlineStreamM::AddSamples(const float* samples, int64_t n) {
  if (disposed) throw Error(PF_ERR_DISPOSED, "OnlineStream");
  if (!samples) throw Error(PF_ERR_NULL_SAMPLES, "source");
  std::vector<float> s;
  size_t n_caller = 0;
  {
    std::lock_guard<std::mutex> lk(mu);
    if (finished_) throw Error(PF_ERR_INVALID_ARG, "OnlineStream: AddSamples after InputFinished");
    cache_samples_.insert(cache_samples_.end(), samples, samples + n);
    const size_t chunk = (size_t)160 * owner->chunk_length();
    if (cache_samples_.size() > chunk) {                        // ONE chunk per call (:94-102), the rest stays cached
      s.assign(cache_samples_.begin(), cache_samples_.begin() + (long)chunk);
      cache_samples_.erase(cache_samples_.begin(), cache_samples_.begin() + (long)chunk);
      n_caller = chunks_in_++ == 0 ? 0 : chunk;                 // the first chunk is the constructor's silence
    }
  }
  if (!s.empty()) InputSpeech(s, n_caller);
}

void OnlineStreamM::InputFinished() {
  if (disposed) throw Error(PF_ERR_DISPOSED, "OnlineStream");
  const size_t chunk = (size_t)160 * owner->chunk_length();
  for (;;) {
    std::vector<float> s;
    size_t n_caller = 0;
    {
      std::lock_guard<std::mutex> lk(mu);
      finished_ = true;
      if (cache_samples_.empty()) return;
      const size_t take = std::min(chunk, cache_samples_.size());
      s.assign(cache_samples_.begin(), cache_samples_.begin() + (long)take);
      cache_samples_.erase(cache_samples_.begin(), cache_samples_.begin() + (long)take);
      n_caller = chunks_in_++ == 0 ? 0 : take;
      s.resize(chunk, 0.f);                                     // the tail: zero-padded to one chunk
    }
    InputSpeech(s, n_caller);
  }
}

void OnlineStreamM::ResetDecoder() {                            // (the caller holds mu)
  Tokens.clear();
  TokenInfo.clear();
  if (owner->token_info_on()) {                                 // the context lives in the slot: its next step starts from zeros
    cif_reset_ = cache_reset_ = true;
  } else {
    for (std::vector<float>& st : States) std::fill(st.begin(), st.end(), 0.f);
    CifHidden.assign(1, std::vector<float>((size_t)512, 0.f));
    CifAlpha.assign(1, 0.f);
  }
  std::fill(cache_idx_.begin(), cache_idx_.end(), (int64_t)-1); // the cached rows become zero rows: no provenance
  carry_idx_ = -1;
  std::fill(cache_feats_.begin(), cache_feats_.end(), 0.f);
  start_idx_ = 0;
}

void OnlineStreamM::InputSpeech(const std::vector<float>& samples, size_t n_caller) {
  std::shared_ptr<Engine> e = owner->engine();
  if (!e) throw Error(PF_ERR_DISPOSED, "OnlineRecognizer");
  std::vector<float> fb;
  int t80 = 0;
  {
    std::lock_guard<std::mutex> lk(e->mutex());
    e->fbank_host(samples.data(), (int64_t)samples.size(), fb, t80);     // x 32768 + kaldi fbank (:129-130)
  }
  std::lock_guard<std::mutex> lk(mu);
  if (n_caller > 0 && owner->endpoint_on() && !ep_flushed_) {             // the detector's share: the caller's frames and samples
    if (ep_origin_ < 0) ep_origin_ = caller_samples_;
    const size_t rows = std::min((n_caller + 159) / 160, (size_t)t80);
    ep_rows_.insert(ep_rows_.end(), fb.begin(), fb.begin() + (long)(rows * 80));
    ep_audio_.insert(ep_audio_.end(), samples.begin(), samples.begin() + (long)n_caller);
    ep_samples_ += (int64_t)n_caller;
  }
  const int64_t first = n_caller > 0 ? caller_samples_ : -1;             // the rows' provenance: frame r starts at first + 160 r
  caller_samples_ += (int64_t)n_caller;
  if (first_input_ && t80 > 0) {                                          // :131-143: the first frame is repeated once
    Speech.insert(Speech.end(), fb.begin(), fb.begin() + 80);
    speech_idx_.push_back(first);
    first_input_ = false;
  }
  Speech.insert(Speech.end(), fb.begin(), fb.end());
  for (int r = 0; r < t80; ++r) speech_idx_.push_back(first < 0 ? -1 : first + 160 * (int64_t)r);
}

bool OnlineStreamM::GetDecodeChunk(std::vector<float>& chunk) {
  std::lock_guard<std::mutex> lk(mu);
  const int F = 80, CL = owner->chunk_length();
  if ((size_t)CL * F > Speech.size()) return false;
  std::vector<float> pad;
  std::vector<int64_t> pidx(1, cache_lfr_splice_.empty() ? speech_idx_[0] : splice_idx_);   // provenance travels with the rows
  pidx.insert(pidx.end(), speech_idx_.begin(), speech_idx_.begin() + CL);
  splice_idx_ = pidx.back();
  if (!cache_lfr_splice_.empty()) pad = cache_lfr_splice_;                // :172-178
  else pad.assign(Speech.begin(), Speech.begin() + F);                    // :180-187: first frame once more
  pad.insert(pad.end(), Speech.begin(), Speech.begin() + (long)CL * F);
  cache_lfr_splice_.assign(pad.end() - F, pad.end());                     // :189-190
  const ConfEntity& c = owner->conf();
  std::vector<float> x = pad;
  if (c.lfr_m != 1 || c.lfr_n != 1) x = online_apply_lfr(pad, F, c.lfr_m, c.lfr_n);
  const std::vector<float>& sh = owner->shift();
  const std::vector<float>& sc = owner->scale();
  if (!sh.empty()) {                                                      // ApplyCmvn, OnlineWavFrontend.cs:46-62
    const size_t dim = sh.size();
    for (size_t i = 0; i + dim <= x.size(); i += dim)
      for (size_t k = 0; k < dim; ++k) { const volatile float s = x[i + k] + sh[k]; x[i + k] = s * sc[k]; }
  }
  const double root = std::pow(512.0, 0.5);
  for (float& v : x) v = (float)((double)v * root);                       // :193
  const int W = 560, timesteps = (int)(x.size() / W);
  online_position_encode(x, timesteps, W, start_idx_);                    // :195-196
  chunk = cache_feats_;
  chunk.insert(chunk.end(), x.begin(), x.end());
  const bool lfr = c.lfr_m != 1 || c.lfr_n != 1;
  chunk_idx_ = cache_idx_;
  for (int i = 0; i < timesteps; ++i) {                                   // an LFR frame takes the index of its first row
    const size_t r = lfr ? (size_t)i * (size_t)c.lfr_n : (size_t)i;
    chunk_idx_.push_back(r < pidx.size() ? pidx[r] : -1);
  }
  cache_idx_.assign(chunk_idx_.end() - (long)cache_idx_.size(), chunk_idx_.end());
  speech_idx_.erase(speech_idx_.begin(), speech_idx_.begin() + CL);
  start_idx_ += timesteps;
  cache_feats_.assign(chunk.end() - (long)cache_feats_.size(), chunk.end());   // :201
  Speech.erase(Speech.begin(), Speech.begin() + (long)CL * F);            // RemoveChunk :210-224
  return true;
}

// ------------------------------------------------------------------ OnlineRecognizer -------
OnlineRecognizerM::OnlineRecognizerM(const std::string& model, const std::string&, const std::string& config,
                                     const std::string& mvn, const std::string& tokens, int, int device) {
  conf_ = load_conf(config);
  if (!tokens.empty() && file_exists(tokens)) tokens_ = read_lines(tokens);
  if (!mvn.empty()) parse_mvn_text(read_text_file(mvn), shift_, scale_);
  pf_engine_config ec;
  std::memset(&ec, 0, sizeof(ec));
  ec.struct_size = sizeof(ec);
  ec.device = device;
  ec.weights_path = model.c_str();
  ec.mvn_path = mvn.c_str();
  ec.fs = conf_.fs; ec.n_mels = conf_.n_mels; ec.lfr_m = conf_.lfr_m; ec.lfr_n = conf_.lfr_n;
  ec.snip_edges = conf_.snip_edges ? 1 : 0;
  ec.dither = conf_.dither;
  ec.frame_length_ms = 0; ec.frame_shift_ms = 0;     // never forwarded by the reference (OnlineWavFrontend.cs:20-27): kaldi defaults apply
  ec.window = conf_.window.c_str();
  engine_ = std::make_shared<Engine>(ec);
  // the streaming mirror carries the reference's literal geometry (OnlineStream.cs:44-46,263-278: 10 x 560 feature
  // cache, 16 x [512, 10] FSMN caches; OnlineWavFrontend.cs:152-188: sqrt(512)); a container of another geometry
  // would make Forward() index past those buffers, where the reference gets an ORT shape error
  const ModelCfg& m = engine_->model();
  PF_CHECK(m.kind_id() != 1, PF_ERR_UNSUPPORTED, "OnlineRecognizer: a SenseVoice container has no streaming graphs");
  PF_CHECK(m.d_model == 512 && m.feat_dim == 560 && m.kernel == 11, PF_ERR_UNSUPPORTED,
           "OnlineRecognizer: the streaming path is built for d_model 512, feature dim 560, FSMN kernel 11 (got " +
               std::to_string(m.d_model) + ", " + std::to_string(m.feat_dim) + ", " + std::to_string(m.kernel) + ")");
  PF_CHECK(conf_.lfr_m * conf_.n_mels == 560, PF_ERR_UNSUPPORTED, "OnlineRecognizer: lfr_m * n_mels must be 560");
}

std::shared_ptr<OnlineStreamM> OnlineRecognizerM::CreateOnlineStream() {
  if (disposed_) throw Error(PF_ERR_DISPOSED, "OnlineRecognizer");
  return std::make_shared<OnlineStreamM>(shared_from_this());
}

void OnlineRecognizerM::Dispose() {
  std::shared_ptr<Engine> e;
  {
    std::lock_guard<std::mutex> lk(mu_);
    if (disposed_.exchange(true)) return;
    e.swap(engine_);
  }
  if (e) {
    std::lock_guard<std::mutex> lk(e->mutex());
    std::lock_guard<std::mutex> lk2(ep_mu_);
    if (ep_states_) { hipSetDevice(e->device()); hipFree(ep_states_); ep_states_ = nullptr; ep_cap_ = 0; ep_free_.clear(); }
    if (ep_net_states_) { hipSetDevice(e->device()); hipFree(ep_net_states_); ep_net_states_ = nullptr; }
    if (ti_states_) { hipSetDevice(e->device()); hipFree(ti_states_); ti_states_ = nullptr; }
    if (pn_states_) { hipSetDevice(e->device()); hipFree(pn_states_); pn_states_ = nullptr; }
    if (pn_ws_) { hipSetDevice(e->device()); hipFree(pn_ws_); pn_ws_ = nullptr; pn_ws_bytes_ = 0; }
    pn_model_.reset();
    pn_on_ = false;
    ep_model_.reset();
    second_.reset();
  }
  e.reset();
}

// ------------------------------------------------------------------ endpointing and the second pass -------
void OnlineRecognizerM::SetEndpoint(const pf_endpoint_config* cfg) {
  if (disposed_) throw Error(PF_ERR_DISPOSED, "OnlineRecognizer");
  if (!cfg) { ep_on_ = false; return; }
  const pf_endpoint_config c = endpoint_check(cfg, (conf_.lfr_m == 1 && conf_.lfr_n == 1) ? 1 : conf_.lfr_n);
  PF_CHECK(!conf_.snip_edges, PF_ERR_UNSUPPORTED, "endpoint: snip_edges = true is not supported");
  PF_CHECK(conf_.n_mels == 80, PF_ERR_UNSUPPORTED, "endpoint: the streaming path carries 80 mel bins");
  std::lock_guard<std::mutex> lk(ep_mu_);
  ep_cfg_ = c;
  ep_on_ = true;
}

void OnlineRecognizerM::SetEndpointModel(const std::string& pfw_path) {
  if (disposed_) throw Error(PF_ERR_DISPOSED, "OnlineRecognizer");
  std::shared_ptr<const VadModel> vm;
  if (!pfw_path.empty()) {
    vm = vad_model_load(pfw_path);                              // throws before anything changes
    Engine::vad_stream_check(*vm);
  }
  std::shared_ptr<Engine> eh = engine();
  if (!eh) throw Error(PF_ERR_DISPOSED, "OnlineRecognizer");
  std::lock_guard<std::mutex> lk(eh->mutex());
  std::lock_guard<std::mutex> lk2(ep_mu_);
  if (!vm && !ep_model_) return;
  PF_CHECK(ep_live_ == 0, PF_ERR_UNSUPPORTED,
           "endpoint model: a live stream has already fed the detector (attach or detach before the first GetResults with audio)");
  eh->set_vad_model(vm);                                        // the refusals of pf_engine_set_vad_model
  PF_HIP(hipSetDevice(eh->device()));
  if (ep_net_states_) {
    PF_HIP(hipStreamSynchronize(eh->stream()));
    PF_HIP(hipFree(ep_net_states_));
    ep_net_states_ = nullptr;
  }
  ep_model_ = vm;
  ep_net_bytes_ = vm ? (size_t)vad_stream_layout(*vm).bytes : 0;
  if (vm && ep_cap_ > 0) {
    PF_HIP(hipMalloc((void**)&ep_net_states_, (size_t)ep_cap_ * ep_net_bytes_));
    PF_HIP(hipMemsetAsync(ep_net_states_, 0, (size_t)ep_cap_ * ep_net_bytes_, eh->stream()));
  }
}

void OnlineRecognizerM::SetSecondPass(std::shared_ptr<Recognizer> offline) {
  if (disposed_) throw Error(PF_ERR_DISPOSED, "OnlineRecognizer");
  if (offline) {
    PF_CHECK(!offline->disposed(), PF_ERR_DISPOSED, "OfflineRecognizer");
    PF_CHECK(!offline->vad_on(), PF_ERR_UNSUPPORTED, "second pass: the offline recognizer has SetVad on (one sentence must stay one stream)");
  }
  std::lock_guard<std::mutex> lk(ep_mu_);
  second_ = std::move(offline);
}

void OnlineRecognizerM::release_stream(int slot, bool ep_joined, bool decoded, bool punc_joined) {
  std::lock_guard<std::mutex> lk(ep_mu_);
  if (ep_states_ && slot >= 0 && slot < ep_cap_) ep_free_.push_back(slot);
  if (ep_joined) --ep_live_;
  if (decoded) --decoded_live_;
  if (punc_joined) --pn_live_;
}

void OnlineRecognizerM::SetPuncModel(const std::string& pfw_path, int max_context) {
  if (disposed_) throw Error(PF_ERR_DISPOSED, "OnlineRecognizer");
  std::shared_ptr<const PuncModel> pm;
  const int mc = max_context == 0 ? kPuncStreamDefaultContext : max_context;
  if (!pfw_path.empty()) {
    pm = punc_model_load(pfw_path);                             // throws before anything changes
    PF_CHECK(pm->causal == 1, PF_ERR_UNSUPPORTED, "streaming punctuation: the model is not causal (header key causal = 1)");
    PF_CHECK(mc >= 2 && mc <= kPuncStreamMaxContext, PF_ERR_INVALID_ARG, "streaming punctuation: max_context outside 2 .. 256");
  }
  std::shared_ptr<Engine> eh = engine();
  if (!eh) throw Error(PF_ERR_DISPOSED, "OnlineRecognizer");
  std::lock_guard<std::mutex> lk(eh->mutex());
  std::lock_guard<std::mutex> lk2(ep_mu_);
  if (!pm && !pn_model_) return;
  PF_CHECK(pn_live_ == 0, PF_ERR_UNSUPPORTED,
           "streaming punctuation: a live stream holds punctuation state (attach or detach when no such stream is alive)");
  eh->set_punc_model(pm);
  PF_HIP(hipSetDevice(eh->device()));
  if (pn_states_ || pn_ws_) {
    PF_HIP(hipStreamSynchronize(eh->stream()));
    if (pn_states_) PF_HIP(hipFree(pn_states_));
    if (pn_ws_) PF_HIP(hipFree(pn_ws_));
    pn_states_ = nullptr; pn_ws_ = nullptr; pn_ws_bytes_ = 0;
  }
  pn_model_ = pm;
  pn_bytes_ = pm ? (size_t)punc_stream_layout(*pm).bytes : 0;
  pn_max_context_ = mc;
  if (pm && ep_cap_ > 0) PF_HIP(hipMalloc((void**)&pn_states_, (size_t)ep_cap_ * pn_bytes_));   // (a block is zeroed where a stream joins)
  pn_on_ = pm != nullptr;
}

void OnlineRecognizerM::SetTokenInfo(bool on) {
  if (disposed_) throw Error(PF_ERR_DISPOSED, "OnlineRecognizer");
  std::shared_ptr<Engine> eh = engine();
  if (!eh) throw Error(PF_ERR_DISPOSED, "OnlineRecognizer");
  std::lock_guard<std::mutex> lk(eh->mutex());
  std::lock_guard<std::mutex> lk2(ep_mu_);
  if (on == ti_on_.load()) return;
  PF_CHECK(decoded_live_ == 0, PF_ERR_UNSUPPORTED,
           "token info: a live stream has already decoded a chunk (turn the mode on or off before the first GetResults with audio)");
  PF_HIP(hipSetDevice(eh->device()));
  if (ti_states_) {
    PF_HIP(hipStreamSynchronize(eh->stream()));
    PF_HIP(hipFree(ti_states_));
    ti_states_ = nullptr;
  }
  ti_bytes_ = on ? eh->online_slot_bytes() : 0;
  if (on && ep_cap_ > 0) PF_HIP(hipMalloc((void**)&ti_states_, (size_t)ep_cap_ * ti_bytes_));
  ti_on_ = on;
}

// grows one per-stream buffer from ep_cap_ to cap slots of `bytes` each (the old blocks copied on the device)
template <class T> static void grow_slots(Engine* e, T*& buf, int old_cap, int cap, size_t bytes) {
  T* p = nullptr;
  PF_HIP(hipMalloc((void**)&p, (size_t)cap * bytes));
  if (buf) {
    PF_HIP(hipMemcpyAsync(p, buf, (size_t)old_cap * bytes, hipMemcpyDeviceToDevice, e->stream()));
    PF_HIP(hipStreamSynchronize(e->stream()));
    PF_HIP(hipFree(buf));
  }
  buf = p;
}

void OnlineRecognizerM::ensure_slot(OnlineStreamM* s, Engine* e) {
  if (s->slot_ >= 0) return;
  std::lock_guard<std::mutex> ls(ep_mu_);
  PF_HIP(hipSetDevice(e->device()));
  if (ep_free_.empty()) {
    const int cap = std::max(64, 2 * ep_cap_);
    grow_slots(e, ep_states_, ep_cap_, cap, (size_t)PF_ENDPOINT_STATE_INTS * 4);
    if (ep_model_) grow_slots(e, ep_net_states_, ep_cap_, cap, ep_net_bytes_);   // the network's states grow with the detector's
    if (ti_on_) grow_slots(e, ti_states_, ep_cap_, cap, ti_bytes_);              // and so does the decoder state
    if (pn_model_) grow_slots(e, pn_states_, ep_cap_, cap, pn_bytes_);           // and the punctuation state
    for (int i = cap - 1; i >= ep_cap_; --i) ep_free_.push_back(i);
    ep_cap_ = cap;
  }
  s->slot_ = ep_free_.back();
  ep_free_.pop_back();
  s->cif_reset_ = s->cache_reset_ = true;                       // a reused slot's decoder state starts from zeros on its first step
}

// The detector's launch set for the call's streams that have new caller frames or a flush to make, the sentences its events
// close, then the second pass over those sentences (one GetResults of the attached offline recognizer).
void OnlineRecognizerM::ForwardEndpoint(const std::vector<OnlineStreamM*>& streams) {
  struct Closed { OnlineStreamM* s; size_t idx; std::vector<float> audio; };
  std::vector<Closed> closed;
  pf_endpoint_config c;
  std::shared_ptr<Recognizer> second;
  std::shared_ptr<const VadModel> net;
  {
    std::lock_guard<std::mutex> lk(ep_mu_);
    c = ep_cfg_;
    second = second_;
  }
  try {
    std::shared_ptr<Engine> eh = engine();
    if (disposed_ || !eh) throw Error(PF_ERR_DISPOSED, "OnlineRecognizer");
    Engine* e = eh.get();
    std::lock_guard<std::mutex> lk(e->mutex());
    std::shared_ptr<const PuncModel> punc;
    { std::lock_guard<std::mutex> ls(ep_mu_); net = ep_model_; punc = pn_model_; }      // (both change under the engine's mutex)
    // who takes part: new rows, or the flush once the model has decoded every chunk of a finished input
    std::vector<OnlineStreamM*> work;
    std::vector<int32_t> n_new, flush, slot;
    std::vector<float> rows;
    const size_t CLF = (size_t)chunk_length() * 80;
    for (OnlineStreamM* s : streams) {
      std::lock_guard<std::mutex> ls(s->mu);
      if (s->ep_flushed_ || std::find(work.begin(), work.end(), s) != work.end()) continue;
      const bool fl = s->finished_ && s->cache_samples_.empty() && s->Speech.size() < CLF && s->ep_origin_ >= 0;
      if (s->ep_rows_.empty() && !fl) continue;
      const int n = (int)(s->ep_rows_.size() / 80);
      PF_CHECK((int64_t)s->ep_fed_ + n <= PF_ENDPOINT_MAX_STREAM_FRAMES, PF_ERR_CAPACITY, "endpoint: more than PF_ENDPOINT_MAX_STREAM_FRAMES frames in one stream");
      work.push_back(s);
      n_new.push_back(n);
      flush.push_back(fl ? 1 : 0);
      rows.insert(rows.end(), s->ep_rows_.begin(), s->ep_rows_.end());
    }
    if (work.empty()) return;
    const int B = (int)work.size();
    for (OnlineStreamM* s : work) {
      ensure_slot(s, e);
      // The detector's and the network's block are zeroed where the stream JOINS the detector, not where its slot was handed
      // out: a stream of a recognizer with SetTokenInfo holds its slot from its first decode on, and the network's buffer may
      // have been allocated (SetEndpointModel) or the detector turned on since.
      if (!s->ep_joined_) {
        std::lock_guard<std::mutex> ls(ep_mu_);
        PF_HIP(hipSetDevice(e->device()));
        PF_HIP(hipMemsetAsync(ep_states_ + (size_t)s->slot_ * PF_ENDPOINT_STATE_INTS, 0, PF_ENDPOINT_STATE_INTS * 4, e->stream()));
        if (net) PF_HIP(hipMemsetAsync(ep_net_states_ + (size_t)s->slot_ * ep_net_bytes_, 0, ep_net_bytes_, e->stream()));
        s->ep_joined_ = true;
        ++ep_live_;
      }
      slot.push_back(s->slot_);
    }
    // an event per level at most and one for the flush; with the model a call releases up to `right` levels more than it brought
    const int right = net ? net->lfr_m - 1 - (net->lfr_m - 1) / 2 : 0;
    const int cap = *std::max_element(n_new.begin(), n_new.end()) + right + 1;
    std::vector<int32_t> out;
    e->endpoint_streams(ep_states_, slot.data(), rows.data(), n_new.data(), flush.data(), B, c, cap, out, net ? ep_net_states_ : nullptr);
    for (int b = 0; b < B; ++b) {
      OnlineStreamM* s = work[(size_t)b];
      std::lock_guard<std::mutex> ls(s->mu);
      s->ep_rows_.clear();
      s->ep_fed_ += n_new[(size_t)b];
      if (flush[(size_t)b]) s->ep_flushed_ = true;
      const int n_ev = out[(size_t)b];
      PF_CHECK(n_ev >= 0 && n_ev <= cap, PF_ERR_DEVICE, "endpoint: event count outside 0 .. cap");
      const int32_t* ev = out.data() + 3 * (size_t)B + (size_t)b * cap * 3;
      for (int k = 0; k < n_ev; ++k) {
        const int64_t fb = ev[3 * k], fe = ev[3 * k + 1];
        OnlineStreamM::SentenceM sen;
        sen.begin_ms = (int)((s->ep_origin_ + 160 * fb) / 16);
        sen.end_ms = (int)((s->ep_origin_ + 160 * fe) / 16);
        sen.kind = ev[3 * k + 2];
        sen.first_pass = online_decode_text(tokens_, s->Tokens);            // after this chunk's ids were appended
        sen.text = sen.first_pass;
        sen.tokens = s->token_info();                                        // (cleared with Tokens at the reset)
        if (punc && !s->pn_close_.on) {                                      // the sentence's words, before the reset forgets them
          s->pn_close_.c = online_committed_words(*punc, tokens_, s->Tokens);
          online_check_committed_prefix(s->pn_words_, s->pn_close_.c);
          s->pn_close_.sentence = s->Sentences.size();
          s->pn_close_.on = true;
        }
        s->ResetDecoder();
        const int64_t a0 = 160 * fb - s->ep_audio_base_, a1 = std::min<int64_t>(s->ep_samples_, 160 * fe) - s->ep_audio_base_;
        PF_CHECK(a0 >= 0 && a1 > a0 && a1 <= (int64_t)s->ep_audio_.size(), PF_ERR_RECOGNITION, "endpoint: a sentence outside the retained audio");
        if (second) closed.push_back(Closed{s, s->Sentences.size(), std::vector<float>(s->ep_audio_.begin() + a0, s->ep_audio_.begin() + a1)});
        s->Sentences.push_back(std::move(sen));
        s->ep_prev_end_ = (int)fe;
      }
      s->InSpeech = out[(size_t)B + b] != 0;
      const int ob = out[2 * (size_t)B + b];
      s->OpenBeginMs = s->InSpeech ? (int)((s->ep_origin_ + 160 * (int64_t)ob) / 16) : -1;
      // what a sentence that is open, or opens later, can still need: from prev_end, and from the open begin or pad_begin + window
      // frames behind the newest frame
      // (with the model the detector has seen the released levels only: `right` frames fewer until the flush)
      const int64_t keep = 160 * (int64_t)std::max(s->ep_prev_end_, s->InSpeech ? ob : std::max(0, s->ep_fed_ - right - c.pad_begin - c.window));
      if (keep > s->ep_audio_base_) {
        const int64_t drop = std::min<int64_t>(keep - s->ep_audio_base_, (int64_t)s->ep_audio_.size());
        s->ep_audio_.erase(s->ep_audio_.begin(), s->ep_audio_.begin() + drop);
        s->ep_audio_base_ += drop;
      }
      if (s->ep_flushed_) { std::vector<float>().swap(s->ep_audio_); }
    }
  } catch (const Error& ex) {
    if (ex.code != PF_ERR_RECOGNITION) throw;
    throw Error(PF_ERR_RECOGNITION, std::string("Online recognition failed: ") + ex.what());
  }
  if (closed.empty() || !second) return;
  // the second pass: one plain offline stream per sentence, in the call's stream order and then in time order, ONE GetResults
  std::vector<std::shared_ptr<Stream>> off;
  std::vector<Stream*> ptrs;
  for (Closed& cl : closed) {
    off.push_back(second->CreateOfflineStream());
    off.back()->AddSamples(cl.audio.data(), (int64_t)cl.audio.size());
    ptrs.push_back(off.back().get());
  }
  second->GetResults(ptrs);
  const std::vector<ResultEntity>& res = second->results_of_this_thread();
  for (size_t i = 0; i < closed.size(); ++i) {
    std::lock_guard<std::mutex> ls(closed[i].s->mu);
    OnlineStreamM::SentenceM& sen = closed[i].s->Sentences[closed[i].idx];
    sen.text = i < res.size() ? res[i].Text : std::string();
    sen.offline = off[i];
  }
}

void OnlineRecognizerM::Forward(const std::vector<OnlineStreamM*>& streams) {
  if (streams.empty()) return;
  if (token_info_on())                                          // the slots of a launch are distinct: refused before a chunk is taken
    for (size_t i = 0; i < streams.size(); ++i)
      for (size_t j = 0; j < i; ++j)
        PF_CHECK(streams[i] != streams[j], PF_ERR_INVALID_ARG, "token info: a stream twice in one GetResults");
  std::vector<OnlineStreamM*> work;
  std::vector<std::vector<float>> chunks;
  for (OnlineStreamM* s : streams) {                            // :349-363
    std::vector<float> c;
    if (!s->GetDecodeChunk(c)) continue;
    chunks.push_back(std::move(c));
    work.push_back(s);
  }
  if (work.empty()) return;
  try {
    std::shared_ptr<Engine> eh = engine();
    if (disposed_ || !eh) throw Error(PF_ERR_DISPOSED, "OnlineRecognizer");
    Engine* e = eh.get();
    std::lock_guard<std::mutex> lk(e->mutex());
    const int B = (int)work.size(), W = 560, D = 512, nd = e->dec_layers(), CW = 10;
    // PadSequence_unittest (:460-473): equal lengths assumed (stream i copied at i * its own length), then every
    // exact 0 becomes -23.025850929940457F (NOT multiplied by 32768 as the offline sentinel is)
    size_t maxlen = 0;
    for (auto& c : chunks) maxlen = std::max(maxlen, c.size());
    std::vector<float> speech(maxlen * (size_t)B, 0.f);
    for (int i = 0; i < B; ++i) {
      if ((size_t)i * chunks[(size_t)i].size() + chunks[(size_t)i].size() > speech.size())
        throw Error(PF_ERR_RECOGNITION, "Destination array was not long enough (PadSequence)");
      std::memcpy(&speech[(size_t)i * chunks[(size_t)i].size()], chunks[(size_t)i].data(), chunks[(size_t)i].size() * 4);
    }
    for (float& v : speech) v = v == 0.f ? -23.025850929940457f : v;
    const int Tc = (int)(maxlen / W);
    for (OnlineStreamM* s : work)
      if (!s->decoded_) { std::lock_guard<std::mutex> ls(ep_mu_); s->decoded_ = true; ++decoded_live_; }
    if (token_info_on()) { ForwardDevice(e, work, speech, Tc); return; }
    // stack_states (OnlineModel.cs:199-220): EVERY layer's in_cache is built from the streams' LAYER-0 state
    std::vector<float> cin((size_t)nd * B * D * CW);
    for (int l = 0; l < nd; ++l)
      for (int n = 0; n < B; ++n)
        std::memcpy(&cin[((size_t)l * B + n) * D * CW], work[(size_t)n]->States[0].data(), (size_t)D * CW * 4);
    // EncoderProj (:49-124)
    std::vector<float> enc((size_t)B * Tc * D), alphas((size_t)B * Tc);
    e->online_encoder(speech.data(), B, Tc, enc.data(), alphas.data());
    // PredictorProj (:126-231)
    std::vector<std::vector<std::vector<float>>> fired((size_t)B);
    const float thr = e->model().cif_threshold;
    size_t len_time = 0;
    for (int b = 0; b < B; ++b) {
      std::vector<float> a(alphas.begin() + (long)b * Tc, alphas.begin() + (long)(b + 1) * Tc);
      online_dynamic_mask(a);
      OnlineStreamM* s = work[(size_t)b];
      for (int t = 0; t < Tc; ++t)
        s->CifHidden.emplace_back(enc.begin() + ((long)b * Tc + t) * D, enc.begin() + ((long)b * Tc + t + 1) * D);
      s->CifAlpha.insert(s->CifAlpha.end(), a.begin(), a.end());
      if (b == 0) len_time = s->CifAlpha.size();                // :150: stream 0's count is used for every stream
    }
    int max_tok = 0;
    for (int b = 0; b < B; ++b) {
      OnlineStreamM* s = work[(size_t)b];
      if (s->CifAlpha.size() < len_time || s->CifHidden.size() < len_time)
        throw Error(PF_ERR_RECOGNITION, "Index was out of range (CIF cache)");
      std::vector<std::vector<float>> h(s->CifHidden.begin(), s->CifHidden.begin() + (long)len_time);
      std::vector<float> a(s->CifAlpha.begin(), s->CifAlpha.begin() + (long)len_time);
      float ca = 0.f;
      std::vector<float> ch;
      online_cif(h, a, thr, fired[(size_t)b], ca, ch);
      s->CifAlpha.assign(1, ca);                                // :214-220
      s->CifHidden.assign(1, ch);
      max_tok = std::max(max_tok, (int)fired[(size_t)b].size());
    }
    if (max_tok == 0) return;                                   // :380: Acoustic_embeds.Length == 0
    std::vector<float> emb((size_t)B * max_tok * D, 0.f);
    std::vector<int32_t> emb_len((size_t)B);
    for (int b = 0; b < B; ++b) {
      emb_len[(size_t)b] = (int32_t)fired[(size_t)b].size();
      for (size_t l = 0; l < fired[(size_t)b].size(); ++l)
        std::memcpy(&emb[((size_t)b * max_tok + l) * D], fired[(size_t)b][l].data(), (size_t)D * 4);
    }
    // DecoderProj (:233-334) + unstack_states (OnlineModel.cs:221-247)
    std::vector<int64_t> ids((size_t)B * max_tok);
    std::vector<float> cout((size_t)nd * B * D * CW);
    e->online_decoder(enc.data(), B, Tc, emb.data(), max_tok, emb_len.data(), cin.data(), nullptr, ids.data(), cout.data());
    for (int b = 0; b < B; ++b) {
      OnlineStreamM* s = work[(size_t)b];
      // :389: ALL max_tok positions are appended, also for streams that fired fewer tokens
      s->Tokens.insert(s->Tokens.end(), ids.begin() + (long)b * max_tok, ids.begin() + (long)(b + 1) * max_tok);
      for (int l = 0; l < nd; ++l)
        s->States[(size_t)l].assign(cout.begin() + ((long)l * B + b) * D * CW, cout.begin() + ((long)l * B + b + 1) * D * CW);
    }
  } catch (const Error& ex) {
    if (ex.code == PF_ERR_RECOGNITION && std::string(ex.what()).rfind("Online recognition failed", 0) == 0) throw;
    throw Error(PF_ERR_RECOGNITION, std::string("Online recognition failed: ") + ex.what());   // :397-400
  }
}

// Forward with SetTokenInfo: the chunk step on the device (Engine::online_step), then ids, scores, fire entries and times per stream.
// The decoder state of a stream is its slot of ti_states_; nothing of it is mirrored on the host.
void OnlineRecognizerM::ForwardDevice(Engine* e, const std::vector<OnlineStreamM*>& work, const std::vector<float>& speech, int Tc) {
  const int B = (int)work.size(), lo = 5, hi = 15;             // DynamicMask (OnlineModel.cs:141-165): chunk_size 5, lfr 10
  PF_CHECK(speech.size() == (size_t)B * Tc * 560, PF_ERR_RECOGNITION, "Destination array was not long enough (PadSequence)");
  for (int i = 0; i < B; ++i)                                   // (Forward has refused this already; a race with SetTokenInfo ends here)
    for (int j = 0; j < i; ++j) PF_CHECK(work[(size_t)i] != work[(size_t)j], PF_ERR_INVALID_ARG, "token info: a stream twice in one GetResults");
  std::vector<int32_t> slot((size_t)B), cif_reset((size_t)B), cache_reset((size_t)B);
  for (int b = 0; b < B; ++b) {
    OnlineStreamM* s = work[(size_t)b];
    ensure_slot(s, e);
    slot[(size_t)b] = s->slot_; cif_reset[(size_t)b] = s->cif_reset_ ? 1 : 0; cache_reset[(size_t)b] = s->cache_reset_ ? 1 : 0;
  }
  char* states = nullptr;
  { std::lock_guard<std::mutex> ls(ep_mu_); states = ti_states_; }
  PF_CHECK(states != nullptr, PF_ERR_DEVICE, "token info: no state buffer");
  Engine::OnlineStepOut out;
  e->online_step(speech.data(), B, Tc, states, slot.data(), cif_reset.data(), cache_reset.data(), lo, hi, out);
  const int L = out.max_tok, cap = out.cap;
  const int64_t fs = conf_.fs > 0 ? conf_.fs : 16000;
  for (int b = 0; b < B; ++b) {
    OnlineStreamM* s = work[(size_t)b];
    std::lock_guard<std::mutex> ls(s->mu);
    s->cif_reset_ = false;
    if (L > 0) s->cache_reset_ = false;                         // (no decoder ran: the caches still await their reset)
    s->token_info();
    // the time rule: the first position >= p of this chunk whose frame has an index, else the caller samples consumed so far
    auto index_from = [&](int p) {
      for (int q = std::max(p, 0); q < Tc && q < (int)s->chunk_idx_.size(); ++q)
        if (s->chunk_idx_[(size_t)q] >= 0) return s->chunk_idx_[(size_t)q];
      return s->caller_samples_;
    };
    const int count = out.counts[(size_t)b];
    for (int l = 0; l < L; ++l) {                               // :389: ALL max_tok positions are appended
      pf_online_token t{out.ids[(size_t)b * L + l], -1, -1, out.scores[(size_t)b * L + l], 0};
      if (l < count) {
        t.entry = out.fire_entry[(size_t)b * cap + l];
        const int64_t idx = t.entry == 0 ? (s->carry_idx_ >= 0 ? s->carry_idx_ : s->caller_samples_) : index_from(t.entry - 1);
        t.time_ms = (int32_t)(idx * 1000 / fs);
        t.flags = PF_ONLINE_TOKEN_FIRED | PF_ONLINE_TOKEN_TIMED;
      }
      s->Tokens.push_back(t.id);
      s->TokenInfo.push_back(t);
    }
    s->carry_idx_ = index_from(hi - 1);                         // what a token fired on the next chunk's carry takes
  }
}

// Streaming punctuation: the newly committed words of the call's streams (at a sentence close and at the end of the input every
// remaining word, with the flush) in ONE punc_stream launch: one staged copy up, one down; no launch when nothing is new.
void OnlineRecognizerM::ForwardPunc(const std::vector<OnlineStreamM*>& streams) {
  struct Job { OnlineStreamM* s; OnlineCommitted c; size_t n_send = 0, sentence = 0; bool flush = false, close = false, launch = false; int n_new = 0; };
  try {
    std::shared_ptr<Engine> eh = engine();
    if (disposed_ || !eh) throw Error(PF_ERR_DISPOSED, "OnlineRecognizer");
    Engine* e = eh.get();
    std::lock_guard<std::mutex> lk(e->mutex());
    std::shared_ptr<const PuncModel> pm;
    int mc = 0;
    { std::lock_guard<std::mutex> ls(ep_mu_); pm = pn_model_; mc = pn_max_context_; }
    if (!pm) return;
    std::vector<Job> jobs;
    const size_t CLF = (size_t)chunk_length() * 80;
    int B = 0, ld = 1;
    for (OnlineStreamM* s : streams) {
      bool seen = false;
      for (const Job& j : jobs) seen = seen || j.s == s;
      if (seen) continue;
      std::lock_guard<std::mutex> ls(s->mu);
      Job j;
      j.s = s;
      if (s->pn_close_.on) {
        j.c = std::move(s->pn_close_.c);
        j.sentence = s->pn_close_.sentence;
        j.close = j.flush = true;
        s->pn_close_ = OnlineStreamM::PuncPending();
      } else {
        if (s->pn_flushed_) continue;                          // the end-of-input flush was made: nothing follows it
        j.c = online_committed_words(*pm, tokens_, s->Tokens);
        online_check_committed_prefix(s->pn_words_, j.c);
        j.flush = s->finished_ && s->cache_samples_.empty() && s->Speech.size() < CLF;
      }
      j.n_send = j.flush ? j.c.words.size() : j.c.n_committed;   // a flush takes the held-back word too
      j.n_new = (int)(j.n_send - s->pn_words_.size());
      j.launch = j.n_new > 0 || (j.flush && s->pn_joined_);
      if (j.launch) { ++B; ld = std::max(ld, j.n_new); }
      jobs.push_back(std::move(j));
    }
    std::vector<int32_t> down;
    if (B > 0) {
      PF_HIP(hipSetDevice(e->device()));
      const size_t nB = (size_t)B, cells = nB * (size_t)ld, up_n = 3 * nB + cells, down_n = 2 * cells + nB;
      std::vector<int32_t> up(up_n, 0);
      int b = 0;
      for (Job& j : jobs) {
        if (!j.launch) continue;
        OnlineStreamM* s = j.s;
        ensure_slot(s, e);
        if (!s->pn_joined_) {                                  // the block is zeroed where the stream first uses it
          std::lock_guard<std::mutex> ls(ep_mu_);
          PF_HIP(hipMemsetAsync(pn_states_ + (size_t)s->slot_ * pn_bytes_, 0, pn_bytes_, e->stream()));
          s->pn_joined_ = true;
          ++pn_live_;
        }
        up[(size_t)b] = s->slot_; up[nB + b] = j.n_new; up[2 * nB + b] = j.flush ? 1 : 0;
        for (int i = 0; i < j.n_new; ++i) up[3 * nB + (size_t)b * ld + i] = j.c.words[j.n_send - (size_t)j.n_new + (size_t)i].id;
        ++b;
      }
      char* states = nullptr;
      {
        std::lock_guard<std::mutex> ls(ep_mu_);
        if (pn_ws_bytes_ < (up_n + down_n) * 4) {
          if (pn_ws_) { PF_HIP(hipStreamSynchronize(e->stream())); PF_HIP(hipFree(pn_ws_)); pn_ws_ = nullptr; pn_ws_bytes_ = 0; }
          PF_HIP(hipMalloc((void**)&pn_ws_, 2 * (up_n + down_n) * 4));
          pn_ws_bytes_ = 2 * (up_n + down_n) * 4;
        }
        states = pn_states_;
      }
      PF_CHECK(states != nullptr, PF_ERR_DEVICE, "streaming punctuation: no state buffer");
      int32_t* d_up = reinterpret_cast<int32_t*>(pn_ws_);
      int32_t* d_down = d_up + up_n;
      PF_HIP(hipMemcpyAsync(d_up, up.data(), up_n * 4, hipMemcpyHostToDevice, e->stream()));
      e->punc_stream_step(states, d_up, d_up + 3 * nB, ld, d_up + nB, d_up + 2 * nB, B, mc, 0, d_down, d_down + cells, nullptr, d_down + 2 * cells);
      down.resize(down_n);
      PF_HIP(hipMemcpyAsync(down.data(), d_down, down_n * 4, hipMemcpyDeviceToHost, e->stream()));
      PF_HIP(hipStreamSynchronize(e->stream()));
    }
    int b = 0;
    for (Job& j : jobs) {
      OnlineStreamM* s = j.s;
      std::lock_guard<std::mutex> ls(s->mu);
      if (j.launch) {
        const size_t cells = (size_t)B * ld;
        for (int i = 0; i < j.n_new; ++i) {
          const int32_t p = down[(size_t)b * ld + i];
          PF_CHECK(p >= 0 && p < pm->n_punc, PF_ERR_DEVICE, "streaming punctuation: a mark outside punc_list");
          s->PuncIds.push_back(p);
          s->PuncFlags.push_back(down[cells + (size_t)b * ld + i]);
          s->pn_words_.push_back(online_word(j.c, j.n_send - (size_t)j.n_new + (size_t)i));
        }
        const int32_t fm = down[2 * cells + b];
        if (j.flush && fm >= 0 && fm < pm->n_punc && !s->PuncIds.empty()) s->PuncIds.back() = fm;   // the flush's edit of the newest word
        ++b;
      }
      std::vector<int32_t> ids(s->PuncIds);
      ids.resize(j.c.words.size(), pm->id_none);               // a held-back word is written raw
      const std::string text = host_punc_assemble(*pm, j.c.text, j.c.words, ids.data(), nullptr);
      if (j.close) {
        if (j.sentence < s->Sentences.size()) {
          s->Sentences[j.sentence].punctuated = text;
          s->Sentences[j.sentence].punc_ids = s->PuncIds;
        }
        s->PuncIds.clear(); s->PuncFlags.clear(); s->pn_words_.clear(); s->Punctuated.clear();   // the next sentence starts a fresh context
      } else {
        s->Punctuated = text;
        if (j.flush) s->pn_flushed_ = true;
      }
    }
  } catch (const Error& ex) {
    if (ex.code != PF_ERR_RECOGNITION) throw;
    throw Error(PF_ERR_RECOGNITION, std::string("Online recognition failed: ") + ex.what());
  }
}

std::vector<std::string> OnlineRecognizerM::GetResults(const std::vector<OnlineStreamM*>& streams) {
  Forward(streams);
  if (endpoint_on()) ForwardEndpoint(streams);
  if (punc_on()) ForwardPunc(streams);
  std::vector<std::string> out;
  for (OnlineStreamM* s : streams) out.push_back(online_decode_text(tokens_, s->Tokens));
  return out;
}

}  // namespace pf
