// c_api.cpp — extern "C" boundary (include/paraformer_hip.h).  Every entry point converts C++
// exceptions into a negative pf_status + thread-local message; no exception crosses the ABI.
#include <algorithm>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>

#include "engine.h"
#include "group.h"
#include "online.h"
#include "recognizer.h"
#include "shards_sim.h"

namespace pf {
static thread_local std::string g_last_error;
void set_last_error(const std::string& m) { g_last_error = m; }
}  // namespace pf

using namespace pf;

// Handle shells outlive the objects they point to: a second pf_engine_destroy / pf_recognizer_free / pf_stream_free on
// the same handle (Dispose followed by a finaliser, OfflineRecognizer.cs:448-476) finds an empty shell instead of freed
// memory.  Engine / recognizer / group shells (a handful per process) are never returned to the allocator; STREAM shells
// — one per utterance in a server — go through a quarantine (ShellPool below): a freed shell answers PF_ERR_DISPOSED for
// as long as it sits in the queue and is handed out again only after kQuarantine younger frees, so the memory is bounded
// (a few MB) instead of growing by one shell per stream for the life of the process.  The device / host state a shell
// pointed to IS released at once.
struct pf_engine {
  std::mutex mu;
  std::shared_ptr<Engine> e;
};
struct pf_recognizer {
  std::mutex mu;
  std::shared_ptr<Recognizer> r;
  pf_engine eng;
};
struct pf_stream {
  std::shared_ptr<Stream> s;
  bool freed = false;
};
struct pf_decoded { ResultEntity r; };
struct pf_online_recognizer {
  std::mutex mu;
  std::shared_ptr<OnlineRecognizerM> r;
  pf_engine eng;
};
struct pf_online_stream {
  std::shared_ptr<OnlineStreamM> s;
  bool freed = false;
  std::vector<std::shared_ptr<pf_stream>> views;    // borrowed offline-stream handles (pf_online_stream_sentence_result), by sentence
};
struct pf_group {
  std::mutex mu;
  std::shared_ptr<Group> g;
  std::vector<std::unique_ptr<pf_engine>> views;    // borrowed engine handles (pf_group_engine)
};

// Recycles shells of type T (default-constructible, with `bool freed`) through a FIFO quarantine.
template <class T>
class ShellPool {
 public:
  static constexpr size_t kQuarantine = 1 << 16;
  T* get() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (q_.size() > kQuarantine) {
        T* t = q_.front();
        q_.pop_front();
        *t = T();                                     // a stale handle older than kQuarantine frees now aliases a live stream
        return t;
      }
    }
    return new T();
  }
  void retire(T* t) {                                 // the caller has emptied the shell and set freed
    std::lock_guard<std::mutex> lk(mu_);
    q_.push_back(t);
  }
 private:
  std::mutex mu_;
  std::deque<T*> q_;
};
static ShellPool<pf_stream>& stream_shells() { static ShellPool<pf_stream>* p = new ShellPool<pf_stream>(); return *p; }
static ShellPool<pf_online_stream>& online_stream_shells() { static ShellPool<pf_online_stream>* p = new ShellPool<pf_online_stream>(); return *p; }

#define PF_TRY try {
#define PF_CATCH                                                          \
  }                                                                       \
  catch (const pf::Error& ex) { pf::set_last_error(ex.what()); return ex.code; } \
  catch (const std::bad_alloc&) { pf::set_last_error("out of host memory"); return PF_ERR_DEVICE; } \
  catch (const std::exception& ex) { pf::set_last_error(ex.what()); return PF_ERR_INVALID_ARG; }

#define NEED(p) PF_CHECK((p) != nullptr, PF_ERR_INVALID_ARG, "null argument: " #p)

// a new handle on an immutable model (pf_vad_model, pf_punc_model) from a path or from memory; *m is null on a failure
template <class H, class Make>
static int new_model_handle(H** m, const void* arg, const char* arg_name, Make&& make) {
  PF_TRY
  NEED(m);
  PF_CHECK(arg != nullptr, PF_ERR_INVALID_ARG, std::string("null argument: ") + arg_name);
  *m = nullptr;
  *m = new H{make()};
  return PF_OK;
  PF_CATCH
}

extern "C" {

int pf_version(void) { return PF_ABI_VERSION; }
const char* pf_last_error(void) { return pf::g_last_error.c_str(); }

int pf_engine_create(const pf_engine_config* cfg, pf_engine** out) {
  PF_TRY
  NEED(cfg); NEED(out);
  PF_CHECK(cfg->struct_size == (int32_t)sizeof(pf_engine_config), PF_ERR_INVALID_ARG, "pf_engine_config.struct_size mismatch");
  *out = nullptr;
  pf_engine* h = new pf_engine();
  try {
    h->e = std::make_shared<Engine>(*cfg);
  } catch (...) {
    delete h;
    throw;
  }
  *out = h;
  return PF_OK;
  PF_CATCH
}

void pf_engine_destroy(pf_engine* h) {
  if (!h) return;
  std::shared_ptr<Engine> e;
  {
    std::lock_guard<std::mutex> lk(h->mu);
    e.swap(h->e);
  }
  if (!e) return;                                   // second destroy: nothing left to do
  try {
    { std::lock_guard<std::mutex> lk(e->mutex()); } // a call in flight on another thread finishes first
    e.reset();
  } catch (...) {}
}

static std::shared_ptr<Engine> E(pf_engine* h) {
  PF_CHECK(h != nullptr, PF_ERR_INVALID_ARG, "null engine");
  std::lock_guard<std::mutex> lk(h->mu);
  PF_CHECK(h->e != nullptr, PF_ERR_DISPOSED, "OfflineRecognizer");
  return h->e;                                      // the caller's copy keeps the engine alive for the call
}

int pf_engine_info(pf_engine* h, int32_t* kind, int32_t* vocab, int32_t* feat_dim, int32_t* has_ts) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  if (kind) *kind = e->model().kind_id();
  if (vocab) *vocab = e->model().vocab;
  if (feat_dim) *feat_dim = e->model().feat_dim;
  if (has_ts) *has_ts = e->model().timestamp_head ? 1 : 0;
  return PF_OK;
  PF_CATCH
}

int pf_frontend_num_frames(pf_engine* h, int64_t n, int32_t* t) {
  PF_TRY
  NEED(t);
  *t = E(h)->num_lfr_frames(n);
  return PF_OK;
  PF_CATCH
}

int pf_frontend(pf_engine* h, const float* samples, int64_t n, float* feats, int64_t cap, int32_t* t_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  if (!samples) throw Error(PF_ERR_NULL_SAMPLES, "source");
  std::lock_guard<std::mutex> lk(e->mutex());
  std::vector<float> f;
  int t = 0;
  e->frontend_host(samples, n, f, t);
  if (t_out) *t_out = t;
  PF_CHECK((int64_t)f.size() <= cap, PF_ERR_CAPACITY, "feats capacity < " + std::to_string(f.size()));
  if (!f.empty()) { NEED(feats); std::memcpy(feats, f.data(), f.size() * 4); }
  return PF_OK;
  PF_CATCH
}

int pf_fbank(pf_engine* h, const float* samples, int64_t n, float* out, int64_t cap, int32_t* t80_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  if (!samples) throw Error(PF_ERR_NULL_SAMPLES, "source");
  std::lock_guard<std::mutex> lk(e->mutex());
  std::vector<float> f;
  int t = 0;
  e->fbank_host(samples, n, f, t);
  if (t80_out) *t80_out = t;
  PF_CHECK((int64_t)f.size() <= cap, PF_ERR_CAPACITY, "fbank capacity < " + std::to_string(f.size()));
  if (!f.empty()) { NEED(out); std::memcpy(out, f.data(), f.size() * 4); }
  return PF_OK;
  PF_CATCH
}

static bool want_logits(const pf_batch_out* o) { return o && o->logits && o->logits_cap > 0; }

int pf_forward_feats(pf_engine* h, const float* speech, int32_t B, int32_t Tmax, const int32_t* hotwords,
                     int32_t n_hotwords, pf_batch_out* out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(out);
  std::lock_guard<std::mutex> lk(e->mutex());
  if (e->model().seaco) e->set_hotwords(hotwords, hotwords ? n_hotwords : 0);
  e->forward_feats_host(speech, B, Tmax, want_logits(out));
  e->publish_thread_result();
  e->fetch(out);
  return PF_OK;
  PF_CATCH
}

int pf_model_proj(pf_engine* h, const float* const* speech, const int32_t* lens, int32_t B,
                  const int32_t* hotwords, int32_t n_hotwords, pf_batch_out* out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(out); NEED(speech); NEED(lens);
  std::lock_guard<std::mutex> lk(e->mutex());
  if (e->model().seaco) e->set_hotwords(hotwords, hotwords ? n_hotwords : 0);
  e->model_proj_host(speech, lens, B, want_logits(out));
  e->publish_thread_result();
  e->fetch(out);
  return PF_OK;
  PF_CATCH
}

int pf_recognize(pf_engine* h, const float* const* samples, const int64_t* n, int32_t B, const int32_t* hotwords,
                 int32_t n_hotwords, pf_batch_out* out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(out); NEED(samples); NEED(n);
  std::lock_guard<std::mutex> lk(e->mutex());
  if (e->model().seaco) e->set_hotwords(hotwords, hotwords ? n_hotwords : 0);
  e->stage_audio(samples, n, B);
  e->run_staged(want_logits(out));
  e->publish_thread_result();
  e->fetch(out);
  return PF_OK;
  PF_CATCH
}

int pf_pcm_num_samples(const pf_pcm_desc* desc, int32_t fs, int64_t n_values, int64_t* n_out) {
  PF_TRY
  NEED(desc); NEED(n_out);
  *n_out = pcm_plan(*desc, fs, n_values).n_out;
  return PF_OK;
  PF_CATCH
}

int pf_stage_pcm(pf_engine* h, const void* const* data, const int64_t* n_values, const pf_pcm_desc* descs, int32_t n_descs,
                 int32_t B) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(data); NEED(n_values); NEED(descs);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->stage_pcm(data, n_values, descs, n_descs, B);
  return PF_OK;
  PF_CATCH
}

int pf_recognize_pcm(pf_engine* h, const void* const* data, const int64_t* n_values, const pf_pcm_desc* descs, int32_t n_descs,
                     int32_t B, const int32_t* hotwords, int32_t n_hotwords, pf_batch_out* out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(out); NEED(data); NEED(n_values); NEED(descs);
  std::lock_guard<std::mutex> lk(e->mutex());
  if (e->model().seaco) e->set_hotwords(hotwords, hotwords ? n_hotwords : 0);
  e->stage_pcm(data, n_values, descs, n_descs, B);
  e->run_staged(want_logits(out));
  e->publish_thread_result();
  e->fetch(out);
  return PF_OK;
  PF_CATCH
}

int pf_engine_set_hotwords(pf_engine* h, const int32_t* hotwords, int32_t n_hotwords) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  PF_CHECK(n_hotwords >= 0 && (n_hotwords == 0 || hotwords), PF_ERR_INVALID_ARG, "set_hotwords: bad arguments");
  std::lock_guard<std::mutex> lk(e->mutex());
  if (e->model().seaco) e->set_hotwords(hotwords, n_hotwords);
  return PF_OK;
  PF_CATCH
}

int pf_stage_audio(pf_engine* h, const float* const* samples, const int64_t* n, int32_t B) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(samples); NEED(n);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->stage_audio(samples, n, B);
  return PF_OK;
  PF_CATCH
}

int pf_run_staged(pf_engine* h) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->drop_thread_result();               // pf_fetch after this call reads the engine's staged result
  e->run_staged(false);
  return PF_OK;
  PF_CATCH
}

int pf_sync(pf_engine* h) {
  PF_TRY
  E(h)->sync();
  return PF_OK;
  PF_CATCH
}

int pf_fetch(pf_engine* h, pf_batch_out* out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->fetch(out);
  return PF_OK;
  PF_CATCH
}

int pf_fetch_ids_device(pf_engine* h, int64_t* ids_dev, int32_t l_cap, int32_t* L_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->fetch_ids_device(ids_dev, l_cap, L_out);
  return PF_OK;
  PF_CATCH
}

int pf_engine_set_decode(pf_engine* h, int32_t flags) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->set_decode(flags);
  return PF_OK;
  PF_CATCH
}

int pf_fetch_scores(pf_engine* h, float* scores, int64_t cap, int32_t* L_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->fetch_scores(scores, cap, L_out);
  return PF_OK;
  PF_CATCH
}

int pf_fetch_ctc(pf_engine* h, int64_t* ids, int32_t* first, int32_t* last, float* score, int32_t cap, int32_t* n,
                 int32_t* n_max) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->fetch_ctc(ids, first, last, score, cap, n, n_max);
  return PF_OK;
  PF_CATCH
}

int pf_engine_set_topk(pf_engine* h, int32_t k) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->set_topk(k);
  return PF_OK;
  PF_CATCH
}

int pf_fetch_topk(pf_engine* h, int64_t* ids, float* val, int32_t* n, int64_t cap_rows, int32_t* L_out, int32_t* K_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->fetch_topk(ids, val, n, cap_rows, L_out, K_out);
  return PF_OK;
  PF_CATCH
}

int pf_host_nbest(const int64_t* /*ids*/, const float* val, const int32_t* n, int32_t L, int32_t K, int32_t n_free, int32_t N,
                  int32_t* out_ranks, double* out_scores, int32_t* n_out) {
  PF_TRY
  NEED(val); NEED(n); NEED(out_ranks); NEED(out_scores); NEED(n_out);
  *n_out = host_nbest(val, n, L, K, n_free, N, out_ranks, out_scores);
  return PF_OK;
  PF_CATCH
}

int pf_engine_set_ctc_beam(pf_engine* h, int32_t W, int32_t N) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->set_ctc_beam(W, N);
  return PF_OK;
  PF_CATCH
}

int pf_fetch_ctc_beam(pf_engine* h, int64_t* ids, int32_t* len, double* score, int32_t cap, int32_t* n_hyp, int32_t* len_max) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->fetch_ctc_beam(ids, len, score, cap, n_hyp, len_max, nullptr);
  return PF_OK;
  PF_CATCH
}

int pf_host_ctc_beam(const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val, const int32_t* n, int32_t T,
                     int32_t K, int32_t blank, int32_t W, int32_t N, int64_t* out_ids, int32_t* out_len, double* out_score,
                     int32_t cap, int32_t* n_hyp) {
  PF_TRY
  NEED(n_hyp);
  *n_hyp = host_ctc_beam(blank_lp, blank_stride, ids, val, n, T, K, blank, W, N, out_ids, out_len, out_score, cap);
  return PF_OK;
  PF_CATCH
}

int pf_host_hotword_graph(const int32_t* ids, const int32_t* lens, int32_t n_hotwords, int32_t V, int32_t* n_states, int32_t* n_cols,
                          int32_t* tok_col, int32_t* table, int64_t table_cap, int32_t* depth, int32_t depth_cap) {
  PF_TRY
  NEED(n_states); NEED(n_cols);
  HotwordGraph g;
  build_hotword_graph(ids, lens, n_hotwords, V, g);
  *n_states = g.S;
  *n_cols = g.A;
  PF_CHECK(!table || table_cap >= (int64_t)g.table.size(), PF_ERR_CAPACITY, "hotword_graph: table_cap < n_states * n_cols");
  PF_CHECK(!depth || depth_cap >= g.S, PF_ERR_CAPACITY, "hotword_graph: depth_cap < n_states");
  if (tok_col) std::copy(g.tok_col.begin(), g.tok_col.end(), tok_col);
  if (table) std::copy(g.table.begin(), g.table.end(), table);
  if (depth) std::copy(g.depth.begin(), g.depth.end(), depth);
  return PF_OK;
  PF_CATCH
}

int pf_engine_set_ctc_hotwords(pf_engine* h, const int32_t* ids, const int32_t* lens, int32_t n_hotwords, float boost) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->set_ctc_hotwords(ids, lens, n_hotwords, boost);
  return PF_OK;
  PF_CATCH
}

int pf_fetch_ctc_beam_hot(pf_engine* h, int32_t* matched, double* loglik_sum) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->fetch_ctc_beam_hot(matched, loglik_sum);
  return PF_OK;
  PF_CATCH
}

int pf_host_ctc_beam_hot(const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val, const int32_t* n, int32_t T,
                         int32_t K, int32_t blank, int32_t W, int32_t N, int64_t* out_ids, int32_t* out_len, double* out_score,
                         int32_t cap, int32_t* n_hyp, const int32_t* hw_ids, const int32_t* hw_lens, int32_t n_hotwords, float boost,
                         int32_t* out_matched, double* out_loglik) {
  PF_TRY
  NEED(n_hyp);
  *n_hyp = host_ctc_beam_hot(blank_lp, blank_stride, ids, val, n, T, K, blank, W, N, hw_ids, hw_lens, n_hotwords, boost, out_ids,
                             out_len, out_score, out_matched, out_loglik, cap);
  return PF_OK;
  PF_CATCH
}

int pf_host_lm_build(int32_t order, const int64_t* n_ngrams, const int32_t* ids, const float* logp, const float* backoff, int32_t V,
                     int32_t bos, int32_t eos, int32_t unk, float oov, const int32_t* transparent, int32_t n_transparent, pf_lm** lm) {
  PF_TRY
  NEED(lm);
  *lm = nullptr;
  std::shared_ptr<const LmImage> p = lm_build(order, n_ngrams, ids, logp, backoff, V, bos, eos, unk, oov, transparent, n_transparent);
  *lm = new pf_lm{std::move(p)};
  return PF_OK;
  PF_CATCH
}

int pf_host_lm_from_arpa(const char* path, const char* const* tokens, int32_t n_tokens, float oov, int64_t* n_dropped, pf_lm** lm) {
  PF_TRY
  NEED(lm); NEED(path);
  *lm = nullptr;
  std::shared_ptr<const LmImage> p = lm_from_arpa(path, tokens, n_tokens, oov, n_dropped);
  *lm = new pf_lm{std::move(p)};
  return PF_OK;
  PF_CATCH
}

int pf_host_lm_info(const pf_lm* lm, int32_t* order, int64_t* n_states, int64_t* n_arcs, int64_t* image_bytes) {
  PF_TRY
  NEED(lm);
  if (order) *order = lm->p->order;
  if (n_states) *n_states = lm->p->states;
  if (n_arcs) *n_arcs = lm->p->arcs;
  if (image_bytes) *image_bytes = (int64_t)lm->p->bytes();
  return PF_OK;
  PF_CATCH
}

int pf_host_lm_score(const pf_lm* lm, const int32_t* ids, int32_t n, float alpha, float beta, int32_t flags, double* g, int32_t* state,
                     double* g_pos, int32_t* state_pos) {
  PF_TRY
  NEED(lm);
  lm_score(*lm->p, ids, n, alpha, beta, flags, g, state, g_pos, state_pos);
  return PF_OK;
  PF_CATCH
}

void pf_lm_free(pf_lm* lm) { delete lm; }

int pf_engine_set_ctc_lm(pf_engine* h, const pf_lm* lm, float alpha, float beta, int32_t flags) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->set_ctc_lm(lm ? lm->p : nullptr, alpha, beta, flags);
  return PF_OK;
  PF_CATCH
}

int pf_fetch_ctc_beam_lm(pf_engine* h, double* lm_sum, double* loglik_sum) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->fetch_ctc_beam_lm(lm_sum, loglik_sum);
  return PF_OK;
  PF_CATCH
}

int pf_host_ctc_beam_lm(const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val, const int32_t* n, int32_t T,
                        int32_t K, int32_t blank, int32_t W, int32_t N, int64_t* out_ids, int32_t* out_len, double* out_score,
                        int32_t cap, int32_t* n_hyp, const int32_t* hw_ids, const int32_t* hw_lens, int32_t n_hotwords, float boost,
                        int32_t* out_matched, double* out_loglik, const pf_lm* lm, float alpha, float beta, int32_t flags, double* out_lm) {
  PF_TRY
  NEED(n_hyp); NEED(lm);
  *n_hyp = host_ctc_beam_lm(blank_lp, blank_stride, ids, val, n, T, K, blank, W, N, hw_ids, hw_lens, n_hotwords, boost, out_ids, out_len,
                            out_score, out_matched, out_loglik, cap, *lm->p, alpha, beta, flags, out_lm);
  return PF_OK;
  PF_CATCH
}

int pf_engine_set_nbest_search(pf_engine* h, int32_t W, int32_t N) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->set_nbest_search(W, N);
  return PF_OK;
  PF_CATCH
}

int pf_engine_set_nbest_lm(pf_engine* h, const pf_lm* lm, float alpha, float beta, int32_t flags) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->set_nbest_lm(lm ? lm->p : nullptr, alpha, beta, flags);
  return PF_OK;
  PF_CATCH
}

int pf_engine_set_nbest_hotwords(pf_engine* h, const int32_t* ids, const int32_t* lens, int32_t n_hotwords, float boost) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->set_nbest_hotwords(ids, lens, n_hotwords, boost);
  return PF_OK;
  PF_CATCH
}

int pf_fetch_nbest_search(pf_engine* h, int32_t* ranks, double* score, double* loglik_sum, double* lm_sum, int32_t* matched,
                          int32_t* n_hyp, int32_t* L_out, int32_t* N_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->fetch_nbest_search(ranks, score, loglik_sum, lm_sum, matched, n_hyp, L_out, N_out);
  return PF_OK;
  PF_CATCH
}

int pf_host_nbest_search(const int64_t* ids, const float* val, const int32_t* n, int32_t L, int32_t K, int32_t token_num, int32_t W,
                         int32_t N, const int32_t* hw_ids, const int32_t* hw_lens, int32_t n_hotwords, float boost, const pf_lm* lm,
                         float alpha, float beta, int32_t flags, int32_t* out_ranks, double* out_score, double* out_loglik,
                         double* out_lm, int32_t* out_matched, int32_t* n_hyp) {
  PF_TRY
  NEED(n_hyp);
  *n_hyp = host_nbest_search(ids, val, n, L, K, token_num, W, N, hw_ids, hw_lens, n_hotwords, boost, lm ? lm->p.get() : nullptr, alpha, beta,
                             flags, out_ranks, out_score, out_loglik, out_lm, out_matched);
  return PF_OK;
  PF_CATCH
}

int pf_engine_set_align_targets(pf_engine* h, const int64_t* ids, const int32_t* len, int32_t B, int32_t cap) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->set_align_targets(ids, len, B, cap);
  return PF_OK;
  PF_CATCH
}

int pf_fetch_align(pf_engine* h, float* path_score, double* loglik, int32_t* ok, int32_t* len, int32_t* first, int32_t* last,
                   float* tok_score, int32_t cap, int32_t* H, int32_t* len_max) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->fetch_align(path_score, loglik, ok, len, first, last, tok_score, cap, H, len_max);
  return PF_OK;
  PF_CATCH
}

int pf_host_ctc_align(const float* lp, int64_t ld, int32_t T, int32_t V, const int64_t* y, int32_t U, float* path_score,
                      double* loglik, int32_t* ok, int32_t* first, int32_t* last, float* tok_score) {
  PF_TRY
  NEED(ok);
  *ok = host_ctc_align(lp, ld, T, V, y, U, path_score, loglik, first, last, tok_score);
  return PF_OK;
  PF_CATCH
}

int pf_profile_enable(pf_engine* h, int32_t on) {
  PF_TRY
  E(h)->profile_enable(on != 0);
  return PF_OK;
  PF_CATCH
}
int pf_profile_reset(pf_engine* h) {
  PF_TRY
  E(h)->profile_reset();
  return PF_OK;
  PF_CATCH
}
int pf_profile_select(pf_engine* h, const char* cls) {
  PF_TRY
  E(h)->profile_select(cls ? cls : "");
  return PF_OK;
  PF_CATCH
}
int pf_profile_get(pf_engine* h, const char* cls, double* ms, int64_t* launches, double* fpl) {
  PF_TRY
  NEED(cls);
  if (!E(h)->profile_get(cls, ms, launches, fpl)) {
    if (ms) *ms = 0;
    if (launches) *launches = 0;
    if (fpl) *fpl = 0;
  }
  return PF_OK;
  PF_CATCH
}
int pf_profile_kernel(pf_engine* h, const char* cls, char* name_out, int32_t cap) {
  PF_TRY
  NEED(cls); NEED(name_out);
  PF_CHECK(cap > 0, PF_ERR_INVALID_ARG, "pf_profile_kernel: cap <= 0");
  const std::string k = E(h)->profile_kernel(cls);
  PF_CHECK((int)k.size() < cap, PF_ERR_CAPACITY, "pf_profile_kernel: name needs " + std::to_string(k.size() + 1) + " bytes");
  std::memcpy(name_out, k.c_str(), k.size() + 1);
  return PF_OK;
  PF_CATCH
}
int pf_last_flops(pf_engine* h, double* f) {
  PF_TRY
  NEED(f);
  *f = E(h)->last_flops();
  return PF_OK;
  PF_CATCH
}

// ---- multi-device group ---------------------------------------------------
int pf_group_create(const pf_engine_config* cfg, const int32_t* devices, int32_t n_devices, pf_group** out) {
  PF_TRY
  NEED(cfg); NEED(out); NEED(devices);
  PF_CHECK(cfg->struct_size == (int32_t)sizeof(pf_engine_config), PF_ERR_INVALID_ARG, "pf_engine_config.struct_size mismatch");
  *out = nullptr;
  std::shared_ptr<Group> g = std::make_shared<Group>(*cfg, devices, n_devices);
  pf_group* h = new pf_group();
  h->g = g;
  for (int i = 0; i < g->size(); ++i) {
    h->views.emplace_back(new pf_engine());
    h->views.back()->e = g->engine(i);
  }
  *out = h;
  return PF_OK;
  PF_CATCH
}

void pf_group_destroy(pf_group* h) {
  if (!h) return;
  std::shared_ptr<Group> g;
  {
    std::lock_guard<std::mutex> lk(h->mu);
    g.swap(h->g);
    for (auto& v : h->views) { std::lock_guard<std::mutex> lk2(v->mu); v->e.reset(); }
  }
  if (!g) return;
  try {
    { std::lock_guard<std::mutex> lk(g->mutex()); }
    g.reset();
  } catch (...) {}
}

static std::shared_ptr<Group> GR(pf_group* h) {
  PF_CHECK(h != nullptr, PF_ERR_INVALID_ARG, "null group");
  std::lock_guard<std::mutex> lk(h->mu);
  PF_CHECK(h->g != nullptr, PF_ERR_DISPOSED, "OfflineRecognizer");
  return h->g;
}

int pf_group_info(pf_group* h, int32_t* n_engines, int32_t* uses_rccl) {
  PF_TRY
  std::shared_ptr<Group> g = GR(h);
  if (n_engines) *n_engines = g->size();
  if (uses_rccl) *uses_rccl = g->uses_rccl() ? 1 : 0;
  return PF_OK;
  PF_CATCH
}

pf_engine* pf_group_engine(pf_group* h, int32_t i) {
  if (!h) return nullptr;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->g || i < 0 || i >= (int32_t)h->views.size()) return nullptr;
  return h->views[(size_t)i].get();
}

int pf_group_recognize(pf_group* h, const float* const* samples, const int64_t* n, int32_t B, const int32_t* hotwords,
                       int32_t n_hotwords, pf_batch_out* out) {
  PF_TRY
  std::shared_ptr<Group> g = GR(h);
  NEED(out);
  std::lock_guard<std::mutex> lk(g->mutex());
  g->recognize(samples, n, B, hotwords, n_hotwords, want_logits(out));
  g->fetch(out);
  return PF_OK;
  PF_CATCH
}

// ---- pf_host_group_sim: the shard runner of pf_group with arithmetic stand-ins for the devices (shards_sim.h) ----
int pf_host_group_sim(int32_t G, int32_t B, const int32_t* fire_count, int32_t has_cif, int32_t fixed_L, int32_t collective,
                      int32_t fail_shard, int32_t fail_stage, int64_t* ids_out, int32_t l_cap, int32_t* token_num_out,
                      int32_t* L_out) {
  PF_TRY
  PF_CHECK(G > 0 && G <= 64 && B >= 0 && (B == 0 || fire_count), PF_ERR_INVALID_ARG, "pf_host_group_sim: bad arguments");
  pf::SimBackend be(G);
  be.B = B; be.has_cif = has_cif; be.fixed_L = fixed_L; be.collective = collective; be.fail_shard = fail_shard;
  be.fail_stage = fail_stage; be.fire = fire_count;
  pf::ShardRunner runner(G);
  pf::HostBatchOut m;
  runner.recognize(be, B, /*Tg=*/1, has_cif != 0, /*V=*/1, false, m);
  if (L_out) *L_out = m.L;
  if (ids_out) {
    PF_CHECK(l_cap >= m.L, PF_ERR_CAPACITY, "pf_host_group_sim: l_cap < L");
    for (int b = 0; b < B; ++b) std::memcpy(ids_out + (size_t)b * l_cap, m.ids.data() + (size_t)b * m.L, (size_t)m.L * 8);
  }
  if (token_num_out && B > 0) std::memcpy(token_num_out, m.token_num.data(), (size_t)B * 4);
  return PF_OK;
  PF_CATCH
}

int pf_group_fetch(pf_group* h, pf_batch_out* out) {
  PF_TRY
  std::shared_ptr<Group> g = GR(h);
  std::lock_guard<std::mutex> lk(g->mutex());
  g->fetch(out);
  return PF_OK;
  PF_CATCH
}

// ---- stand-alone ops -------------------------------------------------------
int pf_op_lfr_cmvn_pad(pf_engine* h, const float* const* fbank, const int32_t* t80, int32_t B, int32_t sentinel,
                       float* out, int64_t cap, int32_t* tmax) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(fbank); NEED(t80);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_lfr_cmvn_pad(fbank, t80, B, sentinel, out, cap, tmax);
  return PF_OK;
  PF_CATCH
}
int pf_op_fbank_batch(pf_engine* h, const float* const* samples, const int64_t* n, int32_t B, float* out, int64_t cap,
                      int32_t* t80) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  PF_CHECK(B >= 0, PF_ERR_INVALID_ARG, "negative batch");
  if (B > 0) { NEED(samples); NEED(n); NEED(t80); }
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_fbank_batch(samples, n, B, out, cap, t80);
  return PF_OK;
  PF_CATCH
}
int pf_op_argmax(pf_engine* h, const float* x, int64_t rows, int32_t V, int64_t* ids) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(x); NEED(ids);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_argmax(x, rows, V, ids);
  return PF_OK;
  PF_CATCH
}
int pf_op_pcm_convert(pf_engine* h, const void* data, int64_t n_values, const pf_pcm_desc* desc, float* out, int64_t cap,
                      int64_t* n_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(desc);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_pcm_convert(data, n_values, *desc, out, cap, n_out);
  return PF_OK;
  PF_CATCH
}

// ---- voice-activity segmentation ----
int pf_vad_default(pf_vad_config* cfg) {
  PF_TRY
  NEED(cfg);
  *cfg = vad_default();
  return PF_OK;
  PF_CATCH
}
int pf_host_vad_levels(const float* rows, int64_t T, int32_t n_mels, int32_t* out) {
  PF_TRY
  PF_CHECK(T >= 0 && n_mels >= 1 && n_mels <= 1024, PF_ERR_INVALID_ARG, "vad_levels: bad shape (n_mels 1 .. 1024)");
  if (T > 0) { NEED(rows); NEED(out); }
  host_vad_levels(rows, T, n_mels, out);
  return PF_OK;
  PF_CATCH
}
int pf_host_vad_segments(const int32_t* levels, int32_t T, int32_t n_mels, int32_t lfr_n, const pf_vad_config* cfg, int32_t* seg,
                         int32_t cap, int32_t* n) {
  PF_TRY
  NEED(n);
  PF_CHECK(T >= 0 && n_mels >= 1 && n_mels <= 1024 && cap >= 0 && lfr_n >= 1, PF_ERR_INVALID_ARG, "vad_segments: bad shape");
  if (T > 0) NEED(levels);
  const pf_vad_config c = vad_check(cfg, lfr_n);
  const std::vector<int32_t> s = host_vad_segments(levels, T, n_mels, c);
  *n = (int32_t)(s.size() / 2);
  PF_CHECK(*n <= cap, PF_ERR_CAPACITY, "vad: capacity " + std::to_string(cap) + " < " + std::to_string(*n) + " segments");
  if (*n > 0) { NEED(seg); std::memcpy(seg, s.data(), s.size() * 4); }
  return PF_OK;
  PF_CATCH
}
int pf_host_long_plan(const int32_t* len, int32_t n, int32_t batch_max, int64_t frame_budget, int32_t* batch, int32_t* row,
                      int32_t* n_batches) {
  PF_TRY
  PF_CHECK(n >= 0, PF_ERR_INVALID_ARG, "long_plan: negative count");
  if (n > 0) { NEED(len); NEED(batch); NEED(row); }
  for (int i = 0; i < n; ++i) PF_CHECK(len[i] >= 0, PF_ERR_INVALID_ARG, "long_plan: negative length");
  const int nb = host_long_plan(len, n, batch_max, frame_budget, batch, row);
  if (n_batches) *n_batches = nb;
  return PF_OK;
  PF_CATCH
}
int pf_vad_segment(pf_engine* h, const float* const* samples, const int64_t* n_samples, int32_t B, const pf_vad_config* cfg,
                   int32_t* seg, int32_t cap, int32_t* n_seg) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  PF_CHECK(B >= 0 && cap >= 0, PF_ERR_INVALID_ARG, "vad_segment: negative batch or capacity");
  if (B > 0) { NEED(samples); NEED(n_samples); NEED(n_seg); if (cap > 0) NEED(seg); }
  std::lock_guard<std::mutex> lk(e->mutex());
  e->vad_segment(samples, n_samples, B, cfg, seg, cap, n_seg);
  return PF_OK;
  PF_CATCH
}
int pf_op_vad_levels(pf_engine* h, const float* rows, int64_t T, int32_t n_mels, int32_t* out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  PF_CHECK(T >= 0 && n_mels >= 1 && n_mels <= 1024, PF_ERR_INVALID_ARG, "vad_levels: bad shape (n_mels 1 .. 1024)");
  if (T > 0) { NEED(rows); NEED(out); }
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_vad_levels(rows, T, n_mels, out);
  return PF_OK;
  PF_CATCH
}
int pf_op_vad_segments(pf_engine* h, const int32_t* levels, const int32_t* T, int32_t B, int32_t ld, int32_t n_mels,
                       const pf_vad_config* cfg, int32_t* seg, int32_t cap, int32_t* n) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  PF_CHECK(B >= 0 && ld >= 0 && cap >= 0 && n_mels >= 1 && n_mels <= 1024, PF_ERR_INVALID_ARG, "vad_segments: bad shape");
  if (B > 0) { NEED(T); NEED(n); if (ld > 0) NEED(levels); if (cap > 0) NEED(seg); }
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_vad_segments(levels, T, B, ld, n_mels, cfg, seg, cap, n);
  return PF_OK;
  PF_CATCH
}

// ---- voice-activity endpointing, streaming ----
int pf_endpoint_default(pf_endpoint_config* cfg) {
  PF_TRY
  NEED(cfg);
  *cfg = endpoint_default();
  return PF_OK;
  PF_CATCH
}
int pf_host_endpoint_update(int32_t* state, const int32_t* levels, int32_t n_new, int32_t flush, int32_t n_mels, int32_t lfr_n,
                            const pf_endpoint_config* cfg, int32_t* events, int32_t cap, int32_t* n_events, int32_t* in_speech,
                            int32_t* open_begin) {
  PF_TRY
  NEED(state); NEED(n_events);
  PF_CHECK(n_new >= 0 && n_mels >= 1 && n_mels <= 1024 && cap >= 0 && lfr_n >= 1, PF_ERR_INVALID_ARG, "endpoint_update: bad shape");
  if (n_new > 0) NEED(levels);
  if (cap > 0) NEED(events);
  const pf_endpoint_config c = endpoint_check(cfg, lfr_n);
  const std::vector<int32_t> ev = host_endpoint_update(state, levels, n_new, flush, n_mels, c, in_speech, open_begin);
  *n_events = (int32_t)(ev.size() / 3);
  const int k = std::min(*n_events, cap);
  if (k > 0) std::memcpy(events, ev.data(), (size_t)k * 12);
  PF_CHECK(*n_events <= cap, PF_ERR_CAPACITY, "endpoint: capacity " + std::to_string(cap) + " < " + std::to_string(*n_events) + " events");
  return PF_OK;
  PF_CATCH
}
int pf_op_endpoint_update(pf_engine* h, int32_t* states, const int32_t* levels, const int32_t* n_new, const int32_t* flush, int32_t B,
                          int32_t ld, int32_t n_mels, const pf_endpoint_config* cfg, int32_t* events, int32_t cap, int32_t* n_events,
                          int32_t* in_speech, int32_t* open_begin) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  PF_CHECK(B >= 0 && ld >= 0 && cap >= 0 && n_mels >= 1 && n_mels <= 1024, PF_ERR_INVALID_ARG, "endpoint_update: bad shape");
  if (B > 0) { NEED(states); NEED(n_new); NEED(n_events); NEED(in_speech); NEED(open_begin); if (ld > 0) NEED(levels); if (cap > 0) NEED(events); }
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_endpoint_update(states, levels, n_new, flush, B, ld, n_mels, cfg, events, cap, n_events, in_speech, open_begin);
  return PF_OK;
  PF_CATCH
}

// ---- voice-activity segmentation, model score ----
int pf_vad_model_load(const char* path, pf_vad_model** m) {
  return new_model_handle(m, path, "path", [&] { return vad_model_load(path); });
}
int pf_vad_model_from_memory(const void* data, int64_t nbytes, pf_vad_model** m) {
  return new_model_handle(m, data, "data", [&] { return vad_model_from_memory(data, nbytes); });
}
int pf_vad_model_info(const pf_vad_model* m, int32_t* dims, int32_t* n_sil, int64_t* image_bytes) {
  PF_TRY
  NEED(m);
  const VadModel& v = *m->p;
  if (dims) {
    const int32_t d[9] = {v.input_dim, v.affine_dim, v.linear_dim, v.proj_dim, v.output_dim, v.n_layers, v.lorder, v.lstride, v.lfr_m};
    std::memcpy(dims, d, sizeof(d));
  }
  if (n_sil) *n_sil = (int32_t)v.sil_ids.size();
  if (image_bytes) *image_bytes = (int64_t)v.image.size();
  return PF_OK;
  PF_CATCH
}
int pf_vad_model_sil_ids(const pf_vad_model* m, int32_t* sil, int32_t cap, int32_t* n) {
  PF_TRY
  NEED(m); NEED(n);
  *n = (int32_t)m->p->sil_ids.size();
  PF_CHECK(cap >= *n, PF_ERR_CAPACITY, "vad model: capacity below the number of silence ids");
  if (*n > 0) { NEED(sil); std::memcpy(sil, m->p->sil_ids.data(), (size_t)*n * 4); }
  return PF_OK;
  PF_CATCH
}
int pf_vad_model_tensor(const pf_vad_model* m, const char* name, float* out, int64_t cap, int64_t* n) {
  PF_TRY
  NEED(m); NEED(name); NEED(n);
  const std::vector<float>* t = m->p->tensor(name);
  PF_CHECK(t != nullptr, PF_ERR_INVALID_ARG, std::string("vad model: no tensor named '") + name + "'");
  *n = (int64_t)t->size();
  if (!out && cap == 0) return PF_OK;
  PF_CHECK(cap >= *n, PF_ERR_CAPACITY, "vad model: capacity below the tensor's size");
  NEED(out);
  std::memcpy(out, t->data(), t->size() * 4);
  return PF_OK;
  PF_CATCH
}
int pf_vad_model_config(pf_vad_config* cfg) {
  PF_TRY
  NEED(cfg);
  *cfg = vad_model_default();
  return PF_OK;
  PF_CATCH
}
void pf_vad_model_free(pf_vad_model* m) { delete m; }
int pf_host_vad_model_logits(const pf_vad_model* m, const float* rows, int64_t T, int32_t n_mels, double* out) {
  PF_TRY
  NEED(m);
  PF_CHECK(T >= 0 && n_mels >= 1 && n_mels <= 1024, PF_ERR_INVALID_ARG, "vad_model_logits: bad shape (n_mels 1 .. 1024)");
  if (T > 0) { NEED(rows); NEED(out); }
  host_vad_model_logits(*m->p, rows, T, n_mels, out);
  return PF_OK;
  PF_CATCH
}
int pf_host_vad_model_levels(const pf_vad_model* m, const float* rows, int64_t T, int32_t n_mels, int32_t* out) {
  PF_TRY
  NEED(m);
  PF_CHECK(T >= 0 && n_mels >= 1 && n_mels <= 1024, PF_ERR_INVALID_ARG, "vad_model_levels: bad shape (n_mels 1 .. 1024)");
  if (T > 0) { NEED(rows); NEED(out); }
  host_vad_model_levels(*m->p, rows, T, n_mels, out);
  return PF_OK;
  PF_CATCH
}
int pf_engine_set_vad_model(pf_engine* h, const pf_vad_model* m) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->set_vad_model(m ? m->p : nullptr);
  return PF_OK;
  PF_CATCH
}
static int op_vad_model(pf_engine* h, const float* rows, const int32_t* T, int32_t B, int32_t n_mels, float* logits, int32_t* levels) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  PF_CHECK(B >= 0 && n_mels >= 1 && n_mels <= 1024, PF_ERR_INVALID_ARG, "vad_model: bad shape (n_mels 1 .. 1024)");
  if (B > 0) NEED(T);
  int64_t total = 0;
  for (int b = 0; b < B; ++b) total += std::max(T[b], 0);
  if (total > 0) { NEED(rows); PF_CHECK(logits || levels, PF_ERR_INVALID_ARG, "null argument: out"); }
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_vad_model(rows, T, B, n_mels, logits, levels);
  return PF_OK;
  PF_CATCH
}
int pf_op_vad_model_logits(pf_engine* h, const float* rows, const int32_t* T, int32_t B, int32_t n_mels, float* out) {
  return op_vad_model(h, rows, T, B, n_mels, out, nullptr);
}
int pf_op_vad_model_levels(pf_engine* h, const float* rows, const int32_t* T, int32_t B, int32_t n_mels, int32_t* out) {
  return op_vad_model(h, rows, T, B, n_mels, nullptr, out);
}

// ---- voice-activity endpointing, streaming, model score ----
int pf_endpoint_model_config(pf_endpoint_config* cfg) {
  PF_TRY
  NEED(cfg);
  *cfg = endpoint_model_default();
  return PF_OK;
  PF_CATCH
}
int pf_vad_model_stream_state_bytes(const pf_vad_model* m, int64_t* bytes) {
  PF_TRY
  NEED(m); NEED(bytes);
  *bytes = vad_stream_layout(*m->p).bytes;
  return PF_OK;
  PF_CATCH
}
int pf_host_vad_model_stream_state_bytes(const pf_vad_model* m, int64_t* bytes) {
  PF_TRY
  NEED(m); NEED(bytes);
  *bytes = host_vad_stream_state_bytes(*m->p);
  return PF_OK;
  PF_CATCH
}
int pf_host_vad_model_stream(const pf_vad_model* m, void* state, const float* rows, int32_t n_new, int32_t flush, int32_t n_mels,
                             int32_t* levels, double* logits, int32_t cap, int32_t* n_out) {
  PF_TRY
  NEED(m); NEED(state); NEED(n_out);
  PF_CHECK(n_new >= 0 && cap >= 0 && n_mels >= 1 && n_mels <= 1024, PF_ERR_INVALID_ARG, "vad_model_stream: bad shape (n_mels 1 .. 1024)");
  if (n_new > 0) NEED(rows);
  *n_out = (int32_t)host_vad_model_stream(*m->p, state, rows, n_new, flush != 0, n_mels, levels, logits, cap);
  return PF_OK;
  PF_CATCH
}
int pf_op_vad_model_stream(pf_engine* h, void* states, const float* rows, const int32_t* n_new, const int32_t* flush, int32_t B,
                           int32_t ld, int32_t n_mels, int32_t* levels, float* logits, int32_t cap, int32_t* n_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  PF_CHECK(B >= 0 && ld >= 0 && cap >= 0 && n_mels >= 1 && n_mels <= 1024, PF_ERR_INVALID_ARG, "vad_model_stream: bad shape (n_mels 1 .. 1024)");
  if (B > 0) { NEED(states); NEED(n_new); NEED(n_out); if (ld > 0) NEED(rows); }
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_vad_model_stream(states, rows, n_new, flush, B, ld, n_mels, levels, logits, cap, n_out);
  return PF_OK;
  PF_CATCH
}

// ---- speaker labels ----
int pf_spk_model_load(const char* path, pf_spk_model** m) {
  return new_model_handle(m, path, "path", [&] { return spk_model_load(path); });
}
int pf_spk_model_from_memory(const void* data, int64_t nbytes, pf_spk_model** m) {
  return new_model_handle(m, data, "data", [&] { return spk_model_from_memory(data, nbytes); });
}
int pf_spk_model_info(const pf_spk_model* m, int32_t* dims, int64_t* image_bytes) {
  PF_TRY
  NEED(m);
  const SpkModel& v = *m->p;
  if (dims) {
    const int32_t d[16] = {v.n_mels, v.m, v.init, v.growth, v.bn, v.blocks[0], v.blocks[1], v.blocks[2], v.dilations[0], v.dilations[1],
                           v.dilations[2], v.seg_len, v.embedding, v.c_out, Engine::kSpkLaunches, 0};
    std::memcpy(dims, d, sizeof(d));
  }
  if (image_bytes) *image_bytes = (int64_t)v.image.size();
  return PF_OK;
  PF_CATCH
}
void pf_spk_model_free(pf_spk_model* m) { delete m; }
int pf_spk_default(pf_spk_config* cfg) {
  PF_TRY
  NEED(cfg);
  *cfg = spk_default();
  return PF_OK;
  PF_CATCH
}
static pf_spk_config spk_cfg_or_default(const pf_spk_config* cfg) {
  const pf_spk_config c = cfg ? *cfg : spk_default();
  spk_check_config(c);
  return c;
}
int pf_engine_set_spk_model(pf_engine* h, const pf_spk_model* m) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->set_spk_model(m ? m->p : nullptr);
  return PF_OK;
  PF_CATCH
}
int pf_host_spk_windows(const int32_t* seg, int32_t n_seg, const pf_spk_config* cfg, int32_t* win, int32_t cap, int32_t* n,
                        int32_t* shift_used) {
  PF_TRY
  NEED(n);
  PF_CHECK(n_seg >= 0 && cap >= 0, PF_ERR_INVALID_ARG, "spk_windows: negative count");
  if (n_seg > 0) NEED(seg);
  for (int32_t i = 0; i < n_seg; ++i)
    PF_CHECK(seg[2 * i] >= 0 && seg[2 * i + 1] >= seg[2 * i], PF_ERR_INVALID_ARG, "spk_windows: a segment that ends before it begins");
  const pf_spk_config c = spk_cfg_or_default(cfg);
  std::vector<int32_t> w;
  host_spk_windows(seg, n_seg, c, w, shift_used);
  *n = (int32_t)(w.size() / 3);
  PF_CHECK(cap >= *n, PF_ERR_CAPACITY, "spk_windows: capacity below the number of windows");
  if (*n > 0) { NEED(win); std::memcpy(win, w.data(), w.size() * 4); }
  return PF_OK;
  PF_CATCH
}
int pf_host_spk_cluster(const float* S, int32_t N, const pf_spk_config* cfg, int32_t* labels, int32_t* n_speakers) {
  PF_TRY
  PF_CHECK(N >= 0 && N <= PF_SPK_MAX_WINDOWS, PF_ERR_INVALID_ARG, "spk_cluster: N outside 0 .. PF_SPK_MAX_WINDOWS");
  if (N > 0) { NEED(S); NEED(labels); }
  const pf_spk_config c = spk_cfg_or_default(cfg);
  host_spk_cluster(S, N, c, labels, n_speakers);
  return PF_OK;
  PF_CATCH
}
int pf_host_spk_segment_labels(const int32_t* seg, int32_t n_seg, const int32_t* win_seg, const int32_t* win_label, int32_t N,
                               int32_t* out) {
  PF_TRY
  PF_CHECK(n_seg >= 0 && N >= 0, PF_ERR_INVALID_ARG, "spk_segment_labels: negative count");
  if (n_seg > 0) { NEED(seg); NEED(out); }
  if (N > 0) { NEED(win_seg); NEED(win_label); }
  host_spk_segment_labels(seg, n_seg, win_seg, win_label, N, out);
  return PF_OK;
  PF_CATCH
}
int pf_host_spk_centroids(const float* emb, const int32_t* labels, int32_t N, int32_t E_, int32_t K, float* out) {
  PF_TRY
  PF_CHECK(N >= 0 && E_ >= 1 && K >= 0, PF_ERR_INVALID_ARG, "spk_centroids: bad shape");
  if (N > 0) { NEED(emb); NEED(labels); }
  if (K > 0) NEED(out);
  host_spk_centroids(emb, labels, N, E_, K, out);
  return PF_OK;
  PF_CATCH
}
int pf_op_spk_embed(pf_engine* h, const float* rows, const int32_t* T, int32_t B, int32_t n_mels, float* emb, float* frames) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  PF_CHECK(B >= 0 && n_mels >= 1 && n_mels <= 1024, PF_ERR_INVALID_ARG, "spk_embed: bad shape (n_mels 1 .. 1024)");
  if (B > 0) { NEED(T); NEED(emb); }
  int64_t total = 0;
  for (int b = 0; b < B; ++b) total += std::max(T[b], 0);
  if (total > 0) NEED(rows);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_spk_embed(rows, T, B, n_mels, emb, frames);
  return PF_OK;
  PF_CATCH
}
int pf_op_spk_affinity(pf_engine* h, const float* emb, const int32_t* n, int32_t S, int32_t E_, float* out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  PF_CHECK(S >= 0 && E_ >= 1 && E_ <= 4096, PF_ERR_INVALID_ARG, "spk_affinity: bad shape (E 1 .. 4096)");
  if (S > 0) NEED(n);
  int64_t rows = 0;
  for (int s = 0; s < S; ++s) rows += std::max(n[s], 0);
  if (rows > 0) { NEED(emb); NEED(out); }
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_spk_affinity(emb, n, S, E_, out);
  return PF_OK;
  PF_CATCH
}

// ---- punctuation ----
int pf_punc_model_load(const char* path, pf_punc_model** m) {
  return new_model_handle(m, path, "path", [&] { return punc_model_load(path); });
}
int pf_punc_model_from_memory(const void* data, int64_t nbytes, pf_punc_model** m) {
  return new_model_handle(m, data, "data", [&] { return punc_model_from_memory(data, nbytes); });
}
int pf_punc_model_info(const pf_punc_model* m, int32_t* dims, int64_t* image_bytes) {
  PF_TRY
  NEED(m);
  const PuncModel& v = *m->p;
  if (dims) {
    const int32_t d[16] = {v.vocab, v.d_model, v.heads, v.ffn, v.kernel, v.n_layers, v.n_punc, v.sentence_end_id, v.unk_word,
                           v.id_unk, v.id_none, v.id_comma, v.id_period, v.id_question, v.id_pause, 0};
    std::memcpy(dims, d, sizeof(d));
  }
  if (image_bytes) *image_bytes = (int64_t)v.image.size();
  return PF_OK;
  PF_CATCH
}
void pf_punc_model_free(pf_punc_model* m) { delete m; }
int pf_host_punc_words(const pf_punc_model* m, const char* text, int32_t* ids, int32_t* begin, int32_t* end, int32_t cap, int32_t* n) {
  PF_TRY
  NEED(m); NEED(text); NEED(n);
  const std::vector<PuncWord> w = host_punc_words(*m->p, text);
  *n = (int32_t)w.size();
  if (cap == 0 && !ids && !begin && !end) return PF_OK;
  PF_CHECK(cap >= *n, PF_ERR_CAPACITY, "punc_words: capacity below the number of words");
  for (size_t i = 0; i < w.size(); ++i) {
    if (ids) ids[i] = w[i].id;
    if (begin) begin[i] = w[i].begin;
    if (end) end[i] = w[i].end;
  }
  return PF_OK;
  PF_CATCH
}
int pf_host_punc_logits(const pf_punc_model* m, const int32_t* ids, int32_t T, double* out) {
  PF_TRY
  NEED(m);
  PF_CHECK(T >= 0 && T <= PF_PUNC_MAX_WINDOW, PF_ERR_INVALID_ARG, "punc_logits: a window holds 0 .. PF_PUNC_MAX_WINDOW ids");
  if (T > 0) { NEED(ids); NEED(out); }
  host_punc_logits(*m->p, ids, T, out);
  return PF_OK;
  PF_CATCH
}
int pf_host_punc_cut(const pf_punc_model* m, int32_t* p, int32_t n, int32_t last, int32_t* cut) {
  PF_TRY
  NEED(m); NEED(cut);
  PF_CHECK(n >= 0, PF_ERR_INVALID_ARG, "punc_cut: negative length");
  if (n > 0) NEED(p);
  *cut = host_punc_cut(*m->p, p, n, last != 0);
  return PF_OK;
  PF_CATCH
}
int pf_host_punc_ids(const pf_punc_model* m, const int32_t* ids, int64_t n, int32_t* punc_ids, int32_t* win_len, int32_t* win_cut,
                     int32_t win_cap, int32_t* n_win) {
  PF_TRY
  NEED(m);
  PF_CHECK(n >= 0, PF_ERR_INVALID_ARG, "punc_ids: negative length");
  if (n > 0) { NEED(ids); NEED(punc_ids); }
  std::vector<std::pair<int32_t, int32_t>> wins;
  host_punc_ids(*m->p, ids, n, punc_ids, &wins);
  if (n_win) *n_win = (int32_t)wins.size();
  if (win_len || win_cut) {
    PF_CHECK(win_cap >= (int32_t)wins.size(), PF_ERR_CAPACITY, "punc_ids: capacity below the number of windows");
    for (size_t i = 0; i < wins.size(); ++i) {
      if (win_len) win_len[i] = wins[i].first;
      if (win_cut) win_cut[i] = wins[i].second;
    }
  }
  return PF_OK;
  PF_CATCH
}
static int punc_assemble(const PuncModel& m, const std::string& text, const std::vector<PuncWord>& w, const int32_t* punc_ids, char* out,
                         int64_t cap, int64_t* out_len, int32_t* sent_end, int32_t sent_cap, int32_t* n_sent) {
  std::vector<int32_t> se;
  const std::string s = host_punc_assemble(m, text, w, punc_ids, &se);
  if (out_len) *out_len = (int64_t)s.size();
  if (n_sent) *n_sent = (int32_t)se.size();
  if (out || cap > 0) {
    PF_CHECK(cap >= (int64_t)s.size() && (out || s.empty()), PF_ERR_CAPACITY, "punc: capacity below the length of the text");
    if (!s.empty()) std::memcpy(out, s.data(), s.size());
  }
  if (sent_end) {
    PF_CHECK(sent_cap >= (int32_t)se.size(), PF_ERR_CAPACITY, "punc: capacity below the number of sentences");
    if (!se.empty()) std::memcpy(sent_end, se.data(), se.size() * 4);
  }
  return PF_OK;
}
int pf_host_punc_assemble(const pf_punc_model* m, const char* text, const int32_t* punc_ids, int32_t n, char* out, int64_t cap,
                          int64_t* out_len, int32_t* sent_end, int32_t sent_cap, int32_t* n_sent) {
  PF_TRY
  NEED(m); NEED(text);
  const std::string t(text);
  const std::vector<PuncWord> w = host_punc_words(*m->p, t);
  PF_CHECK(n == (int32_t)w.size(), PF_ERR_INVALID_ARG, "punc_assemble: n is not the number of words of the text");
  if (n > 0) NEED(punc_ids);
  return punc_assemble(*m->p, t, w, punc_ids, out, cap, out_len, sent_end, sent_cap, n_sent);
  PF_CATCH
}
int pf_host_punc_text(const pf_punc_model* m, const char* text, char* out, int64_t cap, int64_t* out_len, int32_t* punc_ids,
                      int32_t ids_cap, int32_t* n_words) {
  PF_TRY
  NEED(m); NEED(text);
  const std::string t(text);
  const std::vector<PuncWord> w = host_punc_words(*m->p, t);
  if (n_words) *n_words = (int32_t)w.size();
  std::vector<int32_t> ids(w.size()), p(w.size());
  for (size_t i = 0; i < w.size(); ++i) ids[i] = w[i].id;
  host_punc_ids(*m->p, ids.data(), (int64_t)ids.size(), p.data(), nullptr);
  if (punc_ids) {
    PF_CHECK(ids_cap >= (int32_t)w.size(), PF_ERR_CAPACITY, "punc_text: capacity below the number of words");
    if (!p.empty()) std::memcpy(punc_ids, p.data(), p.size() * 4);
  }
  return punc_assemble(*m->p, t, w, p.data(), out, cap, out_len, nullptr, 0, nullptr);
  PF_CATCH
}
int pf_engine_set_punc_model(pf_engine* h, const pf_punc_model* m) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->set_punc_model(m ? m->p : nullptr);
  return PF_OK;
  PF_CATCH
}
int pf_engine_punctuate(pf_engine* h, const int32_t* ids, const int32_t* lens, int32_t B, int32_t* punc_ids, int32_t* rounds) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  PF_CHECK(B >= 0, PF_ERR_INVALID_ARG, "punctuate: negative B");
  int64_t total = 0;
  if (B > 0) NEED(lens);
  for (int b = 0; b < B; ++b) total += std::max(lens[b], 0);
  if (total > 0) { NEED(ids); NEED(punc_ids); }
  std::lock_guard<std::mutex> lk(e->mutex());
  const int r = e->punctuate(ids, lens, B, punc_ids);
  if (rounds) *rounds = r;
  return PF_OK;
  PF_CATCH
}
int pf_op_punc_logits(pf_engine* h, const int32_t* ids, const int32_t* T, int32_t B, float* logits, float* x0) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  PF_CHECK(B >= 0, PF_ERR_INVALID_ARG, "punc_logits: negative B");
  int64_t total = 0;
  if (B > 0) NEED(T);
  for (int b = 0; b < B; ++b) total += std::max(T[b], 0);
  if (total > 0) { NEED(ids); NEED(logits); }
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_punc(ids, T, nullptr, B, logits, x0, nullptr, nullptr);
  return PF_OK;
  PF_CATCH
}
int pf_op_punc_window(pf_engine* h, const int32_t* ids, const int32_t* T, const int32_t* last, int32_t B, int32_t* p, int32_t* cut,
                      float* logits) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  PF_CHECK(B >= 0, PF_ERR_INVALID_ARG, "punc_window: negative B");
  int64_t total = 0;
  if (B > 0) { NEED(T); NEED(last); NEED(cut); }
  for (int b = 0; b < B; ++b) total += std::max(T[b], 0);
  if (total > 0) { NEED(ids); NEED(p); }
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_punc(ids, T, last, B, logits, nullptr, p, cut);
  return PF_OK;
  PF_CATCH
}

// ---- punctuation, streaming ----
int pf_punc_model_causal(const pf_punc_model* m, int32_t* causal) {
  PF_TRY
  NEED(m); NEED(causal);
  *causal = m->p->causal;
  return PF_OK;
  PF_CATCH
}
int pf_punc_stream_state_bytes(const pf_punc_model* m, int64_t* bytes) {
  PF_TRY
  NEED(m); NEED(bytes);
  PF_CHECK(m->p->causal == 1, PF_ERR_UNSUPPORTED, "punc_stream_state_bytes: the model is not causal");
  *bytes = punc_stream_layout(*m->p).bytes;
  return PF_OK;
  PF_CATCH
}
int pf_host_punc_stream_state_bytes(const pf_punc_model* m, int64_t* bytes) {
  PF_TRY
  NEED(m); NEED(bytes);
  PF_CHECK(m->p->causal == 1, PF_ERR_UNSUPPORTED, "punc_stream_state_bytes: the model is not causal");
  *bytes = host_punc_stream_state_bytes(*m->p);
  return PF_OK;
  PF_CATCH
}
int pf_host_punc_stream_step(const pf_punc_model* m, void* state, const int32_t* ids, int32_t n_new, int32_t flush, int32_t max_context,
                             int32_t flags, int32_t* marks, int32_t* mark_flags, double* logits, int32_t* flush_mark) {
  PF_TRY
  NEED(m); NEED(state);
  if (n_new > 0) { NEED(ids); NEED(marks); NEED(mark_flags); }
  host_punc_stream_step(*m->p, state, ids, n_new, flush != 0, max_context, flags, marks, mark_flags, logits, flush_mark);
  return PF_OK;
  PF_CATCH
}
int pf_op_punc_stream_step(pf_engine* h, void* states, const int32_t* ids, const int32_t* n_new, const int32_t* flush, int32_t B,
                           int32_t ld, int32_t max_context, int32_t flags, int32_t* marks, int32_t* mark_flags, float* logits,
                           int32_t* flush_mark) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  PF_CHECK(B >= 0 && ld >= 0, PF_ERR_INVALID_ARG, "punc_stream_step: negative B or ld");
  if (B > 0) { NEED(states); NEED(n_new); NEED(flush_mark); if (ld > 0) { NEED(ids); NEED(marks); NEED(mark_flags); } }
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_punc_stream_step(states, ids, n_new, flush, B, ld, max_context, flags, marks, mark_flags, logits, flush_mark);
  return PF_OK;
  PF_CATCH
}

int pf_op_topk(pf_engine* h, const float* x, int64_t rows, int32_t V, int32_t ld, int32_t K, int64_t* ids, float* val,
               int32_t* n) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(x); NEED(ids); NEED(val); NEED(n);
  PF_CHECK(rows >= 0 && V > 0 && ld >= V && K >= 1 && K <= PF_TOPK_MAX, PF_ERR_INVALID_ARG, "topk: bad shape");
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_topk(x, rows, V, ld, K, ids, val, n);
  return PF_OK;
  PF_CATCH
}
int pf_op_ctc_beam(pf_engine* h, const float* blank_lp, const int64_t* ids, const float* val, const int32_t* n, const int32_t* lens,
                   int32_t B, int32_t T, int32_t K, int32_t blank, int32_t W, int32_t N, int64_t* out_ids, int32_t* out_len,
                   double* out_score, int32_t cap, int32_t* n_hyp) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(lens); NEED(out_ids); NEED(out_len); NEED(out_score); NEED(n_hyp);
  PF_CHECK(B >= 0 && T >= 0 && cap >= 1 && K >= 1 && K <= PF_TOPK_MAX && N >= 1 && N <= W && W <= PF_NBEST_MAX, PF_ERR_INVALID_ARG,
           "ctc_beam: bad shape (1 <= N <= W <= 64, 1 <= K <= 8, cap >= 1)");
  if ((int64_t)B * T > 0) { NEED(blank_lp); NEED(ids); NEED(val); NEED(n); }
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_ctc_beam(blank_lp, ids, val, n, lens, B, T, K, blank, W, N, out_ids, out_len, out_score, cap, n_hyp);
  return PF_OK;
  PF_CATCH
}

int pf_op_ctc_beam_hot(pf_engine* h, const float* blank_lp, const int64_t* ids, const float* val, const int32_t* n, const int32_t* lens,
                       int32_t B, int32_t T, int32_t K, int32_t blank, int32_t W, int32_t N, int64_t* out_ids, int32_t* out_len,
                       double* out_score, int32_t cap, int32_t* n_hyp, const int32_t* hw_ids, const int32_t* hw_lens,
                       int32_t n_hotwords, float boost, int32_t* out_matched, double* out_loglik) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(lens); NEED(out_ids); NEED(out_len); NEED(out_score); NEED(n_hyp); NEED(out_matched); NEED(out_loglik);
  PF_CHECK(B >= 0 && T >= 0 && cap >= 1 && K >= 1 && K <= PF_TOPK_MAX && N >= 1 && N <= W && W <= PF_NBEST_MAX, PF_ERR_INVALID_ARG,
           "ctc_beam: bad shape (1 <= N <= W <= 64, 1 <= K <= 8, cap >= 1)");
  if ((int64_t)B * T > 0) { NEED(blank_lp); NEED(ids); NEED(val); NEED(n); }
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_ctc_beam_hot(blank_lp, ids, val, n, lens, B, T, K, blank, W, N, hw_ids, hw_lens, n_hotwords, boost, out_ids, out_len, out_score,
                     out_matched, out_loglik, cap, n_hyp);
  return PF_OK;
  PF_CATCH
}

int pf_op_nbest_search(pf_engine* h, const int64_t* ids, const float* val, const int32_t* n, const int32_t* token_num, int32_t B,
                       int32_t L, int32_t K, int32_t W, int32_t N, const int32_t* hw_ids, const int32_t* hw_lens, int32_t n_hotwords,
                       float boost, const pf_lm* lm, float alpha, float beta, int32_t flags, int32_t* out_ranks, double* out_score,
                       double* out_loglik, double* out_lm, int32_t* out_matched, int32_t* n_hyp) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_nbest_search(ids, val, n, token_num, B, L, K, W, N, hw_ids, hw_lens, n_hotwords, boost, lm ? lm->p : nullptr, alpha, beta, flags,
                     out_ranks, out_score, out_loglik, out_lm, out_matched, n_hyp);
  return PF_OK;
  PF_CATCH
}

int pf_op_ctc_beam_lm(pf_engine* h, const float* blank_lp, const int64_t* ids, const float* val, const int32_t* n, const int32_t* lens,
                      int32_t B, int32_t T, int32_t K, int32_t blank, int32_t W, int32_t N, int64_t* out_ids, int32_t* out_len,
                      double* out_score, int32_t cap, int32_t* n_hyp, const int32_t* hw_ids, const int32_t* hw_lens,
                      int32_t n_hotwords, float boost, int32_t* out_matched, double* out_loglik, const pf_lm* lm, float alpha,
                      float beta, int32_t flags, double* out_lm) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(lens); NEED(out_ids); NEED(out_len); NEED(out_score); NEED(n_hyp); NEED(out_matched); NEED(out_loglik); NEED(lm); NEED(out_lm);
  PF_CHECK(B >= 0 && T >= 0 && cap >= 1 && K >= 1 && K <= PF_TOPK_MAX && N >= 1 && N <= W && W <= PF_NBEST_MAX, PF_ERR_INVALID_ARG,
           "ctc_beam: bad shape (1 <= N <= W <= 64, 1 <= K <= 8, cap >= 1)");
  if ((int64_t)B * T > 0) { NEED(blank_lp); NEED(ids); NEED(val); NEED(n); }
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_ctc_beam_lm(blank_lp, ids, val, n, lens, B, T, K, blank, W, N, hw_ids, hw_lens, n_hotwords, boost, out_ids, out_len, out_score,
                    out_matched, out_loglik, cap, n_hyp, lm->p, alpha, beta, flags, out_lm);
  return PF_OK;
  PF_CATCH
}

int pf_op_lm_score(pf_engine* h, const pf_lm* lm, const int32_t* ids, const int32_t* lens, int32_t B, int32_t L, float alpha, float beta,
                   double* g, int32_t* state) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(lm);
  PF_CHECK(B >= 0 && L >= 0, PF_ERR_INVALID_ARG, "lm_score: bad shape");
  if ((int64_t)B * L > 0) { NEED(ids); NEED(lens); NEED(g); NEED(state); }
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_lm_score(lm->p, ids, lens, B, L, alpha, beta, g, state);
  return PF_OK;
  PF_CATCH
}

int pf_op_ctc_align(pf_engine* h, const float* lp, int32_t B, int32_t T, int32_t V, int32_t ld, const int32_t* tgt,
                    const int32_t* tlen, const int32_t* lens, int32_t H, int32_t cap, float* path_score, double* loglik,
                    int32_t* ok, int32_t* first, int32_t* last, float* tok_score) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  PF_CHECK(B >= 0 && B <= 65535 && T >= 0 && H >= 0 && cap >= 1 && V >= 1 && ld >= V, PF_ERR_INVALID_ARG,
           "ctc_align: bad shape (cap >= 1, ld >= V >= 1, B <= 65535)");
  if ((int64_t)B * H > 0) {
    NEED(tgt); NEED(tlen); NEED(lens); NEED(path_score); NEED(loglik); NEED(ok); NEED(first); NEED(last); NEED(tok_score);
    if (T > 0) NEED(lp);
  }
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_ctc_align(lp, B, T, V, ld, tgt, tlen, lens, H, cap, path_score, loglik, ok, first, last, tok_score);
  return PF_OK;
  PF_CATCH
}

int pf_op_ctc_collapse(pf_engine* h, const int64_t* ids, const float* scores, const int32_t* lens, int32_t B, int32_t T,
                       int32_t blank, int64_t* ids_out, int32_t* first_out, int32_t* last_out, float* score_out, int32_t cap,
                       int32_t* n_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(ids); NEED(scores); NEED(lens); NEED(ids_out); NEED(first_out); NEED(last_out); NEED(score_out); NEED(n_out);
  PF_CHECK(B >= 0 && T > 0 && cap > 0, PF_ERR_INVALID_ARG, "ctc_collapse: bad shape");
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_ctc_collapse(ids, scores, lens, B, T, blank, ids_out, first_out, last_out, score_out, cap, n_out);
  return PF_OK;
  PF_CATCH
}
int pf_op_gemm(pf_engine* h, const float* A, const float* W, const float* bias, int32_t M, int32_t N, int32_t K,
               int32_t epi, float* C) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(A); NEED(W); NEED(C);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_gemm(A, W, bias, M, N, K, epi, C);
  return PF_OK;
  PF_CATCH
}
int pf_op_qlinear(pf_engine* h, const float* x, const float* W, const float* bias, int32_t M, int32_t N, int32_t K, int32_t relu,
                  int32_t x_is_f16, float* y, uint8_t* xq_out, float* aparams_out, uint8_t* wq_out, float* wscale_out,
                  int32_t* wzp_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(x); NEED(W); NEED(y);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_qlinear(x, W, bias, M, N, K, relu, x_is_f16, y, xq_out, aparams_out, wq_out, wscale_out, wzp_out);
  return PF_OK;
  PF_CATCH
}
int pf_op_quantize(pf_engine* h, const float* x, int32_t rows, int32_t cols, int32_t ldx, int32_t x_is_f16, int32_t ld, const float* gamma,
                   const float* beta, int8_t* codes_out, int32_t* rowsum_out, float* params_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(x); NEED(codes_out); NEED(rowsum_out); NEED(params_out);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_quantize(x, rows, cols, ldx, x_is_f16, ld, gamma, beta, codes_out, rowsum_out, params_out);
  return PF_OK;
  PF_CATCH
}
int pf_op_quantize_weight(pf_engine* h, const float* W, int32_t N, int32_t K, int32_t ld, int8_t* w_out, int32_t* colsum_out, int32_t* wzp_out,
                          float* wscale_out, int32_t* dz_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(W); NEED(w_out); NEED(colsum_out); NEED(wzp_out); NEED(wscale_out); NEED(dz_out);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_weight(W, nullptr, nullptr, nullptr, N, K, ld, w_out, colsum_out, wzp_out, wscale_out, dz_out);
  return PF_OK;
  PF_CATCH
}
int pf_op_import_weight(pf_engine* h, const uint8_t* Q, const uint8_t* zp, const float* scale, int32_t N, int32_t K, int32_t ld, int8_t* w_out,
                        int32_t* colsum_out, int32_t* wzp_out, float* wscale_out, int32_t* dz_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(Q); NEED(zp); NEED(scale); NEED(w_out); NEED(colsum_out); NEED(wzp_out); NEED(wscale_out); NEED(dz_out);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_weight(nullptr, Q, zp, scale, N, K, ld, w_out, colsum_out, wzp_out, wscale_out, dz_out);
  return PF_OK;
  PF_CATCH
}
int pf_op_qgemm_ex(pf_engine* h, const pf_qgemm_desc* d, const uint8_t* a_codes, const uint8_t* w_codes, float* y32, float* y16, float* range_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(d); NEED(a_codes); NEED(w_codes);
  PF_CHECK(d->struct_size == (int32_t)sizeof(pf_qgemm_desc), PF_ERR_INVALID_ARG, "pf_qgemm_desc.struct_size mismatch");
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_qgemm_ex(*d, a_codes, w_codes, y32, y16, range_out);
  return PF_OK;
  PF_CATCH
}
int pf_op_gemm_ex(pf_engine* h, const pf_gemm_desc* d, const float* A, const float* W, float* C) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(d); NEED(A); NEED(W); NEED(C);
  PF_CHECK(d->struct_size == (int32_t)sizeof(pf_gemm_desc), PF_ERR_INVALID_ARG, "pf_gemm_desc.struct_size mismatch");
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_gemm_ex(*d, A, W, C);
  return PF_OK;
  PF_CATCH
}
int pf_op_gemm_panel(pf_engine* h, int32_t M, int32_t N, int32_t out_kind, int32_t form, int32_t padded, const float* bias, const float* A,
                     const float* W, float* C) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(A); NEED(W); NEED(C);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_gemm_panel(M, N, out_kind, form, padded, bias, A, W, C);
  return PF_OK;
  PF_CATCH
}
int pf_op_gemm_rc(pf_engine* h, const pf_gemm_rc_desc* d, const float* A, const float* W, float* x_out, float* n16_out,
                  float* n32_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(d); NEED(A); NEED(W);
  PF_CHECK(d->struct_size == (int32_t)sizeof(pf_gemm_rc_desc), PF_ERR_INVALID_ARG, "pf_gemm_rc_desc.struct_size mismatch");
  PF_CHECK(x_out || n16_out || n32_out, PF_ERR_INVALID_ARG, "gemm_rc: no output requested");
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_gemm_rc(*d, A, W, x_out, n16_out, n32_out);
  return PF_OK;
  PF_CATCH
}
int pf_op_ffn(pf_engine* h, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
              const float* resid, int32_t M, int32_t D, int32_t F, float* y) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(x); NEED(w1); NEED(b1); NEED(w2); NEED(b2); NEED(resid); NEED(y);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_ffn(x, w1, b1, w2, b2, resid, M, D, F, y);
  return PF_OK;
  PF_CATCH
}
int pf_op_ffn_fused(pf_engine* h, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                    const float* resid, const float* g, const float* be, int32_t M, float* x_out, float* n16_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(x); NEED(w1); NEED(b1); NEED(w2); NEED(b2);
  PF_CHECK(x_out || n16_out, PF_ERR_INVALID_ARG, "ffn_fused: no output requested");
  PF_CHECK((g != nullptr) == (be != nullptr) && (g || !n16_out), PF_ERR_INVALID_ARG, "ffn_fused: the LayerNorm output needs gamma and beta");
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_ffn_fused(x, w1, b1, w2, b2, resid, g, be, M, x_out, n16_out);
  return PF_OK;
  PF_CATCH
}
int pf_op_dec_ffn_fused(pf_engine* h, const pf_dec_ffn_desc* d, float* t_out, float* n_out, float* x_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(d);
  PF_CHECK(d->struct_size == (int32_t)sizeof(pf_dec_ffn_desc), PF_ERR_INVALID_ARG, "pf_dec_ffn_desc.struct_size mismatch");
  PF_CHECK(d->reserved == 0, PF_ERR_INVALID_ARG, "pf_dec_ffn_desc.reserved must be 0");
  NEED(d->w1); NEED(d->b1); NEED(d->gamma_f); NEED(d->beta_f); NEED(d->w2);
  if (d->ctx) { NEED(d->wo); NEED(d->bo); NEED(d->resid); NEED(d->ln1_gamma); NEED(d->ln1_beta); }
  else { NEED(d->x); PF_CHECK(!x_out, PF_ERR_INVALID_ARG, "dec_ffn_fused: x_out needs the out-projection form (ctx)"); }
  PF_CHECK(t_out || n_out, PF_ERR_INVALID_ARG, "dec_ffn_fused: no output requested");
  PF_CHECK((d->ln_gamma != nullptr) == (d->ln_beta != nullptr) && (d->ln_gamma || !n_out), PF_ERR_INVALID_ARG,
           "dec_ffn_fused: the LayerNorm output needs gamma and beta");
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_dec_ffn_fused(*d, t_out, n_out, x_out);
  return PF_OK;
  PF_CATCH
}
int pf_op_dec_mid(pf_engine* h, const pf_dec_mid_desc* d, float* x_out, float* q_out, float* tn_out, float* xn16_out, int32_t* ran) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(d);
  PF_CHECK(d->struct_size == (int32_t)sizeof(pf_dec_mid_desc), PF_ERR_INVALID_ARG, "pf_dec_mid_desc.struct_size mismatch");
  PF_CHECK(d->reserved == 0, PF_ERR_INVALID_ARG, "pf_dec_mid_desc.reserved must be 0");
  NEED(d->a); NEED(d->w1); NEED(d->b1); NEED(d->gamma_f); NEED(d->beta_f); NEED(d->w2); NEED(d->n2_gamma); NEED(d->n2_beta);
  NEED(d->taps); NEED(d->token_num); NEED(d->x); NEED(d->n3_gamma); NEED(d->n3_beta); NEED(d->wq); NEED(d->bq);
  NEED(x_out); NEED(q_out); NEED(ran);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_dec_mid(*d, x_out, q_out, tn_out, xn16_out, ran);
  return PF_OK;
  PF_CATCH
}
int pf_op_fsmn_dec_ln(pf_engine* h, const float* tn, const float* taps, const int32_t* token_num, int32_t B, int32_t L, int32_t k,
                      const float* x, const float* gamma, const float* beta, float* x_out, float* xn16_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(tn); NEED(taps); NEED(token_num); NEED(x); NEED(gamma); NEED(beta); NEED(x_out);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_fsmn_dec_ln(tn, taps, token_num, B, L, k, x, gamma, beta, x_out, xn16_out);
  return PF_OK;
  PF_CATCH
}
int pf_op_layernorm_ex(pf_engine* h, const float* x, const float* gamma, const float* beta, int64_t rows, int32_t D, int32_t ld16, int32_t ld32,
                       int32_t posenc_T, uint16_t* out16, float* out32) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(x); NEED(gamma); NEED(beta);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_layernorm_ex(x, gamma, beta, rows, D, ld16, ld32, posenc_T, out16, out32);
  return PF_OK;
  PF_CATCH
}
int pf_op_layernorm_f16(pf_engine* h, const uint16_t* x, const float* gamma, const float* beta, int64_t rows, int32_t D, int32_t in_place,
                        uint16_t* out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(x); NEED(gamma); NEED(beta); NEED(out);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_layernorm_f16(x, gamma, beta, rows, D, in_place, out);
  return PF_OK;
  PF_CATCH
}
int pf_op_fsmn_dec_stream(pf_engine* h, const float* tn, const float* taps, const int32_t* len, const float* cache_in, int32_t B, int32_t L,
                          int32_t D, int32_t k, const float* x, float* x_out, float* cache_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(tn); NEED(taps); NEED(len); NEED(cache_in); NEED(x); NEED(x_out); NEED(cache_out);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_fsmn_dec_stream(tn, taps, len, cache_in, B, L, D, k, x, x_out, cache_out);
  return PF_OK;
  PF_CATCH
}
int pf_op_fsmn_enc_ex(pf_engine* h, const uint16_t* v16, const float* taps, int32_t B, int32_t T, int32_t D, int32_t k, int32_t ldv,
                      int32_t col, float* y_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(v16); NEED(taps); NEED(y_out);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_fsmn_enc_ex(v16, taps, B, T, D, k, ldv, col, y_out);
  return PF_OK;
  PF_CATCH
}
int pf_op_fsmn_f32_ex(pf_engine* h, const float* v, const float* taps, const float* mask, int32_t B, int32_t T, int32_t D, int32_t k,
                      int32_t ldv, int32_t col, int32_t form, float* y_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(v); NEED(taps); NEED(y_out);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_fsmn_f32_ex(v, taps, mask, B, T, D, k, ldv, col, form, y_out);
  return PF_OK;
  PF_CATCH
}
int pf_op_fsmn_dec_ex(pf_engine* h, const float* tn, const float* taps, const int32_t* token_num, int32_t B, int32_t L, int32_t D,
                      int32_t k, int32_t hostile, const float* x, float* x_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(tn); NEED(taps); NEED(token_num); NEED(x); NEED(x_out);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_fsmn_dec_ex(tn, taps, token_num, B, L, D, k, hostile, x, x_out);
  return PF_OK;
  PF_CATCH
}
int pf_op_embed_gather(pf_engine* h, const float* table, const int32_t* ids, int32_t rows, int32_t D, int32_t vocab, float* out32,
                       uint16_t* out16) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(table); NEED(ids); NEED(out32);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_embed_gather(table, ids, rows, D, vocab, out32, out16);
  return PF_OK;
  PF_CATCH
}
int pf_op_add_to_f16(pf_engine* h, const float* a, const float* b, int64_t rows, int32_t D, uint16_t* out16) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(a); NEED(b); NEED(out16);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_add_to_f16(a, b, rows, D, out16);
  return PF_OK;
  PF_CATCH
}
int pf_op_seaco_merge(pf_engine* h, const float* dha, int32_t ld_dha, const int64_t* dha_ids, int64_t rows, int32_t V, int32_t nobias,
                      int32_t copy_logits, const float* logits_in, int32_t ld_logits, const int64_t* ids_in, float* logits_out,
                      int64_t* ids_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(dha); NEED(dha_ids); NEED(logits_in); NEED(ids_in); NEED(logits_out); NEED(ids_out);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_seaco_merge(dha, ld_dha, dha_ids, rows, V, nobias, copy_logits, logits_in, ld_logits, ids_in, logits_out, ids_out);
  return PF_OK;
  PF_CATCH
}
int pf_op_short_input_max_rows(pf_engine* h, int32_t* rows) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  NEED(rows);
  *rows = eh_->short_input_max_rows();
  return PF_OK;
  PF_CATCH
}
int pf_op_attn_ffn_fused(pf_engine* h, const pf_attn_ffn_desc* d, float* x_out, float* n16_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(d);
  PF_CHECK(d->struct_size == (int32_t)sizeof(pf_attn_ffn_desc), PF_ERR_INVALID_ARG, "pf_attn_ffn_desc.struct_size mismatch");
  NEED(d->ctx); NEED(d->wo); NEED(d->bo); NEED(d->v); NEED(d->fsmn_w); NEED(d->ln2_gamma); NEED(d->ln2_beta);
  NEED(d->w1); NEED(d->b1); NEED(d->w2); NEED(d->b2);
  PF_CHECK(x_out || n16_out, PF_ERR_INVALID_ARG, "attn_ffn_fused: no output requested");
  PF_CHECK((d->ln_gamma != nullptr) == (d->ln_beta != nullptr) && (d->ln_gamma || !n16_out), PF_ERR_INVALID_ARG,
           "attn_ffn_fused: the LayerNorm output needs gamma and beta");
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_ffn_fused(nullptr, d->w1, d->b1, d->w2, d->b2, d->resid, d->ln_gamma, d->ln_beta, d->M, x_out, n16_out, d);
  return PF_OK;
  PF_CATCH
}
int pf_op_fsmn_enc(pf_engine* h, const float* v, const float* w, int32_t B, int32_t T, int32_t D, int32_t k, float* y) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(v); NEED(w); NEED(y);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_fsmn_enc(v, w, B, T, D, k, y);
  return PF_OK;
  PF_CATCH
}
int pf_op_linear32(pf_engine* h, const float* x, const float* W, const float* bias, const float* resid, int32_t M, int32_t N,
                   int32_t K, int32_t relu, float* y) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(x); NEED(W); NEED(y);
  PF_CHECK(M > 0 && N > 0 && K > 0, PF_ERR_INVALID_ARG, "linear32: bad shape");
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_linear32(x, W, bias, resid, M, N, K, relu != 0, y);
  return PF_OK;
  PF_CATCH
}
int pf_op_ffn32(pf_engine* h, const float* x, const float* W1, const float* b1, const float* W2, const float* b2, int32_t M,
                int32_t D, int32_t F, float* y) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(x); NEED(W1); NEED(b1); NEED(W2); NEED(b2); NEED(y);
  PF_CHECK(M > 0 && D > 0 && F > 0, PF_ERR_INVALID_ARG, "ffn32: bad shape");
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_ffn32(x, W1, b1, W2, b2, M, D, F, y);
  return PF_OK;
  PF_CATCH
}
int pf_op_linear32_ex(pf_engine* h, const pf_linear32_desc* d, const float* A, const float* W, float* C) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(d); NEED(A); NEED(W); NEED(C);
  PF_CHECK(d->struct_size == (int32_t)sizeof(pf_linear32_desc), PF_ERR_INVALID_ARG, "linear32_ex: struct_size mismatch");
  PF_CHECK(d->M > 0 && d->N > 0 && d->K > 0, PF_ERR_INVALID_ARG, "linear32_ex: bad shape");
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_linear32_ex(*d, A, W, C);
  return PF_OK;
  PF_CATCH
}
int pf_op_split_x3(pf_engine* h, const float* x, int32_t rows, int32_t K, int32_t ldx, int32_t ldo, int32_t Kp, int32_t swap, uint16_t* out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(x); NEED(out);
  PF_CHECK(rows > 0 && K > 0 && Kp >= K && Kp % 4 == 0 && ldx >= K && ldo >= 2 * Kp && ldo % 4 == 0, PF_ERR_INVALID_ARG, "split_x3: bad shape");
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_split_x3(x, rows, K, ldx, ldo, Kp, swap, out);
  return PF_OK;
  PF_CATCH
}
int pf_op_layernorm32(pf_engine* h, const float* x, const float* gamma, const float* beta, int32_t M, int32_t D, int32_t direct_pair,
                      float* out32, uint16_t* pair, int32_t* wrote_pair, const float* W, const float* bias, int32_t N, float* y) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(x); NEED(gamma); NEED(beta); NEED(out32); NEED(pair); NEED(wrote_pair);
  PF_CHECK(M > 0 && D > 0 && D % 4 == 0 && (!W || (N > 0 && y)), PF_ERR_INVALID_ARG, "layernorm32: bad shape");
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_layernorm32(x, gamma, beta, M, D, direct_pair, out32, pair, wrote_pair, W, bias, N, y);
  return PF_OK;
  PF_CATCH
}
int pf_op_ffn32_ex(pf_engine* h, const float* x, const float* W1, const float* b1, const float* W2, const float* b2, int32_t M,
                   int32_t D, int32_t F, float hidden_scale, float* y, uint16_t* hidden_pair, int32_t* pair_written) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(x); NEED(W1); NEED(b1); NEED(W2); NEED(b2); NEED(y); NEED(hidden_pair); NEED(pair_written);
  PF_CHECK(M > 0 && D > 0 && F > 0, PF_ERR_INVALID_ARG, "ffn32_ex: bad shape");
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_ffn32_ex(x, W1, b1, W2, b2, M, D, F, hidden_scale, y, hidden_pair, pair_written);
  return PF_OK;
  PF_CATCH
}
int pf_op_qkv32(pf_engine* h, const float* x, const float* W, const float* bias, int32_t M, int32_t D, int32_t K, float qscale, float* out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(x); NEED(W); NEED(bias); NEED(out);
  PF_CHECK(M > 0 && D > 0 && K > 0 && D % 4 == 0, PF_ERR_INVALID_ARG, "qkv32: bad shape");
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_qkv32(x, W, bias, M, D, K, qscale, out);
  return PF_OK;
  PF_CATCH
}
int pf_op_fsmn_dec(pf_engine* h, const float* tn, const float* w, const int32_t* token_num, int32_t B, int32_t L,
                   int32_t D, int32_t k, float* x) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(tn); NEED(w); NEED(token_num); NEED(x);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_fsmn_dec(tn, w, token_num, B, L, D, k, x);
  return PF_OK;
  PF_CATCH
}
int pf_op_lstm(pf_engine* h, const float* xg, const float* whh, int32_t B, int32_t T3, int32_t D, int32_t ndir, int32_t form,
               float* hout) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(xg); NEED(whh); NEED(hout);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_lstm(xg, whh, B, T3, D, ndir, form, hout);
  return PF_OK;
  PF_CATCH
}
int pf_op_us_peak(pf_engine* h, const float* hout, const float* w, const float* b0, float smooth, float noise, const int32_t* token_num,
                  float thr, int32_t B, int32_t T3, int32_t W, float* alphas_raw, float* alphas, float* peak) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(hout); NEED(w); NEED(b0); NEED(token_num); NEED(alphas_raw); NEED(alphas); NEED(peak);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_us_peak(hout, w, b0, smooth, noise, token_num, thr, B, T3, W, alphas_raw, alphas, peak);
  return PF_OK;
  PF_CATCH
}
int pf_op_logsoftmax_argmax(pf_engine* h, const float* x, int64_t rows, int32_t V, float* y, int64_t* ids) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(x); NEED(ids);
  PF_CHECK(rows >= 0 && V > 0, PF_ERR_INVALID_ARG, "logsoftmax_argmax: bad shape");
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_logsoftmax_argmax(x, rows, V, y, ids);
  return PF_OK;
  PF_CATCH
}
int pf_op_layernorm(pf_engine* h, const float* x, const float* g, const float* b, int64_t rows, int32_t D, float* y) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(x); NEED(g); NEED(b); NEED(y);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_layernorm(x, g, b, rows, D, y);
  return PF_OK;
  PF_CATCH
}
int pf_op_attention(pf_engine* h, const float* q, const float* k, const float* v, int32_t B, int32_t Lq, int32_t Lk,
                    int32_t heads, float* out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(q); NEED(k); NEED(v); NEED(out);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_attention(q, k, v, B, Lq, Lk, heads, out);
  return PF_OK;
  PF_CATCH
}
int pf_op_attention_ex(pf_engine* h, const float* q, const float* k, const float* v, int32_t B, int32_t Lq, int32_t Lk,
                       int32_t heads, const pf_attn_desc* desc, float* out, void* raw, int64_t raw_bytes, float* range_out,
                       int32_t* ran) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(q); NEED(k); NEED(v); NEED(desc); NEED(out); NEED(raw); NEED(ran);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_attention_ex(q, k, v, B, Lq, Lk, heads, *desc, out, raw, raw_bytes, range_out, ran);
  return PF_OK;
  PF_CATCH
}
int pf_op_qkv_attention(pf_engine* h, const float* x, const float* w, const float* bias, int32_t B, int32_t T, int32_t K,
                        float* q_out, float* k_out, float* v_out, float* ctx_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(x); NEED(w);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_qkv_attention(x, w, bias, B, T, K, q_out, k_out, v_out, ctx_out);
  return PF_OK;
  PF_CATCH
}
int pf_op_fsmn(pf_engine* h, const float* v, const float* w, const float* mask, int32_t B, int32_t T, int32_t D,
               int32_t k, float* y) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(v); NEED(w); NEED(y);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_fsmn(v, w, mask, B, T, D, k, y);
  return PF_OK;
  PF_CATCH
}
int pf_op_cif(pf_engine* h, const float* H, const float* alphas, int32_t B, int32_t T, int32_t D, float thr,
              int32_t Lcap, float* E_, int32_t* fire_count, int32_t* token_num, int32_t* L_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(H); NEED(alphas); NEED(fire_count); NEED(token_num);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_cif(H, alphas, B, T, D, thr, Lcap, E_, fire_count, token_num, L_out);
  return PF_OK;
  PF_CATCH
}
int pf_op_cif_alphas(pf_engine* h, const float* H, int32_t B, int32_t T, float* alphas) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  NEED(H); NEED(alphas);
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_cif_alphas(H, B, T, alphas);
  return PF_OK;
  PF_CATCH
}
int pf_op_encoder(pf_engine* h, const float* speech, int32_t B, int32_t T, float* Hout) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  Engine* e = eh_.get();
  std::lock_guard<std::mutex> lk(e->mutex());
  e->op_encoder(speech, B, T, Hout);
  return PF_OK;
  PF_CATCH
}

// ---- recognizer mirror -------------------------------------------------------
int pf_recognizer_create(const char* model, const char* config, const char* mvn, const char* tokens,
                         const char* modeleb, const char* hotword, int32_t batch_size, int32_t threads_num,
                         int32_t device, pf_recognizer** out) {
  PF_TRY
  NEED(out);
  *out = nullptr;
  auto s = [](const char* p) { return std::string(p ? p : ""); };
  std::shared_ptr<Recognizer> r = std::make_shared<Recognizer>(s(model), s(config), s(mvn), s(tokens), s(modeleb),
                                                               s(hotword), batch_size, threads_num, device);
  pf_recognizer* h = new pf_recognizer();
  h->r = r;
  h->eng.e = r->engine();
  *out = h;
  return PF_OK;
  PF_CATCH
}

void pf_recognizer_dispose(pf_recognizer* h) {
  if (!h) return;
  std::shared_ptr<Recognizer> r;
  {
    std::lock_guard<std::mutex> lk(h->mu);
    r = h->r;
  }
  if (!r) return;
  { std::lock_guard<std::mutex> lk(h->eng.mu); h->eng.e.reset(); }
  try { r->Dispose(); } catch (...) {}
}

void pf_recognizer_free(pf_recognizer* h) {
  if (!h) return;
  pf_recognizer_dispose(h);                         // releases the engine even while streams are still alive
  std::lock_guard<std::mutex> lk(h->mu);
  h->r.reset();                                     // the object itself goes with its last stream
}

pf_engine* pf_recognizer_engine(pf_recognizer* h) {
  if (!h) return nullptr;
  std::lock_guard<std::mutex> lk(h->eng.mu);
  return h->eng.e ? &h->eng : nullptr;
}

static std::shared_ptr<Recognizer> R(pf_recognizer* h);
int pf_recognizer_num_engines(pf_recognizer* h) {
  PF_TRY
  std::shared_ptr<Recognizer> r = R(h);
  PF_CHECK(!r->disposed(), PF_ERR_DISPOSED, "OfflineRecognizer");
  return r->engines_created();
  PF_CATCH
}

static std::shared_ptr<Recognizer> R(pf_recognizer* h) {
  PF_CHECK(h != nullptr, PF_ERR_INVALID_ARG, "null recognizer");
  std::lock_guard<std::mutex> lk(h->mu);
  PF_CHECK(h->r != nullptr, PF_ERR_DISPOSED, "OfflineRecognizer");
  return h->r;
}
static Stream* S(pf_stream* h) {
  PF_CHECK(h != nullptr, PF_ERR_INVALID_ARG, "null stream");
  PF_CHECK(!h->freed && h->s != nullptr, PF_ERR_DISPOSED, "OfflineStream");
  PF_CHECK(!h->s->disposed, PF_ERR_DISPOSED, "OfflineStream");         // ObjectDisposedException
  return h->s.get();
}

int pf_recognizer_create_stream(pf_recognizer* h, pf_stream** out) {
  PF_TRY
  NEED(out);
  *out = nullptr;
  std::shared_ptr<Stream> s = R(h)->CreateOfflineStream();
  pf_stream* sh = stream_shells().get();
  sh->s = s;
  *out = sh;
  return PF_OK;
  PF_CATCH
}

int pf_stream_create(const char* mvn_path, int32_t fs, int32_t n_mels, int32_t lfr_m, int32_t lfr_n, int32_t snip_edges,
                     float dither, const char* window, pf_stream** out) {
  PF_TRY
  NEED(out);
  *out = nullptr;
  ConfEntity c;                                     // FrontendConfEntity defaults where the caller passes 0 / NULL
  if (fs > 0) c.fs = fs;
  if (n_mels > 0) c.n_mels = n_mels;
  if (lfr_m > 0) c.lfr_m = lfr_m;
  if (lfr_n > 0) c.lfr_n = lfr_n;
  c.snip_edges = snip_edges != 0;
  c.dither = dither;
  if (window && window[0]) c.window = window;
  std::shared_ptr<Stream> s = std::make_shared<Stream>(std::string(mvn_path ? mvn_path : ""), c);
  pf_stream* sh = stream_shells().get();
  sh->s = s;
  *out = sh;
  return PF_OK;
  PF_CATCH
}

int pf_stream_add_samples(pf_stream* h, const float* samples, int64_t n) {
  PF_TRY
  Stream* s = S(h);
  PF_CHECK(!s->owner || !s->owner->disposed(), PF_ERR_DISPOSED, "OfflineRecognizer");
  s->AddSamples(samples, n);
  return PF_OK;
  PF_CATCH
}

int pf_stream_add_pcm(pf_stream* h, const void* data, int64_t n_values, const pf_pcm_desc* desc) {
  PF_TRY
  Stream* s = S(h);
  NEED(desc);
  PF_CHECK(!s->owner || !s->owner->disposed(), PF_ERR_DISPOSED, "OfflineRecognizer");
  s->AddPcm(data, n_values, *desc);
  return PF_OK;
  PF_CATCH
}

int pf_stream_set_hotwords(pf_stream* h, const int32_t* ids, const int32_t* lens, int32_t n) {
  PF_TRY
  Stream* s = S(h);
  s->Hotwords.clear();
  s->hotwords_null = n < 0;
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    NEED(lens);
    PF_CHECK(lens[i] >= 0, PF_ERR_INVALID_ARG, "negative hotword length");
    if (lens[i] > 0) NEED(ids);
    s->Hotwords.emplace_back(ids + off, ids + off + lens[i]);
    off += (size_t)lens[i];
  }
  return PF_OK;
  PF_CATCH
}

int pf_stream_get_hotwords(pf_stream* h, int32_t* ids, int32_t ids_cap, int32_t* lens, int32_t lens_cap, int32_t* n) {
  PF_TRY
  Stream* s = S(h);
  NEED(n);
  if (s->hotwords_null) { *n = -1; return PF_OK; }
  *n = (int32_t)s->Hotwords.size();
  size_t tot = 0;
  for (auto& w : s->Hotwords) tot += w.size();
  PF_CHECK((int32_t)s->Hotwords.size() <= lens_cap && (int64_t)tot <= ids_cap, PF_ERR_CAPACITY, "hotword buffers too small");
  size_t off = 0;
  for (size_t i = 0; i < s->Hotwords.size(); ++i) {
    lens[i] = (int32_t)s->Hotwords[i].size();
    for (int32_t v : s->Hotwords[i]) ids[off++] = v;
  }
  return PF_OK;
  PF_CATCH
}

int pf_stream_num_feature_floats(pf_stream* h, int32_t* n) {
  PF_TRY
  NEED(n);
  *n = S(h)->SpeechLength;
  return PF_OK;
  PF_CATCH
}

void pf_stream_dispose(pf_stream* h) {
  // DisposeOfflineStream (OfflineRecognizer.cs:441): the buffers go, the handle stays valid and every later
  // call on it answers PF_ERR_DISPOSED (ObjectDisposedException) until pf_stream_free
  if (!h || h->freed || !h->s) return;
  h->s->Dispose();
}

void pf_stream_free(pf_stream* h) {
  if (!h || h->freed) return;
  if (h->s) h->s->Dispose();
  h->s.reset();                                     // drops this stream's share of the recognizer object
  h->freed = true;                                  // the shell stays (double free / use after free -> PF_ERR_DISPOSED) ...
  stream_shells().retire(h);                        // ... in the quarantine
}

int pf_recognizer_get_results(pf_recognizer* h, pf_stream* const* streams, int32_t n) {
  PF_TRY
  std::shared_ptr<Recognizer> r = R(h);
  std::vector<Stream*> ss;
  for (int i = 0; i < n; ++i) { NEED(streams); ss.push_back(S(streams[i])); }
  r->GetResults(ss);
  return PF_OK;
  PF_CATCH
}

static const ResultEntity& RES(pf_recognizer* h, int32_t i) {
  const std::vector<ResultEntity>& res = R(h)->results_of_this_thread();   // thread-local: outlives this call
  PF_CHECK(i >= 0 && i < (int32_t)res.size(), PF_ERR_INVALID_ARG, "result index out of range");
  return res[(size_t)i];
}

int pf_result_text(pf_recognizer* h, int32_t i, const char** utf8, int32_t* len16) {
  PF_TRY
  const ResultEntity& e = RES(h, i);
  if (utf8) *utf8 = e.Text.c_str();
  if (len16) *len16 = e.TextLen;
  return PF_OK;
  PF_CATCH
}
int pf_result_num_tokens(pf_recognizer* h, int32_t i, int32_t* n) {
  PF_TRY
  NEED(n);
  *n = (int32_t)RES(h, i).Tokens.size();
  return PF_OK;
  PF_CATCH
}
int pf_result_token(pf_recognizer* h, int32_t i, int32_t j, const char** utf8) {
  PF_TRY
  const ResultEntity& e = RES(h, i);
  PF_CHECK(j >= 0 && j < (int32_t)e.Tokens.size(), PF_ERR_INVALID_ARG, "token index out of range");
  NEED(utf8);
  *utf8 = e.Tokens[(size_t)j].c_str();
  return PF_OK;
  PF_CATCH
}
int pf_result_num_timestamps(pf_recognizer* h, int32_t i, int32_t* n) {
  PF_TRY
  NEED(n);
  *n = (int32_t)RES(h, i).Timestamps.size();
  return PF_OK;
  PF_CATCH
}
int pf_result_timestamp(pf_recognizer* h, int32_t i, int32_t j, const int32_t** ints, int32_t* n_ints) {
  PF_TRY
  const ResultEntity& e = RES(h, i);
  PF_CHECK(j >= 0 && j < (int32_t)e.Timestamps.size(), PF_ERR_INVALID_ARG, "timestamp index out of range");
  if (ints) *ints = e.Timestamps[(size_t)j].data();
  if (n_ints) *n_ints = (int32_t)e.Timestamps[(size_t)j].size();
  return PF_OK;
  PF_CATCH
}
int pf_stream_tokens(pf_stream* h, const int64_t** ids, int32_t* n) {
  PF_TRY
  Stream* s = S(h);
  if (ids) *ids = s->Tokens.data();
  if (n) *n = (int32_t)s->Tokens.size();
  return PF_OK;
  PF_CATCH
}

int pf_stream_scores(pf_stream* h, const float** scores, int32_t* n) {
  PF_TRY
  Stream* s = S(h);
  if (scores) *scores = s->Scores.data();
  if (n) *n = (int32_t)s->Scores.size();
  return PF_OK;
  PF_CATCH
}

int pf_recognizer_set_decode(pf_recognizer* h, int32_t flags) {
  PF_TRY
  std::shared_ptr<Recognizer> r = R(h);
  PF_CHECK(!r->disposed(), PF_ERR_DISPOSED, "OfflineRecognizer");
  r->SetDecode(flags);
  return PF_OK;
  PF_CATCH
}

int pf_recognizer_set_nbest(pf_recognizer* h, int32_t N, int32_t K) {
  PF_TRY
  std::shared_ptr<Recognizer> r = R(h);
  PF_CHECK(!r->disposed(), PF_ERR_DISPOSED, "OfflineRecognizer");
  r->SetNBest(N, K);
  return PF_OK;
  PF_CATCH
}

int pf_recognizer_set_ctc_beam(pf_recognizer* h, int32_t N, int32_t W, int32_t K) {
  PF_TRY
  std::shared_ptr<Recognizer> r = R(h);
  PF_CHECK(!r->disposed(), PF_ERR_DISPOSED, "OfflineRecognizer");
  r->SetCtcBeam(N, W, K);
  return PF_OK;
  PF_CATCH
}

int pf_recognizer_set_align(pf_recognizer* h, int32_t on) {
  PF_TRY
  std::shared_ptr<Recognizer> r = R(h);
  PF_CHECK(!r->disposed(), PF_ERR_DISPOSED, "OfflineRecognizer");
  r->SetAlign(on != 0);
  return PF_OK;
  PF_CATCH
}

int pf_recognizer_set_vad(pf_recognizer* h, const pf_vad_config* cfg, int32_t batch_max, int64_t frame_budget, const char* sep_utf8) {
  PF_TRY
  std::shared_ptr<Recognizer> r = R(h);
  PF_CHECK(!r->disposed(), PF_ERR_DISPOSED, "OfflineRecognizer");
  r->SetVad(cfg, batch_max, frame_budget, sep_utf8);
  return PF_OK;
  PF_CATCH
}
int pf_recognizer_set_vad_model(pf_recognizer* h, const char* pfw_path) {
  PF_TRY
  std::shared_ptr<Recognizer> r = R(h);
  PF_CHECK(!r->disposed(), PF_ERR_DISPOSED, "OfflineRecognizer");
  r->SetVadModel(pfw_path ? pfw_path : "");
  return PF_OK;
  PF_CATCH
}
int pf_recognizer_set_punc_model(pf_recognizer* h, const char* pfw_path) {
  PF_TRY
  std::shared_ptr<Recognizer> r = R(h);
  PF_CHECK(!r->disposed(), PF_ERR_DISPOSED, "OfflineRecognizer");
  r->SetPuncModel(pfw_path ? pfw_path : "");
  return PF_OK;
  PF_CATCH
}
int pf_recognizer_set_spk_model(pf_recognizer* h, const char* pfw_path, const pf_spk_config* cfg) {
  PF_TRY
  std::shared_ptr<Recognizer> r = R(h);
  PF_CHECK(!r->disposed(), PF_ERR_DISPOSED, "OfflineRecognizer");
  r->SetSpkModel(pfw_path ? pfw_path : "", cfg);
  return PF_OK;
  PF_CATCH
}
int pf_stream_num_speakers(pf_stream* h, int32_t* n) {
  PF_TRY
  Stream* s = S(h);
  NEED(n);
  *n = (int32_t)s->NumSpeakers;
  return PF_OK;
  PF_CATCH
}
int pf_stream_segment_speaker(pf_stream* h, int32_t i, int32_t* spk) {
  PF_TRY
  Stream* s = S(h);
  NEED(spk);
  PF_CHECK(i >= 0 && (size_t)i < s->SegSpeakers.size(), PF_ERR_INVALID_ARG, "segment index out of range (or no speaker model was on)");
  *spk = s->SegSpeakers[(size_t)i];
  return PF_OK;
  PF_CATCH
}
int pf_stream_speaker_centroid(pf_stream* h, int32_t spk, float* out, int32_t cap, int32_t* E_) {
  PF_TRY
  Stream* s = S(h);
  if (E_) *E_ = (int32_t)s->SpkE;
  if (!out && cap == 0) return PF_OK;
  PF_CHECK(spk >= 0 && spk < s->NumSpeakers, PF_ERR_INVALID_ARG, "speaker index out of range");
  PF_CHECK(cap >= s->SpkE, PF_ERR_CAPACITY, "capacity below the embedding's width");
  NEED(out);
  std::memcpy(out, s->SpkCentroids.data() + (size_t)spk * s->SpkE, (size_t)s->SpkE * 4);
  return PF_OK;
  PF_CATCH
}
int pf_stream_num_spk_windows(pf_stream* h, int32_t* n) {
  PF_TRY
  Stream* s = S(h);
  NEED(n);
  *n = (int32_t)s->SpkWindows.size();
  return PF_OK;
  PF_CATCH
}
int pf_stream_spk_window(pf_stream* h, int32_t i, int32_t* begin_ms, int32_t* end_ms, int32_t* label) {
  PF_TRY
  Stream* s = S(h);
  PF_CHECK(i >= 0 && (size_t)i < s->SpkWindows.size(), PF_ERR_INVALID_ARG, "window index out of range");
  const Stream::SpkWindow& w = s->SpkWindows[(size_t)i];
  if (begin_ms) *begin_ms = w.begin_ms;
  if (end_ms) *end_ms = w.end_ms;
  if (label) *label = w.label;
  return PF_OK;
  PF_CATCH
}
int pf_stream_punctuated(pf_stream* h, const char** text_utf8, const int32_t** punc_ids, int32_t* n_words) {
  PF_TRY
  Stream* s = S(h);
  if (text_utf8) *text_utf8 = s->Punctuated.c_str();
  if (punc_ids) *punc_ids = s->PuncIds.data();
  if (n_words) *n_words = (int32_t)s->PuncIds.size();
  return PF_OK;
  PF_CATCH
}
int pf_stream_num_sentences(pf_stream* h, int32_t* n) {
  PF_TRY
  Stream* s = S(h);
  NEED(n);
  *n = (int32_t)s->Sentences.size();
  return PF_OK;
  PF_CATCH
}
int pf_stream_sentence(pf_stream* h, int32_t i, int32_t* word_begin, int32_t* word_end, int32_t* has_time, int32_t* begin_ms,
                       int32_t* end_ms, const char** text_utf8) {
  PF_TRY
  Stream* s = S(h);
  PF_CHECK(i >= 0 && (size_t)i < s->Sentences.size(), PF_ERR_INVALID_ARG, "sentence index out of range");
  const Stream::Sentence& g = s->Sentences[(size_t)i];
  if (word_begin) *word_begin = g.word_begin;
  if (word_end) *word_end = g.word_end;
  if (has_time) *has_time = g.has_time ? 1 : 0;
  if (begin_ms) *begin_ms = g.begin_ms;
  if (end_ms) *end_ms = g.end_ms;
  if (text_utf8) *text_utf8 = g.text.c_str();
  return PF_OK;
  PF_CATCH
}
int pf_stream_num_segments(pf_stream* h, int32_t* n) {
  PF_TRY
  Stream* s = S(h);
  NEED(n);
  *n = (int32_t)s->Segments.size();
  return PF_OK;
  PF_CATCH
}
int pf_stream_segment(pf_stream* h, int32_t i, int32_t* begin_ms, int32_t* end_ms, int32_t* batch, int32_t* row, int32_t* tok_begin,
                      int32_t* tok_end, const char** text_utf8) {
  PF_TRY
  Stream* s = S(h);
  PF_CHECK(i >= 0 && (size_t)i < s->Segments.size(), PF_ERR_INVALID_ARG, "segment index out of range");
  const Stream::Segment& g = s->Segments[(size_t)i];
  if (begin_ms) *begin_ms = g.begin_ms;
  if (end_ms) *end_ms = g.end_ms;
  if (batch) *batch = g.batch;
  if (row) *row = g.row;
  if (tok_begin) *tok_begin = g.tok_begin;
  if (tok_end) *tok_end = g.tok_end;
  if (text_utf8) *text_utf8 = g.text.c_str();
  return PF_OK;
  PF_CATCH
}

int pf_recognizer_set_hotword_boost(pf_recognizer* h, float boost) {
  PF_TRY
  std::shared_ptr<Recognizer> r = R(h);
  PF_CHECK(!r->disposed(), PF_ERR_DISPOSED, "OfflineRecognizer");
  r->SetHotwordBoost(boost);
  return PF_OK;
  PF_CATCH
}

int pf_stream_alternative_hot(pf_stream* h, int32_t i, int32_t* hotword_tokens, double* loglik_sum) {
  PF_TRY
  Stream* s = S(h);
  PF_CHECK(i >= 0 && i < (int32_t)s->Alternatives.size(), PF_ERR_INVALID_ARG, "alternative index out of range");
  const Alternative& a = s->Alternatives[(size_t)i];
  if (hotword_tokens) *hotword_tokens = a.hot_tokens;
  if (loglik_sum) *loglik_sum = a.loglik_sum;
  return PF_OK;
  PF_CATCH
}

int pf_recognizer_set_lm(pf_recognizer* h, const char* arpa_path, float alpha, float beta, int32_t flags) {
  PF_TRY
  std::shared_ptr<Recognizer> r = R(h);
  PF_CHECK(!r->disposed(), PF_ERR_DISPOSED, "OfflineRecognizer");
  r->SetLm(arpa_path ? arpa_path : "", alpha, beta, flags);
  return PF_OK;
  PF_CATCH
}

int pf_stream_alternative_lm(pf_stream* h, int32_t i, double* lm_sum, double* loglik_sum) {
  PF_TRY
  Stream* s = S(h);
  PF_CHECK(i >= 0 && i < (int32_t)s->Alternatives.size(), PF_ERR_INVALID_ARG, "alternative index out of range");
  const Alternative& a = s->Alternatives[(size_t)i];
  if (lm_sum) *lm_sum = a.lm_sum;
  if (loglik_sum) *loglik_sum = a.loglik_sum;
  return PF_OK;
  PF_CATCH
}

int pf_recognizer_set_nbest_search(pf_recognizer* h, int32_t W) {
  PF_TRY
  std::shared_ptr<Recognizer> r = R(h);
  PF_CHECK(!r->disposed(), PF_ERR_DISPOSED, "OfflineRecognizer");
  r->SetNBestSearch(W);
  return PF_OK;
  PF_CATCH
}

int pf_recognizer_set_nbest_lm(pf_recognizer* h, const char* arpa_path, float alpha, float beta, int32_t flags) {
  PF_TRY
  std::shared_ptr<Recognizer> r = R(h);
  PF_CHECK(!r->disposed(), PF_ERR_DISPOSED, "OfflineRecognizer");
  r->SetNBestLm(arpa_path ? arpa_path : "", alpha, beta, flags);
  return PF_OK;
  PF_CATCH
}

int pf_recognizer_set_nbest_hotword_boost(pf_recognizer* h, float boost) {
  PF_TRY
  std::shared_ptr<Recognizer> r = R(h);
  PF_CHECK(!r->disposed(), PF_ERR_DISPOSED, "OfflineRecognizer");
  r->SetNBestHotwordBoost(boost);
  return PF_OK;
  PF_CATCH
}

int pf_stream_set_align_ids(pf_stream* h, const int64_t* ids, int32_t n) {
  PF_TRY
  Stream* s = S(h);
  if (n < 0) { s->AlignIds.clear(); s->has_align = false; return PF_OK; }
  if (n > 0) NEED(ids);
  PF_CHECK(n <= PF_ALIGN_MAX_TOKENS, PF_ERR_CAPACITY, "a target of more than PF_ALIGN_MAX_TOKENS ids");
  const int64_t V = s->owner ? (int64_t)s->owner->tokens().size() : INT64_MAX;
  for (int i = 0; i < n; ++i) PF_CHECK(ids[i] >= 1 && ids[i] < V, PF_ERR_INVALID_ARG, "a target id outside [1, V)");
  s->AlignIds.assign(ids, ids + n);
  s->has_align = true;
  return PF_OK;
  PF_CATCH
}

int pf_stream_alignment(pf_stream* h, const int32_t** begin_end, const float** tok_score, int32_t* n, float* path_score,
                        double* loglik, int32_t* ok) {
  PF_TRY
  Stream* s = S(h);
  if (begin_end) *begin_end = s->AlignTs.data();
  if (tok_score) *tok_score = s->AlignTok.data();
  if (n) *n = s->AlignN;
  if (path_score) *path_score = s->AlignPath;
  if (loglik) *loglik = s->AlignLoglik;
  if (ok) *ok = s->AlignOk;
  return PF_OK;
  PF_CATCH
}

int pf_stream_alternative_timestamps(pf_stream* h, int32_t i, const int32_t** begin_end, int32_t* n, double* loglik) {
  PF_TRY
  Stream* s = S(h);
  PF_CHECK(i >= 0 && i < (int32_t)s->Alternatives.size(), PF_ERR_INVALID_ARG, "alternative index out of range");
  const Alternative& a = s->Alternatives[(size_t)i];
  if (begin_end) *begin_end = a.ts.data();
  if (n) *n = (int32_t)(a.ts.size() / 2);
  if (loglik) *loglik = a.loglik;
  return PF_OK;
  PF_CATCH
}

int pf_stream_token_alternatives(pf_stream* h, const int64_t** ids, const float** val, int32_t* n_tokens, int32_t* K) {
  PF_TRY
  Stream* s = S(h);
  if (ids) *ids = s->AltIds.data();
  if (val) *val = s->AltVal.data();
  if (n_tokens) *n_tokens = s->AltK > 0 ? (int32_t)(s->AltIds.size() / (size_t)s->AltK) : 0;
  if (K) *K = s->AltK;
  return PF_OK;
  PF_CATCH
}

int pf_stream_num_alternatives(pf_stream* h, int32_t* n) {
  PF_TRY
  Stream* s = S(h);
  NEED(n);
  *n = (int32_t)s->Alternatives.size();
  return PF_OK;
  PF_CATCH
}

int pf_stream_alternative(pf_stream* h, int32_t i, const int64_t** ids, int32_t* n_ids, double* score, const char** text_utf8,
                          int32_t* n_tokens) {
  PF_TRY
  Stream* s = S(h);
  PF_CHECK(i >= 0 && i < (int32_t)s->Alternatives.size(), PF_ERR_INVALID_ARG, "alternative index out of range");
  const Alternative& a = s->Alternatives[(size_t)i];
  if (ids) *ids = a.ids.data();
  if (n_ids) *n_ids = (int32_t)a.ids.size();
  if (score) *score = a.score;
  if (text_utf8) *text_utf8 = a.res.Text.c_str();
  if (n_tokens) *n_tokens = (int32_t)a.res.Tokens.size();
  return PF_OK;
  PF_CATCH
}

int pf_stream_alternative_token(pf_stream* h, int32_t i, int32_t j, const char** utf8) {
  PF_TRY
  Stream* s = S(h);
  NEED(utf8);
  PF_CHECK(i >= 0 && i < (int32_t)s->Alternatives.size(), PF_ERR_INVALID_ARG, "alternative index out of range");
  const Alternative& a = s->Alternatives[(size_t)i];
  PF_CHECK(j >= 0 && j < (int32_t)a.res.Tokens.size(), PF_ERR_INVALID_ARG, "token index out of range");
  *utf8 = a.res.Tokens[(size_t)j].c_str();
  return PF_OK;
  PF_CATCH
}

int pf_stream_set_tokens(pf_stream* h, const int64_t* ids, int32_t n) {
  PF_TRY
  Stream* s = S(h);
  PF_CHECK(n >= 0, PF_ERR_INVALID_ARG, "negative token count");
  if (n > 0) NEED(ids);
  s->Tokens.assign(ids, ids + n);
  return PF_OK;
  PF_CATCH
}
int pf_stream_num_timestamps(pf_stream* h, int32_t* n) {
  PF_TRY
  NEED(n);
  *n = (int32_t)S(h)->Timestamps.size();
  return PF_OK;
  PF_CATCH
}
int pf_stream_timestamp(pf_stream* h, int32_t j, const int32_t** ints, int32_t* n_ints) {
  PF_TRY
  Stream* s = S(h);
  PF_CHECK(j >= 0 && j < (int32_t)s->Timestamps.size(), PF_ERR_INVALID_ARG, "timestamp index out of range");
  if (ints) *ints = s->Timestamps[(size_t)j].data();
  if (n_ints) *n_ints = (int32_t)s->Timestamps[(size_t)j].size();
  return PF_OK;
  PF_CATCH
}
int pf_stream_set_timestamps(pf_stream* h, const int32_t* ints, const int32_t* lens, int32_t n) {
  PF_TRY
  Stream* s = S(h);
  PF_CHECK(n >= 0, PF_ERR_INVALID_ARG, "negative timestamp count");
  TsList ts;
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    NEED(lens);
    PF_CHECK(lens[i] >= 0, PF_ERR_INVALID_ARG, "negative timestamp length");
    if (lens[i] > 0) NEED(ints);
    ts.emplace_back(ints + off, ints + off + lens[i]);
    off += (size_t)lens[i];
  }
  s->Timestamps.swap(ts);
  return PF_OK;
  PF_CATCH
}
int pf_stream_get_speech(pf_stream* h, float* out, int64_t cap, int32_t* n_floats) {
  PF_TRY
  Stream* s = S(h);
  NEED(n_floats);
  if (!s->has_speech) { *n_floats = -1; return PF_OK; }            // OfflineInputEntity.Speech == null
  PF_CHECK(s->owner != nullptr || s->pending.empty(), PF_ERR_UNSUPPORTED,
           "OfflineInputEntity.Speech of a stream no recognizer has adopted yet: its features are computed at the first GetResults");
  if (s->device_form) {
    PF_CHECK(!s->owner->disposed(), PF_ERR_DISPOSED, "OfflineRecognizer");
    s->materialize();                                               // device form -> host form (features read back)
  }
  *n_floats = (int32_t)s->Speech.size();
  PF_CHECK((int64_t)s->Speech.size() <= cap, PF_ERR_CAPACITY, "speech buffer too small");
  if (!s->Speech.empty()) { NEED(out); std::memcpy(out, s->Speech.data(), s->Speech.size() * 4); }
  return PF_OK;
  PF_CATCH
}
int pf_stream_set_speech(pf_stream* h, const float* speech, int32_t n_floats, int32_t speech_length) {
  PF_TRY
  Stream* s = S(h);
  s->drop_device_audio();
  s->pending.clear();
  if (n_floats < 0) {                                               // Speech = null
    std::vector<float>().swap(s->Speech);
    s->has_speech = false;
  } else {
    if (n_floats > 0) NEED(speech);
    s->Speech.assign(speech, speech + n_floats);
    s->has_speech = true;
  }
  s->SpeechLength = speech_length;
  return PF_OK;
  PF_CATCH
}

// ---- streaming path ---------------------------------------------------------
static thread_local std::vector<std::string> t_online_texts;

int pf_online_recognizer_create(const char* enc, const char* dec, const char* config, const char* mvn, const char* tokens,
                                int32_t threads, int32_t device, pf_online_recognizer** out) {
  PF_TRY
  NEED(out);
  *out = nullptr;
  auto s = [](const char* p) { return std::string(p ? p : ""); };
  std::shared_ptr<OnlineRecognizerM> r = std::make_shared<OnlineRecognizerM>(s(enc), s(dec), s(config), s(mvn), s(tokens), threads, device);
  pf_online_recognizer* h = new pf_online_recognizer();
  h->r = r;
  h->eng.e = r->engine();
  *out = h;
  return PF_OK;
  PF_CATCH
}
void pf_online_recognizer_dispose(pf_online_recognizer* h) {
  if (!h) return;
  std::shared_ptr<OnlineRecognizerM> r;
  { std::lock_guard<std::mutex> lk(h->mu); r = h->r; }
  if (!r) return;
  { std::lock_guard<std::mutex> lk(h->eng.mu); h->eng.e.reset(); }
  try { r->Dispose(); } catch (...) {}
}
void pf_online_recognizer_free(pf_online_recognizer* h) {
  if (!h) return;
  pf_online_recognizer_dispose(h);
  std::lock_guard<std::mutex> lk(h->mu);
  h->r.reset();
}
pf_engine* pf_online_recognizer_engine(pf_online_recognizer* h) {
  if (!h) return nullptr;
  std::lock_guard<std::mutex> lk(h->eng.mu);
  return h->eng.e ? &h->eng : nullptr;
}
static std::shared_ptr<OnlineRecognizerM> OR(pf_online_recognizer* h) {
  PF_CHECK(h != nullptr, PF_ERR_INVALID_ARG, "null recognizer");
  std::lock_guard<std::mutex> lk(h->mu);
  PF_CHECK(h->r != nullptr, PF_ERR_DISPOSED, "OnlineRecognizer");
  return h->r;
}
static OnlineStreamM* OS(pf_online_stream* h) {
  PF_CHECK(h != nullptr, PF_ERR_INVALID_ARG, "null stream");
  PF_CHECK(!h->freed && h->s != nullptr && !h->s->disposed, PF_ERR_DISPOSED, "OnlineStream");
  return h->s.get();
}
int pf_online_create_stream(pf_online_recognizer* h, pf_online_stream** out) {
  PF_TRY
  NEED(out);
  *out = nullptr;
  std::shared_ptr<OnlineStreamM> s = OR(h)->CreateOnlineStream();
  pf_online_stream* sh = online_stream_shells().get();
  sh->s = s;
  *out = sh;
  return PF_OK;
  PF_CATCH
}
int pf_online_stream_add_samples(pf_online_stream* h, const float* samples, int64_t n) {
  PF_TRY
  OnlineStreamM* s = OS(h);
  PF_CHECK(!s->owner->disposed(), PF_ERR_DISPOSED, "OnlineRecognizer");
  PF_CHECK(n >= 0, PF_ERR_INVALID_ARG, "negative sample count");
  s->AddSamples(samples, n);
  return PF_OK;
  PF_CATCH
}
int pf_online_get_results(pf_online_recognizer* h, pf_online_stream* const* streams, int32_t n) {
  PF_TRY
  std::shared_ptr<OnlineRecognizerM> r = OR(h);
  std::vector<OnlineStreamM*> ss;
  for (int i = 0; i < n; ++i) { NEED(streams); ss.push_back(OS(streams[i])); }
  t_online_texts = r->GetResults(ss);
  return PF_OK;
  PF_CATCH
}
int pf_online_result_text(pf_online_recognizer* h, int32_t i, const char** utf8) {
  PF_TRY
  OR(h);
  NEED(utf8);
  PF_CHECK(i >= 0 && i < (int32_t)t_online_texts.size(), PF_ERR_INVALID_ARG, "result index out of range");
  *utf8 = t_online_texts[(size_t)i].c_str();
  return PF_OK;
  PF_CATCH
}
int pf_online_stream_tokens(pf_online_stream* h, const int64_t** ids, int32_t* n) {
  PF_TRY
  OnlineStreamM* s = OS(h);
  if (ids) *ids = s->Tokens.data();
  if (n) *n = (int32_t)s->Tokens.size();
  return PF_OK;
  PF_CATCH
}
void pf_online_stream_dispose(pf_online_stream* h) {
  if (!h || h->freed || !h->s) return;
  h->s->disposed = true;
  std::vector<float>().swap(h->s->Speech);
}
int pf_online_recognizer_set_endpoint(pf_online_recognizer* h, const pf_endpoint_config* cfg) {
  PF_TRY
  OR(h)->SetEndpoint(cfg);
  return PF_OK;
  PF_CATCH
}
int pf_online_recognizer_set_endpoint_model(pf_online_recognizer* h, const char* pfw_path) {
  PF_TRY
  OR(h)->SetEndpointModel(pfw_path ? pfw_path : "");
  return PF_OK;
  PF_CATCH
}
int pf_online_recognizer_set_second_pass(pf_online_recognizer* h, pf_recognizer* offline) {
  PF_TRY
  std::shared_ptr<Recognizer> r;
  if (offline) {
    std::lock_guard<std::mutex> lk(offline->mu);
    PF_CHECK(offline->r != nullptr, PF_ERR_DISPOSED, "OfflineRecognizer");
    r = offline->r;
  }
  OR(h)->SetSecondPass(r);
  return PF_OK;
  PF_CATCH
}
int pf_online_stream_input_finished(pf_online_stream* h) {
  PF_TRY
  OnlineStreamM* s = OS(h);
  PF_CHECK(!s->owner->disposed(), PF_ERR_DISPOSED, "OnlineRecognizer");
  s->InputFinished();
  return PF_OK;
  PF_CATCH
}
int pf_online_stream_num_sentences(pf_online_stream* h, int32_t* n) {
  PF_TRY
  OnlineStreamM* s = OS(h);
  NEED(n);
  std::lock_guard<std::mutex> lk(s->mu);
  *n = (int32_t)s->Sentences.size();
  return PF_OK;
  PF_CATCH
}
int pf_online_stream_sentence(pf_online_stream* h, int32_t j, int32_t* begin_ms, int32_t* end_ms, int32_t* kind,
                              const char** first_pass_utf8, const char** text_utf8) {
  PF_TRY
  OnlineStreamM* s = OS(h);
  std::lock_guard<std::mutex> lk(s->mu);
  PF_CHECK(j >= 0 && j < (int32_t)s->Sentences.size(), PF_ERR_INVALID_ARG, "sentence index out of range");
  const OnlineStreamM::SentenceM& sen = s->Sentences[(size_t)j];
  if (begin_ms) *begin_ms = sen.begin_ms;
  if (end_ms) *end_ms = sen.end_ms;
  if (kind) *kind = sen.kind;
  if (first_pass_utf8) *first_pass_utf8 = sen.first_pass.c_str();
  if (text_utf8) *text_utf8 = sen.text.c_str();
  return PF_OK;
  PF_CATCH
}
int pf_online_stream_sentence_result(pf_online_stream* h, int32_t j, pf_stream** offline_stream) {
  PF_TRY
  OnlineStreamM* s = OS(h);
  NEED(offline_stream);
  *offline_stream = nullptr;
  std::lock_guard<std::mutex> lk(s->mu);
  PF_CHECK(j >= 0 && j < (int32_t)s->Sentences.size(), PF_ERR_INVALID_ARG, "sentence index out of range");
  if (!s->Sentences[(size_t)j].offline) return PF_OK;
  if (h->views.size() < s->Sentences.size()) h->views.resize(s->Sentences.size());
  if (!h->views[(size_t)j]) {
    h->views[(size_t)j] = std::make_shared<pf_stream>();
    h->views[(size_t)j]->s = s->Sentences[(size_t)j].offline;
  }
  *offline_stream = h->views[(size_t)j].get();
  return PF_OK;
  PF_CATCH
}
int pf_online_stream_in_speech(pf_online_stream* h, int32_t* in_speech, int32_t* begin_ms) {
  PF_TRY
  OnlineStreamM* s = OS(h);
  std::lock_guard<std::mutex> lk(s->mu);
  if (in_speech) *in_speech = s->InSpeech ? 1 : 0;
  if (begin_ms) *begin_ms = s->OpenBeginMs;
  return PF_OK;
  PF_CATCH
}
int pf_online_recognizer_set_token_info(pf_online_recognizer* h, int32_t on) {
  PF_TRY
  OR(h)->SetTokenInfo(on != 0);
  return PF_OK;
  PF_CATCH
}
int pf_online_stream_token_info(pf_online_stream* h, const pf_online_token** toks, int32_t* n) {
  PF_TRY
  OnlineStreamM* s = OS(h);
  std::lock_guard<std::mutex> lk(s->mu);
  const std::vector<pf_online_token>& t = s->token_info();
  if (toks) *toks = t.data();
  if (n) *n = (int32_t)t.size();
  return PF_OK;
  PF_CATCH
}
int pf_online_stream_sentence_tokens(pf_online_stream* h, int32_t j, const pf_online_token** toks, int32_t* n) {
  PF_TRY
  OnlineStreamM* s = OS(h);
  std::lock_guard<std::mutex> lk(s->mu);
  PF_CHECK(j >= 0 && j < (int32_t)s->Sentences.size(), PF_ERR_INVALID_ARG, "sentence index out of range");
  const std::vector<pf_online_token>& t = s->Sentences[(size_t)j].tokens;
  if (toks) *toks = t.data();
  if (n) *n = (int32_t)t.size();
  return PF_OK;
  PF_CATCH
}
int pf_online_recognizer_set_punc_model(pf_online_recognizer* h, const char* pfw_path, int32_t max_context) {
  PF_TRY
  OR(h)->SetPuncModel(pfw_path ? pfw_path : "", max_context);
  return PF_OK;
  PF_CATCH
}
int pf_online_stream_punctuated(pf_online_stream* h, const char** text_utf8, const int32_t** punc_ids, const int32_t** punc_flags,
                                int32_t* n_words) {
  PF_TRY
  OnlineStreamM* s = OS(h);
  std::lock_guard<std::mutex> lk(s->mu);
  if (text_utf8) *text_utf8 = s->Punctuated.c_str();
  if (punc_ids) *punc_ids = s->PuncIds.data();
  if (punc_flags) *punc_flags = s->PuncFlags.data();
  if (n_words) *n_words = (int32_t)s->PuncIds.size();
  return PF_OK;
  PF_CATCH
}
int pf_online_stream_sentence_punctuated(pf_online_stream* h, int32_t j, const char** text_utf8, const int32_t** punc_ids, int32_t* n_words) {
  PF_TRY
  OnlineStreamM* s = OS(h);
  std::lock_guard<std::mutex> lk(s->mu);
  PF_CHECK(j >= 0 && j < (int32_t)s->Sentences.size(), PF_ERR_INVALID_ARG, "sentence index out of range");
  const OnlineStreamM::SentenceM& sen = s->Sentences[(size_t)j];
  if (text_utf8) *text_utf8 = sen.punctuated.c_str();
  if (punc_ids) *punc_ids = sen.punc_ids.data();
  if (n_words) *n_words = (int32_t)sen.punc_ids.size();
  return PF_OK;
  PF_CATCH
}
void pf_online_stream_free(pf_online_stream* h) {
  if (!h || h->freed) return;
  if (h->s) h->s->disposed = true;
  h->s.reset();
  h->views.clear();
  h->freed = true;
  online_stream_shells().retire(h);
}
int pf_online_encoder(pf_engine* h, const float* speech, int32_t B, int32_t Tc, float* enc_out, float* alphas_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  std::lock_guard<std::mutex> lk(eh_->mutex());
  eh_->online_encoder(speech, B, Tc, enc_out, alphas_out);
  return PF_OK;
  PF_CATCH
}
int pf_online_decoder(pf_engine* h, const float* enc, int32_t B, int32_t Tc, const float* embeds, int32_t L,
                      const int32_t* embeds_len, const float* caches_in, int32_t n_caches, float* logits_out,
                      int64_t* ids_out, float* caches_out) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  std::lock_guard<std::mutex> lk(eh_->mutex());
  PF_CHECK(n_caches == eh_->dec_layers(), PF_ERR_INVALID_ARG, "online_decoder: one cache per decoder layer expected");
  eh_->online_decoder(enc, B, Tc, embeds, L, embeds_len, caches_in, logits_out, ids_out, caches_out);
  return PF_OK;
  PF_CATCH
}
int pf_host_online_cif_state_bytes(int32_t D, int64_t* bytes) {
  PF_TRY
  NEED(bytes);
  PF_CHECK(D > 0 && D % 4 == 0, PF_ERR_INVALID_ARG, "online_cif_state_bytes: D % 4 == 0 expected");
  *bytes = (int64_t)online_cif_state_bytes(D);
  return PF_OK;
  PF_CATCH
}
int pf_host_online_cif_step(void* state, const float* hiddens, const float* alphas, int32_t Tc, int32_t D, float threshold, int32_t lo,
                            int32_t hi, int32_t reset, float* fired, int32_t* fire_entry, int32_t cap, int32_t* count) {
  PF_TRY
  NEED(count);
  *count = online_cif_step(state, hiddens, alphas, Tc, D, threshold, lo, hi, reset != 0, fired, fire_entry, cap);
  return PF_OK;
  PF_CATCH
}
int pf_op_online_cif_step(pf_engine* h, void* states, const float* enc, const float* alphas, const int32_t* reset, int32_t B, int32_t Tc,
                          int32_t D, float threshold, int32_t lo, int32_t hi, float* fired, int32_t* fire_entry, int32_t cap,
                          int32_t* counts) {
  PF_TRY
  std::shared_ptr<Engine> eh_ = E(h);
  std::lock_guard<std::mutex> lk(eh_->mutex());
  eh_->op_online_cif_step(states, enc, alphas, reset, B, Tc, D, threshold, lo, hi, fired, fire_entry, cap, counts);
  return PF_OK;
  PF_CATCH
}
int pf_host_online_lfr(const float* fbank, int32_t t80, int32_t lfr_m, int32_t lfr_n, float* out, int64_t cap, int32_t* t_lfr) {
  PF_TRY
  NEED(t_lfr);
  PF_CHECK(t80 >= 0 && (t80 == 0 || fbank) && lfr_m >= 1 && lfr_n >= 1, PF_ERR_INVALID_ARG, "online_lfr: bad arguments");
  std::vector<float> in(fbank, fbank + (size_t)t80 * 80);
  std::vector<float> o = online_apply_lfr(in, 80, lfr_m, lfr_n);
  *t_lfr = (int32_t)(o.size() / ((size_t)lfr_m * 80));
  if (out) {
    PF_CHECK(cap >= (int64_t)o.size(), PF_ERR_CAPACITY, "online_lfr: output capacity too small");
    if (!o.empty()) std::memcpy(out, o.data(), o.size() * 4);
  }
  return PF_OK;
  PF_CATCH
}
int pf_host_online_posenc(float* x, int32_t timesteps, int32_t dim, int32_t start_idx) {
  PF_TRY
  NEED(x);
  PF_CHECK(timesteps >= 0 && dim >= 4 && dim % 2 == 0 && start_idx >= 0, PF_ERR_INVALID_ARG, "online_posenc: bad arguments");
  std::vector<float> v(x, x + (size_t)timesteps * dim);
  online_position_encode(v, timesteps, dim, start_idx);
  if (!v.empty()) std::memcpy(x, v.data(), v.size() * 4);
  return PF_OK;
  PF_CATCH
}
int pf_host_online_dynamic_mask(float* alphas, int32_t n) {
  PF_TRY
  NEED(alphas);
  PF_CHECK(n >= 0, PF_ERR_INVALID_ARG, "online_dynamic_mask: negative length");
  std::vector<float> v(alphas, alphas + n);
  online_dynamic_mask(v);
  if (!v.empty()) std::memcpy(alphas, v.data(), v.size() * 4);
  return PF_OK;
  PF_CATCH
}
int pf_host_online_cif(const float* hiddens, const float* alphas, int32_t n, int32_t D, float threshold, float* fired,
                       int32_t fired_cap, int32_t* n_fired, float* carry_alpha, float* carry_hidden) {
  PF_TRY
  NEED(n_fired); NEED(carry_alpha); NEED(carry_hidden);
  PF_CHECK(n >= 0 && D > 0 && fired_cap >= 0, PF_ERR_INVALID_ARG, "online_cif: bad sizes");
  if (n > 0) { NEED(hiddens); NEED(alphas); }
  std::vector<std::vector<float>> h;
  for (int i = 0; i < n; ++i) h.emplace_back(hiddens + (size_t)i * D, hiddens + (size_t)(i + 1) * D);
  std::vector<float> a(alphas, alphas + n), ch;
  std::vector<std::vector<float>> f;
  float ca = 0.f;
  online_cif(h, a, threshold, f, ca, ch);
  *n_fired = (int32_t)f.size();
  *carry_alpha = ca;
  std::memset(carry_hidden, 0, (size_t)D * 4);                 // n = 0: nothing was integrated, the carried frame is empty
  if (!ch.empty()) std::memcpy(carry_hidden, ch.data(), std::min(ch.size(), (size_t)D) * 4);
  PF_CHECK((int32_t)f.size() <= fired_cap, PF_ERR_CAPACITY, "online_cif: fired capacity too small");
  for (size_t l = 0; l < f.size(); ++l) { NEED(fired); std::memcpy(fired + l * D, f[l].data(), (size_t)D * 4); }
  return PF_OK;
  PF_CATCH
}
int pf_host_online_decode(const char* const* tokens, int32_t n_tokens, const int64_t* ids, int32_t n_ids, char* out, int32_t cap) {
  PF_TRY
  NEED(out);
  PF_CHECK(n_tokens >= 0 && n_ids >= 0 && cap > 0, PF_ERR_INVALID_ARG, "online_decode: bad sizes");
  if (n_tokens > 0) NEED(tokens);
  if (n_ids > 0) NEED(ids);
  std::vector<std::string> tk;
  for (int i = 0; i < n_tokens; ++i) { PF_CHECK(tokens[i] != nullptr, PF_ERR_INVALID_ARG, "online_decode: null token"); tk.emplace_back(tokens[i]); }
  std::vector<int64_t> idv(ids, ids + n_ids);
  const std::string t = online_decode_text(tk, idv);
  PF_CHECK((int32_t)t.size() + 1 <= cap, PF_ERR_CAPACITY, "online_decode: output capacity too small");
  std::memcpy(out, t.c_str(), t.size() + 1);
  return PF_OK;
  PF_CATCH
}

int pf_host_online_committed_words(const pf_punc_model* m, const char* const* tokens, int32_t n_tokens, const int64_t* ids, int32_t n_ids,
                                   const char* before_utf8, char* out, int64_t cap, int64_t* out_len, int32_t* n_committed, int32_t* n_words) {
  PF_TRY
  NEED(m);
  PF_CHECK(n_tokens >= 0 && n_ids >= 0 && cap >= 0, PF_ERR_INVALID_ARG, "online_committed_words: bad sizes");
  if (n_tokens > 0) NEED(tokens);
  if (n_ids > 0) NEED(ids);
  std::vector<std::string> tk;
  for (int i = 0; i < n_tokens; ++i) { PF_CHECK(tokens[i] != nullptr, PF_ERR_INVALID_ARG, "online_committed_words: null token"); tk.emplace_back(tokens[i]); }
  const OnlineCommitted c = online_committed_words(*m->p, tk, std::vector<int64_t>(ids, ids + n_ids));
  if (before_utf8) {                                             // the last call's committed words, one per line
    std::vector<std::string> before;
    const std::string all(before_utf8);
    for (size_t pos = 0; pos < all.size();) {
      size_t e = all.find('\n', pos);
      if (e == std::string::npos) e = all.size();
      before.push_back(all.substr(pos, e - pos));
      pos = e + 1;
    }
    online_check_committed_prefix(before, c);
  }
  std::string joined;
  for (size_t i = 0; i < c.words.size(); ++i) { if (i) joined += '\n'; joined += online_word(c, i); }
  if (out_len) *out_len = (int64_t)joined.size();
  if (n_committed) *n_committed = (int32_t)c.n_committed;
  if (n_words) *n_words = (int32_t)c.words.size();
  if (out || cap > 0) {
    PF_CHECK(cap >= (int64_t)joined.size() && (out || joined.empty()), PF_ERR_CAPACITY, "online_committed_words: capacity below the length of the words");
    if (!joined.empty()) std::memcpy(out, joined.data(), joined.size());
  }
  return PF_OK;
  PF_CATCH
}

// ---- host text stage --------------------------------------------------------
int pf_host_timestamps(const float* peak, int32_t n, const int64_t* tokens, int32_t n_tokens, int32_t* out_pairs,
                       int32_t cap_pairs) {
  PF_TRY
  NEED(peak);
  std::vector<int64_t> tk;
  if (n_tokens > 0) { NEED(tokens); tk.assign(tokens, tokens + n_tokens); }
  auto ts = time_stamp_lfr6(peak, n, tk);
  PF_CHECK((int32_t)ts.size() <= cap_pairs, PF_ERR_CAPACITY, "timestamp capacity too small");
  for (size_t i = 0; i < ts.size(); ++i) { out_pairs[2 * i] = ts[i][0]; out_pairs[2 * i + 1] = ts[i][1]; }
  return (int)ts.size();
  PF_CATCH
}

int pf_host_hotword_ids(const char* const* tokens, int32_t n_tokens, const char* const* lines, int32_t n_lines,
                        int32_t* ids, int32_t ids_cap, int32_t* lens, int32_t lens_cap, int32_t* n_hotwords) {
  PF_TRY
  NEED(n_hotwords);
  std::vector<std::string> tk, ln;
  for (int i = 0; i < n_tokens; ++i) tk.emplace_back(tokens[i]);
  for (int i = 0; i < n_lines; ++i) ln.emplace_back(lines[i]);
  auto hw = hotword_ids(tk, ln, 1);
  size_t tot = 0;
  for (auto& w : hw) tot += w.size();
  PF_CHECK((int32_t)hw.size() <= lens_cap && (int64_t)tot <= ids_cap, PF_ERR_CAPACITY, "hotword buffers too small");
  size_t off = 0;
  for (size_t i = 0; i < hw.size(); ++i) {
    lens[i] = (int32_t)hw[i].size();
    for (int32_t v : hw[i]) ids[off++] = v;
  }
  *n_hotwords = (int32_t)hw.size();
  return PF_OK;
  PF_CATCH
}

int pf_host_decode(const char* const* tokens, int32_t n_tokens, const int64_t* ids, int32_t n_ids,
                   const int32_t* ts_ints, const int32_t* ts_lens, int32_t n_ts, pf_decoded** out) {
  PF_TRY
  NEED(out);
  *out = nullptr;
  std::vector<std::string> tk;
  for (int i = 0; i < n_tokens; ++i) tk.emplace_back(tokens[i]);
  std::vector<int64_t> idv(ids, ids + n_ids);
  TsList ts;
  size_t off = 0;
  for (int i = 0; i < n_ts; ++i) {
    ts.emplace_back(ts_ints + off, ts_ints + off + ts_lens[i]);
    off += (size_t)ts_lens[i];
  }
  pf_decoded* d = new pf_decoded();
  try {
    // both forms of DecodeMulti — per-token derivations on the fly, and out of the table a recognizer builds once — must agree:
    // this entry is what the golden vectors and the fuzz harness drive, the recognizer itself uses the table
    d->r = decode_multi_one(tk, idv, ts);
    const ResultEntity t = decode_multi_one(TokenTable(tk), idv, ts);
    PF_CHECK(t.Text == d->r.Text && t.TextLen == d->r.TextLen && t.Tokens == d->r.Tokens && t.Timestamps == d->r.Timestamps,
             PF_ERR_RECOGNITION, "DecodeMulti: the table form disagrees with the plain form");
  } catch (...) {
    delete d;
    throw;
  }
  *out = d;
  return PF_OK;
  PF_CATCH
}
int pf_decoded_text(pf_decoded* d, const char** utf8, int32_t* len16) {
  PF_TRY
  NEED(d);
  if (utf8) *utf8 = d->r.Text.c_str();
  if (len16) *len16 = d->r.TextLen;
  return PF_OK;
  PF_CATCH
}
int pf_decoded_num_tokens(pf_decoded* d, int32_t* n) {
  PF_TRY
  NEED(d); NEED(n);
  *n = (int32_t)d->r.Tokens.size();
  return PF_OK;
  PF_CATCH
}
int pf_decoded_token(pf_decoded* d, int32_t j, const char** utf8) {
  PF_TRY
  NEED(d); NEED(utf8);
  PF_CHECK(j >= 0 && j < (int32_t)d->r.Tokens.size(), PF_ERR_INVALID_ARG, "token index out of range");
  *utf8 = d->r.Tokens[(size_t)j].c_str();
  return PF_OK;
  PF_CATCH
}
int pf_decoded_num_timestamps(pf_decoded* d, int32_t* n) {
  PF_TRY
  NEED(d); NEED(n);
  *n = (int32_t)d->r.Timestamps.size();
  return PF_OK;
  PF_CATCH
}
int pf_decoded_timestamp(pf_decoded* d, int32_t j, const int32_t** ints, int32_t* n_ints) {
  PF_TRY
  NEED(d);
  PF_CHECK(j >= 0 && j < (int32_t)d->r.Timestamps.size(), PF_ERR_INVALID_ARG, "timestamp index out of range");
  if (ints) *ints = d->r.Timestamps[(size_t)j].data();
  if (n_ints) *n_ints = (int32_t)d->r.Timestamps[(size_t)j].size();
  return PF_OK;
  PF_CATCH
}
void pf_decoded_free(pf_decoded* d) { delete d; }


int pf_host_wav_read(const char* path, float* out, int64_t cap, int64_t* n_out, int32_t* sample_rate, int32_t* channels,
                     double* duration_ms) {
  PF_TRY
  NEED(path); NEED(n_out);
  double dur = 0;
  int sr = 0, ch = 0;
  std::vector<float> v;
  if (!file_exists(path)) {
    v.assign(1, 0.f);                                   // GetFileSample: new float[1]
  } else {
    WavData w = decode_wav_file(path);
    sr = w.sample_rate; ch = w.channels; dur = w.duration_ms;
    v = w.sample_rate != 16000 ? resample_linear(w.samples, w.sample_rate, 16000, w.channels) : std::move(w.samples);
  }
  *n_out = (int64_t)v.size();
  if (sample_rate) *sample_rate = sr;
  if (channels) *channels = ch;
  if (duration_ms) *duration_ms = dur;
  if (out) {
    PF_CHECK(cap >= (int64_t)v.size(), PF_ERR_CAPACITY, "wav_read: output capacity too small");
    if (!v.empty()) std::memcpy(out, v.data(), v.size() * 4);
  }
  return PF_OK;
  PF_CATCH
}

int pf_host_resample(const float* src, int64_t n, int32_t sr_in, int32_t sr_out, int32_t channels, float* out, int64_t cap,
                     int64_t* n_out) {
  PF_TRY
  NEED(n_out);
  PF_CHECK(n >= 0 && (n == 0 || src), PF_ERR_INVALID_ARG, "resample: bad arguments");
  std::vector<float> in(src, src + n);
  std::vector<float> v = resample_linear(in, sr_in, sr_out, channels);
  *n_out = (int64_t)v.size();
  if (out) {
    PF_CHECK(cap >= (int64_t)v.size(), PF_ERR_CAPACITY, "resample: output capacity too small");
    if (!v.empty()) std::memcpy(out, v.data(), v.size() * 4);
  }
  return PF_OK;
  PF_CATCH
}

int pf_host_wav_info(const char* path, pf_pcm_desc* desc, int64_t* data_offset, int64_t* data_bytes, double* duration_ms) {
  PF_TRY
  NEED(path);
  const WavInfo w = wav_info_file(path);
  if (desc) {
    std::memset(desc, 0, sizeof(*desc));
    desc->struct_size = (int32_t)sizeof(*desc);
    desc->format = w.format; desc->sample_rate = w.sample_rate; desc->channels = w.channels;
  }
  if (data_offset) *data_offset = (int64_t)w.data_offset;
  if (data_bytes) *data_bytes = (int64_t)w.data_bytes;
  if (duration_ms) *duration_ms = w.duration_ms;
  return PF_OK;
  PF_CATCH
}

int pf_host_is_audio(const char* path, int32_t* is_audio) {
  PF_TRY
  NEED(path); NEED(is_audio);
  *is_audio = is_wav_header(path) ? 1 : 0;
  return PF_OK;
  PF_CATCH
}
}  // extern "C"
