// engine.cpp — see engine.h.  Orchestrates the gfx950 kernels into the graph the reference
// obtains from InferenceSession.Run (AliParaformerAsr/OfflineProjOfParaformer.cs:68,
// OfflineProjOfSenseVoiceSmall.cs:156): SAN-M encoder -> CIF predictor -> parallel SAN-M
// decoder -> log-softmax, followed by the reference's own last-index arg-max
// (AliParaformerAsr/OfflineRecognizer.cs:139-152).
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <set>

#include "hostutil.h"
#include "op_stage.h"
#include "pfw.h"

namespace pf {

// live engines' main streams and the streams parked by the hardware-queue probe (Engine::own_hardware_queue below)
static std::mutex g_main_mu;
static std::vector<std::pair<int, hipStream_t>> g_main_streams;      // (device, main stream) of the live engines
static std::vector<hipStream_t> g_parked;

// ------------------------------------------------------------------ construction ----------
Engine::Engine(const pf_engine_config& cfg) {
  device_ = cfg.device;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    throw Error(PF_ERR_DEVICE, "no HIP device available (this library has no CPU fallback)");
  PF_CHECK(device_ >= 0 && device_ < ndev, PF_ERR_DEVICE, "device ordinal out of range");
  PF_HIP(hipSetDevice(device_));
  hipDeviceProp_t prop;
  PF_HIP(hipGetDeviceProperties(&prop, device_));
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
    throw Error(PF_ERR_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
  cus_ = cu_limit(prop.multiProcessorCount);

  fc_.fs = cfg.fs > 0 ? cfg.fs : 16000;
  fc_.n_mels = cfg.n_mels > 0 ? cfg.n_mels : 80;
  fc_.lfr_m = cfg.lfr_m > 0 ? cfg.lfr_m : 7;
  fc_.lfr_n = cfg.lfr_n > 0 ? cfg.lfr_n : 6;
  fc_.snip_edges = cfg.snip_edges != 0;
  fc_.dither = cfg.dither;
  fc_.dither_seed = (uint32_t)cfg.dither_seed;
  fc_.window = cfg.window ? cfg.window : "hamming";
  PF_CHECK(fc_.dither >= 0.f && fc_.dither == fc_.dither, PF_ERR_INVALID_ARG, "dither must be >= 0");
  PF_CHECK(fc_.fs == 16000, PF_ERR_UNSUPPORTED, "only fs = 16000 is supported");
  // the fbank kernel is built for 25 ms / 10 ms frames (400 / 160 samples, 512-point FFT): any other framing in
  // the configuration must be refused, not silently ignored
  PF_CHECK((cfg.frame_length_ms == 0 || cfg.frame_length_ms == 25) && (cfg.frame_shift_ms == 0 || cfg.frame_shift_ms == 10),
           PF_ERR_UNSUPPORTED, "only frame_length = 25 ms and frame_shift = 10 ms are supported");
  PF_CHECK(cfg.math_mode >= 0 && cfg.math_mode <= 3, PF_ERR_INVALID_ARG,
           "math_mode must be 0 (f16 MFMA), 1 (fp32 MFMA), 2 (dynamic int8 as model.int8.onnx, int8 MFMA) or 3 (exact: split-f16 products)");
  fp32_mode_ = cfg.math_mode == 1 || cfg.math_mode == 3;
  x3_mode_ = cfg.math_mode == 3;
  int8_mode_ = cfg.math_mode == 2;
  { const char* e = getenv("PF_QKV_MIN"); if (e && e[0]) qkv_split_min_tiles_ = atoi(e); }
  { const char* e = getenv("PF_QKV_FILL"); if (e && e[0]) qkv_split_min_fill_ = atoi(e); }
  { const char* e = getenv("PF_FFN_MIN"); if (e && e[0]) ffn_fused_min_rows_ = atoi(e); }
  { const char* e = getenv("PF_DEC_MID"); if (e && e[0]) dec_mid_ = e[0] != '0'; }     // the decoder's middle as the launches it replaces (tests compare both forms)
  { const char* e = getenv("PF_GEMM_PANEL"); if (e && e[0]) gemm_panel_ = e[0] != '0'; }   // the panel-resident K = 512 GEMM (tests compare both forms)

  // host-only validation BEFORE anything is uploaded (a bad am.mvn must not cost a 0.9 GB upload per retry)
  std::vector<float> shift, scale;
  if (cfg.mvn_path && cfg.mvn_path[0]) {
    parse_mvn_text(read_text_file(cfg.mvn_path), shift, scale);
  } else if (cfg.cmvn_shift && cfg.cmvn_scale && cfg.cmvn_dim > 0) {
    shift.assign(cfg.cmvn_shift, cfg.cmvn_shift + cfg.cmvn_dim);
    scale.assign(cfg.cmvn_scale, cfg.cmvn_scale + cfg.cmvn_dim);
  }
  if (!shift.empty()) {
    PF_CHECK(shift.size() == scale.size(), PF_ERR_FORMAT, "am.mvn: shift/scale length mismatch");
    PF_CHECK((int)shift.size() == fc_.lfr_m * fc_.n_mels, PF_ERR_FORMAT, "am.mvn: CMVN dim must equal lfr_m * n_mels");
  }

  uid_ = register_uid();
  try {
    PF_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    own_hardware_queue();
    PF_HIP(hipStreamCreateWithFlags(&aux_stream_, hipStreamNonBlocking));
    PF_HIP(hipEventCreateWithFlags(&ev_scan_, hipEventDisableTiming));
    PF_HIP(hipStreamCreateWithFlags(&ts_stream_, hipStreamNonBlocking));
    own_hardware_queue_ts();
    PF_HIP(hipEventCreateWithFlags(&ev_ts_, hipEventDisableTiming));
    PF_HIP(hipEventCreateWithFlags(&ev_enc_, hipEventDisableTiming));
    load_weights(cfg);
    mc_.use_itn = cfg.use_itn != 0 || mc_.use_itn;
    fb_ = fbank_tables_create(fc_.n_mels, fc_.fs, fc_.window.c_str());
    // split partials of the short-input GEMM (k_gemm_small.hip): one per engine = one per stream
    small_ws_ = (float*)dalloc(gemm_small_ws_bytes());
    if (!shift.empty()) {
      cmvn_dim_ = (int)shift.size();
      cmvn_shift_ = (float*)dalloc(sizeof(float) * cmvn_dim_);
      cmvn_scale_ = (float*)dalloc(sizeof(float) * cmvn_dim_);
      PF_HIP(hipMemcpy(cmvn_shift_, shift.data(), sizeof(float) * cmvn_dim_, hipMemcpyHostToDevice));
      PF_HIP(hipMemcpy(cmvn_scale_, scale.data(), sizeof(float) * cmvn_dim_, hipMemcpyHostToDevice));
    }
  } catch (...) {
    release();                                       // ~Engine does not run for a throwing constructor
    throw;
  }
}

Engine::~Engine() { release(); }

void Engine::release() {
  if (uid_) { unregister_uid(uid_); uid_ = 0; }
  hipSetDevice(device_);
  if (stream_) hipStreamSynchronize(stream_);
  if (aux_stream_) { hipStreamSynchronize(aux_stream_); hipStreamDestroy(aux_stream_); aux_stream_ = nullptr; }
  if (plan_host_) { hipHostFree(plan_host_); plan_host_ = nullptr; plan_host_dev_ = nullptr; plan_host_cap_ = 0; }
  if (ev_scan_) { hipEventDestroy(ev_scan_); ev_scan_ = nullptr; }
  if (step_host_) { hipHostFree(step_host_); step_host_ = nullptr; step_host_dev_ = nullptr; step_host_cap_ = 0; }
  if (ev_step_) { hipEventDestroy(ev_step_); ev_step_ = nullptr; }
  if (ts_stream_) { hipStreamSynchronize(ts_stream_); hipStreamDestroy(ts_stream_); ts_stream_ = nullptr; }
  if (ev_ts_) { hipEventDestroy(ev_ts_); ev_ts_ = nullptr; }
  if (ev_enc_) { hipEventDestroy(ev_enc_); ev_enc_ = nullptr; }
  if (lstm_graph_exec_) { hipGraphExecDestroy(lstm_graph_exec_); lstm_graph_exec_ = nullptr; }
  profile_reset();
  if (fb_) { fbank_tables_destroy(fb_); fb_ = nullptr; }
  for (void* p : owned_) hipFree(p);
  owned_.clear();
  DevBuf* bufs[] = {&ws_f32_, &ws_pcm_, &ws_audio_, &ws_meta_, &ws_fbank_, &ws_speech_, &ws_enc_, &ws_dec_, &ws_kv_, &ws_pe_, &ws_tmp_,
                    &ws_ts_, &ws_seaco_, &ws_seaco_in_, &ws_seaco_hw_, &ws_q_, &ws_qf_, &ws_seaco_q_, &ws_x3a_, &ws_x3t_, &ws_x3h_, &lm_inst_.buf, &lm_op_.buf, &nbs_hot_.buf, &ws_nbs_,
                    &ws_step_, &vadnet_dev_.buf, &ws_vadnet_, &punc_dev_.buf, &ws_punc_, &spk_dev_.buf, &ws_spk_};
  lm_inst_.src.reset(); lm_op_.src.reset(); lm_.reset(); nbs_lm_.reset();
  vadnet_dev_.src.reset(); vadnet_.reset();
  punc_dev_.src.reset(); punc_.reset();
  spk_dev_.src.reset(); spk_.reset();
  x3_pair_live_ = false; x3a_src_ = nullptr; x3a_pair_only_ = false;
  x3w_.clear();
  ts_whh_x3_ = nullptr;
  seaco_hw_valid_ = false;
  for (DevBuf* b : bufs)
    if (b->p) { hipFree(b->p); b->p = nullptr; b->bytes = 0; }
  if (blob_owned_ && blob_dev_) hipFree(blob_dev_);
  blob_dev_ = nullptr;
  if (stream_) {
    {
      std::lock_guard<std::mutex> lk(g_main_mu);
      for (size_t i = 0; i < g_main_streams.size(); ++i)
        if (g_main_streams[i].second == stream_) { g_main_streams.erase(g_main_streams.begin() + (long)i); break; }
      if (g_main_streams.empty()) {                           // the last engine of the process: the parked streams go too
        for (hipStream_t s : g_parked) hipStreamDestroy(s);
        g_parked.clear();
      }
    }
    hipStreamDestroy(stream_); stream_ = nullptr;
  }
}

// Engines on one device overlap (the recognizer's pool, bench.py's steps in flight) only if their main streams sit on DIFFERENT
// hardware queues: HIP multiplexes its streams onto GPU_MAX_HW_QUEUES (4) queues, and two streams on one queue run their kernels in
// submission order.  Which queue a new stream gets depends on every stream the process has created and destroyed before — measured
// in round 6: the second pair of engines of a process (bench.py's `exact` twin behind the f16 engines) did not overlap at all (38.6 ms
// per step with two in flight against 35.1 in a fresh process; GPU_MAX_HW_QUEUES=8 brought 34.9 back).  So the constructor PROBES: a
// single wave spins ~150 us on a live engine's main stream while an empty kernel goes to the new stream; if the empty kernel does not
// finish well before the spinning one, the two streams share a queue: the new stream is parked (kept alive, so that the runtime's
// allocator moves on) and another one is tried, up to 8 times.  PF_QUEUE_PROBE=0 switches the probe off.

namespace {
struct ProbeEvents {                                          // (the probe's calls may throw: the events go with the scope)
  hipEvent_t a = nullptr, b = nullptr;
  ProbeEvents() { PF_HIP(hipEventCreate(&a)); if (hipEventCreate(&b) != hipSuccess) { hipEventDestroy(a); throw Error(PF_ERR_DEVICE, "hipEventCreate"); } }
  ~ProbeEvents() { hipEventDestroy(a); hipEventDestroy(b); }
};
// a stream parked by the probe has done its work once the next stream exists: keep the last few, destroy the oldest (a process that
// creates and destroys recognizers beside a long-lived one would otherwise collect them for ever)
void park_stream(hipStream_t s) {
  g_parked.push_back(s);
  if (g_parked.size() > 24) {
    for (int i = 0; i < 8; ++i) hipStreamDestroy(g_parked[(size_t)i]);
    g_parked.erase(g_parked.begin(), g_parked.begin() + 8);
  }
}
}  // namespace

void Engine::own_hardware_queue() {
  static const int on = env_int("PF_QUEUE_PROBE", 1);
  std::lock_guard<std::mutex> lk(g_main_mu);
  if (on) {
    ProbeEvents ev;
    hipEvent_t ea = ev.a, eb = ev.b;
    for (int attempt = 0; attempt < 8; ++attempt) {
      bool clash = false;
      int seen = 0;
      for (auto it = g_main_streams.rbegin(); it != g_main_streams.rend() && seen < 3 && !clash; ++it) {
        if (it->first != device_) continue;
        ++seen;
        launch_spin(it->second, 300000ull);                  // ~150 us at ~2 GHz, one wave: every other CU stays free
        launch_nop(stream_);
        PF_HIP(hipEventRecord(eb, stream_));
        PF_HIP(hipEventRecord(ea, it->second));
        PF_HIP(hipEventSynchronize(ea));
        PF_HIP(hipEventSynchronize(eb));
        float ms = 0.f;
        PF_HIP(hipEventElapsedTime(&ms, eb, ea));            // how long before the spinning kernel's end the empty one was done
        clash = ms < 0.05f;
      }
      if (!clash) {
        if (attempt && getenv("PF_QUEUE_PROBE_VERBOSE")) fprintf(stderr, "pf: engine main stream moved to another hardware queue after %d attempt(s)\n", attempt);
        break;
      }
      park_stream(stream_);                                  // stays alive: the next stream gets another queue
      stream_ = nullptr;
      PF_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    }
  }
  g_main_streams.emplace_back(device_, stream_);
}

// the timestamp head runs BESIDE the decoder on ts_stream_: the same requirement against the engine's own main stream
void Engine::own_hardware_queue_ts() {
  static const int on = env_int("PF_QUEUE_PROBE", 1);
  if (!on || !ts_stream_) return;
  std::lock_guard<std::mutex> lk(g_main_mu);
  ProbeEvents ev;
  hipEvent_t ea = ev.a, eb = ev.b;
  for (int attempt = 0; attempt < 8; ++attempt) {
    launch_spin(stream_, 300000ull);
    launch_nop(ts_stream_);
    PF_HIP(hipEventRecord(eb, ts_stream_));
    PF_HIP(hipEventRecord(ea, stream_));
    PF_HIP(hipEventSynchronize(ea));
    PF_HIP(hipEventSynchronize(eb));
    float ms = 0.f;
    PF_HIP(hipEventElapsedTime(&ms, eb, ea));
    if (ms >= 0.05f) {
      if (attempt && getenv("PF_QUEUE_PROBE_VERBOSE")) fprintf(stderr, "pf: timestamp stream moved to another hardware queue after %d attempt(s)\n", attempt);
      break;
    }
    park_stream(ts_stream_);
    ts_stream_ = nullptr;
    PF_HIP(hipStreamCreateWithFlags(&ts_stream_, hipStreamNonBlocking));
  }
}

// pinned host memory the CIF plan's counts are exported into (PF_PLAN_ZERO_COPY=0: the three device-to-host copies of rounds 1-5)
void Engine::ensure_plan_host(int B) {
  static const int on = env_int("PF_PLAN_ZERO_COPY", 1);
  if (!on || plan_host_cap_ >= B) return;
  if (plan_host_) { hipHostFree(plan_host_); plan_host_ = nullptr; plan_host_dev_ = nullptr; plan_host_cap_ = 0; }
  const int cap = std::max(64, (int)round_up(B, 64));
  void* p = nullptr;
  if (hipHostMalloc(&p, (size_t)(1 + 2 * cap) * 4, hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); return; }
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) { (void)hipGetLastError(); hipHostFree(p); return; }
  plan_host_ = (int32_t*)p; plan_host_dev_ = (int32_t*)d; plan_host_cap_ = cap;
}

// The CIF plan's counts on their way to the host (all three arithmetic modes).  export_plan goes right behind the scan: the counts
// are written into pinned host memory by a kernel and ev_scan_ is recorded; read_back_plan waits for that event alone and fills
// last_.fire_count / last_.token_num.  Without pinned memory (or with PF_PLAN_ZERO_COPY=0): three copies on the side stream.
void Engine::export_plan(int B) {
  ensure_plan_host(B);
  if (plan_host_) launch_export_plan(stream_, plan_.max_count, plan_.fire_count, plan_.token_num, B, plan_host_dev_);
  PF_HIP(hipEventRecord(ev_scan_, stream_));
}

int32_t Engine::read_back_plan(int B) {
  int32_t L = 0;
  last_.fire_count.resize(B);
  last_.token_num.resize(B);
  if (plan_host_) {
    PF_HIP(hipEventSynchronize(ev_scan_));
    L = plan_host_[0];
    std::memcpy(last_.fire_count.data(), plan_host_ + 1, (size_t)B * 4);
    std::memcpy(last_.token_num.data(), plan_host_ + 1 + B, (size_t)B * 4);
  } else {
    PF_HIP(hipStreamWaitEvent(aux_stream_, ev_scan_, 0));
    PF_HIP(hipMemcpyAsync(&L, plan_.max_count, 4, hipMemcpyDeviceToHost, aux_stream_));
    PF_HIP(hipMemcpyAsync(last_.fire_count.data(), plan_.fire_count, (size_t)B * 4, hipMemcpyDeviceToHost, aux_stream_));
    PF_HIP(hipMemcpyAsync(last_.token_num.data(), plan_.token_num, (size_t)B * 4, hipMemcpyDeviceToHost, aux_stream_));
    PF_HIP(hipStreamSynchronize(aux_stream_));
  }
  return L;
}

void* Engine::dalloc(size_t bytes) {
  void* p = nullptr;
  PF_HIP(hipMalloc(&p, std::max<size_t>(bytes, 256)));
  owned_.push_back(p);
  return p;
}

void Engine::ensure(DevBuf& b, size_t bytes) {
  if (b.bytes >= bytes && b.p) return;
  if (b.p) {
    PF_HIP(hipStreamSynchronize(stream_));
    if (ts_stream_) PF_HIP(hipStreamSynchronize(ts_stream_));   // (a call that threw may have left the timestamp head unjoined)
    PF_HIP(hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
  }
  const size_t want = round_up((int64_t)(bytes + bytes / 8), 1 << 20);
  PF_HIP(hipMalloc(&b.p, want));
  PF_HIP(hipMemsetAsync(b.p, 0, want, stream_));
  b.bytes = want;
}

void Engine::sync() {
  PF_HIP(hipStreamSynchronize(stream_));
  check_async_errors();
}

void Engine::check_async_errors() {
  if (!lstm_err_) return;                            // the persistent recurrence raises this word when a spin timed out
  unsigned flag = 0;
  unsigned* w = lstm_err_;
  lstm_err_ = nullptr;
  PF_HIP(hipMemcpy(&flag, w, 4, hipMemcpyDeviceToHost));
  PF_CHECK(flag == 0, PF_ERR_DEVICE, "timestamp head: the persistent LSTM timed out waiting for a workgroup");
}

// ------------------------------------------------------------------ weights ---------------
const Engine::Tensor& Engine::tensor(const std::string& name) const {
  auto it = tensors_.find(name);
  if (it == tensors_.end()) throw Error(PF_ERR_FORMAT, "weights: missing tensor '" + name + "'");
  if (it->second.u8) throw Error(PF_ERR_FORMAT, "weights: tensor '" + name + "' must be f32");
  return it->second;
}

const Engine::Tensor* Engine::tensor_u8(const std::string& name) const {
  auto it = tensors_.find(name);
  if (it == tensors_.end()) return nullptr;
  if (!it->second.u8) throw Error(PF_ERR_FORMAT, "weights: tensor '" + name + "' must be u8");
  return &it->second;
}

void Engine::load_weights(const pf_engine_config& cfg) {
  std::vector<char> file;
  const char* host = nullptr;
  int64_t nbytes = 0;
  std::vector<char> head;          // header bytes when the image lives on the device
  const char* dev_image = nullptr;
  if (cfg.weights_path && cfg.weights_path[0]) {
    read_binary_file(cfg.weights_path, file);
    host = file.data();
    nbytes = (int64_t)file.size();
  } else if (cfg.weights_host) {
    host = (const char*)cfg.weights_host;
    nbytes = cfg.weights_bytes;
  } else if (cfg.weights_device) {
    dev_image = (const char*)cfg.weights_device;
    nbytes = cfg.weights_bytes;
    if (nbytes < 16) pfw_bad(kPfwWeights, "image too small");
    head.resize(16);
    PF_HIP(hipMemcpy(head.data(), dev_image, 16, hipMemcpyDeviceToHost));
  } else {
    throw Error(PF_ERR_INVALID_ARG, "weights: no source given (weights_path / weights_host / weights_device)");
  }
  const PfwFrame fr = pfw_frame(host ? host : head.data(), nbytes, kPfwWeights);
  std::string hdr;
  if (host) hdr.assign(host + 16, (size_t)fr.header_len);
  else {
    hdr.resize((size_t)fr.header_len);
    PF_HIP(hipMemcpy(&hdr[0], dev_image + 16, hdr.size(), hipMemcpyDeviceToHost));
  }
  const PfwIndex ix = pfw_index(hdr.data(), fr.header_len, fr.data_bytes, kPfwWeights);
  const Json* jc = &ix.config;
  mc_.kind = jc->str_or("kind", mc_.kind);
  PF_CHECK(mc_.kind != "fsmnvad", PF_ERR_INVALID_ARG,
           "weights: a container of kind \"fsmnvad\" is a voice-activity model (pf_vad_model_load), not a recogniser");
  PF_CHECK(mc_.kind != "cttransformer", PF_ERR_INVALID_ARG,
           "weights: a container of kind \"cttransformer\" is a punctuation model (pf_punc_model_load), not a recogniser");
  PF_CHECK(mc_.kind != "campplus", PF_ERR_INVALID_ARG,
           "weights: a container of kind \"campplus\" is a speaker model (pf_spk_model_load), not a recogniser");
  mc_.feat_dim = (int)jc->int_or("feat_dim", mc_.feat_dim, INT32_MIN, INT32_MAX);
  mc_.d_model = (int)jc->int_or("d_model", mc_.d_model, INT32_MIN, INT32_MAX);
  mc_.heads = (int)jc->int_or("heads", mc_.heads, INT32_MIN, INT32_MAX);
  mc_.ffn = (int)jc->int_or("ffn", mc_.ffn, INT32_MIN, INT32_MAX);
  mc_.enc_layers = (int)jc->int_or("enc_layers", mc_.enc_layers, INT32_MIN, INT32_MAX);
  mc_.tp_layers = (int)jc->int_or("tp_layers", mc_.tp_layers, INT32_MIN, INT32_MAX);
  mc_.kernel = (int)jc->int_or("kernel", mc_.kernel, INT32_MIN, INT32_MAX);
  mc_.dec_layers = (int)jc->int_or("dec_layers", mc_.dec_layers, INT32_MIN, INT32_MAX);
  mc_.vocab = (int)jc->int_or("vocab", mc_.vocab, INT32_MIN, INT32_MAX);
  mc_.cif_threshold = (float)jc->num_or("cif_threshold", mc_.cif_threshold);
  mc_.cif_tail = (float)jc->num_or("cif_tail", mc_.cif_tail);
  mc_.cif_smooth = (float)jc->num_or("cif_smooth", mc_.cif_smooth);
  mc_.cif_noise = (float)jc->num_or("cif_noise", mc_.cif_noise);
  mc_.cif_l_order = (int)jc->int_or("cif_l_order", mc_.cif_l_order, INT32_MIN, INT32_MAX);
  mc_.cif_r_order = (int)jc->int_or("cif_r_order", mc_.cif_r_order, INT32_MIN, INT32_MAX);
  {
    const std::string cv = jc->str_or("cif_variant", "loop");
    PF_CHECK(cv == "loop" || cv == "cumsum", PF_ERR_UNSUPPORTED, "weights: cif_variant must be \"loop\" or \"cumsum\"");
    mc_.cif_cumsum = cv == "cumsum";
    PF_CHECK(!mc_.cif_cumsum || mc_.cif_threshold == 1.0f, PF_ERR_UNSUPPORTED, "cif_variant cumsum is defined for threshold 1.0");
  }
  mc_.timestamp_head = jc->bool_or("timestamp_head", false);
  mc_.seaco = jc->bool_or("seaco", false);
  mc_.use_itn = jc->bool_or("use_itn", false) || cfg.use_itn != 0;
  PF_CHECK(mc_.d_model == 512 && mc_.heads == 4, PF_ERR_UNSUPPORTED,
           "kernels are built for d_model = 512, 4 heads of 128");
  PF_CHECK(mc_.d_model % 8 == 0 && mc_.ffn % 64 == 0 && mc_.feat_dim % 4 == 0, PF_ERR_UNSUPPORTED,
           "unsupported model dimensions");
  mc_.cif_smooth2 = (float)jc->num_or("cif_smooth2", mc_.cif_smooth2);
  mc_.cif_noise2 = (float)jc->num_or("cif_noise2", mc_.cif_noise2);
  mc_.upsample = (int)jc->int_or("upsample", mc_.upsample, INT32_MIN, INT32_MAX);
  mc_.seaco_layers = (int)jc->int_or("seaco_layers", mc_.seaco_layers, INT32_MIN, INT32_MAX);
  mc_.seaco_ffn = (int)jc->int_or("seaco_ffn", mc_.seaco_ffn, INT32_MIN, INT32_MAX);
  mc_.seaco_kernel = (int)jc->int_or("seaco_kernel", mc_.seaco_kernel, INT32_MIN, INT32_MAX);
  mc_.seaco_lstm_layers = (int)jc->int_or("seaco_lstm_layers", mc_.seaco_lstm_layers, INT32_MIN, INT32_MAX);
  mc_.seaco_nobias = (int)jc->int_or("seaco_nobias", mc_.seaco_nobias, INT32_MIN, INT32_MAX);
  if (mc_.kind == "seacoparaformer") mc_.seaco = true;
  PF_CHECK(!mc_.seaco || (mc_.seaco_ffn % 64 == 0 && mc_.seaco_lstm_layers >= 1), PF_ERR_UNSUPPORTED,
           "seaco: unsupported dimensions");
  PF_CHECK(!mc_.timestamp_head || mc_.upsample == 3, PF_ERR_UNSUPPORTED, "timestamp head: only upsample = 3");

  const char* data_dev = nullptr;
  if (host) {
    PF_HIP(hipMalloc(&blob_dev_, std::max<int64_t>(fr.data_bytes, 256)));
    blob_owned_ = true;
    PF_HIP(hipMemcpy(blob_dev_, host + fr.data_off, fr.data_bytes, hipMemcpyHostToDevice));
    data_dev = (const char*)blob_dev_;
  } else {
    data_dev = dev_image + fr.data_off;
  }
  for (const auto& kv : ix.tensors)
    tensors_[kv.first] = Tensor{(const float*)(data_dev + kv.second.offset), kv.second.shape, kv.second.numel, kv.second.u8};
  if (const Json* ex = jc->get("int8_exclude"))
    if (ex->type == Json::Arr)
      for (const Json& e : ex->arr)
        if (e.type == Json::Str && !e.str.empty()) int8_exclude_.push_back(e.str);
  for (const auto& kv : tensors_) {
    const std::string& n = kv.first;
    if (kv.second.u8 && n.size() > 9 && n.compare(n.size() - 9, 9, ".weight_q") == 0) any_stored_q_ = true;
    if (!kv.second.u8 && n.size() > 7 && n.compare(n.size() - 7, 7, ".weight") == 0) lin_names_[kv.second.dev] = n.substr(0, n.size() - 7);
  }

  // ---- bind layers, build f16 GEMM operands
  const int D = mc_.d_model;
  auto enc_layer = [&](const std::string& p, int d_in) {
    EncLayer L;
    L.d_in = d_in;
    L.norm1 = make_ln(p + ".norm1", d_in);
    L.qkv = make_lin(p + ".attn.qkv", true);
    L.fsmn_wT = make_fsmn_wT(p + ".attn.fsmn.weight");
    L.out = make_lin(p + ".attn.out", true);
    L.norm2 = make_ln(p + ".norm2", D);
    L.w1 = make_lin(p + ".ffn.w1", true);
    L.w2 = make_lin(p + ".ffn.w2", true);
    PF_CHECK(L.qkv.K == d_in && L.qkv.N == 3 * D, PF_ERR_FORMAT, "weights: qkv shape mismatch in " + p);
    if (!fp32_mode_ && !int8_mode_) {
      // the same weight with its rows in the tile order of gemm_qkvp_kernel (k_gemm_qkv.hip)
      L.qkv_p = (half_t*)dalloc((size_t)1536 * L.qkv.Kpad * 2);
      L.qkv_bias_p = (float*)dalloc(1536 * 4);
      launch_qkv_permute(stream_, L.qkv.w, L.qkv.Kpad, L.qkv.bias, L.qkv_p, L.qkv_bias_p);
    }
    PF_CHECK(L.out.N == D && L.out.K == D && L.w1.K == D && L.w1.N == mc_.ffn && L.w2.N == D && L.w2.K == L.w1.N,
             PF_ERR_FORMAT, "weights: attn.out / ffn shape mismatch in " + p);
    if (ffn_fused_applicable(D, mc_.ffn) && !fp32_mode_ && !int8_mode_) {
      // W1 and W2 once more, in the fragment order the fused FFN kernel streams (4 MiB per layer)
      L.ffn_wt = (half_t*)dalloc(ffn_fused_weight_bytes());
      launch_ffn_retile(stream_, L.w1.w, L.w1.Kpad, L.w2.w, L.w2.Kpad, L.ffn_wt);
      if (mc_.kernel == 11) {
        L.out_wt = (half_t*)dalloc(ffn_outproj_weight_bytes());
        launch_ffn_retile_out(stream_, L.out.w, L.out.Kpad, L.out_wt);
        if (L.qkv.Kpad == D) {
          L.qkv_t = (half_t*)dalloc(3 * ffn_outproj_weight_bytes());
          for (int part = 0; part < 3; ++part)
            launch_ffn_retile_out(stream_, L.qkv.w + (size_t)part * D * L.qkv.Kpad, L.qkv.Kpad,
                                  L.qkv_t + (size_t)part * (ffn_outproj_weight_bytes() / 2));
        }
      }
    }
    return L;
  };
  for (int i = 0; i < mc_.enc_layers; ++i)
    enc_.push_back(enc_layer("encoder.layers." + std::to_string(i), i == 0 ? mc_.feat_dim : D));
  enc_after_ = make_ln("encoder.after_norm", D);
  for (int i = 0; i < mc_.tp_layers; ++i) tp_.push_back(enc_layer("encoder.tp_layers." + std::to_string(i), D));
  if (mc_.tp_layers) tp_norm_ = make_ln("encoder.tp_norm", D);

  if (mc_.kind == "sensevoicesmall") {
    ctc_ = make_lin("ctc", true);
    if (has_tensor("embed.weight")) {
      const Tensor& t = tensor("embed.weight");
      embed_host_.resize(t.numel);
      PF_HIP(hipMemcpy(embed_host_.data(), t.dev, t.numel * 4, hipMemcpyDeviceToHost));
      // device copy of the 4 query rows [language, 1, 2, textnorm] with the EFFECTIVE ids of the
      // reference (quirk Q7, OfflineProjOfSenseVoiceSmall.cs:57-74): language = 14 if use_itn else 15,
      // textnorm = 15 — used by the audio-in entry points (pf_recognize / pf_run_staged)
      const int W = mc_.feat_dim;
      if (t.numel >= (int64_t)16 * W) {
        const int order[4] = {mc_.use_itn ? 14 : 15, 1, 2, 15};
        sv_prompt_ = (float*)dalloc((size_t)4 * W * 4);
        for (int r = 0; r < 4; ++r)
          PF_HIP(hipMemcpy(sv_prompt_ + (size_t)r * W, embed_host_.data() + (size_t)order[r] * W, (size_t)W * 4,
                           hipMemcpyHostToDevice));
      }
    }
    return;
  }

  // CIF predictor: conv weight [out, in, k] -> GEMM operand [out][j*D + in]
  {
    const Tensor& cw = tensor("predictor.conv.weight");
    const int taps = mc_.cif_l_order + mc_.cif_r_order + 1;
    PF_CHECK(cw.shape.size() == 3 && cw.shape[0] == D && cw.shape[1] == D && cw.shape[2] == taps, PF_ERR_FORMAT,
             "weights: predictor.conv.weight shape");
    std::vector<float> hostw(cw.numel), re(cw.numel);
    PF_HIP(hipMemcpy(hostw.data(), cw.dev, cw.numel * 4, hipMemcpyDeviceToHost));
    for (int o = 0; o < D; ++o)
      for (int i = 0; i < D; ++i)
        for (int jx = 0; jx < taps; ++jx) re[(size_t)o * taps * D + (size_t)jx * D + i] = hostw[((size_t)o * D + i) * taps + jx];
    float* tmp = nullptr;
    PF_HIP(hipMalloc(&tmp, re.size() * 4));
    PF_HIP(hipMemcpy(tmp, re.data(), re.size() * 4, hipMemcpyHostToDevice));
    cif_conv_.N = D; cif_conv_.K = taps * D; cif_conv_.Kpad = (int)round_up(taps * D, 64);
    const int npad = (int)round_up(D, 128);
    cif_conv_.w = (half_t*)dalloc((size_t)npad * cif_conv_.Kpad * 2);
    PF_HIP(hipMemsetAsync(cif_conv_.w, 0, (size_t)npad * cif_conv_.Kpad * 2, stream_));
    launch_f32_to_f16(stream_, tmp, D, taps * D, taps * D, cif_conv_.w, cif_conv_.Kpad);
    PF_HIP(hipStreamSynchronize(stream_));
    if (fp32_mode_) { cif_conv_w32_ = tmp; owned_.push_back(tmp); }
    else PF_HIP(hipFree(tmp));
    cif_conv_.bias = tensor("predictor.conv.bias").dev;
    PF_CHECK(tensor("predictor.conv.bias").numel == D && tensor("predictor.out.weight").numel == D &&
                 tensor("predictor.out.bias").numel == 1,
             PF_ERR_FORMAT, "weights: predictor.conv.bias / predictor.out.* sizes");
    cif_out_w_ = tensor("predictor.out.weight").dev;
    cif_out_b_ = tensor("predictor.out.bias").dev;
  }
  // BiCIF timestamp head: ConvTranspose1d weight [in, out, j] -> GEMM operand [(j, out)][in];
  // W_ih of both directions stacked [8D, D] with b_ih + b_hh folded into one bias; W_hh f16 [2][4D][D].
  if (mc_.timestamp_head) {
    const int up = mc_.upsample;
    const Tensor& uw = tensor("predictor.upsample.weight");
    const Tensor& ub = tensor("predictor.upsample.bias");
    PF_CHECK(uw.shape.size() == 3 && uw.shape[0] == D && uw.shape[1] == D && uw.shape[2] == up && ub.numel == D,
             PF_ERR_FORMAT, "weights: predictor.upsample shape");
    std::vector<float> hw(uw.numel), re(uw.numel), hb(D), rb((size_t)up * D);
    PF_HIP(hipMemcpy(hw.data(), uw.dev, uw.numel * 4, hipMemcpyDeviceToHost));
    PF_HIP(hipMemcpy(hb.data(), ub.dev, (size_t)D * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < D; ++i)
      for (int o = 0; o < D; ++o)
        for (int jx = 0; jx < up; ++jx) re[((size_t)jx * D + o) * D + i] = hw[((size_t)i * D + o) * up + jx];
    for (int jx = 0; jx < up; ++jx) std::memcpy(&rb[(size_t)jx * D], hb.data(), (size_t)D * 4);
    float* tmp = nullptr;
    PF_HIP(hipMalloc(&tmp, std::max(re.size(), (size_t)8 * D * D) * 4));
    PF_HIP(hipMemcpy(tmp, re.data(), re.size() * 4, hipMemcpyHostToDevice));
    ts_up_.N = up * D; ts_up_.K = D; ts_up_.Kpad = D;
    ts_up_.w = (half_t*)dalloc((size_t)round_up(up * D, 128) * D * 2);
    PF_HIP(hipMemsetAsync(ts_up_.w, 0, (size_t)round_up(up * D, 128) * D * 2, stream_));
    launch_f32_to_f16(stream_, tmp, up * D, D, D, ts_up_.w, D);
    float* ubias = (float*)dalloc(rb.size() * 4);
    PF_HIP(hipMemcpyAsync(ubias, rb.data(), rb.size() * 4, hipMemcpyHostToDevice, stream_));
    ts_up_.bias = ubias;
    PF_HIP(hipStreamSynchronize(stream_));

    ts_ih_.N = 8 * D; ts_ih_.K = D; ts_ih_.Kpad = D;
    ts_ih_.w = (half_t*)dalloc((size_t)8 * D * D * 2);
    ts_whh_ = (half_t*)dalloc((size_t)8 * D * D * 2);
    std::vector<float> bsum((size_t)8 * D), b1((size_t)4 * D), b2((size_t)4 * D);
    const char* sfx[2] = {"", "_reverse"};
    for (int d = 0; d < 2; ++d) {
      const Tensor& wih = tensor(std::string("predictor.blstm.weight_ih") + sfx[d]);
      const Tensor& whh = tensor(std::string("predictor.blstm.weight_hh") + sfx[d]);
      const Tensor& bih = tensor(std::string("predictor.blstm.bias_ih") + sfx[d]);
      const Tensor& bhh = tensor(std::string("predictor.blstm.bias_hh") + sfx[d]);
      PF_CHECK(wih.numel == (int64_t)4 * D * D && whh.numel == (int64_t)4 * D * D && bih.numel == 4 * D && bhh.numel == 4 * D,
               PF_ERR_FORMAT, "weights: predictor.blstm shapes");
      launch_f32_to_f16(stream_, wih.dev, 4 * D, D, D, ts_ih_.w + (size_t)d * 4 * D * D, D);
      launch_f32_to_f16(stream_, whh.dev, 4 * D, D, D, ts_whh_ + (size_t)d * 4 * D * D, D);
      PF_HIP(hipMemcpy(b1.data(), bih.dev, (size_t)4 * D * 4, hipMemcpyDeviceToHost));
      PF_HIP(hipMemcpy(b2.data(), bhh.dev, (size_t)4 * D * 4, hipMemcpyDeviceToHost));
      for (int i = 0; i < 4 * D; ++i) bsum[(size_t)d * 4 * D + i] = b1[i] + b2[i];
    }
    float* gb = (float*)dalloc(bsum.size() * 4);
    PF_HIP(hipMemcpyAsync(gb, bsum.data(), bsum.size() * 4, hipMemcpyHostToDevice, stream_));
    ts_ih_.bias = gb;
    const Tensor& ow = tensor("predictor.out2.weight");
    PF_CHECK(ow.numel == 2 * D, PF_ERR_FORMAT, "weights: predictor.out2.weight shape");
    PF_CHECK(tensor("predictor.out2.bias").numel == 1, PF_ERR_FORMAT, "weights: predictor.out2.bias shape");
    ts_out_w_ = ow.dev;
    ts_out_b_ = tensor("predictor.out2.bias").dev;
    PF_HIP(hipStreamSynchronize(stream_));
    if (fp32_mode_) { ts_up_w32_ = tmp; owned_.push_back(tmp); }   // [(j, out)][in] fp32, the operand of the parity mode
    else PF_HIP(hipFree(tmp));
  }
  // decoder
  dec_ = load_dec_stack("decoder", mc_.dec_layers, mc_.ffn, mc_.kernel, true);
  dec_.out = make_lin("decoder.output", true);
  PF_CHECK(dec_.out.N == mc_.vocab && dec_.out.K == D && dec_.final_w1.K == D && dec_.final_w1.N == mc_.ffn &&
               dec_.final_w2.N == D && dec_.final_w2.K == dec_.final_w1.N,
           PF_ERR_FORMAT, "weights: decoder.final / decoder.output shapes");
  // the K | V projection of all layers and the vocabulary layer in the fragment order of the panel-resident kernel
  // (k_gemm_panel.hip; f16 mode only — the row-major weights stay: the tiled and short-input kernels read them)
  if (gemm_panel_ && !fp32_mode_ && !int8_mode_)
    for (Lin* l : {&dec_.kv_all, &dec_.out})
      if (l->w && l->N > 0 && l->K == 512 && l->Kpad == 512) {
        l->w_panel = (half_t*)dalloc(gemm_panel_image_bytes(l->N));
        launch_gemm_panel_retile(stream_, l->w, l->Kpad, l->N, l->w_panel);
      }
  // SeACo: hotword embedder (Embedding + LSTM stack) and the bias decoder
  if (mc_.seaco) {
    const Tensor& ew = tensor("seaco.embed.weight");
    PF_CHECK(ew.shape.size() == 2 && ew.shape[1] == D, PF_ERR_FORMAT, "weights: seaco.embed.weight shape");
    seaco_embed_w_ = ew.dev;
    std::vector<float> b1((size_t)4 * D), b2((size_t)4 * D);
    for (int l = 0; l < mc_.seaco_lstm_layers; ++l) {
      const std::string p = "seaco.lstm.l" + std::to_string(l);
      const Tensor& wih = tensor(p + ".weight_ih");
      const Tensor& whh = tensor(p + ".weight_hh");
      const Tensor& bih = tensor(p + ".bias_ih");
      const Tensor& bhh = tensor(p + ".bias_hh");
      PF_CHECK(wih.numel == (int64_t)4 * D * D && whh.numel == (int64_t)4 * D * D && bih.numel == 4 * D && bhh.numel == 4 * D,
               PF_ERR_FORMAT, "weights: seaco.lstm shapes");
      LstmLayer L;
      L.ih.N = 4 * D; L.ih.K = D; L.ih.Kpad = D;
      L.ih.w = (half_t*)dalloc((size_t)4 * D * D * 2);
      L.whh = (half_t*)dalloc((size_t)4 * D * D * 2);
      launch_f32_to_f16(stream_, wih.dev, 4 * D, D, D, L.ih.w, D);
      launch_f32_to_f16(stream_, whh.dev, 4 * D, D, D, L.whh, D);
      PF_HIP(hipMemcpy(b1.data(), bih.dev, (size_t)4 * D * 4, hipMemcpyDeviceToHost));
      PF_HIP(hipMemcpy(b2.data(), bhh.dev, (size_t)4 * D * 4, hipMemcpyDeviceToHost));
      for (int i = 0; i < 4 * D; ++i) b1[i] += b2[i];
      float* gb = (float*)dalloc((size_t)4 * D * 4);
      PF_HIP(hipMemcpy(gb, b1.data(), (size_t)4 * D * 4, hipMemcpyHostToDevice));
      L.ih.bias = gb;
      seaco_lstm_.push_back(L);
    }
    bias_dec_ = load_dec_stack("seaco.decoder", mc_.seaco_layers, mc_.seaco_ffn, mc_.seaco_kernel, false);
    bias_dec_.out = make_lin("seaco.output", true);
    PF_CHECK(bias_dec_.out.N == mc_.vocab, PF_ERR_FORMAT, "weights: seaco.output rows != vocab");
  }
  PF_HIP(hipStreamSynchronize(stream_));
}

// One decoder stack: `prefix`.layers.N, `prefix`.final, `prefix`.after_norm.  The K | V projections of all layers are also
// kept as ONE f16 Linear [n_layers * 2D, D] (kv_all): they depend on the memory alone and go out as one GEMM.
DecStack Engine::load_dec_stack(const std::string& prefix, int n_layers, int ffn, int fsmn_k, bool fused_images) {
  const int D = mc_.d_model;
  const bool asr = prefix == "decoder";
  DecStack S;
  S.ffn = ffn; S.fsmn_k = fsmn_k;
  if (n_layers > 0) {
    Lin& kva = S.kv_all;
    kva.N = n_layers * 2 * D; kva.K = D; kva.Kpad = D;
    kva.w = (half_t*)dalloc((size_t)round_up(kva.N, 128) * D * 2);
    PF_HIP(hipMemsetAsync(kva.w, 0, (size_t)round_up(kva.N, 128) * D * 2, stream_));
    float* kvb = (float*)dalloc((size_t)kva.N * 4);
    kva.bias = kvb;
    for (int i = 0; i < n_layers; ++i) {
      const std::string p = prefix + ".layers." + std::to_string(i);
      DecLayer L;
      L.norm1 = make_ln(p + ".norm1", D);
      L.w1 = make_lin(p + ".ffn.w1", true);
      L.ffn_norm = make_ln(p + ".ffn.norm", L.w1.N);
      L.w2 = make_lin(p + ".ffn.w2", false);
      L.norm2 = make_ln(p + ".norm2", D);
      L.fsmn_wT = make_fsmn_wT(p + ".fsmn.weight", fsmn_k);
      L.norm3 = make_ln(p + ".norm3", D);
      L.q = make_lin(p + ".src.q", true);
      L.out = make_lin(p + ".src.out", true);
      PF_CHECK(L.w1.K == D && (!asr || L.w1.N == ffn) && L.w2.N == D && L.w2.K == L.w1.N && L.q.N == D && L.q.K == D &&
                   L.out.N == D && L.out.K == D,
               PF_ERR_FORMAT, std::string("weights: ") + (asr ? "" : "seaco ") + "decoder layer shape mismatch in " + p);
      const Tensor& kvw = tensor(p + ".src.kv.weight");
      const Tensor& kvbias = tensor(p + ".src.kv.bias");
      PF_CHECK(kvw.numel == (int64_t)2 * D * D && kvbias.numel == 2 * D, PF_ERR_FORMAT, "weights: src.kv shape in " + p);
      PF_CHECK(asr || L.w1.N == ffn, PF_ERR_FORMAT, "weights: seaco ffn width != seaco_ffn");
      launch_f32_to_f16(stream_, kvw.dev, 2 * D, D, D, kva.w + (size_t)i * 2 * D * D, D);
      PF_HIP(hipMemcpyAsync(kvb + (size_t)i * 2 * D, kvbias.dev, 2 * D * 4, hipMemcpyDeviceToDevice, stream_));
      L.kv32.w32 = kvw.dev; L.kv32.bias = kvbias.dev; L.kv32.N = 2 * D; L.kv32.K = D;
      L.kv32.w = kva.w + (size_t)i * 2 * D * D; L.kv32.Kpad = D;
      if (fused_images) L.ffn_img = make_dec_ffn_image(L.w1, L.ffn_norm, L.w2);
      if (L.ffn_img) {
        L.out_wt = (half_t*)dalloc(ffn_outproj_weight_bytes());
        launch_ffn_retile_out(stream_, L.out.w, L.out.Kpad, L.out_wt);
      }
      if (L.ffn_img && dec_mid_ && L.q.w && L.q.bias && L.q.Kpad == D && L.q.N == D) {
        L.q_wt = (half_t*)dalloc(ffn_outproj_weight_bytes());
        launch_ffn_retile_out(stream_, L.q.w, L.q.Kpad, L.q_wt);
      }
      S.layers.push_back(L);
    }
  }
  S.final_norm1 = make_ln(prefix + ".final.norm1", D);
  S.final_w1 = make_lin(prefix + ".final.ffn.w1", true);
  S.final_ffn_norm = make_ln(prefix + ".final.ffn.norm", S.final_w1.N);
  S.final_w2 = make_lin(prefix + ".final.ffn.w2", false);
  S.after = make_ln(prefix + ".after_norm", D);
  if (fused_images) S.final_img = make_dec_ffn_image(S.final_w1, S.final_ffn_norm, S.final_w2);
  return S;
}

// The decoder's FFN block for the split form of ffn_fused_kernel (k_ffn.hip): W1, gamma_F (.) W2 (from the fp32 tensor, one
// rounding), b1, colsum(gamma_F (.) W2), W2 beta_F.  Null when the form does not apply (mode, shape).
half_t* Engine::make_dec_ffn_image(const Lin& w1, const LNp& fn, const Lin& w2) {
  if (fp32_mode_ || int8_mode_ || !ffn_fused_applicable(w1.K, w1.N) || w2.N != w1.K || w2.K != w1.N ||
      !w1.w || !w1.bias || !w2.w32 || w2.bias || w1.Kpad != w1.K || fn.D != w1.N)
    return nullptr;
  half_t* img = (half_t*)dalloc(ffn_dec_image_bytes());
  launch_ffn_dec_retile(stream_, w1.w, w1.Kpad, w2.w32, fn.g, fn.b, w1.bias, img);
  return img;
}

Lin Engine::make_lin(const std::string& prefix, bool bias) {
  const Tensor& w = tensor(prefix + ".weight");
  PF_CHECK(w.shape.size() == 2, PF_ERR_FORMAT, "weights: '" + prefix + ".weight' must be 2-D [out,in]");
  Lin L;
  L.N = (int)w.shape[0];
  L.K = (int)w.shape[1];
  L.Kpad = (int)round_up(L.K, 64);
  const size_t npad = (size_t)round_up(L.N, 128);
  L.w = (half_t*)dalloc(npad * L.Kpad * 2);
  PF_HIP(hipMemsetAsync(L.w, 0, npad * L.Kpad * 2, stream_));
  launch_f32_to_f16(stream_, w.dev, L.N, L.K, L.K, L.w, L.Kpad);
  L.w32 = w.dev;
  if (bias) {
    const Tensor& b = tensor(prefix + ".bias");
    PF_CHECK(b.numel == L.N, PF_ERR_FORMAT, "weights: bias length mismatch for " + prefix);
    L.bias = b.dev;
  }
  return L;
}

LNp Engine::make_ln(const std::string& prefix, int width) {
  LNp p;
  const Tensor& g = tensor(prefix + ".weight");
  const Tensor& b = tensor(prefix + ".bias");
  PF_CHECK(g.numel == b.numel, PF_ERR_FORMAT, "weights: LayerNorm size mismatch for " + prefix);
  // the kernel normalises rows of `width` floats: a shorter gamma / beta would be read out of bounds
  PF_CHECK(g.numel == width, PF_ERR_FORMAT, "weights: '" + prefix + "' has " + std::to_string(g.numel) +
                                                " elements, the layer is " + std::to_string(width) + " wide");
  p.g = g.dev; p.b = b.dev; p.D = (int)g.numel;
  return p;
}

float* Engine::make_fsmn_wT(const std::string& name, int Kopt) {
  const Tensor& w = tensor(name);
  const int D = mc_.d_model, K = Kopt > 0 ? Kopt : mc_.kernel;
  PF_CHECK(w.shape.size() == 2 && w.shape[0] == D && w.shape[1] == K, PF_ERR_FORMAT,
           "weights: '" + name + "' must be [d_model, kernel]");
  std::vector<float> h(w.numel), t(w.numel);
  PF_HIP(hipMemcpy(h.data(), w.dev, w.numel * 4, hipMemcpyDeviceToHost));
  for (int c = 0; c < D; ++c)
    for (int jx = 0; jx < K; ++jx) t[(size_t)jx * D + c] = h[(size_t)c * K + jx];
  float* d = (float*)dalloc(w.numel * 4);
  PF_HIP(hipMemcpy(d, t.data(), w.numel * 4, hipMemcpyHostToDevice));
  return d;
}

// ------------------------------------------------------------------ profiling -------------
void Engine::profile_reset() {
  for (auto& kv : prof_)
    for (auto& pr : kv.second.ev) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
  prof_.clear();
}
void Engine::prof_begin(const char* cls, double flops) {
  if (!prof_on_) return;
  if (!prof_only_.empty() && prof_only_ != cls) return;
  ProfClass& pc = prof_[cls];
  hipEvent_t a, b;
  PF_HIP(hipEventCreate(&a));
  PF_HIP(hipEventCreate(&b));
  pc.ev.emplace_back(a, b);
  pc.flops += flops;
  pc.n += 1;
  PF_HIP(hipEventRecord(a, stream_));
}
void Engine::prof_end(const char* cls) {
  if (!prof_on_) return;
  if (!prof_only_.empty() && prof_only_ != cls) return;
  ProfClass& pc = prof_[cls];
  PF_HIP(hipEventRecord(pc.ev.back().second, stream_));
  if (cls[0] == 'g' && cls[1] == 'e') pc.kernel = last_gemm_kernel();   // "gemm_*" classes
}
std::string Engine::profile_kernel(const std::string& cls) const {
  auto it = prof_.find(cls);
  return it == prof_.end() ? std::string() : it->second.kernel;
}
bool Engine::profile_get(const std::string& cls, double* ms, int64_t* launches, double* flops_per_launch) {
  auto it = prof_.find(cls);
  if (it == prof_.end()) return false;
  PF_HIP(hipStreamSynchronize(stream_));
  double total = 0;
  for (auto& pr : it->second.ev) {
    float t = 0;
    PF_HIP(hipEventElapsedTime(&t, pr.first, pr.second));
    total += t;
  }
  if (ms) *ms = total;
  if (launches) *launches = it->second.n;
  if (flops_per_launch) *flops_per_launch = it->second.n ? it->second.flops / it->second.n : 0;
  return true;
}

void Engine::gemm(const char* cls, const Lin& w, const half_t* A, int lda, int M, float* out32, int ld32,
                  half_t* out16, int ld16, const float* resid, int ldr, const float* add2, int ld2, bool relu,
                  int scale_cols, float scale, bool bias, int blocked) {
  GemmArgs g{};
  g.A = A; g.lda = lda; g.W = w.w; g.ldw = w.Kpad; g.bias = bias ? w.bias : nullptr;
  g.M = M; g.N = w.N; g.K = w.Kpad;
  g.out_f32 = out32; g.ldc32 = ld32; g.out_f16 = out16; g.ldc16 = ld16;
  g.resid = resid; g.ldr = ldr; g.add2 = add2; g.ld2 = ld2;
  g.relu = relu ? 1 : 0; g.scale_cols = scale_cols; g.scale = scale;
  g.out_padded = 1;   // every pipeline buffer is carved with round_up(rows,128)+128 rows
  g.out_blocked = blocked == 1; g.a_blocked = blocked == 2;
  g.small_ws = small_ws_;
  g.W_panel = gemm_panel_ ? w.w_panel : nullptr;
  prof_begin(cls, 2.0 * M * (double)w.N * w.K);
  launch_gemm(stream_, g);
  prof_end(cls);
}

// short-input form of a projection (k_gemm_small.hip): the caller fills operand / epilogue fields of `g`, this adds
// the weight, shape, scratch and the profile class
void Engine::gemm_small_call(const char* cls, const Lin& w, GemmSmallArgs g, bool bias) {
  g.W = w.w; g.ldw = w.Kpad; g.bias = bias ? w.bias : nullptr; g.N = w.N; g.K = w.Kpad; g.ws = small_ws_;
  prof_begin(cls, 2.0 * g.M * (double)w.N * w.K);
  launch_gemm_small(stream_, g);
  prof_end(cls);
}

// ------------------------------------------------------------------ front-end -------------
int Engine::num_fbank_frames(int64_t n) const {
  if (fc_.snip_edges) return n < 400 ? 0 : (int)(1 + (n - 400) / 160);
  return (int)((n + 80) / 160);
}
int Engine::num_lfr_frames(int64_t n) const {
  const int t80 = num_fbank_frames(n);
  if (fc_.lfr_m == 1 && fc_.lfr_n == 1) return t80;
  return t80 / fc_.lfr_n;
}

void Engine::stage_audio(const float* const* samples, const int64_t* n, int B, int force_T) {
  PF_CHECK(B >= 0, PF_ERR_INVALID_ARG, "negative batch");
  PF_HIP(hipSetDevice(device_));
  st_audio_ext_ = nullptr;
  st_B_ = B;
  st_n_.assign(n, n + B);
  st_t80_.resize(B);
  std::vector<int64_t> meta(3 * (size_t)(B + 1), 0);   // audio_off | n_samples | frame_off
  int64_t tot = 0, frames = 0;
  int tmax = 0;
  for (int b = 0; b < B; ++b) {
    if (!samples[b] && n[b] > 0) throw Error(PF_ERR_NULL_SAMPLES, "source");
    PF_CHECK(n[b] >= 0, PF_ERR_INVALID_ARG, "negative sample count");
    meta[b] = tot;
    meta[(B + 1) + b] = n[b];
    meta[2 * (B + 1) + b] = frames;
    st_t80_[b] = num_fbank_frames(n[b]);
    tot += round_up(n[b], 4);
    frames += st_t80_[b];
    tmax = std::max(tmax, num_lfr_frames(n[b]));
  }
  meta[2 * (B + 1) + B] = frames;
  st_total_frames_ = frames;
  st_T_ = std::max(tmax, force_T);
  ensure(ws_audio_, (size_t)std::max<int64_t>(tot, 1) * 4);
  ensure(ws_meta_, meta.size() * 8 + (size_t)B * 4 + 64);
  for (int b = 0; b < B; ++b)
    if (n[b] > 0)
      PF_HIP(hipMemcpyAsync((float*)ws_audio_.p + meta[b], samples[b], n[b] * 4, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(ws_meta_.p, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync((char*)ws_meta_.p + meta.size() * 8, st_t80_.data(), (size_t)B * 4, hipMemcpyHostToDevice,
                        stream_));
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::stage_pcm(const void* const* data, const int64_t* n_values, const pf_pcm_desc* descs, int n_descs, int B, int force_T) {
  PF_CHECK(B >= 0, PF_ERR_INVALID_ARG, "negative batch");
  PF_CHECK(n_descs == B || n_descs == 1, PF_ERR_INVALID_ARG, "stage_pcm: n_descs must be 1 or B");
  PF_HIP(hipSetDevice(device_));
  st_audio_ext_ = nullptr;
  st_B_ = B;
  st_n_.resize(B);
  st_t80_.resize(B);
  std::vector<int64_t> meta(3 * (size_t)(B + 1), 0);   // audio_off | n_samples | frame_off
  std::vector<PcmJob> jobs((size_t)B);
  std::vector<size_t> raw_bytes((size_t)B);
  int64_t tot = 0, frames = 0, raw_tot = 0, max_out = 0;
  int tmax = 0;
  for (int b = 0; b < B; ++b) {
    const pf_pcm_desc& d = descs[n_descs == 1 ? 0 : b];
    const PcmPlan p = pcm_plan(d, fc_.fs, n_values[b]);
    PF_CHECK(data[b] || n_values[b] == 0, PF_ERR_INVALID_ARG, "pcm: null data");
    raw_bytes[b] = (size_t)n_values[b] * p.bytes_per_value;
    jobs[b] = PcmJob{raw_tot, tot, p.n_mono, p.n_out, p.ratio, d.format, p.downmix ? 1 : 0, p.resample ? 1 : 0, 0};
    st_n_[b] = p.n_out;
    meta[b] = tot;
    meta[(B + 1) + b] = p.n_out;
    meta[2 * (B + 1) + b] = frames;
    st_t80_[b] = num_fbank_frames(p.n_out);
    tot += round_up(p.n_out, 4);
    raw_tot += round_up((int64_t)raw_bytes[b], 16);
    frames += st_t80_[b];
    tmax = std::max(tmax, num_lfr_frames(p.n_out));
    max_out = std::max(max_out, p.n_out);
  }
  meta[2 * (B + 1) + B] = frames;
  st_total_frames_ = frames;
  st_T_ = std::max(tmax, force_T);
  const size_t jobs_off = (size_t)round_up(std::max<int64_t>(raw_tot, 16), 256);
  ensure(ws_pcm_, jobs_off + std::max<size_t>(jobs.size(), 1) * sizeof(PcmJob));
  ensure(ws_audio_, (size_t)std::max<int64_t>(tot, 1) * 4);
  ensure(ws_meta_, meta.size() * 8 + (size_t)B * 4 + 64);
  for (int b = 0; b < B; ++b)
    if (raw_bytes[b] > 0)
      PF_HIP(hipMemcpyAsync((char*)ws_pcm_.p + jobs[b].in_off, data[b], raw_bytes[b], hipMemcpyHostToDevice, stream_));
  if (B > 0) PF_HIP(hipMemcpyAsync((char*)ws_pcm_.p + jobs_off, jobs.data(), jobs.size() * sizeof(PcmJob), hipMemcpyHostToDevice, stream_));
  prof_begin("pcm_to_samples", 0);
  launch_pcm_to_samples(stream_, (const PcmJob*)((char*)ws_pcm_.p + jobs_off), B, max_out, ws_pcm_.p, (float*)ws_audio_.p);
  prof_end("pcm_to_samples");
  PF_HIP(hipMemcpyAsync(ws_meta_.p, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync((char*)ws_meta_.p + meta.size() * 8, st_t80_.data(), (size_t)B * 4, hipMemcpyHostToDevice,
                        stream_));
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::stage_device_audio(const float* const* samples_dev, const int64_t* n, int B, int force_T) {
  PF_CHECK(B >= 0, PF_ERR_INVALID_ARG, "negative batch");
  PF_HIP(hipSetDevice(device_));
  st_B_ = B;
  st_n_.assign(n, n + B);
  st_t80_.resize(B);
  // offsets are relative to the LOWEST of the buffers (element offsets, non-negative): the fbank kernel adds them to one base
  uintptr_t lo = UINTPTR_MAX;
  for (int b = 0; b < B; ++b) {
    if (!samples_dev[b] && n[b] > 0) throw Error(PF_ERR_NULL_SAMPLES, "source");
    PF_CHECK(n[b] >= 0 && ((uintptr_t)samples_dev[b] & 3) == 0, PF_ERR_INVALID_ARG, "device audio must be 4-byte aligned");
    if (n[b] > 0) lo = std::min(lo, (uintptr_t)samples_dev[b]);
  }
  if (lo == UINTPTR_MAX) lo = 0;
  std::vector<int64_t> meta(3 * (size_t)(B + 1), 0);   // audio_off | n_samples | frame_off
  int64_t frames = 0;
  int tmax = 0;
  for (int b = 0; b < B; ++b) {
    meta[b] = n[b] > 0 ? (int64_t)(((uintptr_t)samples_dev[b] - lo) / 4) : 0;
    meta[(B + 1) + b] = n[b];
    meta[2 * (B + 1) + b] = frames;
    st_t80_[b] = num_fbank_frames(n[b]);
    frames += st_t80_[b];
    tmax = std::max(tmax, num_lfr_frames(n[b]));
  }
  meta[2 * (B + 1) + B] = frames;
  st_total_frames_ = frames;
  st_T_ = std::max(tmax, force_T);
  st_audio_ext_ = (const float*)lo;
  ensure(ws_meta_, meta.size() * 8 + (size_t)B * 4 + 64);
  PF_HIP(hipMemcpyAsync(ws_meta_.p, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync((char*)ws_meta_.p + meta.size() * 8, st_t80_.data(), (size_t)B * 4, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipStreamSynchronize(stream_));               // (meta is a stack vector; 1 KB)
}

void Engine::run_staged(bool want_logits) {
  PF_HIP(hipSetDevice(device_));
  const int B = st_B_, T = st_T_;
  if (B == 0) { last_ = HostBatchOut(); return; }
  PF_CHECK(T > 0, PF_ERR_INVALID_ARG, "audio too short: no LFR frame");
  const int W = fc_.lfr_m * fc_.n_mels;
  PF_CHECK(W == mc_.feat_dim, PF_ERR_INVALID_ARG, "lfr_m * n_mels != model feature dim");
  const int64_t* meta = (const int64_t*)ws_meta_.p;
  const int32_t* t80d = (const int32_t*)((const char*)ws_meta_.p + 3 * (size_t)(B + 1) * 8);
  ensure(ws_fbank_, (size_t)std::max<int64_t>(st_total_frames_, 1) * fc_.n_mels * 4);
  const int P = sv_prompt_ ? 4 : 0;                 // SenseVoice: query rows prepended on the device
  ensure(ws_speech_, (size_t)B * (T + P) * W * 4);
  prof_begin("fbank", 0);
  launch_fbank(stream_, fb_, st_audio_ext_ ? st_audio_ext_ : (const float*)ws_audio_.p, meta, meta + (B + 1), meta + 2 * (B + 1), B,
               st_total_frames_, fc_.snip_edges ? 1 : 0, (float*)ws_fbank_.p, fc_.dither, next_dither_seed());
  prof_end("fbank");
  prof_begin("lfr_cmvn_pad", 0);
  launch_lfr_cmvn_pad(stream_, (const float*)ws_fbank_.p, meta + 2 * (B + 1), t80d, B, T, fc_.lfr_m, fc_.lfr_n,
                      fc_.n_mels, cmvn_shift_, cmvn_scale_, cmvn_shift_ ? 1 : 0, 1, (float*)ws_speech_.p, sv_prompt_, P);
  prof_end("lfr_cmvn_pad");
  dec_len_.resize(B);
  for (int b = 0; b < B; ++b) dec_len_[b] = P + num_lfr_frames(st_n_[b]);
  forward_device((const float*)ws_speech_.p, B, T + P, want_logits);
}

void Engine::fbank_host(const float* samples, int64_t n, std::vector<float>& out, int& t80) {
  if (!samples) throw Error(PF_ERR_NULL_SAMPLES, "source");
  const float* arr[1] = {samples};
  const int64_t nn[1] = {n};
  stage_audio(arr, nn, 1);
  t80 = st_t80_[0];
  out.assign((size_t)t80 * fc_.n_mels, 0.f);
  if (t80 == 0) return;
  const int64_t* meta = (const int64_t*)ws_meta_.p;
  ensure(ws_fbank_, (size_t)t80 * fc_.n_mels * 4);
  launch_fbank(stream_, fb_, (const float*)ws_audio_.p, meta, meta + 2, meta + 4, 1, t80, fc_.snip_edges ? 1 : 0,
               (float*)ws_fbank_.p, fc_.dither, next_dither_seed());
  PF_HIP(hipMemcpyAsync(out.data(), ws_fbank_.p, out.size() * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::frontend_host(const float* samples, int64_t n, std::vector<float>& feats, int& t_lfr) {
  if (!samples) throw Error(PF_ERR_NULL_SAMPLES, "source");
  const float* arr[1] = {samples};
  const int64_t nn[1] = {n};
  stage_audio(arr, nn, 1);
  frontend_staged_one(feats, t_lfr);
}

void Engine::frontend_from_device(const float* samples_dev, int64_t n, std::vector<float>& feats, int& t_lfr) {
  const float* arr[1] = {samples_dev};
  const int64_t nn[1] = {n};
  stage_device_audio(arr, nn, 1);
  frontend_staged_one(feats, t_lfr);
}

// fbank + LFR + CMVN of the ONE staged utterance -> host features (no padding, no sentinel)
void Engine::frontend_staged_one(std::vector<float>& feats, int& t_lfr) {
  const int t80 = st_t80_[0];
  const bool lfr = fc_.lfr_m != 1 || fc_.lfr_n != 1;
  const int m = lfr ? fc_.lfr_m : 1, nn_ = lfr ? fc_.lfr_n : 1;
  t_lfr = t80 / nn_;
  const int W = m * fc_.n_mels;
  feats.assign((size_t)t_lfr * W, 0.f);
  if (t_lfr == 0) return;
  const int64_t* meta = (const int64_t*)ws_meta_.p;
  const int32_t* t80d = (const int32_t*)((const char*)ws_meta_.p + 3 * 2 * 8);
  ensure(ws_fbank_, (size_t)t80 * fc_.n_mels * 4);
  ensure(ws_speech_, feats.size() * 4);
  launch_fbank(stream_, fb_, st_audio_ext_ ? st_audio_ext_ : (const float*)ws_audio_.p, meta, meta + 2, meta + 4, 1, t80, fc_.snip_edges ? 1 : 0,
               (float*)ws_fbank_.p, fc_.dither, next_dither_seed());
  const bool cm = cmvn_shift_ && cmvn_dim_ == W;
  launch_lfr_cmvn_pad(stream_, (const float*)ws_fbank_.p, meta + 4, t80d, 1, t_lfr, m, nn_, fc_.n_mels, cmvn_shift_,
                      cmvn_scale_, cm ? 1 : 0, 0, (float*)ws_speech_.p);
  PF_HIP(hipMemcpyAsync(feats.data(), ws_speech_.p, feats.size() * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));
}

// ------------------------------------------------------------------ encoder ---------------
void Engine::build_pe(int T) {
  if (T <= pe_T_) return;
  const int F = mc_.feat_dim, half = F / 2;
  const int Tn = (int)round_up(T, 256);
  std::vector<float> pe((size_t)Tn * F);
  // SinusoidalPositionEncoder.encode in float32: inv_timescales = exp(i * -(ln 1e4 / (half-1)))
  const float inc = (float)(std::log(10000.0) / (double)(half - 1));
  std::vector<float> inv(half);
  for (int i = 0; i < half; ++i) inv[i] = std::exp((float)i * (-inc));
  for (int t = 0; t < Tn; ++t) {
    const float pos = (float)(t + 1);
    for (int i = 0; i < half; ++i) {
      const float st = pos * inv[i];
      pe[(size_t)t * F + i] = (float)std::sin((double)st);
      pe[(size_t)t * F + half + i] = (float)std::cos((double)st);
    }
  }
  ensure(ws_pe_, pe.size() * 4);
  PF_HIP(hipMemcpyAsync(ws_pe_.p, pe.data(), pe.size() * 4, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipStreamSynchronize(stream_));
  pe_T_ = Tn;
}

// One SAN-M encoder layer.  Fused layer tail = 3 launches (2 with the Q | K | V tail of the previous layer): QKV GEMM ->
// attention -> out-projection + FSMN memory + norm2 + FFN block + the NEXT LayerNorm `nx`.  Row-complete form = 5 launches:
// [LayerNorm fused into the previous launch] QKV GEMM -> attention -> row-complete out-projection (+ bias + residual +
// FSMN memory from the V slice + LayerNorm norm2 -> xn16) -> FFN-up (blocked hidden) -> row-complete FFN-down (+ bias +
// residual + `nx` -> its outputs).  Short-input and un-fused forms: see the predicates below.
// Entry: xn16_ holds LayerNorm norm1 of the residual stream (written by the previous layer's FFN-down, by the
// position-encoding kernel for layer 0, or by the stand-alone LayerNorm for the first tp layer).
void Engine::enc_layer(const EncLayer& L, int first, const float* speech_dev, int B, int T, const EncNext& nx) {
  const int D = mc_.d_model, M = B * T, F = mc_.ffn;
  const float qscale = 1.0f / std::sqrt((float)(D / mc_.heads));
  const int lda = first ? L.qkv.Kpad : D;
  // ---- which form this layer takes, from (M, T), the FSMN kernel size, the FFN width and the layer's weight images
  // short inputs (M <= 512 rows): every GEMM goes to k_gemm_small.hip, which has no row-complete epilogue and no blocked
  // layout but takes the FSMN memory as an epilogue term and the LayerNorm behind FFN-down in its reduction
  const bool small = M <= gemm_small_max_rows() && small_ws_;
  // the split FFN-down form must really apply to (M, F) — e.g. F = 4096 needs 16 splits, whose partials outgrow the
  // scratch beyond 256 rows: then the regular kernels run instead of failing the utterance
  auto split_ok = [&](int rows, const Lin& w2, const half_t* Aop) {
    GemmSmallArgs t{};
    t.M = rows; t.N = w2.N; t.K = w2.Kpad; t.A = Aop; t.lda = w2.Kpad; t.W = w2.w; t.ldw = w2.Kpad; t.ws = small_ws_;
    t.post_ln_g = nx.ln.g; t.post_ln_b = nx.ln.b;
    return gemm_small_applicable(t);
  };
  const bool short_form = small && F > 576 && mc_.kernel == 11 && split_ok(M, L.w2, h16_);
  // row-complete form: out-projection and FFN-down carry bias + residual + (FSMN memory) + the LayerNorm behind them.
  // Otherwise (FSMN kernel size other than 11, utterances shorter than 8 frames, a short input the form above does not
  // take) the un-fused sequence runs
  const bool rc = mc_.kernel == 11 && T >= 8 && !small;
  // Q | K blocked + V row-major from the persistent 256 x 192 kernel when the row-complete out-projection (the reader of
  // the row-major V) runs and the launch has at least a round of tiles
  // (chosen by idle rounds: 32 x 500 rows are 504 tiles = 1.97 rounds on 256 CUs — 1.88 vs 2.06 ms per step for the 50 layers;
  // SenseVoice's 10 944 rows are 344 tiles = 1.34 rounds: 2.45 vs 2.30 ms alone, but 10.19 vs 10.73 ms per step with two steps in
  // flight — the second engine's kernels take the CUs its short second round leaves — so the fill bar is 60 %)
  const int qt = 8 * cdiv(M, 256);
  const bool split = rc && L.qkv_p && qt >= qkv_split_min_tiles_ && qt * 100 >= qkv_split_min_fill_ * (int)round_up(qt, cus_) &&
                     gemm_qkvp_applicable(M, L.qkv.Kpad, lda, L.qkv.Kpad, D);
  // fused layer tail: everything behind the attention in one launch per 64-row tile (out_wt is only built beside ffn_wt)
  const bool fused = rc && L.out_wt && M >= ffn_fused_min_rows_;
  // ... with the NEXT layer's Q | K | V projection behind the block when that layer would take the same (blocked-layout)
  // path on the same rows: LayerNorm_next(x) then never visits HBM either
  const bool tail = fused && split && nx.next && nx.next->qkv_t && nx.next->out_wt && nx.n16 == xn16_ && !nx.n32;

  if (first == 1) {
    prof_begin("layernorm", 0);
    launch_posenc_ln_tab(stream_, speech_dev, B, T, mc_.feat_dim, std::sqrt((float)D), (const float*)ws_pe_.p,
                         L.norm1.g, L.norm1.b, xn16_, lda);
    prof_end("layernorm");
  } else if (first == 2) {
    // streaming path: the caller scaled and position-encoded the chunk already (OnlineStream.cs GetDecodeChunk)
    prof_begin("layernorm", 0);
    launch_layernorm(stream_, speech_dev, M, mc_.feat_dim, L.norm1.g, L.norm1.b, xn16_, lda, nullptr, 0);
    prof_end("layernorm");
  }
  AttnArgs a{};
  a.q = qkv16_; a.k = qkv16_ + D; a.v = qkv16_ + 2 * D; a.o = ctx16_;
  a.q_bstride = a.k_bstride = a.v_bstride = (int64_t)T * 3 * D;
  a.q_rstride = a.k_rstride = a.v_rstride = 3 * D;
  a.o_bstride = (int64_t)T * D; a.o_rstride = D;
  a.B = B; a.H = mc_.heads; a.Lq = T; a.Lk = T;
  if (short_form) {
    // 7 launches: QKV | attention | out-projection + FSMN memory + residual | norm2 | FFN-up | FFN-down partials | their
    // sum + bias + residual + the LayerNorm behind the block (next norm1 / after_norm)
    gemm("gemm_qkv", L.qkv, xn16_, lda, M, nullptr, 0, qkv16_, 3 * D, nullptr, 0, nullptr, 0, false, D, qscale);
    prof_begin("attn_self", 4.0 * B * (double)T * T * D);
    launch_attention(stream_, a);
    prof_end("attn_self");
    GemmSmallArgs o{};
    o.M = M; o.A = ctx16_; o.lda = D; o.out_f32 = x_; o.ldc32 = D;
    if (!first) { o.resid = x_; o.ldr = D; }
    o.fsmn_v = qkv16_ + 2 * D; o.ldv = 3 * D; o.fsmn_wT = L.fsmn_wT; o.fsmn_k = 11; o.T = T;
    gemm_small_call("gemm_out", L.out, o);
    prof_begin("layernorm", 0);
    launch_layernorm(stream_, x_, M, D, L.norm2.g, L.norm2.b, xn16_, D, nullptr, 0);
    prof_end("layernorm");
    gemm("gemm_ffn1", L.w1, xn16_, D, M, nullptr, 0, h16_, F, nullptr, 0, nullptr, 0, true, 0, 1.f);
    GemmSmallArgs dn{};
    dn.M = M; dn.A = h16_; dn.lda = F; dn.resid = x_; dn.ldr = D;
    if (nx.keep_x) { dn.out_f32 = x_; dn.ldc32 = D; }
    dn.post_ln_g = nx.ln.g; dn.post_ln_b = nx.ln.b; dn.post_n16 = nx.n16; dn.ldn16 = D; dn.post_n32 = nx.n32; dn.ldn32 = D;
    gemm_small_call("gemm_ffn2", L.w2, dn);
    return;
  }
  const half_t* v16 = qkv16_ + 2 * D;
  int ldv = 3 * D;
  const bool pre = qkv_done_;                                  // written by the previous layer's launch (its Q | K | V tail)
  qkv_done_ = false;
  PF_CHECK(!pre || split, PF_ERR_DEVICE, "encoder: a projected Q | K | V without its consumer");
  const int64_t Mp = round_up((int64_t)M, 128) + 128;          // rows of every encoder buffer (>= round_up(M, 256))
  // two V buffers: the fused launch of layer l reads V_l (FSMN window: rows of NEIGHBOURING tiles too) and writes V_{l+1}
  half_t* const vbufs[2] = {qkv16_ + (size_t)Mp * 2 * D, h16_};
  if (split) {
    half_t* vbuf = vbufs[v_pp_];
    if (!pre) {
      prof_begin("gemm_qkv", 2.0 * M * (double)L.qkv.N * L.qkv.K);
      launch_gemm_qkvp(stream_, xn16_, lda, L.qkv_p, L.qkv.Kpad, L.qkv_bias_p, M, L.qkv.Kpad, qscale, qkv16_, vbuf, D);
      prof_end("gemm_qkv");
    }
    a.q = qkv16_; a.k = qkv16_; a.qk_blocked = 1; a.blk_groups = 2 * D / 8; a.blk_brows = T; a.blk_kgrp = D / 8;
    a.v = vbuf; a.v_bstride = (int64_t)T * D; a.v_rstride = D;
    v16 = vbuf; ldv = D;
  } else {
    gemm("gemm_qkv", L.qkv, xn16_, lda, M, nullptr, 0, qkv16_, 3 * D, nullptr, 0, nullptr, 0, false, D, qscale);
  }
  prof_begin("attn_self", 4.0 * B * (double)T * T * D);
  launch_attention(stream_, a);
  prof_end("attn_self");
  if (fused) {
    // out-projection + bias + residual + FSMN memory + norm2 + the whole FFN block + the NEXT LayerNorm: ONE launch per 64-row
    // tile (k_ffn.hip, OP = 1): norm2's result never leaves LDS, x_mid goes through a scratch the same lanes read back
    FfnFusedArgs f{};
    f.ctx = ctx16_; f.lda_c = D; f.Wot = L.out_wt; f.bo = L.out.bias; f.fsmn_v = v16; f.ldv = ldv; f.fsmn_wT = L.fsmn_wT; f.T = T;
    f.ln2_g = L.norm2.g; f.ln2_b = L.norm2.b;
    f.Wt = L.ffn_wt; f.b1 = L.w1.bias; f.b2 = L.w2.bias; f.M = M;
    f.resid = first ? nullptr : x_; f.ldr = D; f.out_x = nx.keep_x ? x_ : nullptr; f.ldx = D;
    f.ln_g = nx.ln.g; f.ln_b = nx.ln.b; f.eps = 1e-12f; f.out_n16 = nx.n16; f.ldn16 = D; f.out_n32 = nx.n32; f.ldn32 = D;
    double flops = 2.0 * M * (double)D * D + 4.0 * M * (double)D * F;
    if (tail) {
      f.Wqt = nx.next->qkv_t; f.bq = nx.next->qkv.bias; f.out_qk = qkv16_; f.out_v = vbufs[v_pp_ ^ 1]; f.ldvo = D; f.qscale = qscale;
      f.out_n16 = nullptr;
      flops += 2.0 * M * 3.0 * D * D;
    }
    prof_begin("gemm_outffn", flops);
    launch_ffn_fused(stream_, f);
    prof_end("gemm_outffn");
    if (tail) { qkv_done_ = true; v_pp_ ^= 1; }
    return;
  }
  if (rc) {
    GemmRcArgs g{};
    g.A = ctx16_; g.lda = D; g.W = L.out.w; g.ldw = L.out.Kpad; g.bias = L.out.bias; g.M = M; g.K = L.out.Kpad;
    g.resid = first ? nullptr : x_; g.ldr = D; g.out_x = x_; g.ldx = D;
    g.fsmn_v = v16; g.ldv = ldv; g.fsmn_wT = L.fsmn_wT; g.fsmn_k = mc_.kernel; g.T = T;
    g.ln_g = L.norm2.g; g.ln_b = L.norm2.b; g.eps = 1e-12f; g.out_n16 = xn16_; g.ldn16 = D;
    prof_begin("gemm_out", 2.0 * M * (double)D * D);
    launch_gemm_rc(stream_, g);
    prof_end("gemm_out");
  } else {
    prof_begin("fsmn", 0);
    launch_fsmn_enc(stream_, qkv16_ + 2 * D, 3 * D, L.fsmn_wT, B, T, D, mc_.kernel, fsm_);
    prof_end("fsmn");
    gemm("gemm_out", L.out, ctx16_, D, M, x_, D, nullptr, 0, first ? nullptr : x_, D, fsm_, D, false, 0, 1.f);
    prof_begin("layernorm", 0);
    launch_layernorm(stream_, x_, M, D, L.norm2.g, L.norm2.b, xn16_, D, nullptr, 0);
    prof_end("layernorm");
  }
  // the FFN hidden lives in the blocked activation layout (kernels.h): FFN-up stores its fragments as whole
  // lines without the LDS transposition, FFN-down's LDS-DMA reads 1 KiB contiguous pieces
  const int blk = small ? 0 : 1;
  gemm("gemm_ffn1", L.w1, xn16_, D, M, nullptr, 0, h16_, F, nullptr, 0, nullptr, 0, true, 0, 1.f, true, blk);
  if (rc) {
    // row-complete FFN-down (+ the next LayerNorm): 53.6 us against 47.6 + 9-11 us for the persistent 256 x 128 kernel +
    // its LayerNorm launch
    GemmRcArgs f{};
    f.A = h16_; f.lda = F; f.a_blocked = 1; f.W = L.w2.w; f.ldw = L.w2.Kpad; f.bias = L.w2.bias; f.M = M; f.K = L.w2.Kpad;
    f.resid = x_; f.ldr = D; f.out_x = nx.keep_x ? x_ : nullptr; f.ldx = D;
    f.ln_g = nx.ln.g; f.ln_b = nx.ln.b; f.eps = 1e-12f; f.out_n16 = nx.n16; f.ldn16 = D; f.out_n32 = nx.n32; f.ldn32 = D;
    prof_begin("gemm_ffn2", 2.0 * M * (double)D * F);
    launch_gemm_rc(stream_, f);
    prof_end("gemm_ffn2");
    return;
  }
  gemm("gemm_ffn2", L.w2, h16_, F, M, x_, D, nullptr, 0, x_, D, nullptr, 0, false, 0, 1.f, true, blk ? 2 : 0);
  prof_begin("layernorm", 0);
  launch_layernorm(stream_, x_, M, D, nx.ln.g, nx.ln.b, nx.n16, D, nx.n32, D);
  prof_end("layernorm");
}

void Engine::encoder(const float* speech_dev, int B, int T, bool pre_encoded) {
  const int D = mc_.d_model, F = mc_.ffn;
  const int64_t M = (int64_t)B * T;
  const int64_t Mp = round_up(M, 128) + 128;
  PF_CHECK(M < (1ll << 31) / (3 * D), PF_ERR_INVALID_ARG, "batch too large for 32-bit row indexing");
  if (!pre_encoded) build_pe(T);
  const int k0 = enc_.empty() ? D : enc_[0].qkv.Kpad;
  // carve the encoder arena
  size_t off = 0;
  const Carve carve{off};
  const size_t o_x = carve(Mp * D * 4), o_xn = carve(Mp * std::max(k0, D) * 2), o_qkv = carve(Mp * 3 * D * 2);
  const size_t o_ctx = carve(Mp * D * 2), o_fsm = carve(Mp * D * 4), o_h = carve(Mp * std::max(F, 3 * D) * 2);
  const size_t o_H32 = carve(Mp * D * 4), o_H16 = carve(Mp * D * 2);
  const CifCarve o_cif(carve, B, T + 1);
  ensure(ws_enc_, off);
  char* base = (char*)ws_enc_.p;
  x_ = (float*)(base + o_x); xn16_ = (half_t*)(base + o_xn); qkv16_ = (half_t*)(base + o_qkv);
  ctx16_ = (half_t*)(base + o_ctx); fsm_ = (float*)(base + o_fsm); h16_ = (half_t*)(base + o_h);
  H32_ = (float*)(base + o_H32); H16_ = (half_t*)(base + o_H16);
  alphas_ = (float*)(base + o_cif.al); plan_ = o_cif.plan(base);

  // the LayerNorm that FOLLOWS layer i's FFN-down is the next layer's norm1, or after_norm behind the last one
  const bool has_tp = !tp_.empty();
  qkv_done_ = false; v_pp_ = 0;
  for (size_t i = 0; i < enc_.size(); ++i) {
    EncNext nx;
    if (i + 1 < enc_.size()) { nx.ln = enc_[i + 1].norm1; nx.n16 = xn16_; nx.keep_x = true; nx.next = &enc_[i + 1]; }
    else if (has_tp) { nx.ln = enc_after_; nx.n32 = x_; nx.keep_x = false; }     // after_norm output = the tp residual stream
    else { nx.ln = enc_after_; nx.n16 = H16_; nx.n32 = H32_; nx.keep_x = false; }
    enc_layer(enc_[i], i == 0 ? (pre_encoded ? 2 : 1) : 0, speech_dev, B, T, nx);
  }
  if (has_tp) {
    prof_begin("layernorm", 0);
    launch_layernorm(stream_, x_, M, D, tp_[0].norm1.g, tp_[0].norm1.b, xn16_, D, nullptr, 0);
    prof_end("layernorm");
    for (size_t i = 0; i < tp_.size(); ++i) {
      EncNext nx;
      if (i + 1 < tp_.size()) { nx.ln = tp_[i + 1].norm1; nx.n16 = xn16_; nx.keep_x = true; nx.next = &tp_[i + 1]; }
      else { nx.ln = tp_norm_; nx.n16 = H16_; nx.n32 = H32_; nx.keep_x = false; }
      enc_layer(tp_[i], 0, nullptr, B, T, nx);
    }
  }
}

// ------------------------------------------------------------------ CIF + decoder ---------
// FFN-up of a decoder block and the LayerNorm(F) behind it: leaves the normalised hidden in h16.  FFN-up writes the
// hidden as f16 (ReLU output, one rounding — the oracle's 16-bit mode rounds at the same point) and the LayerNorm runs
// in place on it: 40 -> 18 us for the GEMM (no fp32 row-segment epilogue) and a third of the LayerNorm's bytes at
// M = 5344.
void Engine::dec_ffn_hidden(const char* cls, const Lin& w1, const LNp& fn, const half_t* xn16, int lda, int rows, half_t* h16) {
  const int F = w1.N;
  gemm(cls, w1, xn16, lda, rows, nullptr, 0, h16, F, nullptr, 0, nullptr, 0, true, 0, 1.f);
  prof_begin("layernorm", 0);
  launch_layernorm_f16(stream_, h16, rows, F, fn.g, fn.b, h16);
  prof_end("layernorm");
}

// cross-attention of a decoder layer: q / o dense [B * L, D] f16, K / V rows kv_rs apart and kv_bs per utterance (0: shared)
AttnArgs Engine::cross_attn_args(const half_t* q, const half_t* k, const half_t* v, int kv_rs, int64_t kv_bs, half_t* o, int B, int L, int Lk) const {
  const int D = mc_.d_model;
  AttnArgs a{};
  a.q = q; a.q_bstride = (int64_t)L * D; a.q_rstride = D;
  a.k = k; a.v = v;
  a.k_bstride = a.v_bstride = kv_bs; a.k_rstride = a.v_rstride = kv_rs;
  a.o = o; a.o_bstride = (int64_t)L * D; a.o_rstride = D;
  a.B = B; a.H = mc_.heads; a.Lq = L; a.Lk = Lk;
  return a;
}

DecBufs Engine::carve_dec16(Arena& a, int64_t rows, int F, bool with_h32) {
  const int D = mc_.d_model;
  DecBufs d;
  d.x = a.take<float>((size_t)rows * D * 4); d.xn16 = a.take<half_t>((size_t)rows * D * 2);
  if (with_h32) d.h32 = a.take<float>((size_t)rows * F * 4);      // math_mode 2 runs the bias decoder in this arena (decoder_int8)
  d.h16 = a.take<half_t>((size_t)rows * F * 2); d.t32 = a.take<float>((size_t)rows * D * 4); d.tn32 = a.take<float>((size_t)rows * D * 4);
  d.q16 = a.take<half_t>((size_t)rows * D * 2); d.ctx16 = a.take<half_t>((size_t)rows * D * 2);
  return d;
}

// The decoder stack in its plain form, 9 launches a layer: norm1 | FFN-up (f16 hidden) | LayerNorm(F) in place | FFN-down | norm2 |
// FSMN memory + residual | norm3 | q | cross attention | out-projection + residual; then the final block's FFN (-> t32).  The SeACo
// bias decoder and the streaming seam run it; the ASR decoder's fused and short-input forms are asr_decoder_f16's own walk.
void Engine::decoder16(const DecStack& S, const DecRun& r) {
  const int D = mc_.d_model, R = r.B * r.L;
  const DecBufs& b = r.b;
  const float qscale = 1.0f / std::sqrt((float)(D / mc_.heads));
  const size_t cache = (size_t)r.B * D * (S.fsmn_k - 1);   // one layer's slice of the streaming caches
  auto norm = [&](const float* x, const LNp& ln, half_t* n16, float* n32) {
    prof_begin("layernorm", 0);
    launch_layernorm(stream_, x, R, D, ln.g, ln.b, n16, n16 ? D : 0, n32, n32 ? D : 0);
    prof_end("layernorm");
  };
  auto ffn_dec = [&](const LNp& n1, const Lin& w1, const LNp& fn, const Lin& w2) {
    norm(b.x, n1, b.xn16, nullptr);
    dec_ffn_hidden(r.cls_ffn1, w1, fn, b.xn16, D, R, b.h16);
    gemm(r.cls_ffn2, w2, b.h16, S.ffn, R, b.t32, D, nullptr, 0, nullptr, 0, nullptr, 0, false, 0, 1.f, false);
  };
  for (size_t i = 0; i < S.layers.size(); ++i) {
    const DecLayer& Lr = S.layers[i];
    ffn_dec(Lr.norm1, Lr.w1, Lr.ffn_norm, Lr.w2);
    norm(b.t32, Lr.norm2, nullptr, b.tn32);
    prof_begin("fsmn", 0);
    if (r.cache_in)
      launch_fsmn_dec_stream(stream_, b.tn32, Lr.fsmn_wT, r.token_num, r.cache_in + i * cache, r.B, r.L, D, S.fsmn_k, b.x, r.cache_out + i * cache);
    else
      launch_fsmn_dec(stream_, b.tn32, Lr.fsmn_wT, r.token_num, r.B, r.L, D, S.fsmn_k, b.x);
    prof_end("fsmn");
    norm(b.x, Lr.norm3, b.xn16, nullptr);
    gemm(r.cls_q, Lr.q, b.xn16, D, R, nullptr, 0, b.q16, D, nullptr, 0, nullptr, 0, false, D, qscale);
    const half_t* k16 = (const half_t*)r.kv + i * 2 * D;
    prof_begin(r.cls_attn, 4.0 * r.B * (double)r.L * r.Lk * D);
    launch_attention(stream_, cross_attn_args(b.q16, k16, k16 + D, r.kv_rs, r.kv_bs, b.ctx16, r.B, r.L, r.Lk));
    prof_end(r.cls_attn);
    gemm(r.cls_out, Lr.out, b.ctx16, D, R, b.x, D, nullptr, 0, b.x, D, nullptr, 0, false, 0, 1.f);
  }
  ffn_dec(S.final_norm1, S.final_w1, S.final_ffn_norm, S.final_w2);
}

// The predictor's alpha stage, one body for the pipeline, the streaming seam and pf_op_cif_alphas: conv1d(k = l + r + 1) as an
// im2col GEMM with ReLU, then alpha = relu(sigmoid(y . w + b0) * smooth - noise) and the tail weight.  H16 [B*T, D]; col16 holds
// [B*T, taps*D] and conv32 [B*T, D], both in padded rows (round_up(B*T, 128) + 128).  scan: the plan the fire scan fills
// behind it, inside the same profile bracket as the pipeline has always had it, or nullptr for the alphas alone.
void Engine::cif_alpha_stage(const half_t* H16, int B, int T, half_t* col16, float* conv32, float* alphas, const CifPlan* scan) {
  const int D = mc_.d_model, M = B * T, taps = mc_.cif_l_order + mc_.cif_r_order + 1;
  prof_begin("cif_misc", 0);
  launch_cif_im2col(stream_, H16, B, T, D, mc_.cif_l_order, mc_.cif_r_order, col16);
  prof_end("cif_misc");
  gemm("gemm_cif", cif_conv_, col16, taps * D, M, conv32, D, nullptr, 0, nullptr, 0, nullptr, 0, true, 0, 1.f);
  prof_begin("cif_misc", 0);
  launch_cif_alpha(stream_, conv32, B, T, D, cif_out_w_, cif_out_b_, mc_.cif_smooth, mc_.cif_noise, mc_.cif_tail, alphas);
  if (scan) {
    if (mc_.cif_cumsum) launch_cif_scan_cumsum(stream_, alphas, B, T + 1, *scan);
    else launch_cif_scan(stream_, alphas, B, T + 1, mc_.cif_threshold, *scan);
  }
  prof_end("cif_misc");
}

// ---- the stages of forward_device behind the encoder
// The predictor: alphas, the fire scan into plan_, the counts on their way to the host; then the timestamp head starts.  f16 and
// int8 run the same stage (the Conv1d is a Conv node, which quantize_dynamic leaves alone, and so are the head's nodes: it is
// run with op_types_to_quantize = ["MatMul"]) with the head beside the decoder; the fp32 graph runs its own forms in line.
void Engine::predictor(int B, int T) {
  if (fp32_mode_) {
    cif_alpha_stage32(H32_, B, T, col32_, fsm_, alphas_);
    if (mc_.cif_cumsum) launch_cif_scan_cumsum(stream_, alphas_, B, T + 1, plan_);
    else launch_cif_scan(stream_, alphas_, B, T + 1, mc_.cif_threshold, plan_);
    export_plan(B);
    if (mc_.timestamp_head) timestamp_head_fp32(B, T);
    return;
  }
  if (ev_enc_) PF_HIP(hipEventRecord(ev_enc_, stream_));     // the encoder output exists: all the timestamp head's GEMMs and its recurrence need
  // reuse the FFN hidden buffer for the [M, 3D] operand and the FSMN buffer for the fp32 conv output
  cif_alpha_stage(H16_, B, T, h16_, fsm_, alphas_, &plan_);
  export_plan(B);
  if (mc_.timestamp_head) start_timestamp_head(B, T);
}

// The cross-attention K/V projections of all decoder layers depend on the encoder output only, not on the decoder
// length: they go out BEFORE the length is read back and keep the device busy during the host round trip (and,
// in a multi-device group, during the rendez-vous that agrees on the batch-wide length).
void Engine::dec_kv_ahead(int B, int T) {
  const int D = mc_.d_model, M = B * T, nd = (int)dec_.layers.size();
  const int64_t Mp = round_up(M, 128) + 128;
  const int ldkv = std::max(nd, 1) * 2 * D;
  ensure(ws_kv_, (size_t)Mp * ldkv * 2);
  if (nd > 0)
    gemm("gemm_dec_kv", dec_.kv_all, H16_, D, M, nullptr, 0, (half_t*)ws_kv_.p, ldkv, nullptr, 0, nullptr, 0, false, 0, 1.f);
}

// The path's only host sync: the decoder length L is data dependent.  The read-back waits for the CIF scan alone (whatever
// was queued behind export_plan's event, nothing waits for).
int Engine::decoder_length(int B, int T) {
  int32_t L = read_back_plan(B);
  if (fp32_mode_ && mc_.timestamp_head) PF_HIP(hipStreamSynchronize(stream_));   // (the in-line head's results are read by the caller as before)
  if (l_hook_) L = l_hook_(L);                       // shard of a multi-device batch: the batch-wide maximum
  last_.B = B; last_.L = L; last_.V = mc_.vocab; last_.T = T;
  last_.ids.assign((size_t)B * L, 0);
  return L;
}

// The CIF embeds [B * L, D] into the walk's residual stream; with hot words the SeACo bias decoder starts from them too and
// they are set aside, with room for the ASR decoder's after_norm hidden behind them.
void Engine::cif_embeds(DecStage& d, int B, int T, int L, const char* cls) {
  const int D = mc_.d_model;
  if (cls) prof_begin(cls, 0);
  if (mc_.cif_cumsum) launch_cif_gather_cumsum(stream_, H32_, alphas_, B, T, D, T + 1, plan_, L, d.b.x);
  else launch_cif_gather(stream_, H32_, B, T, D, T + 1, plan_, L, d.b.x);
  if (cls) prof_end(cls);
  if (!(mc_.seaco && n_hotwords_ > 0)) return;
  ensure(ws_seaco_in_, (size_t)2 * d.rows * D * 4);
  d.e0 = (float*)ws_seaco_in_.p;
  d.hid = d.e0 + (size_t)d.rows * D;
  PF_HIP(hipMemcpyAsync(d.e0, d.b.x, (size_t)B * L * D * 4, hipMemcpyDeviceToDevice, stream_));
}

void Engine::finish(int B, int L, bool want_logits, const DecStage* d, const char* cls) {
  const int64_t rows = (int64_t)B * L;
  if (cls) prof_begin(cls, 0);
  launch_argmax(stream_, logits_, rows, mc_.vocab, logits_ld_, argmax_mode(want_logits), ids_dev_, score_buf(rows));
  if (cls) prof_end(cls);
  if (d && d->e0) {
    if (fp32_mode_) seaco_head_fp32(B, L, d->e0, d->hid, want_logits);
    else seaco_head(B, L, d->e0, d->hid, want_logits);
  }
  join_ts();
  PF_HIP(hipMemcpyAsync(last_.ids.data(), ids_dev_, (size_t)rows * 8, hipMemcpyDeviceToHost, stream_));
  queue_decode_results(B, L);
}

DecStage Engine::dec_arena_f16(int B, int T, int L) {
  const int D = mc_.d_model, Md = B * L;
  DecStage d;
  d.rows = round_up(Md, 128) + 128;
  d.kv = ws_kv_.p;
  d.b = carve_into(ws_dec_, kAlign, [&](Arena& a) {
    const DecBufs b = carve_dec16(a, d.rows, mc_.ffn, false);
    logits_ = a.take<float>((size_t)d.rows * round_up(mc_.vocab, 4) * 4); ids_dev_ = a.take<int64_t>((size_t)Md * 8);
    d.x_alt = a.take<float>(d.rows * D * 4);
    return b;
  });
  return d;
}

// The f16 ASR decoder in its fused and short-input forms, then the vocabulary product.
void Engine::asr_decoder_f16(DecStage& d, int B, int T, int L) {
  const int D = mc_.d_model, F = mc_.ffn, V = mc_.vocab, Md = B * L, nd = (int)dec_.layers.size();
  const int ldkv = std::max(nd, 1) * 2 * D;
  const half_t* kv16 = (const half_t*)d.kv;
  const DecBufs& w = d.b;
  float* xd = w.x; float* xd_alt = d.x_alt;          // the residual stream ping-pongs when the out-projection rides in front of the next FFN launch
  half_t* xdn16 = w.xn16; half_t* hd16 = w.h16; float* t32 = w.t32; float* tn32 = w.tn32;
  half_t* qd16 = w.q16; half_t* ctxd16 = w.ctx16; float* hid32 = d.hid;
  const float qscale = 1.0f / std::sqrt((float)(D / mc_.heads));

  // Generic decoder layer = 9 launches: norm1 | FFN-up (f16 hidden) | LayerNorm(2048) in place | FFN-down | norm2 | FSMN
  // memory + norm3 (one kernel) | q | cross attention | out-projection + residual.
  // ---- which forms the decoder takes, from Md, the FFN width and the layers' weight images
  // short inputs: the split FFN-down form of k_gemm_small.hip with the LayerNorm behind the block in its reduction
  bool dsmall = Md <= gemm_small_max_rows() && small_ws_ && F > 576;
  if (dsmall) {                                        // the split FFN-down form must apply to (Md, F), else the regular kernels
    GemmSmallArgs t{};
    t.M = Md; t.N = D; t.K = dec_.final_w2.Kpad; t.A = hd16; t.lda = F; t.W = dec_.final_w2.w; t.ldw = dec_.final_w2.Kpad;
    t.ws = small_ws_; t.post_ln_g = dec_.after.g; t.post_ln_b = dec_.after.b;
    dsmall = gemm_small_applicable(t);
  }
  // out-projection chain (k_ffn.hip, OP = 2): layer i's cross-attention out-projection + residual + the next norm1 run in
  // front of the NEXT block's split FFN launch; `pend` = the layer whose context (ctxd16) still waits for its projection
  bool chain = !dsmall && dec_.final_img != nullptr;
  for (int i = 0; i < nd && chain; ++i) chain = dec_.layers[i].ffn_img && dec_.layers[i].out_wt;
  const DecLayer* pend = nullptr;
  // ffn_dec: norm1 -> w_1 + ReLU -> LayerNorm(2048) -> w_2 (no bias) [-> LayerNorm `post`]; leaves t32 (unfused) or
  // post(t) in n32 / n16
  bool mid_next = false;                                // the coming ffn_dec call leaves its shares to launch_dec_mid
  auto ffn_dec = [&](const LNp& n1, const Lin& w1, const LNp& fn, const Lin& w2, const half_t* img, const LNp& post, float* n32, half_t* n16) {
    if (img && !dsmall) {
      // norm1 | the whole block in the split form of the fused FFN kernel + its finishing pass (LayerNorm over the hidden
      // applied from row statistics, then `post`): 2 launches for FFN-up | LayerNorm(2048) | FFN-down | LayerNorm
      if (!pend) {
        prof_begin("layernorm", 0);
        launch_layernorm(stream_, xd, Md, D, n1.g, n1.b, xdn16, D, nullptr, 0);
        prof_end("layernorm");
      }
      ensure(ws_decffn_, ffn_dec_workspace_bytes(Md));
      FfnDecArgs f{};
      f.A = xdn16; f.lda = D; f.img = img; f.ws = ws_decffn_.p; f.M = Md; f.eps_hidden = 1e-12f;
      f.ln_g = post.g; f.ln_b = post.b; f.eps = 1e-12f; f.n32 = n32; f.ldn32 = D; f.n16 = n16; f.ldn16 = D;
      f.no_finish = mid_next;
      if (pend) {
        f.A = nullptr; f.ctx = ctxd16; f.lda_c = D; f.Wot = pend->out_wt; f.bo = pend->out.bias;
        f.resid = xd; f.ldr = D; f.out_x = xd_alt; f.ldx = D; f.ln1_g = n1.g; f.ln1_b = n1.b; f.eps1 = 1e-12f;
      }
      prof_begin("gemm_dec_ffn", 4.0 * Md * (double)D * F + (pend ? 2.0 * Md * (double)D * D : 0.0));
      launch_ffn_dec(stream_, f);
      prof_end("gemm_dec_ffn");
      if (pend) { std::swap(xd, xd_alt); pend = nullptr; }
      return;
    }
    // generic and short-input forms: norm1 | FFN-up | LayerNorm(2048) in place | FFN-down ...
    prof_begin("layernorm", 0);
    launch_layernorm(stream_, xd, Md, D, n1.g, n1.b, xdn16, D, nullptr, 0);
    prof_end("layernorm");
    dec_ffn_hidden("gemm_dec_ffn1", w1, fn, xdn16, D, Md, hd16);
    if (dsmall) {
      // ... as partials | their sum + the LayerNorm behind it
      GemmSmallArgs dn{};
      dn.M = Md; dn.A = hd16; dn.lda = F;
      dn.post_ln_g = post.g; dn.post_ln_b = post.b; dn.post_n16 = n16; dn.ldn16 = D; dn.post_n32 = n32; dn.ldn32 = D;
      gemm_small_call("gemm_dec_ffn2", w2, dn, false);
      return;
    }
    // ... | the LayerNorm behind it.  (The row-complete GEMM with that LayerNorm as its epilogue runs on 84 CUs only at
    // M = B * L = 5344: 47 against 29.5 + 5.6 us.)
    gemm("gemm_dec_ffn2", w2, hd16, F, Md, t32, D, nullptr, 0, nullptr, 0, nullptr, 0, false, 0, 1.f, false);
    prof_begin("layernorm", 0);
    launch_layernorm(stream_, t32, Md, D, post.g, post.b, n16, D, n32, n32 ? D : 0);
    prof_end("layernorm");
  };

  for (int i = 0; i < nd; ++i) {
    const DecLayer& Lr = dec_.layers[i];
    // round 6: the finishing pass of the split FFN form, norm2, the FSMN memory, the residual, norm3 and the q-projection in ONE
    // launch (k_decmid.hip): a decoder layer = split FFN | middle | cross-attention
    const bool mid = dec_mid_ && Lr.ffn_img && Lr.q_wt && !dsmall && mc_.kernel == 11;
    mid_next = mid;
    ffn_dec(Lr.norm1, Lr.w1, Lr.ffn_norm, Lr.w2, Lr.ffn_img, Lr.norm2, tn32, nullptr);
    mid_next = false;
    bool mid_done = false;
    if (mid) {
      DecMidArgs m{};
      m.ws = ws_decffn_.p; m.img = Lr.ffn_img; m.splits = 0; m.eps_hidden = 1e-12f;
      m.n2_g = Lr.norm2.g; m.n2_b = Lr.norm2.b; m.eps2 = 1e-12f;
      m.fsmn_wT = Lr.fsmn_wT; m.k = mc_.kernel; m.token_num = plan_.token_num; m.B = B; m.L = L;
      m.x = xd; m.n3_g = Lr.norm3.g; m.n3_b = Lr.norm3.b;
      m.Wqt = Lr.q_wt; m.bq = Lr.q.bias; m.qscale = qscale; m.q16 = qd16; m.ldq = D;
      prof_begin("dec_mid", 2.0 * Md * (double)D * D);
      mid_done = launch_dec_mid(stream_, m);
      prof_end("dec_mid");
      PF_CHECK(mid_done, PF_ERR_UNSUPPORTED, "decoder: the fused middle launch does not cover this geometry");
    }
    bool fused = mid_done;
    if (!mid_done) {
      prof_begin("fsmn", 0);
      fused = launch_fsmn_dec_ln(stream_, tn32, Lr.fsmn_wT, plan_.token_num, B, L, D, mc_.kernel, xd, Lr.norm3.g, Lr.norm3.b, xdn16);
      prof_end("fsmn");
    }
    if (!fused) {
      prof_begin("fsmn", 0);
      launch_fsmn_dec(stream_, tn32, Lr.fsmn_wT, plan_.token_num, B, L, D, mc_.kernel, xd);
      prof_end("fsmn");
      prof_begin("layernorm", 0);
      launch_layernorm(stream_, xd, Md, D, Lr.norm3.g, Lr.norm3.b, xdn16, D, nullptr, 0);
      prof_end("layernorm");
    }
    if (!mid_done) gemm("gemm_dec_q", Lr.q, xdn16, D, Md, nullptr, 0, qd16, D, nullptr, 0, nullptr, 0, false, D, qscale);
    const half_t* k16 = kv16 + (size_t)i * 2 * D;
    prof_begin("attn_cross", 4.0 * B * (double)L * T * D);
    launch_attention(stream_, cross_attn_args(qd16, k16, k16 + D, ldkv, (int64_t)T * ldkv, ctxd16, B, L, T));
    prof_end("attn_cross");
    if (chain) {
      pend = &Lr;
    } else {
      gemm("gemm_dec_out", Lr.out, ctxd16, D, Md, xd, D, nullptr, 0, xd, D, nullptr, 0, false, 0, 1.f);
    }
  }
  ffn_dec(dec_.final_norm1, dec_.final_w1, dec_.final_ffn_norm, dec_.final_w2, dec_.final_img, dec_.after, hid32, xdn16);
  logits_ld_ = (int)round_up(V, 4);                 // fp32 rows stay 16-byte aligned for any vocabulary size
  gemm("gemm_vocab", dec_.out, xdn16, D, Md, logits_, logits_ld_, nullptr, 0, nullptr, 0, nullptr, 0, false, 0, 1.f);
}

// Starts the BiCIF timestamp head of the current forward: beside the decoder on its own stream (default), or in line.
// Needs ev_enc_ (encoder output) and ev_scan_ (token_num) recorded on stream_.
void Engine::start_timestamp_head(int B, int T) {
  {
    static const int ts_side = env_int("PF_TS_STREAM", 1);
    if (ts_side) {
      // beside the decoder, on its own stream: everything timestamp_head enqueues (two GEMMs, the persistent recurrence,
      // the peaks and their copy to the host) goes to ts_stream_, which waits for the CIF scan (= the encoder too)
      PF_HIP(hipStreamWaitEvent(ts_stream_, ev_enc_, 0));    // (token_num — the CIF scan — is waited for in front of the peaks only)
      std::swap(stream_, ts_stream_);
      ts_defer_copy_ = true;
      try {
        timestamp_head(B, T);
      } catch (...) {
        std::swap(stream_, ts_stream_);
        ts_defer_copy_ = false;
        throw;
      }
      ts_defer_copy_ = false;
      std::swap(stream_, ts_stream_);
      PF_HIP(hipEventRecord(ev_ts_, ts_stream_));
      ts_pending_ = true;
    } else {
      timestamp_head(B, T);
    }
  }
}

void Engine::join_ts() {
  if (!ts_pending_) return;
  PF_HIP(hipStreamWaitEvent(stream_, ev_ts_, 0));      // the caller's sync of stream_ then covers the timestamp head
  if (ts_copy_floats_)
    PF_HIP(hipMemcpyAsync(last_.cif_peak.data(), us_peak_, ts_copy_floats_ * 4, hipMemcpyDeviceToHost, stream_));
  ts_copy_floats_ = 0;
  ts_pending_ = false;
}

// ------------------------------------------------------------------ streaming seams -------
// The two ONNX graphs of the reference's streaming path (AliParaformerAsr/OnlineRecognizer.cs:49-124 EncoderProj,
// :233-334 DecoderProj; sessions built in OnlineModel.cs:23-31).  Their arithmetic is external (FunASR
// paraformer-online export) and restated in oracle/online.py — parity unpinned like every model graph here:
//   encoder: speech [B,Tc,560] (already x sqrt(512) + position-encoded by the caller, OnlineStream.cs:214-221)
//            -> SAN-M encoder WITHOUT the embed stage -> enc [B,Tc,512]; alphas [B,Tc] = CIF weights (no tail frame)
//   decoder: enc, acoustic_embeds [B,L,512] (+ lengths), 16 FSMN caches [B,512,10] -> log-probs [B,L,V], new caches;
//            FSMN memory = conv over cat(cache, x) (no padding), cache_out = its last 10 columns.
void Engine::online_encoder(const float* speech, int B, int Tc, float* enc_out, float* alphas_out) {
  PF_CHECK(speech && enc_out && alphas_out && B > 0 && Tc > 0, PF_ERR_INVALID_ARG, "online_encoder: bad arguments");
  PF_CHECK(mc_.kind != "sensevoicesmall", PF_ERR_UNSUPPORTED, "online_encoder: paraformer models only");
  PF_HIP(hipSetDevice(device_));
  const int D = mc_.d_model, M = B * Tc;
  const size_t n = (size_t)M * mc_.feat_dim;
  ensure(ws_speech_, n * 4);
  PF_HIP(hipMemcpyAsync(ws_speech_.p, speech, n * 4, hipMemcpyHostToDevice, stream_));
  encoder((const float*)ws_speech_.p, B, Tc, true);
  cif_alpha_stage(H16_, B, Tc, h16_, fsm_, alphas_, nullptr);
  PF_HIP(hipMemcpyAsync(enc_out, H32_, (size_t)M * D * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpy2DAsync(alphas_out, (size_t)Tc * 4, alphas_, (size_t)(Tc + 1) * 4, (size_t)Tc * 4, B, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::online_decoder(const float* enc, int B, int Tc, const float* embeds, int L, const int32_t* embeds_len,
                            const float* caches_in, float* logits_out, int64_t* ids_out, float* caches_out) {
  PF_CHECK(enc && embeds && embeds_len && caches_in && ids_out && caches_out && B > 0 && Tc > 0 && L > 0, PF_ERR_INVALID_ARG,
           "online_decoder: bad arguments");
  PF_CHECK(mc_.kernel == 11, PF_ERR_UNSUPPORTED, "online_decoder: FSMN kernel 11 (cache of 10 columns) only");
  PF_HIP(hipSetDevice(device_));
  const int D = mc_.d_model, F = mc_.ffn, V = mc_.vocab, nd = (int)dec_.layers.size(), CW = mc_.kernel - 1;
  const int M = B * Tc, Md = B * L;
  const int64_t Mp = round_up(M, 128) + 128, Mdp = round_up(Md, 128) + 128;
  const int ldV = (int)round_up(V, 4);
  float* e32 = nullptr; half_t* e16 = nullptr; half_t* kv16 = nullptr; float* lg = nullptr; int64_t* ids = nullptr; int32_t* lens = nullptr;
  float* ci = nullptr; float* co = nullptr;
  DecRun r;
  r.b = carve_into(ws_dec_, kAlign, [&](Arena& a) {
    e32 = a.take<float>((size_t)M * D * 4); e16 = a.take<half_t>((size_t)Mp * D * 2); kv16 = a.take<half_t>((size_t)Mp * std::max(nd, 1) * 2 * D * 2);
    const DecBufs d = carve_dec16(a, Mdp, F, false);
    lg = a.take<float>((size_t)Mdp * ldV * 4); ids = a.take<int64_t>((size_t)Md * 8); lens = a.take<int32_t>((size_t)B * 4);
    ci = a.take<float>((size_t)nd * B * D * CW * 4); co = a.take<float>((size_t)nd * B * D * CW * 4);
    return d;
  });
  float* xd = r.b.x; float* t32 = r.b.t32; half_t* xdn16 = r.b.xn16;
  PF_HIP(hipMemsetAsync(e16, 0, (size_t)Mp * D * 2, stream_));
  PF_HIP(hipMemcpyAsync(e32, enc, (size_t)M * D * 4, hipMemcpyHostToDevice, stream_));
  launch_f32_to_f16(stream_, e32, M, D, D, e16, D);
  PF_HIP(hipMemcpyAsync(xd, embeds, (size_t)Md * D * 4, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(lens, embeds_len, (size_t)B * 4, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(ci, caches_in, (size_t)nd * B * D * CW * 4, hipMemcpyHostToDevice, stream_));
  const int ldkv = nd * 2 * D;
  if (nd > 0) gemm("gemm_dec_kv", dec_.kv_all, e16, D, M, nullptr, 0, kv16, ldkv, nullptr, 0, nullptr, 0, false, 0, 1.f);
  r.B = B; r.L = L; r.token_num = lens;
  r.kv = kv16; r.kv_rs = ldkv; r.kv_bs = (int64_t)Tc * ldkv; r.Lk = Tc;
  r.cache_in = ci; r.cache_out = co;
  decoder16(dec_, r);
  launch_layernorm(stream_, t32, Md, D, dec_.after.g, dec_.after.b, xdn16, D, nullptr, 0);
  gemm("gemm_vocab", dec_.out, xdn16, D, Md, lg, ldV, nullptr, 0, nullptr, 0, nullptr, 0, false, 0, 1.f);
  launch_argmax(stream_, lg, Md, V, ldV, logits_out ? 2 : 1, ids);
  if (logits_out) PF_HIP(hipMemcpy2DAsync(logits_out, (size_t)V * 4, lg, (size_t)ldV * 4, (size_t)V * 4, Md, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpyAsync(ids_out, ids, (size_t)Md * 8, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpyAsync(caches_out, co, (size_t)nd * B * D * CW * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));
}

// ---- the device-resident chunk step (engine.h) ----
size_t Engine::online_slot_cache_off() const { return (size_t)round_up((int64_t)block_at_zero<CifStreamBlock>(mc_.d_model).bytes(), kAlign); }
size_t Engine::online_slot_bytes() const {
  return online_slot_cache_off() + (size_t)round_up((int64_t)dec_.layers.size() * mc_.d_model * (mc_.kernel - 1) * 4, kAlign);
}

void Engine::online_step(const float* speech, int B, int Tc, char* slots_dev, const int32_t* slot, const int32_t* cif_reset,
                         const int32_t* cache_reset, int lo, int hi, OnlineStepOut& out) {
  PF_CHECK(speech && slots_dev && slot && cif_reset && cache_reset && B > 0 && Tc > 0, PF_ERR_INVALID_ARG, "online_step: bad arguments");
  PF_CHECK(mc_.kind != "sensevoicesmall", PF_ERR_UNSUPPORTED, "online_step: paraformer models only");
  PF_CHECK(mc_.kernel == 11, PF_ERR_UNSUPPORTED, "online_step: FSMN kernel 11 (cache of 10 columns) only");
  PF_HIP(hipSetDevice(device_));
  const int D = mc_.d_model, F = mc_.ffn, V = mc_.vocab, nd = (int)dec_.layers.size(), CW = mc_.kernel - 1;
  const int M = B * Tc, cap = Tc + 1;
  const size_t nB = (size_t)B;
  out.max_tok = 0; out.cap = cap;
  out.counts.assign(nB, 0); out.fire_entry.assign(nB * cap, -1); out.ids.clear(); out.scores.clear();
  // 1 - 3: the chunk up, the encoder, the alphas (online_encoder without its downloads)
  const size_t n = (size_t)M * mc_.feat_dim;
  ensure(ws_speech_, n * 4);
  PF_HIP(hipMemcpyAsync(ws_speech_.p, speech, n * 4, hipMemcpyHostToDevice, stream_));
  encoder((const float*)ws_speech_.p, B, Tc, true);
  cif_alpha_stage(H16_, B, Tc, h16_, fsm_, alphas_, nullptr);
  // 4: the carried CIF on the streams' blocks; slot | cif_reset | cache_reset in one upload, counts | fire entries in one export
  StageCarve st;
  const auto d_meta = st.take<int32_t>(3 * nB), d_words = st.take<int32_t>(nB + nB * cap);
  const auto d_fired = st.take<float>(nB * cap * D);
  ensure(ws_step_, st.off);
  void* ws = ws_step_.p;
  std::vector<int32_t> meta(3 * nB);
  for (int b = 0; b < B; ++b) { meta[b] = slot[b]; meta[nB + b] = cif_reset[b]; meta[2 * nB + b] = cache_reset[b]; }
  upload(stream_, d_meta(ws), (const int32_t*)meta.data(), meta.size());
  const int32_t* d_slot = d_meta(ws);
  int32_t* d_counts = d_words(ws);
  const int64_t stride = (int64_t)online_slot_bytes(), cache_off = (int64_t)online_slot_cache_off();
  CifStreamLaunch c{};
  c.states = slots_dev; c.state_stride = stride; c.slot = d_slot;
  c.enc = H32_; c.alphas = alphas_; c.lda = Tc + 1; c.reset = d_meta(ws) + nB;
  c.B = B; c.Tc = Tc; c.D = D; c.threshold = mc_.cif_threshold; c.lo = lo; c.hi = hi;
  c.fired = d_fired(ws); c.fire_entry = d_words(ws) + nB; c.cap = cap; c.counts = d_counts;
  prof_begin("cif_stream", 0);
  launch_cif_stream(stream_, c);
  prof_end("cif_stream");
  const int n_words = (int)d_words.count;
  if (!step_host_tried_ || (step_host_ && step_host_cap_ < n_words)) {
    step_host_tried_ = true;
    if (step_host_) { PF_HIP(hipStreamSynchronize(stream_)); hipHostFree(step_host_); step_host_ = nullptr; step_host_dev_ = nullptr; step_host_cap_ = 0; }
    void* p = nullptr; void* d = nullptr;
    const int words = std::max(2 * n_words, 1024);
    if (hipHostMalloc(&p, (size_t)words * 4, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&d, p, 0) == hipSuccess) {
      step_host_ = (int32_t*)p; step_host_dev_ = (int32_t*)d; step_host_cap_ = words;
    } else {
      (void)hipGetLastError();
      if (p) hipHostFree(p);
    }
    if (!ev_step_) PF_HIP(hipEventCreateWithFlags(&ev_step_, hipEventDisableTiming));
  }
  std::vector<int32_t> words((size_t)n_words);
  if (step_host_) {
    launch_export_words(stream_, d_words(ws), n_words, step_host_dev_);
    PF_HIP(hipEventRecord(ev_step_, stream_));
    PF_HIP(hipEventSynchronize(ev_step_));
    std::memcpy(words.data(), step_host_, (size_t)n_words * 4);
  } else {
    download(stream_, words.data(), (const int32_t*)d_words(ws), (size_t)n_words);
    PF_HIP(hipStreamSynchronize(stream_));
  }
  // 5: the decoder length
  int L = 0;
  for (int b = 0; b < B; ++b) {
    PF_CHECK(words[b] >= 0 && words[b] <= cap, PF_ERR_DEVICE, "online_step: a fire count outside 0 .. Tc + 1");
    L = std::max(L, (int)words[b]);
  }
  std::copy(words.begin(), words.begin() + B, out.counts.begin());
  std::copy(words.begin() + B, words.end(), out.fire_entry.begin());
  if (L == 0) return;                                            // OnlineRecognizer.cs:380
  out.max_tok = L;
  // 6 - 12: online_decoder on what is already on the device
  const int Md = B * L;
  const int64_t Mp = round_up(M, 128) + 128, Mdp = round_up(Md, 128) + 128;
  const int ldV = (int)round_up(V, 4);
  half_t* e16 = nullptr; half_t* kv16 = nullptr; float* lg = nullptr; int64_t* ids = nullptr; float* best = nullptr;
  float* ci = nullptr; float* co = nullptr;
  DecRun r;
  r.b = carve_into(ws_dec_, kAlign, [&](Arena& a) {
    e16 = a.take<half_t>((size_t)Mp * D * 2); kv16 = a.take<half_t>((size_t)Mp * std::max(nd, 1) * 2 * D * 2);
    const DecBufs d = carve_dec16(a, Mdp, F, false);
    lg = a.take<float>((size_t)Mdp * ldV * 4); ids = a.take<int64_t>((size_t)Md * 8); best = a.take<float>((size_t)Md * 4);
    ci = a.take<float>((size_t)nd * B * D * CW * 4); co = a.take<float>((size_t)nd * B * D * CW * 4);
    return d;
  });
  float* xd = r.b.x; float* t32 = r.b.t32; half_t* xdn16 = r.b.xn16;
  launch_cif_pack(stream_, d_fired(ws), B, cap, L, D, xd);
  PF_HIP(hipMemsetAsync(e16, 0, (size_t)Mp * D * 2, stream_));
  launch_f32_to_f16(stream_, H32_, M, D, D, e16, D);
  const int ldkv = nd * 2 * D;
  if (nd > 0) {
    gemm("gemm_dec_kv", dec_.kv_all, e16, D, M, nullptr, 0, kv16, ldkv, nullptr, 0, nullptr, 0, false, 0, 1.f);
    launch_cif_cache_gather(stream_, slots_dev, stride, cache_off, d_slot, d_meta(ws) + 2 * nB, B, nd, D * CW, ci);
  }
  r.B = B; r.L = L; r.token_num = d_counts;
  r.kv = kv16; r.kv_rs = ldkv; r.kv_bs = (int64_t)Tc * ldkv; r.Lk = Tc;
  r.cache_in = ci; r.cache_out = co;
  decoder16(dec_, r);
  launch_layernorm(stream_, t32, Md, D, dec_.after.g, dec_.after.b, xdn16, D, nullptr, 0);
  gemm("gemm_vocab", dec_.out, xdn16, D, Md, lg, ldV, nullptr, 0, nullptr, 0, nullptr, 0, false, 0, 1.f);
  launch_argmax(stream_, lg, Md, V, ldV, 1, ids, best);
  if (nd > 0) launch_cif_cache_scatter(stream_, slots_dev, stride, cache_off, d_slot, B, nd, D * CW, co);
  out.ids.resize((size_t)Md); out.scores.resize((size_t)Md);
  PF_HIP(hipMemcpyAsync(out.ids.data(), ids, (size_t)Md * 8, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpyAsync(out.scores.data(), best, (size_t)Md * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::set_hotwords(const int32_t* hw, int n) {
  PF_CHECK(n >= 0 && (n == 0 || hw), PF_ERR_INVALID_ARG, "set_hotwords: bad arguments");
  if (n == n_hotwords_ && hotwords_.size() == (size_t)n * 10 && (n == 0 || std::memcmp(hotwords_.data(), hw, (size_t)n * 40) == 0)) return;
  hotwords_.assign(hw, hw + (size_t)n * 10);
  n_hotwords_ = n;
  seaco_hw_valid_ = false;                            // the embedder output / K,V rows of the old list are stale
}

// SeACo bias branch (export_forward of the FunASR SeACo export; reference call site
// OfflineProjOfSeacoParaformer.cs:48-135).  hotwords [N,10] -> Embedding -> LSTM stack -> hw_embed; bias_embed
// row n*10+j = hw_embed[j,n] is the same for every utterance (OfflineProjOfSeacoParaformer.cs:83-111 tiles it
// over B), so its K/V projections are computed once and every (utterance, head) attends the same rows.  The
// bias decoder runs once on 2*B*L rows: [CIF embeds ; ASR decoder hidden].
void Engine::seaco_head(int B, int L, const float* e0, const float* hid32, bool want_logits) {
  const int D = mc_.d_model, V = mc_.vocab, Fs = mc_.seaco_ffn, ns = (int)bias_dec_.layers.size();
  const int N = n_hotwords_, J = 10, NJ = N * J;
  const int Md = B * L, R = 2 * Md;
  const int64_t NJp = round_up(NJ, 128) + 128, Rp = round_up(R, 128) + 128, Mdp = round_up(Md, 128) + 128;
  const int ldV = (int)round_up(V, 4);
  // the hot-word side (ids, embedder, its K / V rows) lives in its own buffer and is computed once per hot-word LIST, not
  // once per call: it is a function of the weights and the list alone (the reference re-runs model_eb every call,
  // OfflineProjOfSeacoParaformer.cs:83-111, with the same result)
  size_t hoff = 0;
  const Carve hcarve{hoff};
  const size_t o_ids = hcarve((size_t)NJ * 4), o_e32 = hcarve((size_t)NJp * D * 4), o_in16 = hcarve((size_t)NJp * D * 2);
  const size_t o_xg = hcarve((size_t)NJp * 4 * D * 4), o_ho = hcarve((size_t)NJp * D * 4), o_hs = hcarve((size_t)2 * N * D * 2);
  const size_t o_cs = hcarve((size_t)N * D * 4), o_kv = hcarve((size_t)NJp * std::max(ns, 1) * 2 * D * 2);
  if (!ws_seaco_hw_.p || ws_seaco_hw_.bytes < hoff) seaco_hw_valid_ = false;
  ensure(ws_seaco_hw_, hoff);
  float* hid = nullptr; half_t* m16 = nullptr; float* dha = nullptr; int64_t* dha_ids = nullptr; int32_t* tn2 = nullptr;
  DecRun r;
  r.b = carve_into(ws_seaco_, kAlign, [&](Arena& a) {
    const DecBufs d = carve_dec16(a, Rp, Fs, true);
    hid = a.take<float>((size_t)Rp * D * 4); m16 = a.take<half_t>((size_t)Mdp * D * 2);
    dha = a.take<float>((size_t)Mdp * ldV * 4); dha_ids = a.take<int64_t>((size_t)Md * 8); tn2 = a.take<int32_t>((size_t)2 * B * 4);
    return d;
  });
  float* xs = r.b.x; float* t32 = r.b.t32;
  char* hbase = (char*)ws_seaco_hw_.p;
  int32_t* ids = (int32_t*)(hbase + o_ids);
  float* e32 = (float*)(hbase + o_e32); half_t* in16 = (half_t*)(hbase + o_in16);
  float* xg = (float*)(hbase + o_xg); float* hout = (float*)(hbase + o_ho);
  half_t* hs = (half_t*)(hbase + o_hs); float* cs = (float*)(hbase + o_cs);
  half_t* kv16 = (half_t*)(hbase + o_kv);
  const int ldkv = ns * 2 * D;

  if (!seaco_hw_valid_) {
  // ---- hotword embedder: Embedding -> LSTM stack (all J outputs kept), batch-major rows n*J + j
  prof_begin("seaco_embed", 0);
  PF_HIP(hipMemcpyAsync(ids, hotwords_.data(), (size_t)NJ * 4, hipMemcpyHostToDevice, stream_));
  launch_embed_gather(stream_, seaco_embed_w_, ids, NJ, D, (int)tensor("seaco.embed.weight").shape[0], e32, in16);
  prof_end("seaco_embed");
  for (size_t l = 0; l < seaco_lstm_.size(); ++l) {
    gemm("gemm_seaco", seaco_lstm_[l].ih, in16, D, NJ, xg, 4 * D, nullptr, 0, nullptr, 0, nullptr, 0, false, 0, 1.f);
    prof_begin("seaco_embed", 0);
    LstmArgs a{};
    a.whh = seaco_lstm_[l].whh; a.xg = xg; a.hstate = hs; a.cstate = cs; a.hout = hout; a.B = N; a.T3 = J; a.D = D; a.ndir = 1;
    lstm_clear16(a);
    lstm_steps16(a);
    launch_f32_to_f16(stream_, hout, NJ, D, D, in16, D);
    prof_end("seaco_embed");
  }
  if (ns > 0 && !int8_mode_)
    gemm("gemm_seaco", bias_dec_.kv_all, in16, D, NJ, nullptr, 0, kv16, ldkv, nullptr, 0, nullptr, 0, false, 0, 1.f);
  if (ns > 0 && int8_mode_) seaco_kv_int8(hout, in16, NJ, kv16, ldkv);
  seaco_hw_valid_ = true;
  }

  // ---- bias decoder on [CIF embeds ; decoder hidden]
  PF_HIP(hipMemcpyAsync(xs, e0, (size_t)Md * D * 4, hipMemcpyDeviceToDevice, stream_));
  PF_HIP(hipMemcpyAsync(xs + (size_t)Md * D, hid32, (size_t)Md * D * 4, hipMemcpyDeviceToDevice, stream_));
  PF_HIP(hipMemcpyAsync(tn2, plan_.token_num, (size_t)B * 4, hipMemcpyDeviceToDevice, stream_));
  PF_HIP(hipMemcpyAsync(tn2 + B, plan_.token_num, (size_t)B * 4, hipMemcpyDeviceToDevice, stream_));
  r.B = 2 * B; r.L = L; r.token_num = tn2;
  r.kv = kv16; r.kv_rs = ldkv; r.kv_bs = 0; r.Lk = NJ;                  // one bias_embed for every utterance
  r.cls_ffn1 = r.cls_ffn2 = r.cls_q = r.cls_out = "gemm_seaco"; r.cls_attn = "attn_seaco";
  if (int8_mode_) {
    // math_mode 2: the bias decoder's Linears are MatMulInteger pairs in model.int8.onnx like the ASR decoder's.  The graph runs
    // the decoder twice — on the CIF embeds and on the ASR decoder hidden — and each run has its own DynamicQuantizeLinear nodes,
    // i.e. its own per-tensor ranges: the f16 path's single pass over 2 * B * L rows would merge the two ranges, so this mode
    // runs one pass of B * L rows per half
    r.B = B;
    for (int half = 0; half < 2; ++half) {
      r.b.x = xs + (size_t)half * Md * D;
      decoder_int8(bias_dec_, r);
      prof_begin("layernorm", 0);
      launch_layernorm(stream_, t32, Md, D, bias_dec_.after.g, bias_dec_.after.b, nullptr, 0, hid + (size_t)half * Md * D, D);
      prof_end("layernorm");
    }
  } else {
    decoder16(bias_dec_, r);
    prof_begin("layernorm", 0);
    launch_layernorm(stream_, t32, R, D, bias_dec_.after.g, bias_dec_.after.b, nullptr, 0, hid, D);
    prof_end("layernorm");
  }
  // ---- merged = cif_attended + dec_attended -> hotword_output_layer -> NO-BIAS merge with the ASR rows
  prof_begin("seaco_merge", 0);
  if (int8_mode_) launch_add_f32(stream_, hid, hid + (size_t)Md * D, (int64_t)Md * D);
  else launch_add_to_f16(stream_, hid, hid + (size_t)Md * D, Md, D, m16);
  prof_end("seaco_merge");
  if (int8_mode_) qgemm("gemm_seaco", bias_dec_.out, true, hid, nullptr, D, Md, dha, ldV, nullptr, 0, nullptr, 0, nullptr, 0, false, 0, 1.f);
  else gemm("gemm_seaco", bias_dec_.out, m16, D, Md, dha, ldV, nullptr, 0, nullptr, 0, nullptr, 0, false, 0, 1.f);
  prof_begin("seaco_merge", 0);
  launch_argmax(stream_, dha, Md, V, ldV, 2, dha_ids);   // the NO-BIAS decision below is taken on the log-probs too
  launch_seaco_merge(stream_, dha, ldV, dha_ids, Md, V, mc_.seaco_nobias, want_logits ? 1 : 0, logits_, logits_ld_, ids_dev_);
  prof_end("seaco_merge");
}

// The recurrence of the f16 timestamp head (k_bicif.hip): ONE persistent launch (W_hh resident in registers, h exchanged through
// a ring of write-through stores) when every workgroup fits on the device at once; otherwise (B > 64) the T3 dependent launches,
// captured once per (shape, buffers) into a hipGraph and replayed.
void Engine::lstm_clear16(const LstmArgs& a) {
  PF_HIP(hipMemsetAsync(a.hstate, 0, (size_t)a.ndir * 2 * a.B * a.D * 2, stream_));
  PF_HIP(hipMemsetAsync(a.cstate, 0, (size_t)a.ndir * a.B * a.D * 4, stream_));
}

void Engine::lstm_steps16(LstmArgs a) {
  for (int s = 0; s < a.T3; ++s) { a.step = s; launch_lstm_step(stream_, a); }
}

bool Engine::lstm_recurrence16(LstmArgs a, unsigned* sw, bool ring_only) {
  lstm_clear16(a);
  if (launch_lstm_persistent(stream_, a, sw)) {
    lstm_err_ = sw + 63;
    return true;
  }
  PF_CHECK(!ring_only, PF_ERR_UNSUPPORTED, "lstm: the persistent recurrence does not fit on the device at this shape");
  auto& k = lstm_graph_key_;
  const void* rest[4] = {a.whh, a.hstate, a.cstate, a.hout};
  if (!lstm_graph_exec_ || k.xg != a.xg || k.B != a.B || k.T3 != a.T3 || k.ndir != a.ndir || std::memcmp(k.rest, rest, sizeof(rest)) != 0) {
    if (lstm_graph_exec_) { hipGraphExecDestroy(lstm_graph_exec_); lstm_graph_exec_ = nullptr; }
    hipGraph_t g = nullptr;
    PF_HIP(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
    lstm_steps16(a);
    PF_HIP(hipStreamEndCapture(stream_, &g));
    PF_HIP(hipGraphInstantiate(&lstm_graph_exec_, g, nullptr, nullptr, 0));
    hipGraphDestroy(g);
    k.xg = a.xg; k.B = a.B; k.T3 = a.T3; k.ndir = a.ndir;
    std::memcpy(k.rest, rest, sizeof(rest));
  }
  PF_HIP(hipGraphLaunch(lstm_graph_exec_, stream_));
  return false;
}

// BiCIF timestamp head (k_bicif.hip): us_cif_peak [B, 3T]; needs token_num (device) only.
void Engine::timestamp_head(int B, int T) {
  const int D = mc_.d_model, up = mc_.upsample;
  const int M = B * T, T3 = up * T;
  const int64_t M3 = (int64_t)B * T3;
  const int64_t Mp = round_up(M, 128) + 128, M3p = round_up(M3, 128) + 128;
  size_t off = 0;
  const Carve carve{off};
  const size_t o_up = carve((size_t)std::max<int64_t>(Mp * up, M3p) * D * 2), o_xg = carve((size_t)M3p * 8 * D * 4);
  const size_t o_ho = carve((size_t)M3 * 2 * D * 4), o_hs = carve((size_t)8 * B * D * 2), o_cs = carve((size_t)2 * B * D * 4);
  const size_t o_al = carve((size_t)M3 * 4), o_pk = carve((size_t)M3 * 4), o_sw = carve(256);
  ensure(ws_ts_, off);
  char* base = (char*)ws_ts_.p;
  half_t* up16 = (half_t*)(base + o_up);
  float* xg = (float*)(base + o_xg);
  float* hout = (float*)(base + o_ho);
  half_t* hs = (half_t*)(base + o_hs);
  float* cs = (float*)(base + o_cs);
  float* al = (float*)(base + o_al);
  us_peak_ = (float*)(base + o_pk);
  // [M, 3D] row-major IS [3M, D]: output row m of the transposed conv holds frames 3t, 3t+1, 3t+2
  gemm("gemm_ts", ts_up_, H16_, D, M, nullptr, 0, up16, up * D, nullptr, 0, nullptr, 0, false, 0, 1.f);
  gemm("gemm_ts", ts_ih_, up16, D, (int)M3, xg, 8 * D, nullptr, 0, nullptr, 0, nullptr, 0, false, 0, 1.f);
  prof_begin("lstm", 2.0 * 2 * M3 * 4.0 * D * D);
  LstmArgs a{};
  a.whh = ts_whh_; a.xg = xg; a.hstate = hs; a.cstate = cs; a.hout = hout; a.B = B; a.T3 = T3; a.D = D; a.ndir = 2;
  lstm_recurrence16(a, (unsigned*)(base + o_sw));
  prof_end("lstm");
  if (ts_defer_copy_) PF_HIP(hipStreamWaitEvent(stream_, ev_scan_, 0));   // on the side stream: token_num comes from the CIF scan
  prof_begin("ts_misc", 0);
  launch_us_alpha(stream_, hout, M3, 2 * D, ts_out_w_, ts_out_b_, mc_.cif_smooth2, mc_.cif_noise2, al);
  launch_us_peak(stream_, al, plan_.token_num, B, T3, mc_.cif_threshold - 1e-4f, us_peak_);
  prof_end("ts_misc");
  last_.peak_len = T3;
  last_.cif_peak.resize((size_t)M3);
  // the copy to (pageable) host memory blocks the calling thread until the recurrence has finished: when the head runs
  // beside the decoder it is issued at the join instead (join_ts), after the decoder has been enqueued
  if (ts_defer_copy_) ts_copy_floats_ = (size_t)M3;
  else PF_HIP(hipMemcpyAsync(last_.cif_peak.data(), us_peak_, (size_t)M3 * 4, hipMemcpyDeviceToHost, stream_));
}

void Engine::sensevoice_head(int B, int T, bool want_logits) {
  const int D = mc_.d_model, V = mc_.vocab, M = B * T;
  const int64_t Mp = round_up(M, 128) + 128;
  logits_ld_ = (int)round_up(V, 4);
  carve_into(ws_dec_, kAlign, [&](Arena& a) { logits_ = a.take<float>((size_t)Mp * logits_ld_ * 4); ids_dev_ = a.take<int64_t>((size_t)M * 8); });
  // the vocabulary product is the arithmetic's own (fp32: in the class the encoder left, "gemm32_misc")
  if (fp32_mode_) gemm32(H32_, D, ctc_.w32, D, ctc_.bias, M, V, D, logits_, logits_ld_, nullptr, 0, false, 0, 1.f);
  else if (int8_mode_) qgemm("gemm_vocab", ctc_, true, H32_, nullptr, D, M, logits_, logits_ld_, nullptr, 0, nullptr, 0, nullptr, 0, false, 0, 1.f);
  else gemm("gemm_vocab", ctc_, H16_, D, M, logits_, logits_ld_, nullptr, 0, nullptr, 0, nullptr, 0, false, 0, 1.f);
  last_.B = B; last_.L = T; last_.V = V; last_.T = T;
  last_.ids.assign((size_t)M, 0);
  last_.token_num.assign(B, T);
  last_.fire_count.assign(B, T);
  finish(B, T, want_logits, nullptr, fp32_mode_ ? nullptr : "argmax");
}

// ------------------------------------------------------------------ decoding extras ---------
void Engine::set_decode(int flags) {
  PF_CHECK((flags & ~(PF_DECODE_SCORES | PF_DECODE_CTC | PF_DECODE_TOPK | PF_DECODE_CTC_BEAM | PF_DECODE_ALIGN)) == 0,
           PF_ERR_INVALID_ARG, "set_decode: unknown flag bits");
  if (flags & PF_DECODE_ALIGN) {
    PF_CHECK(mc_.kind_id() == 1 && !mc_.seaco, PF_ERR_UNSUPPORTED, "PF_DECODE_ALIGN: only a SenseVoice model has a CTC head");
    flags |= PF_DECODE_SCORES;
  }
  if (flags & PF_DECODE_CTC_BEAM) {
    PF_CHECK(mc_.kind_id() == 1 && !mc_.seaco, PF_ERR_UNSUPPORTED, "PF_DECODE_CTC_BEAM: only a SenseVoice model has a CTC head");
    flags |= PF_DECODE_TOPK;
  }
  if (flags & PF_DECODE_TOPK) flags |= PF_DECODE_SCORES;
  if (flags & PF_DECODE_CTC) {
    PF_CHECK(mc_.kind_id() == 1, PF_ERR_UNSUPPORTED, "PF_DECODE_CTC: only a SenseVoice model has a CTC head");
    flags |= PF_DECODE_SCORES;
  }
  // the SeACo bias merge replaces rows of the result after the arg-max; their scores would need a path of their own
  PF_CHECK(flags == 0 || !mc_.seaco, PF_ERR_UNSUPPORTED, "PF_DECODE_SCORES: not available for a SeACo model");
  decode_flags_ = flags;
  if (!(flags & PF_DECODE_ALIGN)) { align_B_ = 0; align_tgt_.clear(); align_len_.clear(); }
}

void Engine::set_align_targets(const int64_t* ids, const int32_t* len, int B, int cap) {
  PF_CHECK(decode_flags_ & PF_DECODE_ALIGN, PF_ERR_INVALID_ARG, "set_align_targets: PF_DECODE_ALIGN is not set");
  PF_CHECK(B >= 0 && cap >= 0 && (B == 0 || len), PF_ERR_INVALID_ARG, "set_align_targets: bad B / cap / len");
  int mx = 0;
  for (int b = 0; b < B; ++b) {
    PF_CHECK(len[b] >= -1, PF_ERR_INVALID_ARG, "set_align_targets: len[b] is -1 (no target) or a length");
    PF_CHECK(len[b] <= PF_ALIGN_MAX_TOKENS && len[b] <= cap, PF_ERR_CAPACITY,
             "set_align_targets: a target of " + std::to_string(len[b]) + " tokens > min(cap, PF_ALIGN_MAX_TOKENS)");
    mx = std::max(mx, len[b]);
  }
  PF_CHECK(mx == 0 || ids, PF_ERR_INVALID_ARG, "set_align_targets: null ids");
  for (int b = 0; b < B; ++b)
    for (int p = 0; p < len[b]; ++p) {
      const int64_t c = ids[(size_t)b * cap + p];
      PF_CHECK(c >= 1 && c < mc_.vocab, PF_ERR_INVALID_ARG, "set_align_targets: an id outside [1, V)");
    }
  const int c1 = std::max(mx, 1);
  align_tgt_.assign((size_t)B * c1, -1);
  align_len_.assign(len, len + B);
  for (int b = 0; b < B; ++b)
    for (int p = 0; p < len[b]; ++p) align_tgt_[(size_t)b * c1 + p] = (int32_t)ids[(size_t)b * cap + p];
  align_B_ = B;
  align_cap_ = c1;
}

void Engine::set_topk(int k) {
  PF_CHECK(k >= 1 && k <= PF_TOPK_MAX, PF_ERR_INVALID_ARG, "set_topk: K must be 1 .. " + std::to_string(PF_TOPK_MAX));
  topk_k_ = k;
}

void Engine::set_ctc_beam(int W, int N) {
  PF_CHECK(N >= 1 && N <= W && W <= PF_NBEST_MAX, PF_ERR_INVALID_ARG, "set_ctc_beam: 1 <= N <= W <= " + std::to_string(PF_NBEST_MAX));
  beam_w_ = W;
  beam_n_ = N;
}

void Engine::set_ctc_hotwords(const int32_t* ids, const int32_t* lens, int n, float boost) {
  PF_CHECK(mc_.kind_id() == 1 && !mc_.seaco, PF_ERR_UNSUPPORTED, "set_ctc_hotwords: only a SenseVoice model has a CTC head");
  install_hotwords(hot_, "set_ctc_hotwords", ids, lens, n, boost);
}

// the argument rules, the content test and the one upload of both hot-word setters
void Engine::install_hotwords(HotDev& d, const char* who_, const int32_t* ids, const int32_t* lens, int n, float boost) {
  const std::string who = who_;
  PF_CHECK(boost >= 0.f && boost <= 3.4028234e38f, PF_ERR_INVALID_ARG, who + ": the boost is finite and >= 0");
  PF_CHECK(n >= 0, PF_ERR_INVALID_ARG, who + ": negative n_hotwords");
  PF_CHECK(n == 0 || lens, PF_ERR_INVALID_ARG, who + ": null lens");
  if (n == 0 || boost == 0.f) { d.clear(); return; }
  size_t total = 0;
  for (int i = 0; i < n; ++i) { PF_CHECK(lens[i] >= 0, PF_ERR_INVALID_ARG, who + ": negative hot-word length"); total += (size_t)lens[i]; }
  PF_CHECK(total == 0 || ids, PF_ERR_INVALID_ARG, who + ": null ids");
  // the automaton is kept while the set is the same (by content): only the boost may have changed
  if (d.boost > 0.f && d.lens.size() == (size_t)n && d.ids.size() == total && std::equal(lens, lens + n, d.lens.begin()) &&
      std::equal(ids, ids + total, d.ids.begin())) {
    d.boost = boost;
    return;
  }
  HotwordGraph g;
  build_hotword_graph(ids, lens, n, mc_.vocab, g);   // throws before anything changes
  if (g.empty()) { d.clear(); return; }
  d.ids.assign(ids, ids + total);
  d.lens.assign(lens, lens + n);
  PF_HIP(hipSetDevice(device_));
  PF_HIP(hipStreamSynchronize(stream_));            // a queued search may still read the table about to be replaced
  const size_t V = g.tok_col.size(), words = V + g.table.size();
  ensure(d.buf, words * 4);
  // on stream_, behind the zero fill that ensure() queues there when it allocates: the stream is non-blocking, so a copy on
  // the null stream is not ordered against that fill and could be overwritten by it (a fresh engine's first table)
  PF_HIP(hipMemcpyAsync(d.buf.p, g.tok_col.data(), V * 4, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync((int32_t*)d.buf.p + V, g.table.data(), g.table.size() * 4, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipStreamSynchronize(stream_));              // (g goes with this scope)
  d.boost = boost;
  d.A = g.A;
}

void Engine::set_ctc_lm(const std::shared_ptr<const LmImage>& lm, float alpha, float beta, int flags) {
  PF_CHECK(mc_.kind_id() == 1 && !mc_.seaco, PF_ERR_UNSUPPORTED, "set_ctc_lm: only a SenseVoice model has a CTC head");
  if (!lm) { lm_.reset(); return; }                 // (the image stays where it is: the same model again costs no upload)
  lm_check_weights(alpha, beta, flags);
  PF_HIP(hipSetDevice(device_));
  if (lm_inst_.src != lm) PF_HIP(hipStreamSynchronize(stream_));   // a queued search may still read the image about to be replaced
  lm_device_image(lm_inst_, lm);
  lm_ = lm;
  lm_alpha_ = alpha; lm_beta_ = beta; lm_flags_ = flags;
}

void Engine::set_nbest_search(int W, int N) {
  PF_CHECK(mc_.kind_id() == 0 && !mc_.seaco, PF_ERR_UNSUPPORTED, "set_nbest_search: only a paraformer model (not SeACo, not SenseVoice) has this search");
  if (W == 0) { nbs_w_ = 0; nbs_n_ = 0; return; }
  PF_CHECK(N >= 1 && N <= W && W <= PF_NBEST_MAX, PF_ERR_INVALID_ARG, "set_nbest_search: W == 0 or 1 <= N <= W <= " + std::to_string(PF_NBEST_MAX));
  nbs_w_ = W;
  nbs_n_ = N;
}

void Engine::set_nbest_lm(const std::shared_ptr<const LmImage>& lm, float alpha, float beta, int flags) {
  PF_CHECK(mc_.kind_id() == 0 && !mc_.seaco, PF_ERR_UNSUPPORTED, "set_nbest_lm: only a paraformer model (not SeACo, not SenseVoice) has this search");
  if (!lm) { nbs_lm_.reset(); return; }             // (the image stays where it is: the same model again costs no upload)
  lm_check_weights(alpha, beta, flags);
  PF_HIP(hipSetDevice(device_));
  if (lm_inst_.src != lm) PF_HIP(hipStreamSynchronize(stream_));   // a queued search may still read the image about to be replaced
  lm_device_image(lm_inst_, lm);
  nbs_lm_ = lm;
  nbs_alpha_ = alpha; nbs_beta_ = beta; nbs_flags_ = flags;
}

void Engine::set_nbest_hotwords(const int32_t* ids, const int32_t* lens, int n, float boost) {
  PF_CHECK(mc_.kind_id() == 0 && !mc_.seaco, PF_ERR_UNSUPPORTED, "set_nbest_hotwords: only a paraformer model (not SeACo, not SenseVoice) has this search");
  install_hotwords(nbs_hot_, "set_nbest_hotwords", ids, lens, n, boost);
}

float* Engine::score_buf(int64_t rows) {
  if (!decode_flags_) return nullptr;
  ensure(ws_score_, (size_t)std::max<int64_t>(rows, 1) * 4);
  return (float*)ws_score_.p;
}

void Engine::queue_decode_results(int B, int L) {
  std::vector<int32_t>& len = ctc_len_;              // (a member: the host-to-device copies below may read it after this call returns)
  len.clear();
  len.swap(dec_len_);                                // consumed: a later forward without lengths decodes every row
  if (!decode_flags_ || B * L == 0) return;
  const float* sc = (const float*)ws_score_.p;
  last_.scores.resize((size_t)B * L);
  PF_HIP(hipMemcpyAsync(last_.scores.data(), sc, (size_t)B * L * 4, hipMemcpyDeviceToHost, stream_));
  if (decode_flags_ & (PF_DECODE_CTC | PF_DECODE_CTC_BEAM | PF_DECODE_ALIGN)) {
    if ((int)len.size() != B) len.assign(B, L);
    for (int b = 0; b < B; ++b) len[b] = std::min(std::max(len[b], 0), L);
  }
  if (decode_flags_ & PF_DECODE_TOPK) queue_topk(B, L);
  if ((decode_flags_ & PF_DECODE_TOPK) && nbs_w_ > 0) queue_nbest_search(B, L);
  if (decode_flags_ & PF_DECODE_CTC_BEAM) queue_ctc_beam(B, L);      // (set_decode: implies TOPK)
  if (decode_flags_ & PF_DECODE_ALIGN) queue_align(B, L);
  if (decode_flags_ & PF_DECODE_CTC) queue_ctc_collapse(B, L);
}

void Engine::queue_topk(int B, int L) {
  // the arg-max ran in its store-in-place form (argmax_mode): logits_ holds the log-probs it scanned
  const int64_t rows = (int64_t)B * L;
  const int K = topk_k_;
  Cursor c;
  const TopkBlock k(c, rows, K);
  ensure(ws_topk_, c.off);
  last_.topk.resize(k.words());
  last_.topk_k = K;
  void* ws = ws_topk_.p;
  prof_begin("topk", 0);
  launch_topk(stream_, logits_, rows, last_.V, logits_ld_, K, k.ids(ws), k.val(ws), k.n(ws));
  prof_end("topk");
  PF_HIP(hipMemcpyAsync(last_.topk.data(), ws, k.bytes(), hipMemcpyDeviceToHost, stream_));
}

void Engine::queue_nbest_search(int B, int L) {
  // the search reads the lists queue_topk just made and the CIF plan's token counts where the decoder read them
  const int W = nbs_w_, Nh = nbs_n_, K = topk_k_;
  const bool hot = nbs_hot_.boost > 0.f, lm = (bool)nbs_lm_;
  const TopkBlock tk = block_at_zero<TopkBlock>((size_t)B * L, K);
  Cursor c;
  const NbestSearchBlock k(c, B, Nh, L);
  const Field<int32_t> bp = c.take<int32_t>((size_t)B * L * W);
  ensure(ws_nbs_, c.off);
  last_.nbs.resize(k.words());
  last_.nbs_n = Nh;
  void* ws = ws_nbs_.p;
  const void* wt = ws_topk_.p;
  const int32_t* tok_col = hot ? (const int32_t*)nbs_hot_.buf.p : nullptr;
  NbestSearchArgs a{};
  a.ids = tk.ids(wt); a.val = tk.val(wt); a.n = tk.n(wt); a.token_num = plan_.token_num;
  a.L = L; a.K = K; a.W = W; a.N = Nh;
  a.bp = bp(ws);
  a.tok_col = tok_col; a.table = hot ? tok_col + mc_.vocab : nullptr; a.V = mc_.vocab; a.A = nbs_hot_.A; a.boost = (double)nbs_hot_.boost;
  a.lm_image = lm ? (const int32_t*)lm_inst_.buf.p : nullptr; a.alpha = (double)nbs_alpha_; a.beta = (double)nbs_beta_;
  a.lm_eos = (nbs_flags_ & PF_LM_EOS) != 0;
  a.out_ranks = k.ranks(ws); a.out_score = k.score(ws); a.out_loglik = k.loglik(ws); a.out_lm = k.lm_sum(ws);
  a.out_matched = k.matched(ws); a.n_hyp = k.n_hyp(ws);
  prof_begin("nbest_search", 0);
  launch_nbest_search(stream_, a, B);
  prof_end("nbest_search");
  PF_HIP(hipMemcpyAsync(last_.nbs.data(), ws, k.words() * 8, hipMemcpyDeviceToHost, stream_));
}

void Engine::queue_ctc_beam(int B, int L) {
  // the search reads the lists queue_topk just made and the blank column (id 0) of the in-place log-prob rows
  const int W = beam_w_, Nh = beam_n_, cap = L, K = topk_k_;
  const bool hot = hot_.boost > 0.f, lm = (bool)lm_;
  const size_t nodes = (size_t)B * ((size_t)L * W + 1);
  const TopkBlock tk = block_at_zero<TopkBlock>((size_t)B * L, K);
  Cursor c;
  const BeamBlock k(c, B, Nh, cap);
  const Field<int32_t> len_d = c.take<int32_t>(B), node_par = c.take<int32_t>(nodes), node_tok = c.take<int32_t>(nodes);
  Cursor ch = c;
  const BeamHotBlock h(ch, B, Nh);                   // the biased form only: loglik_sum | matched behind the node workspace
  const size_t hot_end = ch.off;
  const BeamLmBlock l(ch, B, Nh);                    // the fused forms only: lm_sum behind that (loglik_sum is the biased form's)
  ensure(ws_beam_, lm ? ch.off : hot ? hot_end : c.off);
  last_.beam.resize(k.words());
  last_.beam_n = Nh;
  last_.beam_cap = cap;
  void* ws = ws_beam_.p;
  const void* wt = ws_topk_.p;
  PF_HIP(hipMemcpyAsync(len_d(ws), ctc_len_.data(), ctc_len_.size() * 4, hipMemcpyHostToDevice, stream_));
  prof_begin("ctc_beam", 0);
  last_.beam_biased = hot;
  if (lm) {
    const int32_t* tok_col = hot ? (const int32_t*)hot_.buf.p : nullptr;
    last_.beam_hot.resize(h.words());
    last_.beam_lm.resize(l.words());
    if (!hot) PF_HIP(hipMemsetAsync(h.matched(ws), 0, h.matched.count * 4, stream_));   // no set: nothing matched
    launch_ctc_beam_lm(stream_, logits_, logits_ld_, tk.ids(wt), tk.val(wt), tk.n(wt), len_d(ws), B, L, K, 0, W, Nh, cap, node_par(ws),
                       node_tok(ws), tok_col, mc_.vocab, hot ? tok_col + mc_.vocab : nullptr, hot_.A, hot_.boost,
                       (const int32_t*)lm_inst_.buf.p, lm_alpha_, lm_beta_, lm_flags_, k.ids(ws), k.len(ws), k.score(ws), h.matched(ws),
                       h.loglik(ws), l.lm_sum(ws), k.n_hyp(ws));
  } else if (hot) {
    const int32_t* tok_col = (const int32_t*)hot_.buf.p;
    last_.beam_hot.resize(h.words());
    launch_ctc_beam_hot(stream_, logits_, logits_ld_, tk.ids(wt), tk.val(wt), tk.n(wt), len_d(ws), B, L, K, 0, W, Nh, cap, node_par(ws),
                        node_tok(ws), tok_col, mc_.vocab, tok_col + mc_.vocab, hot_.A, hot_.boost, k.ids(ws), k.len(ws), k.score(ws),
                        h.matched(ws), h.loglik(ws), k.n_hyp(ws));
  } else {
    launch_ctc_beam(stream_, logits_, logits_ld_, tk.ids(wt), tk.val(wt), tk.n(wt), len_d(ws), B, L, K, 0, W, Nh, cap, node_par(ws),
                    node_tok(ws), k.ids(ws), k.len(ws), k.score(ws), k.n_hyp(ws));
  }
  prof_end("ctc_beam");
  PF_HIP(hipMemcpyAsync(last_.beam.data(), ws, k.words() * 8, hipMemcpyDeviceToHost, stream_));
  if (hot || lm) PF_HIP(hipMemcpyAsync(last_.beam_hot.data(), (char*)ws + h.begin, h.words() * 8, hipMemcpyDeviceToHost, stream_));
  if (lm) PF_HIP(hipMemcpyAsync(last_.beam_lm.data(), (char*)ws + l.begin, l.words() * 8, hipMemcpyDeviceToHost, stream_));
}

void Engine::queue_align(int B, int L) {
  // jobs per utterance: the caller's target (when set for this forward), then the hypotheses queue_ctc_beam left in ws_beam_
  const bool tg = align_B_ == B;
  const int Nb = (decode_flags_ & PF_DECODE_CTC_BEAM) ? last_.beam_n : 0, b_cap = last_.beam_cap;
  const int H = (tg ? 1 : 0) + Nb;
  align_tgt_q_.clear(); align_len_q_.clear();
  align_tgt_q_.swap(align_tgt_);                    // consumed, like the lengths
  align_len_q_.swap(align_len_);
  const int c_cap = align_cap_;
  align_B_ = 0;
  if (H == 0) return;
  const int cap = std::max(1, std::max(tg ? c_cap : 0, Nb ? std::min(L, (int)PF_ALIGN_MAX_TOKENS) : 0));
  const size_t bp_stride = ctc_align_bp_words(L, cap);
  Cursor c;
  const AlignBlock k(c, B, H, cap);
  const Field<int32_t> tgt_d = c.take<int32_t>(k.first.count), len_d = c.take<int32_t>(B);
  const Field<int32_t> ctgt_d = c.take<int32_t>(tg ? align_tgt_q_.size() : 0), clen_d = c.take<int32_t>(tg ? align_len_q_.size() : 0);
  const Field<uint32_t> bp_d = c.take<uint32_t>(k.ok.count * bp_stride);
  ensure(ws_align_, c.off);
  last_.align.resize(k.words());
  last_.align_h = H;
  last_.align_cap = cap;
  void* ws = ws_align_.p;
  PF_HIP(hipMemcpyAsync(len_d(ws), ctc_len_.data(), ctc_len_.size() * 4, hipMemcpyHostToDevice, stream_));
  if (tg) {
    PF_HIP(hipMemcpyAsync(ctgt_d(ws), align_tgt_q_.data(), align_tgt_q_.size() * 4, hipMemcpyHostToDevice, stream_));
    PF_HIP(hipMemcpyAsync(clen_d(ws), align_len_q_.data(), align_len_q_.size() * 4, hipMemcpyHostToDevice, stream_));
  }
  const BeamBlock bm = block_at_zero<BeamBlock>(B, Nb, b_cap);
  const void* wb = ws_beam_.p;
  prof_begin("ctc_align", 0);
  launch_ctc_align_jobs(stream_, tg ? ctgt_d(ws) : nullptr, tg ? clen_d(ws) : nullptr, c_cap, Nb ? bm.ids(wb) : nullptr,
                        Nb ? bm.len(wb) : nullptr, Nb ? bm.n_hyp(wb) : nullptr, Nb, b_cap, B, H, cap, tgt_d(ws), k.len(ws));
  launch_ctc_align(stream_, logits_, logits_ld_, last_.V, tgt_d(ws), k.len(ws), len_d(ws), B, L, H, cap, bp_d(ws), (int64_t)bp_stride,
                   k.path(ws), k.loglik(ws), k.ok(ws), k.first(ws), k.last(ws), k.tok(ws));
  prof_end("ctc_align");
  PF_HIP(hipMemcpyAsync(last_.align.data(), ws, k.words() * 8, hipMemcpyDeviceToHost, stream_));
}

void Engine::queue_ctc_collapse(int B, int L) {
  const int cap = L;
  Cursor c;
  const CtcBlock k(c, B, cap);
  const Field<int32_t> len_d = c.take<int32_t>(B);
  ensure(ws_ctc_, c.off);
  last_.ctc.resize(k.words());
  last_.ctc_cap = cap;
  void* ws = ws_ctc_.p;
  PF_HIP(hipMemcpyAsync(len_d(ws), ctc_len_.data(), ctc_len_.size() * 4, hipMemcpyHostToDevice, stream_));
  prof_begin("ctc_collapse", 0);
  launch_ctc_collapse(stream_, ids_dev_, (const float*)ws_score_.p, len_d(ws), B, L, 0, cap, k.n(ws), k.ids(ws), k.first(ws), k.last(ws),
                      k.score(ws));
  prof_end("ctc_collapse");
  PF_HIP(hipMemcpyAsync(last_.ctc.data(), ws, k.words() * 8, hipMemcpyDeviceToHost, stream_));
}

void Engine::forward_device(const float* speech_dev, int B, int T, bool want_logits) {
  PF_HIP(hipSetDevice(device_));
  PF_CHECK(B > 0 && T > 0, PF_ERR_INVALID_ARG, "forward: empty batch");
  last_logits_ = want_logits;
  last_.decode_flags = decode_flags_;
  last_.scores.clear(); last_.ctc.clear(); last_.ctc_cap = 0;
  last_.topk.clear(); last_.topk_k = 0;
  last_.beam.clear(); last_.beam_n = 0; last_.beam_cap = 0; last_.beam_hot.clear(); last_.beam_lm.clear(); last_.beam_biased = false;
  last_.align.clear(); last_.align_h = 0; last_.align_cap = 0;
  last_.nbs.clear(); last_.nbs_n = 0;
  if (align_B_ != 0 && align_B_ != B) {             // before anything is launched; the targets are dropped
    const int want = align_B_;
    align_B_ = 0; align_tgt_.clear(); align_len_.clear();
    PF_CHECK(false, PF_ERR_INVALID_ARG, "forward: align targets were set for a batch of " + std::to_string(want) + ", not " + std::to_string(B));
  }
  last_.peak_len = 0;
  last_.cif_peak.clear();
  last_flops_ = 0;
  // ---- the pipeline.  Of its own an arithmetic has the encoder, the decoder arena, and the walk with its vocabulary product.
  PF_CHECK((int64_t)B * T < (1ll << 31) / (3 * mc_.d_model), PF_ERR_INVALID_ARG, "batch too large for 32-bit row indexing");
  build_pe(T);
  const bool f16 = !fp32_mode_ && !int8_mode_;
  if (fp32_mode_) encoder_fp32(speech_dev, B, T);
  else if (int8_mode_) encoder_int8(speech_dev, B, T);
  else encoder(speech_dev, B, T);                    // (repeats the two lines above for its stand-alone callers)
  if (mc_.kind == "sensevoicesmall") {
    sensevoice_head(B, T, want_logits);
  } else {
    const char* cif_cls = fp32_mode_ ? nullptr : "cif_misc";   // the fp32 graph brackets its products only
    predictor(B, T);
    if (f16) dec_kv_ahead(B, T);
    const int L = decoder_length(B, T);
    if (L == 0) {
      join_ts();
    } else {
      DecStage d = fp32_mode_ ? dec_arena_fp32(B, T, L) : int8_mode_ ? dec_arena_int8(B, T, L) : dec_arena_f16(B, T, L);
      cif_embeds(d, B, T, L, cif_cls);
      if (fp32_mode_) asr_decoder_fp32(d, B, T, L);
      else if (int8_mode_) asr_decoder_int8(d, B, T, L);
      else asr_decoder_f16(d, B, T, L);
      finish(B, L, want_logits, &d, fp32_mode_ ? nullptr : "argmax");
    }
  }
  if (!f16) return;
  // algorithmic FLOPs
  const double D = mc_.d_model, F = mc_.ffn, Td = T, Ld = last_.L, K = mc_.kernel, V = mc_.vocab;
  double enc = 2 * Td * mc_.feat_dim * 3 * D + (mc_.enc_layers - 1 + mc_.tp_layers) * 2 * Td * D * 3 * D +
               (mc_.enc_layers + mc_.tp_layers) * (4 * Td * Td * D + 2 * Td * D * D + 4 * Td * D * F + 2 * Td * D * K);
  double fl = enc;
  if (mc_.kind == "sensevoicesmall") fl += 2 * Td * D * V;
  else {
    fl += 2 * Td * D * D * 3 + 2 * Td * D;
    if (mc_.timestamp_head) fl += 2 * Td * D * 3 * D + 2 * (2 * 3 * Td * D * 8 * D);
    fl += mc_.dec_layers * (4 * Ld * D * F + 2 * Ld * D * K + 2 * Ld * D * D + 4 * Td * D * D + 4 * Ld * Td * D + 2 * Ld * D * D) +
          4 * Ld * D * F + 2 * Ld * D * V;
  }
  last_flops_ = fl * B;
}


// Per-thread result slots live in thread-local storage keyed by the engine's uid: a slot dies with its thread
// (no growth under thread-pool churn; a new thread that happens to re-use an OS thread id starts empty), is
// released by the pf_fetch that delivers token_ids, and slots of engines that no longer exist are purged here.
static std::mutex g_live_mu;
static std::set<uint64_t> g_live;
static uint64_t g_next_uid = 1;
static thread_local std::map<uint64_t, HostBatchOut> t_slots;

uint64_t Engine::register_uid() {
  std::lock_guard<std::mutex> lk(g_live_mu);
  const uint64_t id = g_next_uid++;
  g_live.insert(id);
  return id;
}
void Engine::unregister_uid(uint64_t id) {
  std::lock_guard<std::mutex> lk(g_live_mu);
  g_live.erase(id);
}

void Engine::publish_thread_result() {
  PF_HIP(hipStreamSynchronize(stream_));
  check_async_errors();
  {
    std::lock_guard<std::mutex> lk(g_live_mu);
    for (auto it = t_slots.begin(); it != t_slots.end();)
      it = g_live.count(it->first) ? std::next(it) : t_slots.erase(it);
  }
  HostBatchOut& sl = t_slots[uid_];
  sl = last_;
  sl.has_logits = last_logits_;
  sl.logits.clear();
  const int64_t need = (int64_t)last_.B * last_.L * last_.V;
  if (last_logits_ && need > 0) {
    sl.logits.resize((size_t)need);
    PF_HIP(hipMemcpy2D(sl.logits.data(), (size_t)last_.V * 4, logits_, (size_t)logits_ld_ * 4, (size_t)last_.V * 4,
                       (size_t)last_.B * last_.L, hipMemcpyDeviceToHost));
  }
}

void Engine::drop_thread_result() { t_slots.erase(uid_); }

void Engine::copy_logits(HostBatchOut& r) {
  const int64_t need = (int64_t)last_.B * last_.L * last_.V;
  r.logits.assign((size_t)std::max<int64_t>(need, 0), 0.f);
  r.has_logits = last_logits_;
  if (!last_logits_ || need <= 0) return;
  PF_HIP(hipMemcpy2D(r.logits.data(), (size_t)last_.V * 4, logits_, (size_t)logits_ld_ * 4, (size_t)last_.V * 4,
                     (size_t)last_.B * last_.L, hipMemcpyDeviceToHost));
}

void Engine::fetch_ids_device(int64_t* ids_dev, int l_cap, int32_t* L_out) {
  PF_HIP(hipSetDevice(device_));
  const int B = last_.B, L = last_.L;
  PF_CHECK(ids_dev && l_cap > 0, PF_ERR_INVALID_ARG, "fetch_ids_device: null buffer");
  PF_CHECK(l_cap >= L, PF_ERR_CAPACITY, "fetch_ids_device: capacity " + std::to_string(l_cap) + " < L = " + std::to_string(L));
  if (L_out) *L_out = L;
  if (B > 0) {
    PF_HIP(hipMemsetAsync(ids_dev, 0xFF, (size_t)B * l_cap * 8, stream_));
    if (L > 0)
      PF_HIP(hipMemcpy2DAsync(ids_dev, (size_t)l_cap * 8, ids_dev_, (size_t)L * 8, (size_t)L * 8, B, hipMemcpyDeviceToDevice, stream_));
  }
  sync();
}

const HostBatchOut& Engine::fetch_result(int flags, const char* refusal) {
  PF_HIP(hipStreamSynchronize(stream_));
  check_async_errors();
  auto it = t_slots.find(uid_);
  const HostBatchOut& r = it != t_slots.end() ? it->second : last_;
  PF_CHECK((r.decode_flags & flags) == flags, PF_ERR_INVALID_ARG, refusal);
  return r;
}

void Engine::fetch(pf_batch_out* out) {
  PF_CHECK(out, PF_ERR_INVALID_ARG, "fetch: null out");
  const HostBatchOut& r = fetch_result(0, "");   // no decode flag is needed for the ids
  const bool slot = &r != &last_;
  const int B = r.B, L = r.L, V = r.V;
  out->L = L; out->V = V; out->cif_peak_len = r.peak_len;
  if (out->cif_peak && out->cif_peak_cap > 0 && r.peak_len > 0) {
    PF_CHECK(out->cif_peak_cap >= (int64_t)r.cif_peak.size(), PF_ERR_CAPACITY, "cif_peak capacity < B*3T");
    std::memcpy(out->cif_peak, r.cif_peak.data(), r.cif_peak.size() * 4);
  }
  if (out->token_ids) {
    PF_CHECK(out->l_cap >= L, PF_ERR_CAPACITY, "token_ids capacity " + std::to_string(out->l_cap) + " < L = " + std::to_string(L));
    for (int b = 0; b < B; ++b) {
      std::memcpy(out->token_ids + (size_t)b * out->l_cap, r.ids.data() + (size_t)b * L, (size_t)L * 8);
    }
  }
  if (out->token_num) std::memcpy(out->token_num, r.token_num.data(), (size_t)B * 4);
  if (out->logits && out->logits_cap > 0) {
    PF_CHECK(slot ? r.has_logits : last_logits_, PF_ERR_INVALID_ARG, "logits were not requested for the last forward");
    const int64_t need = (int64_t)B * L * V;
    PF_CHECK(out->logits_cap >= need, PF_ERR_CAPACITY, "logits capacity < B*L*V = " + std::to_string(need));
    if (need > 0) {
      if (slot) std::memcpy(out->logits, r.logits.data(), (size_t)need * 4);
      else
        PF_HIP(hipMemcpy2D(out->logits, (size_t)V * 4, logits_, (size_t)logits_ld_ * 4, (size_t)V * 4, (size_t)B * L,
                           hipMemcpyDeviceToHost));
    }
  }
  // the call that receives the ids completes the learn-L-then-fetch protocol: release the slot (a B*L*V host
  // copy of the log-probs may hang off it)
  if (slot && out->token_ids) t_slots.erase(uid_);
}

void Engine::fetch_scores(float* scores, int64_t cap, int32_t* L_out) {
  const HostBatchOut& r = fetch_result(PF_DECODE_SCORES, "fetch_scores: PF_DECODE_SCORES was not set for the last forward");
  if (L_out) *L_out = r.L;
  const int64_t need = (int64_t)r.B * r.L;
  if (!scores) return;
  PF_CHECK(cap >= need, PF_ERR_CAPACITY, "scores capacity < B*L = " + std::to_string(need));
  if (need > 0) std::memcpy(scores, r.scores.data(), (size_t)need * 4);
}

void Engine::fetch_topk(int64_t* ids, float* val, int32_t* n, int64_t cap_rows, int32_t* L_out, int32_t* K_out) {
  const HostBatchOut& r = fetch_result(PF_DECODE_TOPK, "fetch_topk: PF_DECODE_TOPK was not set for the last forward");
  if (L_out) *L_out = r.L;
  if (K_out) *K_out = r.topk_k;
  if (!ids && !val && !n) return;
  const int64_t rows = (int64_t)r.B * r.L;
  PF_CHECK(cap_rows >= rows, PF_ERR_CAPACITY, "topk capacity < B*L = " + std::to_string(rows));
  if (rows == 0 || r.topk.empty()) return;
  const TopkBlock k = r.topk_block();
  const void* p = r.topk.data();
  if (ids) std::memcpy(ids, k.ids(p), k.ids.count * 8);
  if (val) std::memcpy(val, k.val(p), k.val.count * 4);
  if (n) std::memcpy(n, k.n(p), k.n.count * 4);
}

void Engine::fetch_ctc_beam(int64_t* ids, int32_t* len, double* score, int32_t cap, int32_t* n_hyp, int32_t* len_max, int32_t* N_out) {
  const HostBatchOut& r = fetch_result(PF_DECODE_CTC_BEAM, "fetch_ctc_beam: PF_DECODE_CTC_BEAM was not set for the last forward");
  const int B = r.B, Nh = r.beam_n;
  const bool have = !r.beam.empty();
  const BeamBlock k = r.beam_block();
  const void* p = r.beam.data();
  int mx = 0;
  for (int x = 0; x < B * Nh && have; ++x) mx = std::max(mx, k.len(p)[x]);
  if (len_max) *len_max = mx;
  if (N_out) *N_out = Nh;
  if (n_hyp) for (int b = 0; b < B; ++b) n_hyp[b] = have ? k.n_hyp(p)[b] : 0;
  if (!have) return;
  if (len) std::memcpy(len, k.len(p), k.len.count * 4);
  if (score) std::memcpy(score, k.score(p), k.score.count * 8);
  if (!ids) return;
  PF_CHECK(cap >= mx, PF_ERR_CAPACITY, "ctc_beam capacity " + std::to_string(cap) + " < len_max = " + std::to_string(mx));
  copy_rows_padded(ids, cap, k.ids(p), r.beam_cap, k.len.count, (int64_t)-1);
}

void Engine::fetch_ctc_beam_hot(int32_t* matched, double* loglik) {
  const char* refusal = "fetch_ctc_beam_hot: the last forward ran no biased beam search (PF_DECODE_CTC_BEAM with pf_engine_set_ctc_hotwords)";
  const HostBatchOut& r = fetch_result(PF_DECODE_CTC_BEAM, refusal);
  PF_CHECK(!r.beam_hot.empty() && r.beam_biased, PF_ERR_INVALID_ARG, refusal);
  const BeamHotBlock k = r.beam_hot_block();
  const void* p = r.beam_hot.data();
  if (matched) std::memcpy(matched, k.matched(p), k.matched.count * 4);
  if (loglik) std::memcpy(loglik, k.loglik(p), k.loglik.count * 8);
}

void Engine::fetch_ctc_beam_lm(double* lm_sum, double* loglik) {
  const char* refusal = "fetch_ctc_beam_lm: the last forward ran no fused beam search (PF_DECODE_CTC_BEAM with pf_engine_set_ctc_lm)";
  const HostBatchOut& r = fetch_result(PF_DECODE_CTC_BEAM, refusal);
  PF_CHECK(!r.beam_lm.empty() && !r.beam_hot.empty(), PF_ERR_INVALID_ARG, refusal);
  const BeamLmBlock k = r.beam_lm_block();
  const BeamHotBlock h = r.beam_hot_block();
  if (lm_sum) std::memcpy(lm_sum, k.lm_sum(r.beam_lm.data()), k.lm_sum.count * 8);
  if (loglik) std::memcpy(loglik, h.loglik(r.beam_hot.data()), h.loglik.count * 8);
}

void Engine::fetch_nbest_search(int32_t* ranks, double* score, double* loglik, double* lm_sum, int32_t* matched, int32_t* n_hyp,
                                int32_t* L_out, int32_t* N_out) {
  const char* refusal = "fetch_nbest_search: the last forward ran no n-best search (PF_DECODE_TOPK with pf_engine_set_nbest_search)";
  const HostBatchOut& r = fetch_result(PF_DECODE_TOPK, refusal);
  PF_CHECK(r.nbs_n > 0, PF_ERR_INVALID_ARG, refusal);
  if (L_out) *L_out = r.L;
  if (N_out) *N_out = r.nbs_n;
  const NbestSearchBlock k = r.nbs_block();
  const void* p = r.nbs.data();
  if (ranks) std::memcpy(ranks, k.ranks(p), k.ranks.count * 4);
  if (score) std::memcpy(score, k.score(p), k.score.count * 8);
  if (loglik) std::memcpy(loglik, k.loglik(p), k.loglik.count * 8);
  if (lm_sum) std::memcpy(lm_sum, k.lm_sum(p), k.lm_sum.count * 8);
  if (matched) std::memcpy(matched, k.matched(p), k.matched.count * 4);
  if (n_hyp) std::memcpy(n_hyp, k.n_hyp(p), k.n_hyp.count * 4);
}

void Engine::fetch_align(float* path_score, double* loglik, int32_t* ok, int32_t* len, int32_t* first, int32_t* last, float* tok_score,
                         int32_t cap, int32_t* H_out, int32_t* len_max) {
  const HostBatchOut& r = fetch_result(PF_DECODE_ALIGN, "fetch_align: PF_DECODE_ALIGN was not set for the last forward");
  const int H = r.align.empty() ? 0 : r.align_h;
  const AlignBlock k = r.align_block();
  const void* p = r.align.data();
  const size_t jobs = H ? k.len.count : 0;
  int mx = 0;
  for (size_t x = 0; x < jobs; ++x) mx = std::max(mx, k.len(p)[x]);
  if (H_out) *H_out = H;
  if (len_max) *len_max = mx;
  if (jobs == 0) return;
  if (path_score) std::memcpy(path_score, k.path(p), k.path.count * 4);
  if (loglik) std::memcpy(loglik, k.loglik(p), k.loglik.count * 8);
  if (ok) std::memcpy(ok, k.ok(p), k.ok.count * 4);
  if (len) std::memcpy(len, k.len(p), k.len.count * 4);
  if (!first && !last && !tok_score) return;
  PF_CHECK(cap >= mx, PF_ERR_CAPACITY, "align capacity " + std::to_string(cap) + " < len_max = " + std::to_string(mx));
  copy_rows_padded(first, cap, k.first(p), r.align_cap, jobs, -1);
  copy_rows_padded(last, cap, k.last(p), r.align_cap, jobs, -1);
  copy_rows_padded(tok_score, cap, k.tok(p), r.align_cap, jobs, 0.f);
}

void Engine::fetch_ctc(int64_t* ids, int32_t* first, int32_t* last, float* score, int32_t cap, int32_t* n, int32_t* n_max) {
  const HostBatchOut& r = fetch_result(PF_DECODE_CTC, "fetch_ctc: PF_DECODE_CTC was not set for the last forward");
  const int B = r.B;
  const bool have = !r.ctc.empty();
  const CtcBlock k = r.ctc_block();
  const void* p = r.ctc.data();
  int mx = 0;
  for (int b = 0; b < B && have; ++b) mx = std::max(mx, k.n(p)[b]);
  if (n_max) *n_max = mx;
  if (n) for (int b = 0; b < B; ++b) n[b] = have ? k.n(p)[b] : 0;
  if (!ids && !first && !last && !score) return;
  PF_CHECK(cap >= mx, PF_ERR_CAPACITY, "ctc capacity " + std::to_string(cap) + " < n_max = " + std::to_string(mx));
  if (!have) return;
  copy_rows_padded(ids, cap, k.ids(p), r.ctc_cap, B, (int64_t)-1);
  copy_rows_padded(first, cap, k.first(p), r.ctc_cap, B, -1);
  copy_rows_padded(last, cap, k.last(p), r.ctc_cap, B, -1);
  copy_rows_padded(score, cap, k.score(p), r.ctc_cap, B, 0.f);
}

}  // namespace pf
