// engine_ops.cpp — stand-alone operator entry points of the engine (pf_op_*: what the parity tests and the tools/ benches call
// to run ONE kernel form on caller data).  Split out of engine.cpp in round 6.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <set>

#include "hostutil.h"
#include "op_stage.h"

namespace pf {

// ---- hostile hosts: the stand-alone GEMM ops hand their kernels what the pipeline may hand them, not what is convenient.
// Operand rows the contract only calls "readable" (A rows [M, Mp), W rows [N, Np), V rows outside [0, M)) hold a large
// finite f16 pattern instead of zeros (the K pad columns stay zero: that IS the contract), and every output buffer is
// pre-filled with a NaN-payload sentinel: after the launch every cell of [M, N] must have been written, nothing may have
// changed in columns [N, ld) or in rows at or beyond round_up(M, 256) (the 128 spare rows the ops carve are the guard).
// The layer ops (dec_ffn_fused, ffn_fused / attn_ffn_fused, dec_mid, fsmn_dec_ln) check the tighter contracts kernels.h states
// for their kernels: no store at or beyond row M (round_up(M, 64) for the blocked Q | K and V of the encoder tail), the fp32
// residual's rows behind M - 1 hostile as well, sentinel bytes behind the split form's workspace.
namespace {
constexpr int kVLead = 64;                                    // rows in front of the V slice of the FSMN ops
constexpr size_t kWsGuard = 4096;                             // sentinel bytes behind a kernel's workspace
}  // namespace

// the op's workspace: ws_tmp_, grown to what the carve measured
void* Engine::op_ws(const StageCarve& st) {
  ensure(ws_tmp_, st.off);
  return ws_tmp_.p;
}

// tools/: PF_OP_REPEAT launches of one op, the first timed as class "gemm_op", the repeats (warm caches) as "gemm_op_warm"
template <class Fn> void Engine::op_timed(double flops, Fn launch) {
  const char* e = getenv("PF_OP_REPEAT");
  const int reps = e ? std::max(1, atoi(e)) : 1;
  for (int r = 0; r < reps; ++r) {
    prof_begin(r == 0 ? "gemm_op" : "gemm_op_warm", flops);
    launch();
    prof_end(r == 0 ? "gemm_op" : "gemm_op_warm");
  }
}

// ------------------------------------------------------------------ stand-alone ops -------
void Engine::op_lfr_cmvn_pad(const float* const* fbank, const int32_t* t80, int B, int sentinel, float* out,
                             int64_t cap, int32_t* tmax_out) {
  PF_HIP(hipSetDevice(device_));
  const int nm = fc_.n_mels, W = fc_.lfr_m * nm;
  std::vector<int64_t> foff(B + 1, 0);
  int tmax = 0;
  for (int b = 0; b < B; ++b) { foff[b + 1] = foff[b] + t80[b]; tmax = std::max(tmax, t80[b] / fc_.lfr_n); }
  if (tmax_out) *tmax_out = tmax;
  const int64_t need = (int64_t)B * tmax * W;
  PF_CHECK(cap >= need, PF_ERR_CAPACITY, "lfr_cmvn_pad: out capacity < " + std::to_string(need));
  if (need == 0) return;
  StageCarve st;                                                // of ws_meta_: the frame offsets, the frame counts
  const auto doff = st.take<int64_t>((size_t)B + 1); const auto dt80 = st.take<int32_t>(B);
  ensure(ws_fbank_, (size_t)std::max<int64_t>(foff[B], 1) * nm * 4);
  ensure(ws_meta_, st.off);
  ensure(ws_speech_, (size_t)need * 4);
  void* meta = ws_meta_.p; float* rows = (float*)ws_fbank_.p;
  for (int b = 0; b < B; ++b)
    if (t80[b] > 0) upload(stream_, rows + foff[b] * nm, fbank[b], (size_t)t80[b] * nm);
  upload(stream_, doff(meta), foff.data(), (size_t)B + 1);
  upload(stream_, dt80(meta), t80, B);
  launch_lfr_cmvn_pad(stream_, rows, doff(meta), dt80(meta), B, tmax, fc_.lfr_m, fc_.lfr_n, nm, cmvn_shift_, cmvn_scale_, cmvn_shift_ ? 1 : 0,
                      sentinel, (float*)ws_speech_.p);
  download(stream_, out, (const float*)ws_speech_.p, (size_t)need);
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_fbank_batch(const float* const* samples, const int64_t* n, int B, float* out, int64_t cap, int32_t* t80) {
  stage_audio(samples, n, B);
  for (int b = 0; b < B; ++b) t80[b] = st_t80_[b];
  const int64_t need = st_total_frames_ * fc_.n_mels;
  PF_CHECK(cap >= need, PF_ERR_CAPACITY, "fbank_batch: out capacity < " + std::to_string(need));
  if (need == 0) return;
  PF_CHECK(out != nullptr, PF_ERR_INVALID_ARG, "fbank_batch: null out");
  const int64_t* meta = (const int64_t*)ws_meta_.p;
  ensure(ws_fbank_, (size_t)need * 4);
  launch_fbank(stream_, fb_, (const float*)ws_audio_.p, meta, meta + (B + 1), meta + 2 * (B + 1), B, st_total_frames_,
               fc_.snip_edges ? 1 : 0, (float*)ws_fbank_.p, fc_.dither, next_dither_seed());
  PF_HIP(hipMemcpyAsync(out, ws_fbank_.p, (size_t)need * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_argmax(const float* x, int64_t rows, int V, int64_t* ids) {
  PF_HIP(hipSetDevice(device_));
  if (rows == 0) return;
  StageCarve st;
  const auto dx = st.take<float>((size_t)rows * V); const auto did = st.take<int64_t>(rows);
  void* ws = op_ws(st);
  upload(stream_, dx(ws), x, (size_t)rows * V);
  launch_argmax(stream_, dx(ws), rows, V, V, 0, did(ws));
  download(stream_, ids, (const int64_t*)did(ws), rows);
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_pcm_convert(const void* data, int64_t n_values, const pf_pcm_desc& desc, float* out, int64_t cap, int64_t* n_out) {
  const PcmPlan p = pcm_plan(desc, fc_.fs, n_values);
  PF_CHECK(data || n_values == 0, PF_ERR_INVALID_ARG, "pcm: null data");
  if (n_out) *n_out = p.n_out;
  if (!out) return;
  PF_CHECK(cap >= p.n_out, PF_ERR_CAPACITY, "pcm_convert: out capacity < " + std::to_string(p.n_out));
  const void* arr[1] = {data};
  const int64_t nn[1] = {n_values};
  stage_pcm(arr, nn, &desc, 1, 1);                       // upload + the pipeline's launch, into the staged-sample layout
  if (p.n_out == 0) return;
  PF_HIP(hipMemcpyAsync(out, ws_audio_.p, (size_t)p.n_out * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));
}

// ---- voice-activity segmentation (k_vad.hip).  ws_tmp_: levels | seg [B, cap, 2] | n [B] | T [B] | off [B]
namespace {
VadParams vad_params(const pf_vad_config& c, int n_mels) {
  // a run is never longer than PF_VAD_MAX_FRAMES: a larger max_len means the same and keeps b + max_len inside int32
  return VadParams{c.floor_pct, c.margin_q, c.abs_level, c.window, c.on_count, c.off_count, c.pad_begin, c.pad_end, c.min_speech,
                   std::min(c.max_len, 2 * PF_VAD_MAX_FRAMES), c.split_search, n_mels};
}
struct VadLayout {
  Field<int32_t> lev, seg, n, T; Field<int64_t> off;
  size_t bytes;
  VadLayout(size_t frames, size_t B, size_t cap) {
    Cursor c;
    lev = c.take<int32_t>(frames); seg = c.take<int32_t>(B * cap * 2); n = c.take<int32_t>(B); T = c.take<int32_t>(B);
    off = c.take<int64_t>(B);
    bytes = c.off;
  }
};
// n [B] first, then the lists of the rows that have one: min(n[b], cap) pairs each
void vad_read_back(hipStream_t s, const void* ws, const VadLayout& L, int B, int cap, int dev_cap, int32_t* seg, int32_t* n) {
  PF_HIP(hipMemcpyAsync(n, L.n(ws), (size_t)B * 4, hipMemcpyDeviceToHost, s));
  PF_HIP(hipStreamSynchronize(s));
  int worst = 0;
  for (int b = 0; b < B; ++b) {
    const int k = std::min(n[b], std::min(cap, dev_cap));
    if (k > 0) PF_HIP(hipMemcpyAsync(seg + (size_t)b * cap * 2, L.seg(ws) + (size_t)b * dev_cap * 2, (size_t)k * 8, hipMemcpyDeviceToHost, s));
    worst = std::max(worst, n[b]);
  }
  PF_HIP(hipStreamSynchronize(s));
  PF_CHECK(worst <= PF_VAD_MAX_SEGMENTS, PF_ERR_CAPACITY, "vad: more than PF_VAD_MAX_SEGMENTS segments");
  PF_CHECK(worst <= cap, PF_ERR_CAPACITY, "vad: capacity " + std::to_string(cap) + " < " + std::to_string(worst) + " segments");
}
}  // namespace

void Engine::op_vad_levels(const float* rows, int64_t T, int n_mels, int32_t* out) {
  PF_HIP(hipSetDevice(device_));
  if (T == 0) return;
  Cursor c;
  const Field<float> d_x = c.take<float>((size_t)T * n_mels + 4);
  c.off = (size_t)round_up((int64_t)c.off, 16);
  const Field<int32_t> d_e = c.take<int32_t>((size_t)T);
  ensure(ws_tmp_, c.off);
  void* ws = ws_tmp_.p;
  PF_HIP(hipMemcpyAsync(d_x(ws), rows, (size_t)T * n_mels * 4, hipMemcpyHostToDevice, stream_));
  launch_vad_levels(stream_, d_x(ws), T, n_mels, d_e(ws));
  PF_HIP(hipMemcpyAsync(out, d_e(ws), (size_t)T * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_vad_segments(const int32_t* levels, const int32_t* T, int B, int ld, int n_mels, const pf_vad_config* cfg, int32_t* seg,
                             int cap, int32_t* n) {
  const pf_vad_config c = vad_check(cfg, fc_.lfr_n);
  for (int b = 0; b < B; ++b) {
    PF_CHECK(T[b] >= 0 && T[b] <= ld, PF_ERR_INVALID_ARG, "vad_segments: T[b] outside 0 .. ld");
    PF_CHECK(T[b] <= PF_VAD_MAX_FRAMES, PF_ERR_CAPACITY, "vad: more than PF_VAD_MAX_FRAMES frames");
  }
  PF_HIP(hipSetDevice(device_));
  if (B == 0) return;
  const int dev_cap = std::max(std::min(cap, PF_VAD_MAX_SEGMENTS), 1);
  const VadLayout L((size_t)B * ld, B, dev_cap);
  ensure(ws_tmp_, L.bytes);
  void* ws = ws_tmp_.p;
  std::vector<int64_t> off((size_t)B);
  for (int b = 0; b < B; ++b) off[b] = (int64_t)b * ld;
  if ((int64_t)B * ld > 0) PF_HIP(hipMemcpyAsync(L.lev(ws), levels, (size_t)B * ld * 4, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(L.T(ws), T, (size_t)B * 4, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(L.off(ws), off.data(), (size_t)B * 8, hipMemcpyHostToDevice, stream_));
  launch_vad_segments(stream_, L.lev(ws), L.off(ws), L.T(ws), B, vad_params(c, n_mels), L.seg(ws), dev_cap, L.n(ws));
  vad_read_back(stream_, ws, L, B, cap, dev_cap, seg, n);         // (waits for the stream: `off` is read by its copy until then)
}

// ---- streaming endpointing (k_endpoint.hip).  The levels behind n_new[b] are hostile, every output is sentinel-filled: the
// counts and the status must have been written, of a stream's events exactly the first min(n, cap) rows.
void Engine::op_endpoint_update(int32_t* states, const int32_t* levels, const int32_t* n_new, const int32_t* flush, int B, int ld,
                                int n_mels, const pf_endpoint_config* cfg, int32_t* events, int cap, int32_t* n_events,
                                int32_t* in_speech, int32_t* open_begin) {
  const pf_endpoint_config c = endpoint_check(cfg, fc_.lfr_n);
  for (int b = 0; b < B; ++b) {
    PF_CHECK(n_new[b] >= 0 && n_new[b] <= ld, PF_ERR_INVALID_ARG, "endpoint_update: n_new[b] outside 0 .. ld");
    endpoint_admit(states + (size_t)b * PF_ENDPOINT_STATE_INTS, n_new[b]);
  }
  PF_HIP(hipSetDevice(device_));
  if (B == 0) return;
  const int dev_cap = std::max(cap, 1);
  const size_t nB = (size_t)B;
  StageCarve st;
  const auto d_state = st.take<int32_t>(nB * PF_ENDPOINT_STATE_INTS), d_lev = st.take<int32_t>(nB * ld + 1), d_new = st.take<int32_t>(nB),
             d_flush = st.take<int32_t>(nB), d_ev = st.take<int32_t>(nB * dev_cap * 3), d_out = st.take<int32_t>(3 * nB);
  void* ws = op_ws(st);
  std::vector<int32_t> lev(nB * ld + 1), fl(nB, 0);
  for (size_t i = 0; i < lev.size(); ++i) lev[i] = hostile_i32(i);
  for (int b = 0; b < B; ++b) {
    if (n_new[b] > 0) std::memcpy(&lev[(size_t)b * ld], levels + (size_t)b * ld, (size_t)n_new[b] * 4);
    if (flush) fl[b] = flush[b];
  }
  upload(stream_, d_state(ws), (const int32_t*)states, d_state.count);
  upload(stream_, d_lev(ws), (const int32_t*)lev.data(), lev.size());
  upload(stream_, d_new(ws), n_new, nB);
  upload(stream_, d_flush(ws), (const int32_t*)fl.data(), nB);
  fill_sentinel(stream_, d_ev(ws), d_ev.count);
  fill_sentinel(stream_, d_out(ws), d_out.count);
  const EndpointParams p{c.rise, c.margin_q, c.abs_level, c.window, c.on_count, c.off_count, c.pad_begin, c.pad_end, c.end_silence,
                         c.min_speech, c.max_len, n_mels};
  prof_begin("endpoint", 0);
  launch_endpoint_update(stream_, d_state(ws), nullptr, d_lev(ws), nullptr, ld, d_new(ws), d_flush(ws), B, p, d_ev(ws), dev_cap, d_out(ws), d_out(ws) + nB,
                         d_out(ws) + 2 * nB);
  prof_end("endpoint");
  const std::vector<uint32_t> out = check_guard<uint32_t>(stream_, "endpoint_update: n_events | in_speech | open_begin", d_out(ws), kSentinel32,
                                                          result_geom(3 * B, 3 * B, 1, 1, 3 * B));
  std::vector<uint32_t> evh(d_ev.count);                         // the guard rule is applied per stream below
  download(stream_, (int32_t*)evh.data(), (const int32_t*)d_ev(ws), d_ev.count);
  download(stream_, states, (const int32_t*)d_state(ws), d_state.count);
  PF_HIP(hipStreamSynchronize(stream_));
  int worst = 0;
  for (int b = 0; b < B; ++b) {
    const int n = (int)out[b], k = std::min(n, dev_cap);
    PF_CHECK(n >= 0, PF_ERR_DEVICE, "endpoint_update: a negative event count");
    const uint32_t* e = evh.data() + (size_t)b * dev_cap * 3;
    if (const GuardHit hit = guard_scan<uint32_t>(e, nullptr, kSentinel32, result_geom(dev_cap, k, 3, 3, k)))
      throw Error(PF_ERR_DEVICE, guard_message("endpoint_update: events of stream " + std::to_string(b), result_geom(dev_cap, k, 3, 3, k), hit));
    n_events[b] = n; in_speech[b] = (int32_t)out[nB + b]; open_begin[b] = (int32_t)out[2 * nB + b];
    const int kc = std::min(n, cap);
    if (kc > 0) std::memcpy(events + (size_t)b * cap * 3, e, (size_t)kc * 12);
    worst = std::max(worst, n);
  }
  PF_CHECK(worst <= cap, PF_ERR_CAPACITY, "endpoint: capacity " + std::to_string(cap) + " < " + std::to_string(worst) + " events");
}

void Engine::endpoint_streams(int32_t* states_dev, const int32_t* slot, const float* rows, const int32_t* n_new, const int32_t* flush, int B,
                              const pf_endpoint_config& c, int cap, std::vector<int32_t>& out, char* net_states_dev) {
  PF_HIP(hipSetDevice(device_));
  out.clear();
  if (B == 0) return;
  PF_CHECK(!net_states_dev || vadnet_, PF_ERR_INVALID_ARG, "endpoint_streams: no model is attached");
  const size_t nB = (size_t)B, nm = (size_t)fc_.n_mels;
  const size_t meta_words = (4 * nB + 63) / 64 * 64;            // the rows behind the meta words start on a 256-byte boundary
  std::vector<int32_t> stage(meta_words, 0);
  size_t total = 0;
  for (int b = 0; b < B; ++b) {
    stage[b] = n_new[b]; stage[nB + b] = flush[b]; stage[2 * nB + b] = slot[b]; stage[3 * nB + b] = (int32_t)total;
    total += (size_t)n_new[b];
  }
  stage.resize(meta_words + total * nm);
  if (total) std::memcpy(stage.data() + meta_words, rows, total * nm * 4);
  StageCarve st;
  // with the model a stream's levels are its released ones: a row of lev_ld = max n_new + right cells per stream
  const size_t lev_ld = net_states_dev ? (size_t)*std::max_element(n_new, n_new + B) + (size_t)vadnet_->lfr_m : 0;
  const auto d_in = st.take<int32_t>(stage.size() + 4), d_lev = st.take<int32_t>(net_states_dev ? nB * lev_ld + nB : total + 1),
             d_out = st.take<int32_t>(3 * nB + nB * cap * 3);
  void* ws = op_ws(st);
  upload(stream_, d_in(ws), (const int32_t*)stage.data(), stage.size());
  const EndpointParams p{c.rise, c.margin_q, c.abs_level, c.window, c.on_count, c.off_count, c.pad_begin, c.pad_end, c.end_silence,
                         c.min_speech, c.max_len, fc_.n_mels};
  if (net_states_dev) {                                          // the released counts sit behind the level rows
    int32_t* d_rel = d_lev(ws) + nB * lev_ld;
    run_vadnet_stream(net_states_dev, d_in(ws) + 2 * nB, (const float*)(d_in(ws) + meta_words), d_in(ws) + 3 * nB, 0, d_in(ws), d_in(ws) + nB, B,
                      nullptr, d_lev(ws), (int64_t)lev_ld, d_rel);
    prof_begin("endpoint", 0);
    launch_endpoint_update(stream_, states_dev, d_in(ws) + 2 * nB, d_lev(ws), nullptr, (int64_t)lev_ld, d_rel, d_in(ws) + nB, B, p,
                           d_out(ws) + 3 * nB, cap, d_out(ws), d_out(ws) + nB, d_out(ws) + 2 * nB);
    prof_end("endpoint");
  } else {
    if (total) {
      prof_begin("endpoint", 0);
      launch_vad_levels(stream_, (const float*)(d_in(ws) + meta_words), (int64_t)total, fc_.n_mels, d_lev(ws));
      prof_end("endpoint");
    }
    prof_begin("endpoint", 0);
    launch_endpoint_update(stream_, states_dev, d_in(ws) + 2 * nB, d_lev(ws), d_in(ws) + 3 * nB, 0, d_in(ws), d_in(ws) + nB, B, p,
                           d_out(ws) + 3 * nB, cap, d_out(ws), d_out(ws) + nB, d_out(ws) + 2 * nB);
    prof_end("endpoint");
  }
  out.resize(d_out.count);
  download(stream_, out.data(), (const int32_t*)d_out(ws), d_out.count);
  PF_HIP(hipStreamSynchronize(stream_));
}

// ---- the carried CIF of the streaming path (k_cif_stream.hip).  The alphas travel with the pipeline's row stride Tc + 1, the
// cell behind each row hostile, like the rows behind the encoder output; every output is sentinel-filled and must have been
// written everywhere (the kernel zeroes what it does not fire); the cells behind the state blocks must keep their bits.
void Engine::op_online_cif_step(void* states, const float* enc, const float* alphas, const int32_t* reset, int B, int Tc, int D, float threshold,
                                int lo, int hi, float* fired, int32_t* fire_entry, int cap, int32_t* counts) {
  PF_CHECK(states && enc && alphas && reset && fired && fire_entry && counts, PF_ERR_INVALID_ARG, "online_cif_step: null pointer");
  PF_CHECK(B > 0 && Tc > 0 && D > 0 && D % 4 == 0 && cap >= Tc + 1, PF_ERR_INVALID_ARG,
           "online_cif_step: B, Tc > 0, D % 4 == 0 and cap >= Tc + 1 expected");
  PF_HIP(hipSetDevice(device_));
  const size_t nB = (size_t)B, sb = block_at_zero<CifStreamBlock>(D).bytes(), lda = (size_t)Tc + 1, tail = 64;
  StageCarve st;
  const auto d_state = st.take<uint32_t>(nB * sb / 4 + tail);
  const auto d_enc = st.take<float>(nB * Tc * D + (size_t)D), d_al = st.take<float>(nB * lda), d_fired = st.take<float>(nB * cap * D);
  const auto d_reset = st.take<int32_t>(nB), d_ent = st.take<int32_t>(nB * cap), d_cnt = st.take<int32_t>(nB);
  void* ws = op_ws(st);
  std::vector<float> e(d_enc.count), al(d_al.count);
  for (size_t i = 0; i < e.size(); ++i) e[i] = hostile32(i);
  std::memcpy(e.data(), enc, nB * Tc * D * 4);
  for (size_t i = 0; i < al.size(); ++i) al[i] = hostile32(i);
  for (int b = 0; b < B; ++b) std::memcpy(&al[(size_t)b * lda], alphas + (size_t)b * Tc, (size_t)Tc * 4);
  fill_sentinel(stream_, d_state(ws), d_state.count);
  upload(stream_, d_state(ws), (const uint32_t*)states, nB * sb / 4);
  upload(stream_, d_enc(ws), (const float*)e.data(), e.size());
  upload(stream_, d_al(ws), (const float*)al.data(), al.size());
  upload(stream_, d_reset(ws), reset, nB);
  fill_sentinel(stream_, d_fired(ws), d_fired.count);
  fill_sentinel(stream_, d_ent(ws), d_ent.count);
  fill_sentinel(stream_, d_cnt(ws), d_cnt.count);
  CifStreamLaunch c{};
  c.states = (char*)d_state(ws); c.state_stride = (int64_t)sb; c.slot = nullptr;
  c.enc = d_enc(ws); c.alphas = d_al(ws); c.lda = (int)lda; c.reset = d_reset(ws);
  c.B = B; c.Tc = Tc; c.D = D; c.threshold = threshold; c.lo = lo; c.hi = hi;
  c.fired = d_fired(ws); c.fire_entry = d_ent(ws); c.cap = cap; c.counts = d_cnt(ws);
  prof_begin("cif_stream", 0);
  launch_cif_stream(stream_, c);
  prof_end("cif_stream");
  const int rows = B * cap;
  const std::vector<uint32_t> hf = check_guard<uint32_t>(stream_, "online_cif_step: fired", d_fired(ws), kSentinel32, result_geom(rows, rows, D, D, rows));
  const std::vector<uint32_t> he = check_guard<uint32_t>(stream_, "online_cif_step: fire_entry", d_ent(ws), kSentinel32, result_geom(rows, rows, 1, 1, rows));
  const std::vector<uint32_t> hc = check_guard<uint32_t>(stream_, "online_cif_step: counts", d_cnt(ws), kSentinel32, result_geom(B, B, 1, 1, B));
  check_guard<uint32_t>(stream_, "online_cif_step: behind the state blocks", d_state(ws) + nB * sb / 4, kSentinel32, untouched_geom((int64_t)tail));
  for (int b = 0; b < B; ++b) PF_CHECK((int32_t)hc[b] >= 0 && (int32_t)hc[b] <= Tc + 1, PF_ERR_DEVICE, "online_cif_step: a count outside 0 .. Tc + 1");
  download(stream_, (uint32_t*)states, (const uint32_t*)d_state(ws), nB * sb / 4);
  PF_HIP(hipStreamSynchronize(stream_));
  std::memcpy(fired, hf.data(), hf.size() * 4);
  std::memcpy(fire_entry, he.data(), he.size() * 4);
  std::memcpy(counts, hc.data(), hc.size() * 4);
}

void Engine::vad_segment(const float* const* samples, const int64_t* n, int B, const pf_vad_config* cfg, int32_t* seg, int cap,
                         int32_t* n_seg) {
  vad_check(cfg, fc_.lfr_n);
  PF_CHECK(!fc_.snip_edges, PF_ERR_UNSUPPORTED, "vad: snip_edges = true is not supported");
  stage_audio(samples, n, B);
  vad_staged(cfg, seg, cap, n_seg);
}

void Engine::vad_segment_device(const float* const* samples_dev, const int64_t* n, int B, const pf_vad_config* cfg, int32_t* seg, int cap,
                                int32_t* n_seg) {
  vad_check(cfg, fc_.lfr_n);
  PF_CHECK(!fc_.snip_edges, PF_ERR_UNSUPPORTED, "vad: snip_edges = true is not supported");
  stage_device_audio(samples_dev, n, B);
  vad_staged(cfg, seg, cap, n_seg);
}

// the staged utterances (host or device audio): run_staged's fbank launch, the detector, the lists back
void Engine::vad_staged(const pf_vad_config* cfg, int32_t* seg, int cap, int32_t* n_seg) {
  const pf_vad_config c = vad_check(cfg, fc_.lfr_n);
  const int B = st_B_;
  if (B == 0) return;
  for (int b = 0; b < B; ++b) PF_CHECK(st_t80_[b] <= PF_VAD_MAX_FRAMES, PF_ERR_CAPACITY, "vad: more than PF_VAD_MAX_FRAMES frames");
  const int64_t* meta = (const int64_t*)ws_meta_.p;
  const int32_t* t80d = (const int32_t*)((const char*)ws_meta_.p + 3 * (size_t)(B + 1) * 8);
  const int dev_cap = std::max(std::min(cap, PF_VAD_MAX_SEGMENTS), 1);
  const VadLayout L((size_t)st_total_frames_, B, dev_cap);
  ensure(ws_tmp_, L.bytes);
  void* ws = ws_tmp_.p;
  if (st_total_frames_ > 0) {
    ensure(ws_fbank_, (size_t)st_total_frames_ * fc_.n_mels * 4);
    prof_begin("fbank", 0);
    launch_fbank(stream_, fb_, st_audio_ext_ ? st_audio_ext_ : (const float*)ws_audio_.p, meta, meta + (B + 1), meta + 2 * (B + 1), B,
                 st_total_frames_, 0, (float*)ws_fbank_.p, fc_.dither, next_dither_seed());
    prof_end("fbank");
  }
  if (vadnet_) {
    run_vadnet((const float*)ws_fbank_.p, meta + 2 * (B + 1), B, st_total_frames_, fc_.n_mels, nullptr, L.lev(ws));
  } else {
    prof_begin("vad", 0);
    launch_vad_levels(stream_, (const float*)ws_fbank_.p, st_total_frames_, fc_.n_mels, L.lev(ws));
    prof_end("vad");
  }
  prof_begin("vad", 0);
  launch_vad_segments(stream_, L.lev(ws), meta + 2 * (B + 1), t80d, B, vad_params(c, fc_.n_mels), L.seg(ws), dev_cap, L.n(ws));
  prof_end("vad");
  vad_read_back(stream_, ws, L, B, cap, dev_cap, seg, n_seg);
}

// ---- attach / detach of an auxiliary network (the FSMN-VAD model, the punctuation model): `on` is the attached model, `dev`
// its image on the device with the model it was uploaded from, `ws` the workspace its runs grow.  nullptr detaches: nothing
// of the network stays allocated.  The stream is synchronised before an image is replaced and before anything is freed: a
// queued launch may still read the image or the workspace.
template <class M>
void Engine::attach_model(std::shared_ptr<const M>& on, ModelDev<M>& dev, DevBuf& ws, const std::shared_ptr<const M>& m) {
  if (!m) {
    on.reset();
    dev.src.reset();
    if (dev.buf.p || ws.p) {
      PF_HIP(hipSetDevice(device_));
      PF_HIP(hipStreamSynchronize(stream_));
      for (DevBuf* b : {&dev.buf, &ws})
        if (b->p) { PF_HIP(hipFree(b->p)); b->p = nullptr; b->bytes = 0; }
    }
    return;
  }
  PF_HIP(hipSetDevice(device_));
  if (dev.src != m) {
    PF_HIP(hipStreamSynchronize(stream_));
    dev.src.reset();
    ensure(dev.buf, m->image.size());
    PF_HIP(hipMemcpyAsync(dev.buf.p, m->image.data(), m->image.size(), hipMemcpyHostToDevice, stream_));
    PF_HIP(hipStreamSynchronize(stream_));
    dev.src = m;
  }
  on = m;
}

// ---- the FSMN-VAD model score (k_vadnet.hip; the launch plan is at the head of that file)
void Engine::set_vad_model(const std::shared_ptr<const VadModel>& m) {
  if (m) {
    PF_CHECK((int64_t)fc_.n_mels * m->lfr_m == m->input_dim, PF_ERR_INVALID_ARG,
             "set_vad_model: n_mels * lfr_m does not equal the model's input width");
    PF_CHECK(!fc_.snip_edges, PF_ERR_UNSUPPORTED, "set_vad_model: snip_edges = true is not supported");
  }
  attach_model(vadnet_, vadnet_dev_, ws_vadnet_, m);
}

void Engine::run_vadnet(const float* rows_dev, const int64_t* off_dev, int B, int64_t total, int n_mels, float* logits_dev,
                        int32_t* levels_dev) {
  const VadModel& m = *vadnet_;
  PF_CHECK((int64_t)n_mels * m.lfr_m == m.input_dim, PF_ERR_INVALID_ARG, "vad model: n_mels * lfr_m does not equal the model's input width");
  if (total <= 0 || B <= 0) return;
  const size_t pbytes = (size_t)round_up((int64_t)total * m.ldp * 4, 256);
  ensure(ws_vadnet_, 2 * pbytes);
  float* p[2] = {(float*)ws_vadnet_.p, (float*)((char*)ws_vadnet_.p + pbytes)};
  for (int l = 0; l <= m.n_layers; ++l) {
    VadNetLaunch a{};
    a.img = (const char*)vadnet_dev_.buf.p; a.off = off_dev; a.B = B; a.total = total; a.ld = m.lds_ld;
    a.ldp = m.ldp; a.lorder = m.lorder; a.lstride = m.lstride;
    double flops = 0;
    auto mid = [&](const TileGemm& g, bool relu) { a.mid[a.n_mid] = g; a.mid_relu[a.n_mid] = relu ? 1 : 0; ++a.n_mid; flops += 2.0 * g.Npad * g.Kpad; };
    if (l == 0) {
      a.head = 0; a.head_w = m.g_in1.Kpad;
      a.x = rows_dev; a.n_mels = n_mels; a.lfr_m = m.lfr_m; a.in_dim = m.input_dim; a.shift_off = m.shift_off; a.scale_off = m.scale_off;
      mid(m.g_in1, false); mid(m.g_in2, true);
    } else {
      a.head = 1; a.head_w = m.g_aff[l - 1].Kpad;
      a.p_in = p[(l - 1) & 1]; a.taps_off = m.taps_off[l - 1];
      mid(m.g_aff[l - 1], true);
    }
    if (l < m.n_layers) {
      a.tail = 0; a.last = m.g_lin[l]; a.p_out = p[l & 1];
    } else {
      mid(m.g_out1, false);
      a.tail = 1; a.last = m.g_out2; a.sil_off = m.sil_off; a.out_dim = m.output_dim; a.logits = logits_dev; a.levels = levels_dev;
    }
    flops += 2.0 * a.last.Npad * a.last.Kpad;
    prof_begin("vadnet", flops * (double)total);
    launch_vadnet(stream_, a);
    prof_end("vadnet");
  }
}

void Engine::op_vad_model(const float* rows, const int32_t* T, int B, int n_mels, float* logits, int32_t* levels) {
  PF_CHECK(vadnet_ != nullptr, PF_ERR_INVALID_ARG, "op_vad_model: no model is attached (pf_engine_set_vad_model)");
  PF_CHECK((int64_t)n_mels * vadnet_->lfr_m == vadnet_->input_dim, PF_ERR_INVALID_ARG,
           "op_vad_model: n_mels * lfr_m does not equal the model's input width");
  std::vector<int64_t> off((size_t)B + 1, 0);
  for (int b = 0; b < B; ++b) {
    PF_CHECK(T[b] >= 0, PF_ERR_INVALID_ARG, "op_vad_model: negative frame count");
    PF_CHECK(T[b] <= PF_VAD_MAX_FRAMES, PF_ERR_CAPACITY, "vad: more than PF_VAD_MAX_FRAMES frames");
    off[b + 1] = off[b] + T[b];
  }
  PF_HIP(hipSetDevice(device_));
  const int64_t total = off[(size_t)B];
  if (total == 0) return;
  const int O = vadnet_->output_dim;
  Cursor c;
  const Field<float> d_x = c.take<float>((size_t)total * n_mels + 4);
  const Field<int64_t> d_off = c.take<int64_t>((size_t)B + 1);
  const Field<int32_t> d_e = c.take<int32_t>((size_t)total);
  c.off = (size_t)round_up((int64_t)c.off, 16);
  const Field<float> d_z = c.take<float>(logits ? (size_t)total * O : 0);
  ensure(ws_tmp_, c.off);
  void* ws = ws_tmp_.p;
  PF_HIP(hipMemcpyAsync(d_x(ws), rows, (size_t)total * n_mels * 4, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(d_off(ws), off.data(), off.size() * 8, hipMemcpyHostToDevice, stream_));
  run_vadnet(d_x(ws), d_off(ws), B, total, n_mels, logits ? d_z(ws) : nullptr, d_e(ws));
  if (logits) PF_HIP(hipMemcpyAsync(logits, d_z(ws), (size_t)total * O * 4, hipMemcpyDeviceToHost, stream_));
  if (levels) PF_HIP(hipMemcpyAsync(levels, d_e(ws), (size_t)total * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));                          // (`off` is read by its copy until then)
}

// ---- the FSMN-VAD model score, streaming (k_vadnet_stream.hip): ONE launch for B streams
void Engine::vad_stream_check(const VadModel& m) {
  PF_CHECK(vadnet_stream_lds_bytes(m.lds_ld, m.ldp, (m.lorder - 1) * m.lstride) <= kVadStreamMaxLds, PF_ERR_UNSUPPORTED,
           "vad model stream: two [64, widest + 8] f16 tiles and the [(lorder - 1) * lstride + 64, proj + 4] fp32 window exceed 159 744 bytes of LDS");
}

void Engine::run_vadnet_stream(char* states_dev, const int32_t* slot_dev, const float* rows_dev, const int32_t* off_dev, int64_t ldx,
                               const int32_t* n_new_dev, const int32_t* flush_dev, int B, float* logits_dev, int32_t* levels_dev,
                               int64_t cap, int32_t* n_out_dev) {
  const VadModel& m = *vadnet_;
  vad_stream_check(m);
  if (B <= 0) return;
  VadNetStreamLaunch a{};
  a.img = (const char*)vadnet_dev_.buf.p; a.ld = m.lds_ld; a.ldp = m.ldp; a.ldw = m.ldp + 4;
  a.n_layers = m.n_layers; a.lorder = m.lorder; a.lstride = m.lstride; a.reach = (m.lorder - 1) * m.lstride;
  a.states = states_dev; a.state_bytes = vad_stream_layout(m).bytes; a.words_off = vad_stream_layout(m).words_off; a.slot = slot_dev;
  a.x = rows_dev; a.off = off_dev; a.ldx = ldx; a.n_mels = m.input_dim / m.lfr_m; a.lfr_m = m.lfr_m; a.in_dim = m.input_dim;
  a.shift_off = m.shift_off; a.scale_off = m.scale_off;
  a.n_new = n_new_dev; a.flush = flush_dev;
  a.in1 = m.g_in1; a.in2 = m.g_in2; a.out1 = m.g_out1; a.out2 = m.g_out2;
  for (int l = 0; l < m.n_layers; ++l) { a.lin[l] = m.g_lin[(size_t)l]; a.aff[l] = m.g_aff[(size_t)l]; a.taps_off[l] = m.taps_off[(size_t)l]; }
  a.sil_off = m.sil_off; a.out_dim = m.output_dim; a.logits = logits_dev; a.levels = levels_dev; a.cap = cap; a.n_out = n_out_dev;
  prof_begin("vadnet_stream", 0);
  launch_vadnet_stream(stream_, a, B);
  prof_end("vadnet_stream");
}

void Engine::op_vad_model_stream(void* states, const float* rows, const int32_t* n_new, const int32_t* flush, int B, int ld, int n_mels,
                                 int32_t* levels, float* logits, int cap, int32_t* n_out) {
  PF_CHECK(vadnet_ != nullptr, PF_ERR_INVALID_ARG, "op_vad_model_stream: no model is attached (pf_engine_set_vad_model)");
  const VadModel& m = *vadnet_;
  PF_CHECK((int64_t)n_mels * m.lfr_m == m.input_dim, PF_ERR_INVALID_ARG,
           "op_vad_model_stream: n_mels * lfr_m does not equal the model's input width");
  vad_stream_check(m);
  const VadStreamLayout L = vad_stream_layout(m);
  const size_t nB = (size_t)B, sbytes = (size_t)L.bytes, O = (size_t)m.output_dim;
  std::vector<int32_t> want(nB, 0), fl(nB, 0);
  for (int b = 0; b < B; ++b) {                                  // every stream is admitted before anything changes
    PF_CHECK(n_new[b] >= 0 && n_new[b] <= ld, PF_ERR_INVALID_ARG, "op_vad_model_stream: n_new[b] outside 0 .. ld");
    int32_t words[2];
    std::memcpy(words, (const char*)states + b * sbytes + L.words_off, 8);
    vad_stream_admit(words[0], words[1], n_new[b]);
    if (flush) fl[(size_t)b] = flush[b] != 0;
    want[(size_t)b] = (int32_t)(vad_stream_released(m, (int64_t)words[0] + n_new[b], fl[(size_t)b] || words[1]) -
                                vad_stream_released(m, words[0], words[1] != 0));
    PF_CHECK(want[(size_t)b] <= cap, PF_ERR_CAPACITY,
             "vad model stream: capacity " + std::to_string(cap) + " < " + std::to_string(want[(size_t)b]) + " released levels");
  }
  PF_HIP(hipSetDevice(device_));
  if (B == 0) return;
  const size_t dev_cap = (size_t)std::max(cap, 1), row_cells = (size_t)ld * n_mels;
  StageCarve st;
  const auto d_state = st.take<char>(nB * sbytes);
  const auto d_x = st.take<float>(nB * row_cells + 4);
  const auto d_new = st.take<int32_t>(nB), d_flush = st.take<int32_t>(nB), d_lev = st.take<int32_t>(nB * dev_cap);
  const auto d_z = st.take<float>(logits ? nB * dev_cap * O : 0);
  const auto d_out = st.take<int32_t>(nB);
  void* ws = op_ws(st);
  std::vector<float> x(nB * row_cells + 4);                      // hostile behind every stream's n_new rows
  for (size_t i = 0; i < x.size(); ++i) x[i] = hostile32(i);
  for (int b = 0; b < B; ++b)
    if (n_new[b] > 0) std::memcpy(&x[b * row_cells], rows + b * row_cells, (size_t)n_new[b] * n_mels * 4);
  upload(stream_, d_state(ws), (const char*)states, d_state.count);
  upload(stream_, d_x(ws), (const float*)x.data(), x.size());
  upload(stream_, d_new(ws), n_new, nB);
  upload(stream_, d_flush(ws), (const int32_t*)fl.data(), nB);
  fill_sentinel(stream_, d_lev(ws), d_lev.count);
  if (logits) fill_sentinel(stream_, d_z(ws), d_z.count);
  fill_sentinel(stream_, d_out(ws), d_out.count);
  run_vadnet_stream(d_state(ws), nullptr, d_x(ws), nullptr, ld, d_new(ws), d_flush(ws), B, logits ? d_z(ws) : nullptr, d_lev(ws),
                    (int64_t)dev_cap, d_out(ws));
  const std::vector<uint32_t> out = check_guard<uint32_t>(stream_, "vad_model_stream: n_out", d_out(ws), kSentinel32, result_geom(B, B, 1, 1, B));
  std::vector<uint32_t> lev(d_lev.count), z(d_z.count);          // the guard rule is applied per stream below
  download(stream_, (int32_t*)lev.data(), (const int32_t*)d_lev(ws), d_lev.count);
  if (logits) download(stream_, (float*)z.data(), (const float*)d_z(ws), d_z.count);
  PF_HIP(hipStreamSynchronize(stream_));
  for (int b = 0; b < B; ++b) {
    const int k = (int)out[(size_t)b];
    PF_CHECK(k == want[(size_t)b], PF_ERR_DEVICE, "vad_model_stream: stream " + std::to_string(b) + " released " + std::to_string(k) +
                                                      " levels where the schedule says " + std::to_string(want[(size_t)b]));
    const GuardGeom gl = result_geom((int64_t)dev_cap, k, 1, 1, k);
    if (const GuardHit hit = guard_scan<uint32_t>(lev.data() + b * dev_cap, nullptr, kSentinel32, gl))
      throw Error(PF_ERR_DEVICE, guard_message("vad_model_stream: levels of stream " + std::to_string(b), gl, hit));
    if (logits) {                                                // (a logit may be a NaN, never the sentinel's payload)
      const GuardGeom gz = result_geom((int64_t)dev_cap, k, (int)O, (int)O, k);
      if (const GuardHit hit = guard_scan<uint32_t>(z.data() + b * dev_cap * O, nullptr, kSentinel32, gz))
        throw Error(PF_ERR_DEVICE, guard_message("vad_model_stream: logits of stream " + std::to_string(b), gz, hit));
    }
  }
  download(stream_, (char*)states, (const char*)d_state(ws), d_state.count);
  PF_HIP(hipStreamSynchronize(stream_));
  for (int b = 0; b < B; ++b) {
    const size_t k = (size_t)want[(size_t)b];
    n_out[b] = (int32_t)k;
    if (levels && k) std::memcpy(levels + (size_t)b * cap, lev.data() + b * dev_cap, k * 4);
    if (logits && k) std::memcpy(logits + (size_t)b * cap * O, z.data() + b * dev_cap * O, k * O * 4);
  }
}

// ---- the CAM++ speaker model (k_spk.hip; the launch plan is at the head of that file)
void Engine::set_spk_model(const std::shared_ptr<const SpkModel>& m) {
  if (m) PF_CHECK(fc_.n_mels == m->n_mels, PF_ERR_INVALID_ARG, "set_spk_model: the model's n_mels is not the front-end's");
  attach_model(spk_, spk_dev_, ws_spk_, m);
}

namespace {
struct SpkScratch { size_t act[3], frames, X[4], total; };
SpkScratch spk_scratch(const SpkModel& m, int64_t total, int64_t totalp) {
  SpkScratch s{};
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += (size_t)round_up((int64_t)bytes + 16, 256); return at; };   // (+ 16: a vector read may pass the last row's end)
  for (int i = 0; i < 3; ++i) s.act[i] = take((size_t)total * (i == 0 ? m.n_mels : m.n_mels / 2) * m.m * sizeof(half_t));
  s.frames = take((size_t)total * m.frame_ld * sizeof(half_t));
  for (int i = 0; i < 4; ++i) s.X[i] = take((size_t)totalp * m.ldx[i] * sizeof(half_t));
  s.total = off;
  return s;
}
}  // namespace

size_t Engine::spk_scratch_bytes(const SpkModel& m, int64_t total, int64_t totalp) { return spk_scratch(m, total, totalp).total; }

void Engine::run_spk(const float* rows_dev, const int32_t* T_dev, const int64_t* toff_dev, const int64_t* tpoff_dev, const int64_t* xoff_dev, int B,
                     int Tmax, int64_t total, int64_t totalp, char* scratch, float* emb_dev, float* frames_dev) {
  const SpkModel& m = *spk_;
  if (B <= 0) return;
  const SpkScratch sc = spk_scratch(m, total, totalp);
  half_t* act[3] = {(half_t*)(scratch + sc.act[0]), (half_t*)(scratch + sc.act[1]), (half_t*)(scratch + sc.act[2])};
  half_t* frames = (half_t*)(scratch + sc.frames);
  half_t* X[4] = {(half_t*)(scratch + sc.X[0]), (half_t*)(scratch + sc.X[1]), (half_t*)(scratch + sc.X[2]), (half_t*)(scratch + sc.X[3])};
  const SpkWin w{(const char*)spk_dev_.buf.p, T_dev, toff_dev, tpoff_dev, xoff_dev, B, Tmax};
  // every class "spk" launch is timed even where the call has no frame: the count is the model's, not the call's
  const double share = m.flops_per_frame * (double)total / kSpkLaunches;
  int F = m.n_mels;
  for (int i = 0; i < 10; ++i) {
    SpkConvLaunch a{};
    a.w = w; a.d = m.conv[i]; a.m = m.m; a.n_mels = m.n_mels; a.frame_ld = m.frame_ld;
    a.Fin = F; a.Fout = F / a.d.sf; F = a.Fout;
    a.x = rows_dev;
    a.in = a.d.in >= 0 ? act[a.d.in] : nullptr;
    a.aux = a.d.aux >= 0 ? act[a.d.aux] : nullptr;
    a.out = a.d.to_frames ? frames : act[a.d.out];
    prof_begin("spk", share);
    launch_spk_conv(stream_, a);
    prof_end("spk");
  }
  {
    SpkTdnnLaunch a{};
    a.w = w; a.g = m.tdnn; a.frame_w = m.frame_w; a.frame_ld = m.frame_ld; a.N = m.init; a.frames = frames; a.X = X[0]; a.ldx = m.ldx[0];
    prof_begin("spk", share);
    launch_spk_tdnn(stream_, a);
    prof_end("spk");
  }
  for (int b = 0; b < 3; ++b) {
    SpkBlockLaunch a{};
    a.w = w; a.layers_off = m.layers_off[b]; a.n_layers = m.blocks[b]; a.growth = m.growth; a.bn = m.bn; a.dilation = m.dilations[b];
    a.seg_len = m.seg_len; a.X = X[b]; a.ldx = m.ldx[b]; a.C1 = m.C1[b]; a.tr_scale_off = m.tr_scale_off[b]; a.tr_shift_off = m.tr_shift_off[b];
    a.transit = m.transit[b]; a.Xn = X[b + 1]; a.ldxn = m.ldx[b + 1];
    prof_begin("spk", share);
    launch_spk_block(stream_, a);
    prof_end("spk");
  }
  {
    SpkPoolLaunch a{};
    a.w = w; a.X = X[3]; a.ldx = m.ldx[3]; a.C = m.c_out; a.scale_off = m.out_scale_off; a.shift_off = m.out_shift_off; a.dense = m.dense;
    a.E = m.embedding; a.emb = emb_dev; a.frames = frames_dev;
    prof_begin("spk", share);
    launch_spk_pool(stream_, a);
    prof_end("spk");
  }
}

void Engine::op_spk_embed(const float* rows, const int32_t* T, int B, int n_mels, float* emb, float* frames) {
  PF_CHECK(spk_ != nullptr, PF_ERR_INVALID_ARG, "op_spk_embed: no model is attached (pf_engine_set_spk_model)");
  PF_CHECK(n_mels == spk_->n_mels, PF_ERR_INVALID_ARG, "op_spk_embed: n_mels is not the model's");
  if (B <= 0) return;
  PF_CHECK(B <= 65535, PF_ERR_CAPACITY, "op_spk_embed: more than 65535 windows in one call");
  const SpkModel& m = *spk_;
  std::vector<int64_t> off(2 * ((size_t)B + 1), 0);                 // toff | tpoff
  int Tmax = 0;
  for (int b = 0; b < B; ++b) {
    PF_CHECK(T[b] >= 0 && T[b] <= PF_SPK_MAX_FRAMES, PF_ERR_INVALID_ARG, "op_spk_embed: a window of fewer than 0 or more than PF_SPK_MAX_FRAMES frames");
    off[(size_t)b + 1] = off[(size_t)b] + T[b];
    off[(size_t)B + 1 + b + 1] = off[(size_t)B + 1 + b] + (T[b] + 1) / 2;
    Tmax = std::max(Tmax, (int)T[b]);
  }
  const int64_t total = off[(size_t)B], totalp = off[2 * (size_t)B + 1];
  PF_HIP(hipSetDevice(device_));
  const int E = m.embedding, C = m.c_out;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t a0 = at; at += (size_t)round_up((int64_t)bytes + 16, 256); return a0; };
  const size_t o_off = take(off.size() * 8), o_T = take((size_t)B * 4), o_x = take((size_t)total * n_mels * 4), o_emb = take((size_t)B * E * 4),
               o_fr = take(frames ? (size_t)totalp * C * 4 : 0), o_scr = take(spk_scratch_bytes(m, total, totalp));
  ensure(ws_spk_, at);
  char* ws = (char*)ws_spk_.p;
  PF_HIP(hipMemcpyAsync(ws + o_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(ws + o_T, T, (size_t)B * 4, hipMemcpyHostToDevice, stream_));
  if (total > 0) PF_HIP(hipMemcpyAsync(ws + o_x, rows, (size_t)total * n_mels * 4, hipMemcpyHostToDevice, stream_));
  run_spk((const float*)(ws + o_x), (const int32_t*)(ws + o_T), (const int64_t*)(ws + o_off), (const int64_t*)(ws + o_off) + B + 1,
          (const int64_t*)(ws + o_off), B, Tmax, total, totalp, ws + o_scr, (float*)(ws + o_emb), frames ? (float*)(ws + o_fr) : nullptr);
  PF_HIP(hipMemcpyAsync(emb, ws + o_emb, (size_t)B * E * 4, hipMemcpyDeviceToHost, stream_));
  if (frames && totalp > 0) PF_HIP(hipMemcpyAsync(frames, ws + o_fr, (size_t)totalp * C * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));                          // (`off` and T are read by their copies until then)
}

void Engine::spk_staged(const int32_t* win, int N, const int32_t* n_utt, float* emb, float* aff) {
  PF_CHECK(spk_ != nullptr, PF_ERR_INVALID_ARG, "spk_staged: no model is attached");
  const SpkModel& m = *spk_;
  const int B = st_B_, E = m.embedding;
  if (N <= 0 || B <= 0) return;
  std::vector<int64_t> first((size_t)B + 1, 0);                     // the first staged frame of every utterance
  for (int b = 0; b < B; ++b) first[(size_t)b + 1] = first[(size_t)b] + st_t80_[b];
  int64_t counted = 0;
  for (int b = 0; b < B; ++b) {
    PF_CHECK(n_utt[b] >= 0 && n_utt[b] <= PF_SPK_MAX_WINDOWS, PF_ERR_INVALID_ARG, "spk_staged: a stream of more than PF_SPK_MAX_WINDOWS windows");
    counted += n_utt[b];
  }
  PF_CHECK(counted == N, PF_ERR_INVALID_ARG, "spk_staged: the windows per utterance do not add up");
  PF_HIP(hipSetDevice(device_));
  // the per-chunk tables and the largest chunk's scratch; a chunk is sized for the call's longest window
  int longest = 1;
  for (int i = 0; i < N; ++i) longest = std::max(longest, (int)std::min<int64_t>(std::max(win[3 * (size_t)i + 2] - win[3 * (size_t)i + 1], 0), PF_SPK_MAX_FRAMES));
  const size_t per_window = spk_scratch_bytes(m, longest, (longest + 1) / 2);
  const int chunk = (int)std::min<size_t>((size_t)std::min(N, 65535), std::max<size_t>(kSpkScratchBudget / per_window, 1));
  std::vector<int64_t> off;                                         // per chunk: toff [n + 1] | tpoff [n + 1] | xoff [n + 1]
  std::vector<int32_t> T((size_t)N);
  size_t scratch = 0;
  std::vector<int> tmax;
  for (int c0 = 0; c0 < N; c0 += chunk) {
    const int n = std::min(chunk, N - c0);
    const size_t at = off.size();
    off.resize(at + 3 * ((size_t)n + 1), 0);
    int64_t* toff = off.data() + at; int64_t* tpoff = toff + n + 1; int64_t* xoff = tpoff + n + 1;
    int mx = 0;
    for (int i = 0; i < n; ++i) {
      const int32_t* w = win + 3 * (size_t)(c0 + i);
      PF_CHECK(w[0] >= 0 && w[0] < B && w[1] >= 0 && w[2] >= w[1] && w[2] <= st_t80_[w[0]] && w[2] - w[1] <= PF_SPK_MAX_FRAMES, PF_ERR_INVALID_ARG,
               "spk_staged: a window outside its utterance or above PF_SPK_MAX_FRAMES frames");
      const int t = w[2] - w[1];
      T[(size_t)(c0 + i)] = t;
      toff[i + 1] = toff[i] + t; tpoff[i + 1] = tpoff[i] + (t + 1) / 2; xoff[i] = first[(size_t)w[0]] + w[1];
      mx = std::max(mx, t);
    }
    tmax.push_back(mx);
    scratch = std::max(scratch, spk_scratch_bytes(m, toff[n], tpoff[n]));
  }
  std::vector<int64_t> aoff(2 * ((size_t)B + 1), 0);                // eoff | ooff
  int nmax = 0;
  for (int b = 0; b < B; ++b) {
    aoff[(size_t)b + 1] = aoff[(size_t)b] + n_utt[b];
    aoff[(size_t)B + 1 + b + 1] = aoff[(size_t)B + 1 + b] + (int64_t)n_utt[b] * n_utt[b];
    nmax = std::max(nmax, (int)n_utt[b]);
  }
  const int64_t cells = aoff[2 * (size_t)B + 1];
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t a0 = at; at += (size_t)round_up((int64_t)bytes + 16, 256); return a0; };
  const size_t o_off = take(off.size() * 8), o_T = take((size_t)N * 4), o_aoff = take(aoff.size() * 8), o_emb = take((size_t)N * E * 4),
               o_aff = take((size_t)cells * 4), o_scr = take(scratch);
  ensure(ws_spk_, at);
  char* ws = (char*)ws_spk_.p;
  PF_HIP(hipMemcpyAsync(ws + o_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(ws + o_T, T.data(), (size_t)N * 4, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(ws + o_aoff, aoff.data(), aoff.size() * 8, hipMemcpyHostToDevice, stream_));
  size_t tab = 0;
  for (int c0 = 0, ci = 0; c0 < N; c0 += chunk, ++ci) {
    const int n = std::min(chunk, N - c0);
    const int64_t* toff = (const int64_t*)(ws + o_off) + tab;
    const int64_t* h_toff = off.data() + tab;
    run_spk((const float*)ws_fbank_.p, (const int32_t*)(ws + o_T) + c0, toff, toff + n + 1, toff + 2 * ((size_t)n + 1), n, tmax[(size_t)ci], h_toff[n],
            h_toff[2 * (size_t)n + 1], ws + o_scr, (float*)(ws + o_emb) + (size_t)c0 * E, nullptr);
    tab += 3 * ((size_t)n + 1);
  }
  if (cells > 0) {
    SpkAffinityLaunch a{(const float*)(ws + o_emb), (const int64_t*)(ws + o_aoff), (const int64_t*)(ws + o_aoff) + B + 1, B, E, nmax, (float*)(ws + o_aff)};
    prof_begin("spk", 6.0 * E * (double)cells);
    launch_spk_affinity(stream_, a);
    prof_end("spk");
    PF_HIP(hipMemcpyAsync(aff, ws + o_aff, (size_t)cells * 4, hipMemcpyDeviceToHost, stream_));
  }
  PF_HIP(hipMemcpyAsync(emb, ws + o_emb, (size_t)N * E * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));                          // (the tables are read by their copies until then)
}

void Engine::op_spk_affinity(const float* emb, const int32_t* n, int S, int E, float* out) {
  if (S <= 0) return;
  std::vector<int64_t> off(2 * ((size_t)S + 1), 0);                 // eoff | ooff
  int nmax = 0;
  for (int s = 0; s < S; ++s) {
    PF_CHECK(n[s] >= 0 && n[s] <= PF_SPK_MAX_WINDOWS, PF_ERR_INVALID_ARG, "op_spk_affinity: a stream of fewer than 0 or more than PF_SPK_MAX_WINDOWS embeddings");
    off[(size_t)s + 1] = off[(size_t)s] + n[s];
    off[(size_t)S + 1 + s + 1] = off[(size_t)S + 1 + s] + (int64_t)n[s] * n[s];
    nmax = std::max(nmax, (int)n[s]);
  }
  const int64_t rows = off[(size_t)S], cells = off[2 * (size_t)S + 1];
  if (cells == 0) return;
  PF_CHECK(S <= 65535 && E >= 1, PF_ERR_CAPACITY, "op_spk_affinity: more than 65535 streams in one call");
  PF_HIP(hipSetDevice(device_));
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t a0 = at; at += (size_t)round_up((int64_t)bytes, 256); return a0; };
  const size_t o_off = take(off.size() * 8), o_e = take((size_t)rows * E * 4), o_s = take((size_t)cells * 4);
  ensure(ws_tmp_, at);
  char* ws = (char*)ws_tmp_.p;
  PF_HIP(hipMemcpyAsync(ws + o_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(ws + o_e, emb, (size_t)rows * E * 4, hipMemcpyHostToDevice, stream_));
  SpkAffinityLaunch a{(const float*)(ws + o_e), (const int64_t*)(ws + o_off), (const int64_t*)(ws + o_off) + S + 1, S, E, nmax, (float*)(ws + o_s)};
  prof_begin("spk", 6.0 * E * (double)cells);
  launch_spk_affinity(stream_, a);
  prof_end("spk");
  PF_HIP(hipMemcpyAsync(out, ws + o_s, (size_t)cells * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));
}

// ---- the CT-Transformer punctuation model (k_punc.hip; the launch plan is at the head of that file)
void Engine::set_punc_model(const std::shared_ptr<const PuncModel>& m) { attach_model(punc_, punc_dev_, ws_punc_, m); }

// one forward over B windows (host arrays in, host arrays out; returns after the results have arrived)
void Engine::run_punc(const int32_t* ids, const int64_t* off, const int32_t* last, int B, float* logits, float* x0, int32_t* p,
                      int32_t* cut) {
  const PuncModel& m = *punc_;
  const int64_t total = off[B];
  for (int b = 0; b < B; ++b)
    PF_CHECK(off[b + 1] >= off[b] && off[b + 1] - off[b] <= PF_PUNC_MAX_WINDOW, PF_ERR_CAPACITY, "punc: a window above PF_PUNC_MAX_WINDOW ids");
  if (total == 0) {                                 // nothing to launch: every window is empty
    if (cut) std::fill(cut, cut + B, -1);
    return;
  }
  const int D = m.d_model, P = m.n_punc, NL = m.n_layers;
  Cursor c;
  const Field<int64_t> d_off = c.take<int64_t>((size_t)B + 1);
  const Field<int32_t> d_ids = c.take<int32_t>((size_t)total), d_last = c.take<int32_t>((size_t)B), d_cut = c.take<int32_t>((size_t)B),
                       d_p = c.take<int32_t>((size_t)total);
  c.off = (size_t)round_up((int64_t)c.off, 256);
  const Field<float> d_x = c.take<float>((size_t)total * D), d_z = c.take<float>((size_t)total * P);
  c.off = (size_t)round_up((int64_t)c.off, 256);
  const Field<half_t> d_q0 = c.take<half_t>((size_t)total * 3 * D), d_q1 = c.take<half_t>((size_t)total * 3 * D),
                      d_ctx = c.take<half_t>((size_t)total * D);
  ensure(ws_punc_, c.off);
  void* ws = ws_punc_.p;
  PF_HIP(hipMemcpyAsync(d_off(ws), off, ((size_t)B + 1) * 8, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(d_ids(ws), ids, (size_t)total * 4, hipMemcpyHostToDevice, stream_));
  if (cut) PF_HIP(hipMemcpyAsync(d_last(ws), last, (size_t)B * 4, hipMemcpyHostToDevice, stream_));
  half_t* qkv[2] = {d_q0(ws), d_q1(ws)};
  const double rows = (double)round_up(total, 64);
  const double f_qkv = 2.0 * 3 * D * D, f_layer = 2.0 * D * D + 4.0 * D * m.ffn;
  auto tail = [&](PuncRowsLaunch& a, int l) {       // what follows layer l - 1 (l = 0: the embedding)
    if (l < NL) {
      a.tail = 0; a.n_g = m.limg[(size_t)l].n1_g; a.n_b = m.limg[(size_t)l].n1_b; a.last = m.limg[(size_t)l].qkv; a.qkv_out = qkv[l & 1];
    } else {
      a.tail = 1; a.n_g = m.after_g_off; a.n_b = m.after_b_off; a.last = m.dec; a.n_punc = P; a.logits = d_z(ws); a.p = d_p(ws);
    }
  };
  PuncRowsLaunch a{};
  a.img = (const char*)punc_dev_.buf.p; a.off = d_off(ws); a.B = B; a.total = total; a.x = d_x(ws);
  a.head = 0; a.ids = d_ids(ws); a.pe_off = m.pe_off; a.embed_off = m.embed_off;
  tail(a, 0);
  prof_begin("punc", f_qkv * rows);
  launch_punc_rows(stream_, a);
  prof_end("punc");
  if (x0) PF_HIP(hipMemcpyAsync(x0, d_x(ws), (size_t)total * D * 4, hipMemcpyDeviceToHost, stream_));   // before layer 0 rewrites x
  for (int l = 0; l < NL; ++l) {
    const PuncModel::LayerImg& g = m.limg[(size_t)l];
    prof_begin("punc", 0);                          // (4 T^2 d_model per window: not counted, T varies per window)
    launch_punc_attn(stream_, PuncAttnLaunch{qkv[l & 1], d_off(ws), B, d_ctx(ws)});
    prof_end("punc");
    PuncRowsLaunch r{};
    r.img = a.img; r.off = a.off; r.B = B; r.total = total; r.x = a.x;
    r.head = 1; r.ctx = d_ctx(ws); r.qkv_in = qkv[l & 1]; r.taps_off = g.taps; r.kernel = m.kernel; r.out = g.out;
    r.n2_g = g.n2_g; r.n2_b = g.n2_b; r.w1 = g.w1; r.w2 = g.w2;
    tail(r, l + 1);
    prof_begin("punc", (f_layer + (l + 1 < NL ? f_qkv : 2.0 * 32 * D)) * rows);
    launch_punc_rows(stream_, r);
    prof_end("punc");
  }
  if (cut) {
    PuncCutLaunch k{d_p(ws), d_off(ws), d_last(ws), B, d_cut(ws), m.id_none, m.id_comma, m.id_period, m.id_question, m.id_pause,
                    m.sentence_end_id, kPuncCommaWindow, kPuncHardWindow};
    prof_begin("punc", 0);
    launch_punc_cut(stream_, k);
    prof_end("punc");
    PF_HIP(hipMemcpyAsync(cut, d_cut(ws), (size_t)B * 4, hipMemcpyDeviceToHost, stream_));
  }
  if (logits) PF_HIP(hipMemcpyAsync(logits, d_z(ws), (size_t)total * P * 4, hipMemcpyDeviceToHost, stream_));
  if (p) PF_HIP(hipMemcpyAsync(p, d_p(ws), (size_t)total * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_punc(const int32_t* ids, const int32_t* T, const int32_t* last, int B, float* logits, float* x0, int32_t* p, int32_t* cut) {
  PF_CHECK(punc_ != nullptr, PF_ERR_INVALID_ARG, "op_punc: no model is attached (pf_engine_set_punc_model)");
  PF_CHECK(!punc_->causal, PF_ERR_UNSUPPORTED, "op_punc: a causal model runs in streaming form only (pf_op_punc_stream_step)");
  PF_CHECK(B >= 0 && B <= PF_PUNC_MAX_BATCH, PF_ERR_INVALID_ARG, "op_punc: B outside 0 .. PF_PUNC_MAX_BATCH");
  std::vector<int64_t> off((size_t)B + 1, 0);
  for (int b = 0; b < B; ++b) {
    PF_CHECK(T[b] >= 0 && T[b] <= PF_PUNC_MAX_WINDOW, PF_ERR_INVALID_ARG, "op_punc: a window holds 0 .. PF_PUNC_MAX_WINDOW ids");
    off[(size_t)b + 1] = off[(size_t)b] + T[b];
  }
  for (int64_t i = 0; i < off[(size_t)B]; ++i)
    PF_CHECK(ids[i] >= 0 && ids[i] < punc_->vocab, PF_ERR_INVALID_ARG, "op_punc: a word id is outside the vocabulary");
  if (B == 0) return;
  PF_HIP(hipSetDevice(device_));
  run_punc(ids, off.data(), last, B, logits, x0, p, cut);
}

// ---- the punctuation model, streaming (k_punc_stream.hip): ONE launch for B streams
void Engine::punc_stream_step(char* states_dev, const int32_t* slot_dev, const int32_t* ids_dev, int64_t ld, const int32_t* n_new_dev,
                              const int32_t* flush_dev, int B, int max_context, int flags, int32_t* marks_dev, int32_t* mark_flags_dev,
                              float* logits_dev, int32_t* flush_mark_dev) {
  PF_CHECK(punc_ != nullptr, PF_ERR_INVALID_ARG, "punc_stream_step: no model is attached (pf_engine_set_punc_model)");
  const PuncModel& m = *punc_;
  PF_CHECK(m.causal == 1, PF_ERR_UNSUPPORTED, "punc_stream_step: the model is not causal (header key causal = 1)");
  PF_CHECK(max_context >= 2 && max_context <= kPuncStreamMaxContext && (flags & ~1) == 0, PF_ERR_INVALID_ARG,
           "punc_stream_step: max_context outside 2 .. 256 or an unknown flag");
  if (B <= 0) return;
  const PuncStreamLayout L = punc_stream_layout(m);
  PuncStreamLaunch a{};
  a.img = (const char*)punc_dev_.buf.p; a.n_layers = m.n_layers; a.kernel = m.kernel; a.n_punc = m.n_punc;
  a.max_context = max_context; a.no_restart = flags & 1;
  a.pe_off = m.pe_off; a.embed_off = m.embed_off; a.after_g = m.after_g_off; a.after_b = m.after_b_off; a.dec = m.dec;
  for (int l = 0; l < m.n_layers; ++l) {
    const PuncModel::LayerImg& g = m.limg[(size_t)l];
    a.n1_g[l] = g.n1_g; a.n1_b[l] = g.n1_b; a.taps[l] = g.taps; a.n2_g[l] = g.n2_g; a.n2_b[l] = g.n2_b;
    a.qkv[l] = g.qkv; a.out[l] = g.out; a.w1[l] = g.w1; a.w2[l] = g.w2;
  }
  a.states = states_dev; a.state_bytes = L.bytes; a.words_off = L.words_off; a.slot = slot_dev;
  a.ids = ids_dev; a.ld = ld; a.n_new = n_new_dev; a.flush = flush_dev;
  a.id_none = m.id_none; a.id_comma = m.id_comma; a.id_period = m.id_period; a.id_question = m.id_question; a.id_pause = m.id_pause;
  a.sentence_end_id = m.sentence_end_id;
  a.marks = marks_dev; a.mark_flags = mark_flags_dev; a.logits = logits_dev; a.flush_mark = flush_mark_dev;
  prof_begin("punc_stream", 0);
  launch_punc_stream(stream_, a, B);
  prof_end("punc_stream");
}

void Engine::op_punc_stream_step(void* states, const int32_t* ids, const int32_t* n_new, const int32_t* flush, int B, int ld,
                                 int max_context, int flags, int32_t* marks, int32_t* mark_flags, float* logits, int32_t* flush_mark) {
  PF_CHECK(punc_ != nullptr, PF_ERR_INVALID_ARG, "op_punc_stream_step: no model is attached (pf_engine_set_punc_model)");
  const PuncModel& m = *punc_;
  PF_CHECK(m.causal == 1, PF_ERR_UNSUPPORTED, "op_punc_stream_step: the model is not causal (header key causal = 1)");
  PF_CHECK(B >= 0 && B <= PF_PUNC_MAX_BATCH && ld >= 0, PF_ERR_INVALID_ARG, "op_punc_stream_step: B outside 0 .. PF_PUNC_MAX_BATCH or a negative ld");
  const PuncStreamLayout L = punc_stream_layout(m);
  const size_t nB = (size_t)B, sbytes = (size_t)L.bytes, nld = (size_t)ld, P = (size_t)m.n_punc;
  std::vector<int32_t> fl(nB, 0);
  for (int b = 0; b < B; ++b) {                                  // every stream is admitted before anything changes
    PF_CHECK(n_new[b] >= 0 && n_new[b] <= ld, PF_ERR_INVALID_ARG, "op_punc_stream_step: n_new[b] outside 0 .. ld");
    int32_t words[4];
    std::memcpy(words, (const char*)states + b * sbytes + L.words_off, 16);
    punc_stream_admit(m, words[0], ids + b * nld, n_new[b], max_context, flags);
    if (flush) fl[(size_t)b] = flush[b] != 0;
  }
  PF_HIP(hipSetDevice(device_));
  if (B == 0) return;
  const size_t cells = std::max<size_t>(nB * nld, 1);
  StageCarve st;
  const auto d_state = st.take<char>(nB * sbytes);
  const auto d_ids = st.take<int32_t>(cells), d_new = st.take<int32_t>(nB), d_flush = st.take<int32_t>(nB);
  const auto d_marks = st.take<int32_t>(cells), d_mf = st.take<int32_t>(cells);
  const auto d_z = st.take<float>(logits ? cells * P : 0);
  const auto d_fm = st.take<int32_t>(nB);
  void* ws = op_ws(st);
  std::vector<int32_t> x(cells);                                 // hostile behind every stream's n_new ids
  for (size_t i = 0; i < x.size(); ++i) x[i] = hostile_i32(i);
  for (int b = 0; b < B; ++b)
    if (n_new[b] > 0) std::memcpy(&x[b * nld], ids + b * nld, (size_t)n_new[b] * 4);
  upload(stream_, d_state(ws), (const char*)states, d_state.count);
  upload(stream_, d_ids(ws), (const int32_t*)x.data(), x.size());
  upload(stream_, d_new(ws), n_new, nB);
  upload(stream_, d_flush(ws), (const int32_t*)fl.data(), nB);
  fill_sentinel(stream_, d_marks(ws), d_marks.count);
  fill_sentinel(stream_, d_mf(ws), d_mf.count);
  if (logits) fill_sentinel(stream_, d_z(ws), d_z.count);
  fill_sentinel(stream_, d_fm(ws), d_fm.count);
  punc_stream_step(d_state(ws), nullptr, d_ids(ws), ld, d_new(ws), d_flush(ws), B, max_context, flags, d_marks(ws), d_mf(ws),
                   logits ? d_z(ws) : nullptr, d_fm(ws));
  const std::vector<uint32_t> fm = check_guard<uint32_t>(stream_, "punc_stream_step: flush_mark", d_fm(ws), kSentinel32, result_geom(B, B, 1, 1, B));
  std::vector<uint32_t> mk(cells), mf(cells), z(d_z.count);      // the guard rule is applied per stream below
  download(stream_, (int32_t*)mk.data(), (const int32_t*)d_marks(ws), cells);
  download(stream_, (int32_t*)mf.data(), (const int32_t*)d_mf(ws), cells);
  if (logits) download(stream_, (float*)z.data(), (const float*)d_z(ws), d_z.count);
  PF_HIP(hipStreamSynchronize(stream_));
  for (int b = 0; b < B; ++b) {
    const int k = n_new[b];
    const GuardGeom g1 = result_geom(ld, k, 1, 1, k);
    if (const GuardHit hit = guard_scan<uint32_t>(mk.data() + b * nld, nullptr, kSentinel32, g1))
      throw Error(PF_ERR_DEVICE, guard_message("punc_stream_step: marks of stream " + std::to_string(b), g1, hit));
    if (const GuardHit hit = guard_scan<uint32_t>(mf.data() + b * nld, nullptr, kSentinel32, g1))
      throw Error(PF_ERR_DEVICE, guard_message("punc_stream_step: mark_flags of stream " + std::to_string(b), g1, hit));
    if (logits) {                                                // (a logit may be a NaN, never the sentinel's payload)
      const GuardGeom gz = result_geom(ld, k, (int)P, (int)P, k);
      if (const GuardHit hit = guard_scan<uint32_t>(z.data() + b * nld * P, nullptr, kSentinel32, gz))
        throw Error(PF_ERR_DEVICE, guard_message("punc_stream_step: logits of stream " + std::to_string(b), gz, hit));
    }
  }
  download(stream_, (char*)states, (const char*)d_state(ws), d_state.count);
  PF_HIP(hipStreamSynchronize(stream_));
  for (int b = 0; b < B; ++b) {
    const size_t k = (size_t)n_new[b];
    flush_mark[b] = (int32_t)fm[(size_t)b];
    if (k) std::memcpy(marks + b * nld, mk.data() + b * nld, k * 4);
    if (k) std::memcpy(mark_flags + b * nld, mf.data() + b * nld, k * 4);
    if (logits && k) std::memcpy(logits + b * nld * P, z.data() + b * nld * P, k * P * 4);
  }
}

int Engine::punctuate(const int32_t* ids, const int32_t* lens, int B, int32_t* punc_ids) {
  PF_CHECK(punc_ != nullptr, PF_ERR_INVALID_ARG, "punctuate: no model is attached (pf_engine_set_punc_model)");
  PF_CHECK(!punc_->causal, PF_ERR_UNSUPPORTED, "punctuate: a causal model runs in streaming form only (pf_op_punc_stream_step)");
  PF_CHECK(B >= 0 && B <= PF_PUNC_MAX_BATCH, PF_ERR_INVALID_ARG, "punctuate: B outside 0 .. PF_PUNC_MAX_BATCH");
  struct Text { int64_t begin = 0, n = 0, n_mini = 0, mini = 0, done = 0; std::vector<int32_t> win; };
  std::vector<Text> tx((size_t)B);
  int64_t at = 0, most = 0;
  for (int b = 0; b < B; ++b) {
    PF_CHECK(lens[b] >= 0, PF_ERR_INVALID_ARG, "punctuate: a negative length");
    tx[(size_t)b].begin = at; tx[(size_t)b].n = lens[b]; tx[(size_t)b].n_mini = (lens[b] + kPuncMini - 1) / kPuncMini;
    most = std::max(most, tx[(size_t)b].n_mini);
    at += lens[b];
  }
  for (int64_t i = 0; i < at; ++i)
    PF_CHECK(ids[i] >= 0 && ids[i] < punc_->vocab, PF_ERR_INVALID_ARG, "punctuate: a word id is outside the vocabulary");
  PF_HIP(hipSetDevice(device_));
  std::vector<int> who;
  std::vector<int32_t> w_ids, w_last, w_cut, w_p;
  std::vector<int64_t> w_off;
  int rounds = 0;
  for (; rounds < most; ++rounds) {                 // round r: mini-sentence r of every text that has one
    who.clear(); w_ids.clear(); w_last.clear(); w_off.assign(1, 0);
    for (int b = 0; b < B; ++b) {
      Text& t = tx[(size_t)b];
      if (t.mini >= t.n_mini) continue;
      const int64_t lo = t.mini * kPuncMini, hi = std::min(t.n, lo + kPuncMini);
      t.win.insert(t.win.end(), ids + t.begin + lo, ids + t.begin + hi);
      // the cut rule keeps a carried tail at or below kPuncHardWindow; the kernels' LDS and the pe table end at PF_PUNC_MAX_WINDOW
      PF_CHECK(t.win.size() <= (size_t)PF_PUNC_MAX_WINDOW, PF_ERR_CAPACITY, "punctuate: a window above PF_PUNC_MAX_WINDOW words");
      who.push_back(b);
      w_ids.insert(w_ids.end(), t.win.begin(), t.win.end());
      w_last.push_back(t.mini == t.n_mini - 1 ? 1 : 0);
      w_off.push_back((int64_t)w_ids.size());
    }
    const int W = (int)who.size();
    w_cut.assign((size_t)W, -1);
    w_p.assign(w_ids.size(), 0);
    run_punc(w_ids.data(), w_off.data(), w_last.data(), W, nullptr, nullptr, w_p.data(), w_cut.data());
    for (int w = 0; w < W; ++w) {
      Text& t = tx[(size_t)who[(size_t)w]];
      const int cut = w_cut[(size_t)w];
      PF_CHECK(cut >= -1 && cut < (int)t.win.size(), PF_ERR_DEVICE, "punctuate: a cut outside its window");
      for (int i = 0; i <= cut; ++i) punc_ids[t.begin + t.done++] = w_p[(size_t)w_off[(size_t)w] + (size_t)i];
      t.win.erase(t.win.begin(), t.win.begin() + (cut + 1));
      ++t.mini;
    }
  }
  return rounds;
}

// the five decoders on caller data; ws_tmp_: the result block of decode_blocks.h, then the uploaded inputs and the scratch
void Engine::op_topk(const float* x, int64_t rows, int V, int ld, int K, int64_t* ids, float* val, int32_t* n) {
  PF_HIP(hipSetDevice(device_));
  if (rows == 0) return;
  Cursor c;
  const TopkBlock k(c, rows, K);
  const Field<float> d_x = c.take<float>((size_t)rows * ld);
  ensure(ws_tmp_, c.off);
  void* ws = ws_tmp_.p;
  PF_HIP(hipMemcpyAsync(d_x(ws), x, d_x.count * 4, hipMemcpyHostToDevice, stream_));
  launch_topk(stream_, d_x(ws), rows, V, ld, K, k.ids(ws), k.val(ws), k.n(ws));
  PF_HIP(hipMemcpyAsync(ids, k.ids(ws), k.ids.count * 8, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpyAsync(val, k.val(ws), k.val.count * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpyAsync(n, k.n(ws), k.n.count * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_ctc_beam(const float* blank_lp, const int64_t* ids, const float* val, const int32_t* n, const int32_t* lens, int B,
                         int T, int K, int blank, int W, int N, int64_t* out_ids, int32_t* out_len, double* out_score, int cap,
                         int32_t* n_hyp) {
  op_ctc_beam_lm(blank_lp, ids, val, n, lens, B, T, K, blank, W, N, nullptr, nullptr, 0, 0.f, out_ids, out_len, out_score, nullptr, nullptr,
                 cap, n_hyp, nullptr, 0.f, 0.f, 0, nullptr);
}

void Engine::op_ctc_beam_hot(const float* blank_lp, const int64_t* ids, const float* val, const int32_t* n, const int32_t* lens, int B,
                             int T, int K, int blank, int W, int N, const int32_t* hw_ids, const int32_t* hw_lens, int n_hw, float boost,
                             int64_t* out_ids, int32_t* out_len, double* out_score, int32_t* out_matched, double* out_loglik, int cap,
                             int32_t* n_hyp) {
  op_ctc_beam_lm(blank_lp, ids, val, n, lens, B, T, K, blank, W, N, hw_ids, hw_lens, n_hw, boost, out_ids, out_len, out_score, out_matched,
                 out_loglik, cap, n_hyp, nullptr, 0.f, 0.f, 0, nullptr);
}

// the model's image on this engine's device: one upload per model
const int32_t* Engine::lm_device_image(LmDev& d, const std::shared_ptr<const LmImage>& lm) {
  if (d.src != lm) {
    d.src.reset();
    ensure(d.buf, lm->bytes());
    PF_HIP(hipMemcpyAsync(d.buf.p, lm->words.data(), lm->bytes(), hipMemcpyHostToDevice, stream_));
    PF_HIP(hipStreamSynchronize(stream_));
    d.src = lm;
  }
  return (const int32_t*)d.buf.p;
}

void Engine::op_lm_score(const std::shared_ptr<const LmImage>& lm, const int32_t* ids, const int32_t* lens, int B, int L, float alpha,
                         float beta, double* g, int32_t* state) {
  lm_check_weights(alpha, beta, 0);
  PF_HIP(hipSetDevice(device_));
  if (B == 0 || L == 0) return;
  const int32_t* image = lm_device_image(lm_inst_.src == lm ? lm_inst_ : lm_op_, lm);
  const size_t rows = (size_t)B * L;
  Cursor c;
  const Field<double> d_g = c.take<double>(rows);
  const Field<int32_t> d_st = c.take<int32_t>(rows), d_ids = c.take<int32_t>(rows), d_len = c.take<int32_t>(B);
  ensure(ws_tmp_, c.off);
  void* ws = ws_tmp_.p;
  // the caller's outputs go up first: the positions the kernel does not write come back as they were
  PF_HIP(hipMemcpyAsync(d_g(ws), g, rows * 8, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(d_st(ws), state, rows * 4, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(d_ids(ws), ids, rows * 4, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(d_len(ws), lens, (size_t)B * 4, hipMemcpyHostToDevice, stream_));
  launch_lm_walk(stream_, image, d_ids(ws), d_len(ws), B, L, alpha, beta, d_g(ws), d_st(ws));
  PF_HIP(hipMemcpyAsync(g, d_g(ws), rows * 8, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpyAsync(state, d_st(ws), rows * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));
}

// the one body of all three: a hot-word set that biases (its tables, the boost, the two extra outputs) and a language model
// (its image, the weights, out_lm) are the optional parts
void Engine::op_ctc_beam_lm(const float* blank_lp, const int64_t* ids, const float* val, const int32_t* n, const int32_t* lens, int B,
                            int T, int K, int blank, int W, int N, const int32_t* hw_ids, const int32_t* hw_lens, int n_hw, float boost,
                            int64_t* out_ids, int32_t* out_len, double* out_score, int32_t* out_matched, double* out_loglik, int cap,
                            int32_t* n_hyp, const std::shared_ptr<const LmImage>& lm, float alpha, float beta, int lm_flags,
                            double* out_lm) {
  PF_CHECK(boost >= 0.f && boost <= 3.4028234e38f, PF_ERR_INVALID_ARG, "ctc_beam_hot: the boost is finite and >= 0");
  if (lm) lm_check_weights(alpha, beta, lm_flags);
  HotwordGraph graph;                               // (op_ctc_beam gives no set: nothing is built for it)
  if (n_hw != 0) build_hotword_graph(hw_ids, hw_lens, n_hw, hotword_vocab_bound(hw_ids, hw_lens, n_hw), graph);
  const HotwordGraph* g = boost == 0.f || graph.empty() ? nullptr : &graph;
  PF_HIP(hipSetDevice(device_));
  if (B == 0) return;
  const int32_t* lm_image = lm ? lm_device_image(lm_inst_.src == lm ? lm_inst_ : lm_op_, lm) : nullptr;
  const size_t rows = (size_t)B * T, nodes = (size_t)B * ((size_t)T * W + 1);
  Cursor c;
  const BeamBlock k(c, B, N, cap);
  const BeamHotBlock h(c, g || lm ? B : 0, N);
  const BeamLmBlock l(c, lm ? B : 0, N);
  const TopkBlock in(c, rows, K);                   // the lists as op_topk gives them
  const Field<float> d_lb = c.take<float>(rows);
  const Field<int32_t> d_len = c.take<int32_t>(B), d_par = c.take<int32_t>(nodes), d_tok = c.take<int32_t>(nodes);
  const Field<int32_t> d_col = c.take<int32_t>(g ? g->tok_col.size() : 0), d_tab = c.take<int32_t>(g ? g->table.size() : 0);
  ensure(ws_tmp_, c.off);
  void* ws = ws_tmp_.p;
  if (rows > 0) {
    PF_HIP(hipMemcpyAsync(in.ids(ws), ids, in.ids.count * 8, hipMemcpyHostToDevice, stream_));
    PF_HIP(hipMemcpyAsync(in.val(ws), val, in.val.count * 4, hipMemcpyHostToDevice, stream_));
    PF_HIP(hipMemcpyAsync(d_lb(ws), blank_lp, rows * 4, hipMemcpyHostToDevice, stream_));
    PF_HIP(hipMemcpyAsync(in.n(ws), n, rows * 4, hipMemcpyHostToDevice, stream_));
  }
  PF_HIP(hipMemcpyAsync(d_len(ws), lens, d_len.count * 4, hipMemcpyHostToDevice, stream_));
  if (g) {
    PF_HIP(hipMemcpyAsync(d_col(ws), g->tok_col.data(), d_col.count * 4, hipMemcpyHostToDevice, stream_));
    PF_HIP(hipMemcpyAsync(d_tab(ws), g->table.data(), d_tab.count * 4, hipMemcpyHostToDevice, stream_));
  }
  if (lm) {
    launch_ctc_beam_lm(stream_, d_lb(ws), 1, in.ids(ws), in.val(ws), in.n(ws), d_len(ws), B, T, K, blank, W, N, cap, d_par(ws), d_tok(ws),
                       g ? d_col(ws) : nullptr, (int)d_col.count, d_tab(ws), g ? g->A : 0, boost, lm_image, alpha, beta, lm_flags, k.ids(ws),
                       k.len(ws), k.score(ws), h.matched(ws), h.loglik(ws), l.lm_sum(ws), k.n_hyp(ws));
  } else if (g) {
    launch_ctc_beam_hot(stream_, d_lb(ws), 1, in.ids(ws), in.val(ws), in.n(ws), d_len(ws), B, T, K, blank, W, N, cap, d_par(ws), d_tok(ws),
                        d_col(ws), (int)d_col.count, d_tab(ws), g->A, boost, k.ids(ws), k.len(ws), k.score(ws), h.matched(ws), h.loglik(ws),
                        k.n_hyp(ws));
  } else {
    launch_ctc_beam(stream_, d_lb(ws), 1, in.ids(ws), in.val(ws), in.n(ws), d_len(ws), B, T, K, blank, W, N, cap, d_par(ws), d_tok(ws),
                    k.ids(ws), k.len(ws), k.score(ws), k.n_hyp(ws));
  }
  std::vector<int32_t> h_ids(k.ids.count);
  if (!h_ids.empty()) PF_HIP(hipMemcpyAsync(h_ids.data(), k.ids(ws), h_ids.size() * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpyAsync(out_len, k.len(ws), k.len.count * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpyAsync(out_score, k.score(ws), k.score.count * 8, hipMemcpyDeviceToHost, stream_));
  if (g || lm) PF_HIP(hipMemcpyAsync(out_loglik, h.loglik(ws), h.loglik.count * 8, hipMemcpyDeviceToHost, stream_));
  if (g) PF_HIP(hipMemcpyAsync(out_matched, h.matched(ws), h.matched.count * 4, hipMemcpyDeviceToHost, stream_));
  if (lm) PF_HIP(hipMemcpyAsync(out_lm, l.lm_sum(ws), l.lm_sum.count * 8, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpyAsync(n_hyp, k.n_hyp(ws), k.n_hyp.count * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));            // g's host arrays are read by the copies queued above until here
  std::copy(h_ids.begin(), h_ids.end(), out_ids);
  if (!g && out_matched)                            // a set that does not bias: no hot-word term was added
    for (size_t x = 0; x < k.score.count; ++x) {
      out_matched[x] = 0;
      if (!lm) out_loglik[x] = out_score[x];
    }
}

// the n-best search kernel alone on caller lists; the result block is sentinel-filled and every cell must come back written
void Engine::op_nbest_search(const int64_t* ids, const float* val, const int32_t* n, const int32_t* token_num, int B, int L, int K, int W,
                             int N, const int32_t* hw_ids, const int32_t* hw_lens, int n_hw, float boost,
                             const std::shared_ptr<const LmImage>& lm, float alpha, float beta, int lm_flags, int32_t* out_ranks,
                             double* out_score, double* out_loglik, double* out_lm, int32_t* out_matched, int32_t* n_hyp) {
  PF_CHECK(B >= 0 && L >= 0 && K >= 1 && K <= PF_TOPK_MAX && N >= 1 && N <= W && W <= PF_NBEST_MAX, PF_ERR_INVALID_ARG,
           "nbest_search: bad B / L / K / W / N");
  PF_CHECK(boost >= 0.f && boost <= 3.4028234e38f, PF_ERR_INVALID_ARG, "nbest_search: the boost is finite and >= 0");
  if (lm) lm_check_weights(alpha, beta, lm_flags);
  const size_t rows = (size_t)B * L;
  PF_CHECK(B == 0 || (token_num && n_hyp && out_score && out_loglik && out_lm && out_matched), PF_ERR_INVALID_ARG, "nbest_search: null argument");
  PF_CHECK(rows == 0 || (ids && val && n && out_ranks), PF_ERR_INVALID_ARG, "nbest_search: null argument");
  for (size_t x = 0; x < rows; ++x) PF_CHECK(n[x] >= 0 && n[x] <= K, PF_ERR_INVALID_ARG, "nbest_search: n[l] outside 0 .. K");
  HotwordGraph graph;
  if (n_hw != 0) build_hotword_graph(hw_ids, hw_lens, n_hw, hotword_vocab_bound(hw_ids, hw_lens, n_hw), graph);
  const HotwordGraph* g = boost == 0.f || graph.empty() ? nullptr : &graph;
  PF_HIP(hipSetDevice(device_));
  if (B == 0) return;
  const int32_t* lm_image = lm ? lm_device_image(lm_inst_.src == lm ? lm_inst_ : lm_op_, lm) : nullptr;
  Cursor c;
  const NbestSearchBlock k(c, B, N, L);
  const TopkBlock in(c, rows, K);
  const Field<int32_t> d_tn = c.take<int32_t>(B), d_bp = c.take<int32_t>(rows * W);
  const Field<int32_t> d_col = c.take<int32_t>(g ? g->tok_col.size() : 0), d_tab = c.take<int32_t>(g ? g->table.size() : 0);
  ensure(ws_tmp_, c.off);
  void* ws = ws_tmp_.p;
  fill_sentinel(stream_, (uint32_t*)((char*)ws + k.begin), k.words() * 2);
  if (rows > 0) {
    PF_HIP(hipMemcpyAsync(in.ids(ws), ids, in.ids.count * 8, hipMemcpyHostToDevice, stream_));
    PF_HIP(hipMemcpyAsync(in.val(ws), val, in.val.count * 4, hipMemcpyHostToDevice, stream_));
    PF_HIP(hipMemcpyAsync(in.n(ws), n, rows * 4, hipMemcpyHostToDevice, stream_));
  }
  PF_HIP(hipMemcpyAsync(d_tn(ws), token_num, d_tn.count * 4, hipMemcpyHostToDevice, stream_));
  if (g) {
    PF_HIP(hipMemcpyAsync(d_col(ws), g->tok_col.data(), d_col.count * 4, hipMemcpyHostToDevice, stream_));
    PF_HIP(hipMemcpyAsync(d_tab(ws), g->table.data(), d_tab.count * 4, hipMemcpyHostToDevice, stream_));
  }
  NbestSearchArgs a{};
  a.ids = in.ids(ws); a.val = in.val(ws); a.n = in.n(ws); a.token_num = d_tn(ws);
  a.L = L; a.K = K; a.W = W; a.N = N;
  a.bp = d_bp(ws);
  a.tok_col = g ? d_col(ws) : nullptr; a.table = g ? d_tab(ws) : nullptr; a.V = (int)d_col.count; a.A = g ? g->A : 0; a.boost = (double)boost;
  a.lm_image = lm_image; a.alpha = (double)alpha; a.beta = (double)beta; a.lm_eos = (lm_flags & PF_LM_EOS) != 0;
  a.out_ranks = k.ranks(ws); a.out_score = k.score(ws); a.out_loglik = k.loglik(ws); a.out_lm = k.lm_sum(ws);
  a.out_matched = k.matched(ws); a.n_hyp = k.n_hyp(ws);
  launch_nbest_search(stream_, a, B);
  std::vector<int64_t> h(k.words());
  PF_HIP(hipMemcpyAsync(h.data(), (char*)ws + k.begin, h.size() * 8, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));            // g's host arrays are read by the copies queued above until here
  const NbestSearchBlock hk = block_at_zero<NbestSearchBlock>(B, N, L);
  const void* p = h.data();
  const uint64_t sent64 = ((uint64_t)kSentinel32 << 32) | kSentinel32;
  auto written32 = [&](const Field<int32_t>& f, const char* what) {
    for (size_t x = 0; x < f.count; ++x)
      PF_CHECK((uint32_t)f(p)[x] != kSentinel32, PF_ERR_DEVICE, std::string("nbest_search: ") + what + " cell " + std::to_string(x) + " was not written");
  };
  auto written64 = [&](const Field<double>& f, const char* what) {
    for (size_t x = 0; x < f.count; ++x) {
      uint64_t u;
      std::memcpy(&u, f(p) + x, 8);
      PF_CHECK(u != sent64, PF_ERR_DEVICE, std::string("nbest_search: ") + what + " cell " + std::to_string(x) + " was not written");
    }
  };
  written32(hk.ranks, "ranks"); written32(hk.matched, "matched"); written32(hk.n_hyp, "n_hyp");
  written64(hk.score, "score"); written64(hk.loglik, "loglik_sum"); written64(hk.lm_sum, "lm_sum");
  if (hk.ranks.count) std::memcpy(out_ranks, hk.ranks(p), hk.ranks.count * 4);
  std::memcpy(out_score, hk.score(p), hk.score.count * 8);
  std::memcpy(out_loglik, hk.loglik(p), hk.loglik.count * 8);
  std::memcpy(out_lm, hk.lm_sum(p), hk.lm_sum.count * 8);
  std::memcpy(out_matched, hk.matched(p), hk.matched.count * 4);
  std::memcpy(n_hyp, hk.n_hyp(p), hk.n_hyp.count * 4);
}

void Engine::op_ctc_align(const float* lp, int B, int T, int V, int ld, const int32_t* tgt, const int32_t* tlen, const int32_t* lens,
                          int H, int cap, float* path_score, double* loglik, int32_t* ok, int32_t* first, int32_t* last,
                          float* tok_score) {
  PF_HIP(hipSetDevice(device_));
  if (B == 0 || H == 0) return;
  const size_t rows = (size_t)B * T, bp_stride = ctc_align_bp_words(T, cap);
  Cursor c;
  const AlignBlock k(c, B, H, cap);                 // len: the targets' lengths, uploaded
  const Field<int32_t> d_tgt = c.take<int32_t>(k.first.count), d_len = c.take<int32_t>(B);   // a target slot per token slot
  const Field<float> d_lp = c.take<float>(rows * ld);
  const Field<uint32_t> d_bp = c.take<uint32_t>(k.ok.count * bp_stride);          // per job
  ensure(ws_tmp_, c.off);
  void* ws = ws_tmp_.p;
  if (rows > 0) PF_HIP(hipMemcpyAsync(d_lp(ws), lp, d_lp.count * 4, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(d_tgt(ws), tgt, d_tgt.count * 4, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(k.len(ws), tlen, k.len.count * 4, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(d_len(ws), lens, d_len.count * 4, hipMemcpyHostToDevice, stream_));
  launch_ctc_align(stream_, d_lp(ws), ld, V, d_tgt(ws), k.len(ws), d_len(ws), B, T, H, cap, d_bp(ws), (int64_t)bp_stride, k.path(ws),
                   k.loglik(ws), k.ok(ws), k.first(ws), k.last(ws), k.tok(ws));
  PF_HIP(hipMemcpyAsync(path_score, k.path(ws), k.path.count * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpyAsync(loglik, k.loglik(ws), k.loglik.count * 8, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpyAsync(ok, k.ok(ws), k.ok.count * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpyAsync(first, k.first(ws), k.first.count * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpyAsync(last, k.last(ws), k.last.count * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpyAsync(tok_score, k.tok(ws), k.tok.count * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_ctc_collapse(const int64_t* ids, const float* scores, const int32_t* lens, int B, int T, int blank,
                             int64_t* ids_out, int32_t* first_out, int32_t* last_out, float* score_out, int cap, int32_t* n_out) {
  PF_HIP(hipSetDevice(device_));
  if (B == 0) return;
  const size_t in = (size_t)B * T;
  Cursor c;
  const CtcBlock k(c, B, cap);
  const Field<int64_t> d_ids = c.take<int64_t>(in);
  const Field<float> d_sc = c.take<float>(in);
  const Field<int32_t> d_len = c.take<int32_t>(B);
  ensure(ws_tmp_, c.off);
  void* ws = ws_tmp_.p;
  PF_HIP(hipMemcpyAsync(d_ids(ws), ids, in * 8, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(d_sc(ws), scores, in * 4, hipMemcpyHostToDevice, stream_));
  PF_HIP(hipMemcpyAsync(d_len(ws), lens, d_len.count * 4, hipMemcpyHostToDevice, stream_));
  launch_ctc_collapse(stream_, d_ids(ws), d_sc(ws), d_len(ws), B, T, blank, cap, k.n(ws), k.ids(ws), k.first(ws), k.last(ws), k.score(ws));
  PF_HIP(hipMemcpyAsync(ids_out, k.ids(ws), k.ids.count * 8, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpyAsync(first_out, k.first(ws), k.first.count * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpyAsync(last_out, k.last(ws), k.last.count * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpyAsync(score_out, k.score(ws), k.score.count * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipMemcpyAsync(n_out, k.n(ws), k.n.count * 4, hipMemcpyDeviceToHost, stream_));
  PF_HIP(hipStreamSynchronize(stream_));
  for (int b = 0; b < B; ++b)
    PF_CHECK(n_out[b] <= cap, PF_ERR_CAPACITY, "ctc_collapse: capacity " + std::to_string(cap) + " < " + std::to_string(n_out[b]) + " tokens");
}

void Engine::op_gemm(const float* A, const float* W, const float* bias, int M, int N, int K, int epi, float* C) {
  PF_HIP(hipSetDevice(device_));
  if (M == 0 || N == 0) return;
  const int Kp = (int)round_up(K, 64);
  const int64_t Mp = round_up(M, 256), Np = round_up(N, 256);
  StageCarve st;
  const auto dA = st.take<float>((size_t)M * K), dW = st.take<float>((size_t)N * K), db = st.take<float>(N);
  const auto dA16 = st.take<half_t>((size_t)Mp * Kp), dW16 = st.take<half_t>((size_t)Np * Kp);
  const auto dC = st.take<float>((size_t)Mp * N);                // (the f16 result of epi 2 lives here too)
  void* ws = op_ws(st);
  if (bias) upload(stream_, db(ws), bias, N);
  PF_HIP(hipMemsetAsync(dA16(ws), 0, (size_t)Mp * Kp * 2, stream_));
  PF_HIP(hipMemsetAsync(dW16(ws), 0, (size_t)Np * Kp * 2, stream_));
  upload_f16(stream_, dA(ws), A, M, K, dA16(ws), Kp);
  upload_f16(stream_, dW(ws), W, N, K, dW16(ws), Kp);
  GemmArgs g{};
  g.A = dA16(ws); g.lda = Kp; g.W = dW16(ws); g.ldw = Kp;
  g.bias = bias ? db(ws) : nullptr;
  g.M = M; g.N = N; g.K = Kp; g.relu = epi == 1;
  g.out_padded = 1;
  const bool f16out = epi == 2;
  if (f16out) { g.out_f16 = (half_t*)dC(ws); g.ldc16 = N; }
  else { g.out_f32 = dC(ws); g.ldc32 = N; }
  prof_begin("gemm_op", 2.0 * M * (double)N * K);
  launch_gemm(stream_, g);
  prof_end("gemm_op");
  if (f16out) {
    download_f16(stream_, C, (const half_t*)dC(ws), M, N, N);
  } else {
    download(stream_, C, (const float*)dC(ws), (size_t)M * N);
    PF_HIP(hipStreamSynchronize(stream_));
  }
}

void Engine::x3_forget(const float* W) {
  for (auto it = x3w_.begin(); it != x3w_.end();) {
    if (it->first.first != W) { ++it; continue; }
    for (size_t i = 0; i < owned_.size(); ++i)
      if (owned_[i] == (void*)it->second) { owned_.erase(owned_.begin() + i); break; }
    hipFree(it->second);
    it = x3w_.erase(it);
  }
}

// A Linear / the FFN block of the fp32 graph exactly as enc_layer_fp32() launches them (gemm32: math_mode 1 on the fp32
// matrix path, math_mode 3 as x3 products with the K-loop wrap and, in the block, the operand-pair epilogue).
void Engine::op_linear32(const float* x, const float* W, const float* bias, const float* resid, int M, int N, int K, bool relu, float* y) {
  PF_CHECK(fp32_mode_, PF_ERR_UNSUPPORTED, "linear32: the engine was not created with math_mode 1 or 3");
  PF_HIP(hipSetDevice(device_));
  const int ldc = (int)round_up(N, 4);
  const int64_t Mp = round_up(M, 256) + 128, Np = round_up(N, 256);
  StageCarve st;
  const auto dx = st.take<float>((size_t)Mp * K), dW = st.take<float>((size_t)Np * K), db = st.take<float>(Np);
  const auto dr = st.take<float>((size_t)Mp * ldc), dy = st.take<float>((size_t)Mp * ldc);
  void* ws = op_ws(st);
  PF_HIP(hipMemsetAsync(ws, 0, st.off, stream_));
  upload(stream_, dx(ws), x, (size_t)M * K);
  upload(stream_, dW(ws), W, (size_t)N * K);
  if (bias) upload(stream_, db(ws), bias, N);
  if (resid) upload2d(stream_, dr(ws), ldc, resid, N, N, M);
  gemm32(dx(ws), K, dW(ws), K, bias ? db(ws) : nullptr, M, N, K, dy(ws), ldc, resid ? dr(ws) : nullptr, ldc, relu, 0, 1.f);
  download2d(stream_, y, N, (const float*)dy(ws), ldc, N, M);
  PF_HIP(hipStreamSynchronize(stream_));
  x3_forget(dW(ws));
  x3a_src_ = nullptr;
}

void Engine::op_ffn32(const float* x, const float* W1, const float* b1, const float* W2, const float* b2, int M, int D, int F, float* y) {
  PF_CHECK(fp32_mode_, PF_ERR_UNSUPPORTED, "ffn32: the engine was not created with math_mode 1 or 3");
  PF_CHECK(D % 4 == 0 && F % 4 == 0, PF_ERR_INVALID_ARG, "ffn32: D and F must be multiples of 4");
  PF_HIP(hipSetDevice(device_));
  const int64_t Mp = round_up(M, 256) + 128, Dp = round_up(D, 256), Fp = round_up(F, 256);
  StageCarve st;
  const auto dx = st.take<float>((size_t)Mp * D), d1 = st.take<float>((size_t)Fp * D), db1 = st.take<float>(Fp), d2 = st.take<float>((size_t)Dp * F),
             db2 = st.take<float>(Dp), dh = st.take<float>((size_t)Mp * F), dy = st.take<float>((size_t)Mp * D);
  void* ws = op_ws(st);
  PF_HIP(hipMemsetAsync(ws, 0, st.off, stream_));
  upload(stream_, dx(ws), x, (size_t)M * D);
  upload(stream_, d1(ws), W1, (size_t)F * D);
  upload(stream_, db1(ws), b1, F);
  upload(stream_, d2(ws), W2, (size_t)D * F);
  upload(stream_, db2(ws), b2, D);
  gemm32(dx(ws), D, d1(ws), D, db1(ws), M, F, D, dh(ws), F, nullptr, 0, true, 0, 1.f, kX3OutPair);
  gemm32(dh(ws), F, d2(ws), F, db2(ws), M, D, F, dy(ws), D, dx(ws), D, false, 0, 1.f, kX3InPair);
  download(stream_, y, (const float*)dy(ws), (size_t)M * D);
  PF_HIP(hipStreamSynchronize(stream_));
  x3_forget(d1(ws));
  x3_forget(d2(ws));
  x3a_src_ = nullptr;
}

// ---- the fp32 graph's Linear on hostile hosts (tests/test_gpu_fp32_conformance.py): every fp32 matrix is uploaded as an image
// whose cells outside the matrix hold the large finite pattern (rows behind the last, the columns between the width and the row
// stride), the three x3 arenas are filled with a large finite pattern before the call (so a pad row or pad column that reached
// a cell of [M, N] would be seen), every result sits in a sentinel-filled buffer.
void Engine::x3_poison(int M, int N, int K) {
  if (!x3_mode_) return;
  const int64_t Mp = round_up(M, 256) + 128, Kp = round_up(K, 64);
  ensure(ws_x3a_, (size_t)Mp * 2 * Kp * 2);
  ensure(ws_x3t_, (size_t)Mp * round_up(N, 4) * 4);
  ensure(ws_x3h_, (size_t)Mp * 2 * round_up(N, 64) * 2);
  for (DevBuf* b : {&ws_x3a_, &ws_x3t_, &ws_x3h_}) PF_HIP(hipMemsetD16Async((hipDeviceptr_t)b->p, kPoison16, b->bytes / 2, stream_));
}

void Engine::op_linear32_ex(const pf_linear32_desc& ds, const float* A, const float* W, float* C) {
  PF_CHECK(fp32_mode_, PF_ERR_UNSUPPORTED, "linear32_ex: the engine was not created with math_mode 1 or 3");
  PF_HIP(hipSetDevice(device_));
  const int M = ds.M, N = ds.N, K = ds.K;
  const bool alias = ds.resid_aliases_out != 0;
  const int lda = ds.lda ? ds.lda : K, ldw = ds.ldw ? ds.ldw : K, ldc = ds.ldc ? ds.ldc : (int)round_up(N, 4);
  const int ldr = alias ? ldc : (ds.ldr ? ds.ldr : ldc);
  PF_CHECK(lda >= K && ldw >= K && ldc >= N && ldr >= N, PF_ERR_INVALID_ARG, "linear32_ex: a row stride is narrower than its matrix");
  PF_CHECK(!alias || ds.resid, PF_ERR_INVALID_ARG, "linear32_ex: resid_aliases_out without a residual");
  const int64_t Mp = round_up(M, 256) + 128, Np = round_up(N, 256);
  StageCarve st;
  const auto dA = st.take<float>((size_t)Mp * lda), dW = st.take<float>((size_t)Np * ldw), db = st.take<float>(Np);
  const auto dR = st.take<float>((size_t)Mp * ldr), dR2 = st.take<float>((size_t)Mp * ldr), dC = st.take<float>((size_t)Mp * ldc);
  void* ws = op_ws(st);
  upload_hostile32(stream_, dA(ws), Mp, lda, A, M, K);
  upload_hostile32(stream_, dW(ws), Np, ldw, W, N, K);
  upload_hostile32(stream_, db(ws), 1, (int)Np, ds.bias, 1, N);
  if (ds.resid && !alias) upload_hostile32(stream_, dR(ws), Mp, ldr, ds.resid, M, N);
  if (ds.resid2) upload_hostile32(stream_, dR2(ws), Mp, ldr, ds.resid2, M, N);
  float* out = dC(ws);
  fill_sentinel(stream_, out, (size_t)Mp * ldc);
  if (alias) upload2d(stream_, out, ldc, ds.resid, N, N, M);
  x3_poison(M, N, K);
  const float* Wd = dW(ws);
  const auto done = at_exit([&] { x3_forget(Wd); x3a_src_ = nullptr; x3a_pair_only_ = false; x3_pair_live_ = false; cls32_ = "gemm32_misc"; });
  cls32_ = "gemm32_op";
  gemm32(dA(ws), lda, Wd, ldw, ds.bias ? db(ws) : nullptr, M, N, K, out, ldc, ds.resid ? (alias ? out : dR(ws)) : nullptr, ldr, ds.relu != 0,
         ds.scale_cols, ds.scale, ds.flags, ds.resid2 ? dR2(ws) : nullptr);
  check_guard(stream_, "linear32_ex: the fp32 result", out, kSentinel32, result_geom(Mp, M, N, ldc, M, false, !alias));
  download2d(stream_, C, N, (const float*)out, ldc, N, M);
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_split_x3(const float* x, int rows, int K, int ldx, int ldo, int Kp, int swap, uint16_t* out) {
  PF_HIP(hipSetDevice(device_));
  const int64_t Rp = (int64_t)rows + 64;
  StageCarve st;
  const auto dx = st.take<float>((size_t)Rp * ldx);
  const auto dout = st.take<half_t>((size_t)Rp * ldo);
  void* ws = op_ws(st);
  upload_hostile32(stream_, dx(ws), Rp, ldx, x, rows, K);
  fill_sentinel(stream_, dout(ws), (size_t)Rp * ldo);
  launch_split_x3(stream_, dx(ws), rows, K, ldx, dout(ws), ldo, Kp, swap);
  check_guard(stream_, "split_x3: the pair", dout(ws), kSentinel16, result_geom(Rp, rows, 2 * Kp, ldo, rows));
  download(stream_, out, (const uint16_t*)dout(ws), (size_t)rows * ldo);
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_layernorm32(const float* x, const float* gamma, const float* beta, int M, int D, int direct_pair, float* out32, uint16_t* pair,
                            int32_t* wrote_pair, const float* W, const float* bias, int N, float* y) {
  PF_CHECK(fp32_mode_, PF_ERR_UNSUPPORTED, "layernorm32: the engine was not created with math_mode 1 or 3");
  PF_HIP(hipSetDevice(device_));
  if (!W) N = 4;
  const int ldc = (int)round_up(N, 4), ldo = 2 * D + 8;
  const int64_t Mp = round_up(M, 256) + 128, Np = round_up(N, 256);
  StageCarve st;
  const auto dx = st.take<float>((size_t)Mp * D), dg = st.take<float>(D), dbt = st.take<float>(D), dn = st.take<float>((size_t)Mp * D);
  const auto dp = st.take<uint16_t>((size_t)Mp * ldo);
  const auto dW = st.take<float>((size_t)Np * D), db = st.take<float>(Np), dy = st.take<float>((size_t)Mp * ldc);
  void* ws = op_ws(st);
  upload_hostile32(stream_, dx(ws), Mp, D, x, M, D);
  upload(stream_, dg(ws), gamma, D);
  upload(stream_, dbt(ws), beta, D);
  const float* xd = dx(ws);
  float* xn = dn(ws);
  *wrote_pair = 0;
  if (direct_pair) {
    PF_CHECK(D == 512, PF_ERR_INVALID_ARG, "layernorm32: the pair kernel is the D = 512 kernel");
    fill_sentinel(stream_, dp(ws), (size_t)Mp * ldo);
    launch_layernorm_pair(stream_, xd, M, dg(ws), dbt(ws), (half_t*)dp(ws), ldo, D);
    check_guard(stream_, "layernorm32: the pair", dp(ws), kSentinel16, result_geom(Mp, M, 2 * D, ldo, M));
    download2d(stream_, pair, 2 * D, (const uint16_t*)dp(ws), ldo, 2 * D, M);
    PF_HIP(hipStreamSynchronize(stream_));
    *wrote_pair = 1;
    return;
  }
  if (W) {
    upload_hostile32(stream_, dW(ws), Np, D, W, N, D);
    upload_hostile32(stream_, db(ws), 1, (int)Np, bias, 1, N);
    fill_sentinel(stream_, dy(ws), (size_t)Mp * ldc);
  }
  fill_sentinel(stream_, xn, (size_t)Mp * D);
  x3_poison(M, N, D);
  const float* Wd = dW(ws);
  const auto done = at_exit([&] { x3_forget(Wd); x3a_src_ = nullptr; x3a_pair_only_ = false; x3_pair_live_ = false; cls32_ = "gemm32_misc"; });
  LNp ln;
  ln.g = dg(ws); ln.b = dbt(ws); ln.D = D;
  layernorm32(xd, M, D, ln, xn);
  if (x3a_pair_only_ && x3a_src_ == xn) {
    *wrote_pair = 1;
    check_guard(stream_, "layernorm32: the fp32 row buffer beside the pair", xn, kSentinel32, untouched_geom(Mp * D));
    check_guard(stream_, "layernorm32: the pair arena behind row M - 1", (const uint16_t*)ws_x3a_.p + (size_t)M * 2 * D, kPoison16,
                untouched_geom(Mp - M, 2 * D), nullptr, M);
    download(stream_, pair, (const uint16_t*)ws_x3a_.p, (size_t)M * 2 * D);
  } else {
    check_guard(stream_, "layernorm32: the fp32 rows", xn, kSentinel32, result_geom(Mp, M, D, D, M));
    download(stream_, out32, (const float*)xn, (size_t)M * D);
  }
  PF_HIP(hipStreamSynchronize(stream_));
  if (W) {
    cls32_ = "gemm32_op";
    gemm32(xn, D, Wd, D, bias ? db(ws) : nullptr, M, N, D, dy(ws), ldc, nullptr, 0, false, 0, 1.f);
    check_guard(stream_, "layernorm32: the product behind it", dy(ws), kSentinel32, result_geom(Mp, M, N, ldc, M));
    download2d(stream_, y, N, (const float*)dy(ws), ldc, N, M);
    PF_HIP(hipStreamSynchronize(stream_));
  }
}

void Engine::op_ffn32_ex(const float* x, const float* W1, const float* b1, const float* W2, const float* b2, int M, int D, int F, float hidden_scale,
                         float* y, uint16_t* hidden_pair, int32_t* pair_written) {
  PF_CHECK(fp32_mode_, PF_ERR_UNSUPPORTED, "ffn32_ex: the engine was not created with math_mode 1 or 3");
  PF_CHECK(D % 4 == 0 && F % 4 == 0, PF_ERR_INVALID_ARG, "ffn32_ex: D and F must be multiples of 4");
  PF_HIP(hipSetDevice(device_));
  const int64_t Mp = round_up(M, 256) + 128, Dp = round_up(D, 256), Fp = round_up(F, 256);
  StageCarve st;
  const auto dx = st.take<float>((size_t)Mp * D), d1 = st.take<float>((size_t)Fp * D), db1 = st.take<float>(Fp), d2 = st.take<float>((size_t)Dp * F),
             db2 = st.take<float>(Dp), dh = st.take<float>((size_t)Mp * F), dy = st.take<float>((size_t)Mp * D);
  void* ws = op_ws(st);
  upload_hostile32(stream_, dx(ws), Mp, D, x, M, D);
  upload_hostile32(stream_, d1(ws), Fp, D, W1, F, D);
  upload_hostile32(stream_, db1(ws), 1, (int)Fp, b1, 1, F);
  upload_hostile32(stream_, d2(ws), Dp, F, W2, D, F);
  upload_hostile32(stream_, db2(ws), 1, (int)Dp, b2, 1, D);
  fill_sentinel(stream_, dh(ws), (size_t)Mp * F);
  fill_sentinel(stream_, dy(ws), (size_t)Mp * D);
  x3_poison(M, std::max(D, F), std::max(D, F));
  const float* xd = dx(ws);
  const float* w1 = d1(ws);
  const float* w2 = d2(ws);
  const auto done = at_exit([&] { x3_forget(w1); x3_forget(w2); x3a_src_ = nullptr; x3a_pair_only_ = false; x3_pair_live_ = false; cls32_ = "gemm32_misc"; });
  *pair_written = 0;
  const bool scaled = hidden_scale != 1.0f;
  cls32_ = "gemm32_ffn1";
  gemm32(xd, D, w1, D, db1(ws), M, F, D, dh(ws), F, nullptr, 0, true, scaled ? F : 0, hidden_scale, kX3OutPair);
  if (x3_pair_live_) {
    *pair_written = 1;
    const int ldp = 2 * (int)round_up(F, 64);
    const int64_t g0 = round_up(M, 256);
    const uint16_t* arena = (const uint16_t*)ws_x3h_.p;
    check_guard(stream_, "ffn32_ex: the fp32 hidden beside its pair", dh(ws), kSentinel32, untouched_geom(Mp * F));
    check_guard(stream_, "ffn32_ex: the pair arena at and beyond round_up(M, 256)", arena + (size_t)g0 * ldp, kPoison16,
                untouched_geom(Mp - g0, ldp), nullptr, g0);
    download2d(stream_, hidden_pair, 2 * F, arena, ldp, F, M);
    download2d(stream_, hidden_pair + F, 2 * F, arena + ldp / 2, ldp, F, M);
    PF_HIP(hipStreamSynchronize(stream_));
  } else {
    check_guard(stream_, "ffn32_ex: the fp32 hidden", dh(ws), kSentinel32, result_geom(Mp, M, F, F, M));
  }
  cls32_ = "gemm32_ffn2";
  gemm32(dh(ws), F, w2, F, db2(ws), M, D, F, dy(ws), D, xd, D, false, 0, 1.f, kX3InPair);
  check_guard(stream_, "ffn32_ex: the fp32 result", dy(ws), kSentinel32, result_geom(Mp, M, D, D, M));
  download(stream_, y, (const float*)dy(ws), (size_t)M * D);
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_qkv32(const float* x, const float* W, const float* bias, int M, int D, int K, float qscale, float* out) {
  PF_CHECK(fp32_mode_, PF_ERR_UNSUPPORTED, "qkv32: the engine was not created with math_mode 1 or 3");
  PF_HIP(hipSetDevice(device_));
  const int64_t Mp = round_up(M, 256) + 128, Np = round_up(3 * D, 256);
  StageCarve st;
  const auto dx = st.take<float>((size_t)Mp * K), dW = st.take<float>((size_t)Np * K), db = st.take<float>(Np);
  const Field<float> dq[3] = {st.take<float>((size_t)Mp * D), st.take<float>((size_t)Mp * D), st.take<float>((size_t)Mp * D)};
  void* ws = op_ws(st);
  upload_hostile32(stream_, dx(ws), Mp, K, x, M, K);
  upload_hostile32(stream_, dW(ws), Np, K, W, 3 * D, K);
  upload_hostile32(stream_, db(ws), 1, (int)Np, bias, 1, 3 * D);
  for (int i = 0; i < 3; ++i) fill_sentinel(stream_, dq[i](ws), (size_t)Mp * D);
  x3_poison(M, D, K);
  const float* xd = dx(ws);
  const float* Wd = dW(ws);
  const float* bd = db(ws);
  const auto done = at_exit([&] {
    for (int i = 0; i < 3; ++i) x3_forget(Wd + (size_t)i * D * K);
    x3a_src_ = nullptr; x3a_pair_only_ = false; x3_pair_live_ = false; cls32_ = "gemm32_misc";
  });
  static const char* const cls[3] = {"gemm32_op_q", "gemm32_op_k", "gemm32_op_v"};
  for (int i = 0; i < 3; ++i) {                                // as enc_layer_fp32 launches the three
    cls32_ = cls[i];
    gemm32(xd, K, Wd + (size_t)i * D * K, K, bd + (size_t)i * D, M, D, K, dq[i](ws), D, nullptr, 0, false, i == 0 ? D : 0,
           i == 0 ? qscale : 1.f, i == 0 ? 0 : kX3SameInput);
    check_guard(stream_, std::string("qkv32: ") + cls[i], dq[i](ws), kSentinel32, result_geom(Mp, M, D, D, M));
  }
  for (int i = 0; i < 3; ++i) download2d(stream_, out + (size_t)i * D, 3 * D, (const float*)dq[i](ws), D, D, M);
  PF_HIP(hipStreamSynchronize(stream_));
}

// GEMM exactly as the pipeline launches it: kernel kind (fp32 / f16 row-major / f16 blocked result), tile height,
// blocked A operand, residual / second addend, column scaling — the stand-alone counterpart of Engine::gemm().
void Engine::op_gemm_ex(const pf_gemm_desc& ds, const float* A, const float* W, float* C) {
  PF_HIP(hipSetDevice(device_));
  const int M = ds.M, N = ds.N, K = ds.K;
  PF_CHECK(M > 0 && N > 0 && K > 0, PF_ERR_INVALID_ARG, "gemm_ex: empty problem");
  PF_CHECK(ds.out_kind >= 0 && ds.out_kind <= 2, PF_ERR_INVALID_ARG, "gemm_ex: out_kind must be 0, 1 or 2");
  PF_CHECK(ds.tile_rows == 0 || ds.tile_rows == 32 || ds.tile_rows == 128 || ds.tile_rows == 256 || ds.tile_rows == 512 || ds.tile_rows == 1024 ||
               ds.tile_rows == 2048,
           PF_ERR_INVALID_ARG, "gemm_ex: tile_rows must be 0, 32 (= the short-input kernel), 128, 256, 512 (= the 256 x {192,256} tile kernel), "
           "1024 (= its persistent form for the blocked result) or 2048 (= the k-step-32 fp32-result kernel)");
  PF_CHECK(ds.out_kind == 0 || (!ds.resid && !ds.add2), PF_ERR_INVALID_ARG, "gemm_ex: residual / addend need the fp32 result kind");
  PF_CHECK(ds.out_kind != 2 || N % 64 == 0, PF_ERR_INVALID_ARG, "gemm_ex: blocked result needs N % 64 == 0");
  const int Kp = (int)round_up(K, 64);
  const int64_t Mp = round_up(M, 256) + 128, Np = round_up(N, 256);
  const int ld32 = (int)round_up(N, 4), ld16 = (int)round_up(N, 8);
  const int ldc16 = ds.out_kind == 2 ? N : ld16;
  StageCarve st;
  const auto dA = st.take<float>((size_t)M * K), dW = st.take<float>((size_t)N * K), db = st.take<float>(N);
  const auto dA16 = st.take<half_t>((size_t)Mp * Kp), dW16 = st.take<half_t>((size_t)Np * Kp);
  const auto dR = st.take<float>((size_t)Mp * ld32), dD = st.take<float>((size_t)Mp * ld32);
  const auto dC = st.take<float>((size_t)Mp * std::max(ld32, ld16));     // (either result kind)
  void* ws = op_ws(st);
  float* c32 = dC(ws);
  half_t* c16 = (half_t*)dC(ws);
  if (ds.a_blocked) upload_blocked16(stream_, A, M, K, dA16(ws), Kp, Mp);
  else upload_operand16(stream_, dA(ws), A, M, K, dA16(ws), Kp, Mp);
  upload_operand16(stream_, dW(ws), W, N, K, dW16(ws), Kp, Np);
  if (ds.out_kind == 0) fill_sentinel(stream_, c32, (size_t)Mp * ld32);
  else fill_sentinel(stream_, c16, (size_t)Mp * ldc16);
  if (ds.bias) upload(stream_, db(ws), ds.bias, N);
  if (ds.resid) upload2d(stream_, dR(ws), ld32, ds.resid, N, N, M);
  if (ds.add2) upload2d(stream_, dD(ws), ld32, ds.add2, N, N, M);
  GemmArgs g{};
  g.A = dA16(ws); g.lda = Kp; g.W = dW16(ws); g.ldw = Kp;
  g.bias = ds.bias ? db(ws) : nullptr;
  g.M = M; g.N = N; g.K = Kp; g.relu = ds.relu ? 1 : 0;
  g.scale_cols = ds.scale_cols; g.scale = ds.scale;
  g.out_padded = 1;
  g.a_blocked = ds.a_blocked ? 1 : 0;
  g.force_mi = ds.tile_rows == 128 ? 1 : (ds.tile_rows == 256 ? 2 : (ds.tile_rows == 32 ? 4 : (ds.tile_rows == 1024 ? 5 : (ds.tile_rows == 2048 ? 6 : 0))));
  g.small_ws = small_ws_;
  if (ds.out_kind == 0) {
    g.out_f32 = c32; g.ldc32 = ld32;
    if (ds.resid) { g.resid = dR(ws); g.ldr = ld32; }
    if (ds.add2) { g.add2 = dD(ws); g.ld2 = ld32; }
  } else {
    g.out_f16 = c16; g.ldc16 = ldc16;
    g.out_blocked = ds.out_kind == 2;
  }
  op_timed(2.0 * M * (double)N * K, [&] { launch_gemm(stream_, g); });
  if (ds.out_kind == 0) {
    check_guard(stream_, "gemm_ex: the fp32 result", c32, kSentinel32, result_geom(Mp, M, N, ld32, round_up(M, 256)));
    download2d(stream_, C, N, (const float*)c32, ld32, N, M);
    PF_HIP(hipStreamSynchronize(stream_));
  } else {
    check_guard(stream_, "gemm_ex: the f16 result", c16, kSentinel16, result_geom(Mp, M, N, ldc16, round_up(M, 256), ds.out_kind == 2));
    if (ds.out_kind == 2) download_blocked16(stream_, C, c16, M, N, 0, N);
    else download_f16(stream_, C, c16, M, N, ld16);
  }
}

// The K = 512 product  C = A W^T + bias  on the panel-resident kernel (form 7) or, for comparison, on gemm_f16_pp3 (form 1 / 2 =
// 128- / 256-row tiles) or by launch_gemm's rule (form 0), with the hosts at their most hostile: the A rows behind M - 1 and
// the W rows behind N - 1 hold NaNs, the result (out_kind 0: fp32, ld = round_up(N, 4); 1: f16, ld = N + 64) sits in a
// sentinel-filled buffer in which nothing but [M, N] may change — unless `padded` declares the rows up to round_up(M, 256)
// writable, as the pipeline's buffers are.
void Engine::op_gemm_panel(int M, int N, int out_kind, int form, int padded, const float* bias, const float* A, const float* W, float* C) {
  PF_HIP(hipSetDevice(device_));
  constexpr int K = 512;
  PF_CHECK(M > 0 && N > 0, PF_ERR_INVALID_ARG, "gemm_panel: empty problem");
  PF_CHECK(out_kind == 0 || out_kind == 1, PF_ERR_INVALID_ARG, "gemm_panel: out_kind must be 0 (fp32) or 1 (f16)");
  PF_CHECK(form == 0 || form == 1 || form == 2 || form == 7, PF_ERR_INVALID_ARG, "gemm_panel: form must be 0, 1, 2 or 7");
  const int64_t Mp = round_up(M, 256) + 128, Np = round_up(N, 256);
  const int ld = out_kind == 1 ? N + 64 : (int)round_up(N, 4);
  PF_CHECK(ld % 4 == 0, PF_ERR_INVALID_ARG, "gemm_panel: the f16 form needs N % 4 == 0");
  StageCarve st;
  const auto dA = st.take<float>((size_t)M * K), dW = st.take<float>((size_t)N * K), db = st.take<float>(N);
  const auto dA16 = st.take<half_t>((size_t)Mp * K), dW16 = st.take<half_t>((size_t)Np * K), dI = st.take<half_t>(gemm_panel_image_bytes(N) / 2);
  const auto dC = st.take<uint8_t>((size_t)Mp * ld * (out_kind == 1 ? 2 : 4));   // (either result kind)
  void* ws = op_ws(st);
  float* c32 = (float*)dC(ws);
  half_t* c16 = (half_t*)dC(ws);
  PF_HIP(hipMemsetD16Async((hipDeviceptr_t)dA16(ws), 0x7E00, (size_t)Mp * K, stream_));     // NaN behind the operands
  PF_HIP(hipMemsetD16Async((hipDeviceptr_t)dW16(ws), 0x7E00, (size_t)Np * K, stream_));
  upload_f16(stream_, dA(ws), A, M, K, dA16(ws), K);
  upload_f16(stream_, dW(ws), W, N, K, dW16(ws), K);
  launch_gemm_panel_retile(stream_, dW16(ws), K, N, dI(ws));
  if (bias) upload(stream_, db(ws), bias, N);
  if (out_kind == 0) fill_sentinel(stream_, c32, (size_t)Mp * ld);
  else fill_sentinel(stream_, c16, (size_t)Mp * ld);
  GemmArgs g{};
  g.A = dA16(ws); g.lda = K; g.W = dW16(ws); g.ldw = K; g.W_panel = dI(ws);
  g.bias = bias ? db(ws) : nullptr;
  g.M = M; g.N = N; g.K = K;
  g.out_padded = padded ? 1 : 0;
  g.force_mi = form;
  if (out_kind == 0) { g.out_f32 = c32; g.ldc32 = ld; }
  else { g.out_f16 = c16; g.ldc16 = ld; }
  op_timed(2.0 * M * (double)N * K, [&] { launch_gemm(stream_, g); });
  const GuardGeom geom = result_geom(Mp, M, N, ld, padded ? round_up(M, 256) : M);   // (rows the destination does not declare writable)
  if (out_kind == 0) {
    check_guard(stream_, "gemm_panel: the fp32 result", c32, kSentinel32, geom);
    download2d(stream_, C, N, (const float*)c32, ld, N, M);
    PF_HIP(hipStreamSynchronize(stream_));
  } else {
    check_guard(stream_, "gemm_panel: the f16 result", c16, kSentinel16, geom);
    download_f16(stream_, C, c16, M, N, ld);
  }
}

void Engine::op_gemm_rc(const pf_gemm_rc_desc& ds, const float* A, const float* W, float* x_out, float* n16_out,
                        float* n32_out) {
  PF_HIP(hipSetDevice(device_));
  const int M = ds.M, K = ds.K, N = 512;
  PF_CHECK(M > 0 && K > 0 && K % 64 == 0, PF_ERR_INVALID_ARG, "gemm_rc: K must be a positive multiple of 64");
  PF_CHECK(!ds.fsmn_v || (ds.fsmn_w && ds.fsmn_k > 0), PF_ERR_INVALID_ARG, "gemm_rc: FSMN needs weights");
  PF_CHECK((ds.ln_gamma != nullptr) == (ds.ln_beta != nullptr), PF_ERR_INVALID_ARG, "gemm_rc: gamma and beta go together");
  const int64_t Mp = round_up(M, 256) + 128;
  const int k = ds.fsmn_k;
  StageCarve st;
  const auto d32 = st.take<float>((size_t)std::max<int64_t>((int64_t)M * std::max(K, N), (int64_t)N * K));   // the fp32 staging slot
  const auto dA16 = st.take<half_t>((size_t)Mp * K), dW16 = st.take<half_t>((size_t)N * K);
  const auto db = st.take<float>(N), dR = st.take<float>((size_t)Mp * N);
  const auto dV = st.take<half_t>((size_t)(Mp + 128) * 3 * N);
  const auto dwT = st.take<float>((size_t)std::max(k, 1) * N), dg = st.take<float>(N), dbe = st.take<float>(N), dX = st.take<float>((size_t)Mp * N);
  const auto dN16 = st.take<half_t>((size_t)Mp * N);
  const auto dN32 = st.take<float>((size_t)Mp * N);
  void* ws = op_ws(st);
  if (ds.a_blocked) upload_blocked16(stream_, A, M, K, dA16(ws), K, Mp);
  else upload_operand16(stream_, d32(ws), A, M, K, dA16(ws), K, Mp);
  upload_f16(stream_, d32(ws), W, N, K, dW16(ws), K);
  GemmRcArgs g{};
  g.A = dA16(ws); g.lda = K; g.a_blocked = ds.a_blocked ? 1 : 0;
  g.W = dW16(ws); g.ldw = K; g.M = M; g.K = K;
  if (ds.bias) { upload(stream_, db(ws), ds.bias, N); g.bias = db(ws); }
  if (ds.resid) { upload(stream_, dR(ws), ds.resid, (size_t)M * N); g.resid = dR(ws); g.ldr = N; }
  std::vector<float> wT;
  if (ds.fsmn_v) {
    // the V slice of a [M, 3*512] QKV buffer, as in the pipeline (row stride 1536 halves); the rows in front of it and
    // behind it, and the Q | K columns, are hostile
    fill_hostile_rows(stream_, dV(ws), 3 * N, 0, Mp + 128, 3 * N);
    half_t* vs = dV(ws) + (size_t)kVLead * 3 * N + 2 * N;
    upload_f16(stream_, d32(ws), ds.fsmn_v, M, N, vs, 3 * N);
    wT = fsmn_taps(ds.fsmn_w, N, k);
    upload(stream_, dwT(ws), wT.data(), wT.size());
    g.fsmn_v = vs; g.ldv = 3 * N; g.fsmn_wT = dwT(ws); g.fsmn_k = k;
  }
  g.T = ds.T > 0 ? ds.T : M;
  fill_sentinel(stream_, dX(ws), (size_t)Mp * N);
  fill_sentinel(stream_, dN16(ws), (size_t)Mp * N);
  fill_sentinel(stream_, dN32(ws), (size_t)Mp * N);
  if (ds.ln_gamma) {
    upload(stream_, dg(ws), ds.ln_gamma, N);
    upload(stream_, dbe(ws), ds.ln_beta, N);
    g.ln_g = dg(ws); g.ln_b = dbe(ws); g.eps = 1e-12f;
    if (n16_out) { g.out_n16 = dN16(ws); g.ldn16 = N; }
    if (n32_out) { g.out_n32 = dN32(ws); g.ldn32 = N; }
  }
  if (x_out) { g.out_x = dX(ws); g.ldx = N; }
  PF_CHECK(!ds.split_k, PF_ERR_UNSUPPORTED, "gemm_rc: the split-K forms (k_gemm_sk.hip) were removed in round 5 — the fused FFN block replaced them (numbers: profiles/round4_splitk_pairs.txt)");
  const GuardGeom geom = result_geom(Mp, M, N, N, round_up(M, 256));
  if (ds.short_input) {
    // the short-input forms of the same nodes, as enc_layer / the decoder run them for M <= 512 rows
    PF_CHECK(!ds.a_blocked, PF_ERR_INVALID_ARG, "gemm_rc: the short-input kernels take a row-major A");
    GemmSmallArgs q{};
    q.A = g.A; q.lda = K; q.W = g.W; q.ldw = K; q.bias = g.bias; q.M = M; q.N = N; q.K = K; q.ws = small_ws_;
    q.resid = g.resid; q.ldr = N;
    const bool need_x = g.out_x || (g.ln_g && K <= 576);
    if (need_x) { q.out_f32 = dX(ws); q.ldc32 = N; }
    if (K <= 576) {
      q.fsmn_v = g.fsmn_v; q.ldv = g.ldv; q.fsmn_wT = g.fsmn_wT; q.fsmn_k = g.fsmn_k; q.T = g.T;
      prof_begin("gemm_op", 2.0 * M * (double)N * K);
      launch_gemm_small(stream_, q);
      prof_end("gemm_op");
      if (g.ln_g) launch_layernorm(stream_, q.out_f32, M, N, g.ln_g, g.ln_b, g.out_n16, N, g.out_n32, N);
    } else {
      PF_CHECK(!g.fsmn_v, PF_ERR_INVALID_ARG, "gemm_rc: the split short-input form has no FSMN term");
      q.post_ln_g = g.ln_g; q.post_ln_b = g.ln_b; q.post_n16 = g.out_n16; q.ldn16 = N; q.post_n32 = g.out_n32; q.ldn32 = N;
      prof_begin("gemm_op", 2.0 * M * (double)N * K);
      launch_gemm_small(stream_, q);
      prof_end("gemm_op");
    }
    if (q.out_f32) check_guard(stream_, "gemm_rc: x", dX(ws), kSentinel32, geom);
  } else {
    prof_begin("gemm_op", 2.0 * M * (double)N * K);
    launch_gemm_rc(stream_, g);
    prof_end("gemm_op");
    if (g.out_x) check_guard(stream_, "gemm_rc: x", dX(ws), kSentinel32, geom);
  }
  if (g.out_n16) check_guard(stream_, "gemm_rc: the f16 LayerNorm result", dN16(ws), kSentinel16, geom);
  if (g.out_n32) check_guard(stream_, "gemm_rc: the fp32 LayerNorm result", dN32(ws), kSentinel32, geom);
  if (x_out) download(stream_, x_out, (const float*)dX(ws), (size_t)M * N);
  if (g.out_n32) download(stream_, n32_out, (const float*)dN32(ws), (size_t)M * N);
  PF_HIP(hipStreamSynchronize(stream_));
  if (g.out_n16) download_f16(stream_, n16_out, dN16(ws), M, N, N);
}

// Encoder FFN as enc_layer() runs it: FFN-up writes the hidden in the blocked activation layout (kind 3),
// FFN-down reads it as a blocked A operand and adds bias + residual (kind 2).  y = resid + W2 relu(W1 x + b1) + b2.
void Engine::op_ffn(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                    const float* resid, int M, int D, int F, float* y) {
  PF_HIP(hipSetDevice(device_));
  PF_CHECK(M > 0 && D % 64 == 0 && F % 64 == 0, PF_ERR_INVALID_ARG, "ffn: D and F must be multiples of 64");
  const int64_t Mp = round_up(M, 256) + 128, Fp = round_up(F, 256), Dp = round_up(D, 256);
  StageCarve st;
  const auto d32 = st.take<float>((size_t)std::max<int64_t>((int64_t)M * D, (int64_t)F * D));   // the fp32 staging slot
  const auto dx16 = st.take<half_t>((size_t)Mp * D), dw1 = st.take<half_t>((size_t)Fp * D), dw2 = st.take<half_t>((size_t)Dp * F);
  const auto db1 = st.take<float>(F), db2 = st.take<float>(D);
  const auto dh = st.take<half_t>((size_t)Mp * F);
  const auto dxr = st.take<float>((size_t)Mp * D);
  void* ws = op_ws(st);
  fill_sentinel(stream_, dh(ws), (size_t)Mp * F);
  fill_sentinel(stream_, dxr(ws), (size_t)Mp * D);
  upload_operand16(stream_, d32(ws), x, M, D, dx16(ws), D, Mp);
  upload_operand16(stream_, d32(ws), w1, F, D, dw1(ws), D, Fp);
  upload_operand16(stream_, d32(ws), w2, D, F, dw2(ws), F, Dp);
  upload(stream_, db1(ws), b1, F);
  upload(stream_, db2(ws), b2, D);
  upload(stream_, dxr(ws), resid, (size_t)M * D);
  Lin L1, L2;
  L1.w = dw1(ws); L1.bias = db1(ws); L1.N = F; L1.K = D; L1.Kpad = D;
  L2.w = dw2(ws); L2.bias = db2(ws); L2.N = D; L2.K = F; L2.Kpad = F;
  float* xr = dxr(ws);
  gemm("gemm_ffn1", L1, dx16(ws), D, M, nullptr, 0, dh(ws), F, nullptr, 0, nullptr, 0, true, 0, 1.f, true, 1);
  gemm("gemm_ffn2", L2, dh(ws), F, M, xr, D, nullptr, 0, xr, D, nullptr, 0, false, 0, 1.f, true, 2);
  check_guard(stream_, "ffn: the blocked hidden", dh(ws), kSentinel16, result_geom(Mp, M, F, F, round_up(M, 256), true));
  check_guard(stream_, "ffn: the result (in place on the residual)", xr, kSentinel32, result_geom(Mp, M, D, D, round_up(M, 256), false, false));
  download(stream_, y, (const float*)xr, (size_t)M * D);
  PF_HIP(hipStreamSynchronize(stream_));
}

// The decoder's FFN block in the split form of the fused kernel (k_ffn.hip), standalone: t = LN_F(relu(f16(x) W1^T + b1)) W2^T,
// n = LayerNorm(t); x = the block's normalised input, or (ds.ctx) LayerNorm norm1 of x_out = resid + ctx Wo^T + bo computed by
// the same launch.  A hostile host (see the top of the file): the operand rows behind M - 1 hold the large finite pattern, the
// residual's too, every output and the bytes behind the workspace are sentinel-filled and checked against kernels.h's contract.
void Engine::op_dec_ffn_fused(const pf_dec_ffn_desc& ds, float* t_out, float* n_out, float* x_out) {
  PF_HIP(hipSetDevice(device_));
  const int D = 512, F = 2048, M = ds.M, splits = ds.splits;
  PF_CHECK(M > 0, PF_ERR_INVALID_ARG, "dec_ffn_fused: M must be positive");
  PF_CHECK(splits == 0 || splits == 1 || splits == 2 || splits == 3 || splits == 4 || splits == 8, PF_ERR_INVALID_ARG,
           "dec_ffn_fused: splits must be 0 (automatic) | 1 | 2 | 3 | 4 | 8");
  const bool op = ds.ctx != nullptr;
  const int64_t Mp = round_up(M, 256) + 128;
  const size_t wsb = ffn_dec_workspace_bytes(M, splits);
  StageCarve st;
  const auto d32 = st.take<float>((size_t)std::max<int64_t>((int64_t)M * D, (int64_t)F * D));   // the fp32 staging slot
  const auto dx16 = st.take<half_t>((size_t)Mp * D), dw1 = st.take<half_t>((size_t)F * D);
  const auto dw2 = st.take<float>((size_t)D * F);
  const auto dimg = st.take<half_t>(ffn_dec_image_bytes() / 2);
  const auto dws = st.take<uint8_t>(wsb + kWsGuard);
  const auto db1 = st.take<float>(F), dgf = st.take<float>(F), dbf = st.take<float>(F), dg = st.take<float>(D), dbe = st.take<float>(D);
  const auto dt = st.take<float>((size_t)Mp * D), dn = st.take<float>((size_t)Mp * D);
  const auto dwo = st.take<half_t>((size_t)D * D), dwot = st.take<half_t>(ffn_outproj_weight_bytes() / 2);
  const auto dbo = st.take<float>(D), dg1 = st.take<float>(D), dbe1 = st.take<float>(D);
  const auto dxr = st.take<float>((size_t)Mp * D), dxo = st.take<float>((size_t)Mp * D);
  void* ws = op_ws(st);
  uint32_t* behind_ws = (uint32_t*)(dws(ws) + wsb);
  fill_sentinel(stream_, dt(ws), (size_t)Mp * D);
  fill_sentinel(stream_, dn(ws), (size_t)Mp * D);
  fill_sentinel(stream_, dxo(ws), (size_t)Mp * D);
  fill_sentinel(stream_, behind_ws, kWsGuard / 4);
  upload_operand16(stream_, d32(ws), op ? ds.ctx : ds.x, M, D, dx16(ws), D, Mp);
  upload_f16(stream_, d32(ws), ds.w1, F, D, dw1(ws), D);
  upload(stream_, dw2(ws), ds.w2, (size_t)D * F); upload(stream_, db1(ws), ds.b1, F);
  upload(stream_, dgf(ws), ds.gamma_f, F); upload(stream_, dbf(ws), ds.beta_f, F);
  if (ds.ln_gamma) { upload(stream_, dg(ws), ds.ln_gamma, D); upload(stream_, dbe(ws), ds.ln_beta, D); }
  launch_ffn_dec_retile(stream_, dw1(ws), D, dw2(ws), dgf(ws), dbf(ws), db1(ws), dimg(ws));
  FfnDecArgs f{};
  f.A = dx16(ws); f.lda = D; f.img = dimg(ws); f.ws = dws(ws); f.M = M; f.splits = splits;
  f.eps_hidden = 1e-12f; f.eps = 1e-12f;
  if (op) {
    upload_f16(stream_, d32(ws), ds.wo, D, D, dwo(ws), D);
    launch_ffn_retile_out(stream_, dwo(ws), D, dwot(ws));
    upload(stream_, dbo(ws), ds.bo, D); upload(stream_, dg1(ws), ds.ln1_gamma, D); upload(stream_, dbe1(ws), ds.ln1_beta, D);
    fill_hostile_rows32(stream_, dxr(ws), D, M, Mp);
    upload(stream_, dxr(ws), ds.resid, (size_t)M * D);
    f.A = nullptr; f.ctx = dx16(ws); f.lda_c = D; f.Wot = dwot(ws); f.bo = dbo(ws);
    f.resid = dxr(ws); f.ldr = D; f.out_x = dxo(ws); f.ldx = D;
    f.ln1_g = dg1(ws); f.ln1_b = dbe1(ws); f.eps1 = 1e-12f;
  }
  if (t_out) { f.t32 = dt(ws); f.ldt = D; }
  if (ds.ln_gamma) { f.ln_g = dg(ws); f.ln_b = dbe(ws); }
  if (n_out) { f.n32 = dn(ws); f.ldn32 = D; }
  op_timed(4.0 * M * (double)D * F + (op ? 2.0 * M * (double)D * D : 0.0), [&] { launch_ffn_dec(stream_, f); });
  const GuardGeom geom = result_geom(Mp, M, D, D, M);
  if (f.t32) check_guard(stream_, "dec_ffn_fused: t", dt(ws), kSentinel32, geom);
  if (f.n32) check_guard(stream_, "dec_ffn_fused: the LayerNorm result", dn(ws), kSentinel32, geom);
  if (op) check_guard(stream_, "dec_ffn_fused: x_out", dxo(ws), kSentinel32, geom);
  check_guard(stream_, "dec_ffn_fused: the bytes behind ffn_dec_workspace_bytes", behind_ws, kSentinel32, untouched_geom(kWsGuard / 4));
  if (t_out) download(stream_, t_out, (const float*)dt(ws), (size_t)M * D);
  if (n_out) download(stream_, n_out, (const float*)dn(ws), (size_t)M * D);
  if (x_out && op) download(stream_, x_out, (const float*)dxo(ws), (size_t)M * D);
  PF_HIP(hipStreamSynchronize(stream_));
}

// The encoder FFN block as enc_layer() launches it for long inputs: retile W1 / W2, then ONE launch of ffn_fused_kernel.
void Engine::op_ffn_fused(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* resid,
                          const float* g, const float* be, int M, float* x_out, float* n16_out, const pf_attn_ffn_desc* op) {
  PF_HIP(hipSetDevice(device_));
  const int D = 512, F = 2048;
  PF_CHECK(M > 0, PF_ERR_INVALID_ARG, "ffn_fused: M must be positive");
  PF_CHECK(op || x, PF_ERR_INVALID_ARG, "ffn_fused: missing operand");
  const int64_t Mp = round_up(M, 256) + 128;
  const bool tail = op && op->wqkv;
  StageCarve st;
  const auto d32 = st.take<float>((size_t)std::max<int64_t>((int64_t)M * D, (int64_t)F * D));   // the fp32 staging slot
  const auto dx16 = st.take<half_t>((size_t)Mp * D), dw1 = st.take<half_t>((size_t)F * D), dw2 = st.take<half_t>((size_t)D * F);
  const auto dwt = st.take<half_t>(ffn_fused_weight_bytes() / 2);
  const auto db1 = st.take<float>(F), db2 = st.take<float>(D), dg = st.take<float>(D), dbe = st.take<float>(D);
  const auto dxr = st.take<float>((size_t)Mp * D), dxo = st.take<float>((size_t)Mp * D);
  const auto dn16 = st.take<half_t>((size_t)Mp * D);
  // out-projection form: Wo (f16 + its image), bias, the V slice inside a [M, 3 D] QKV-shaped buffer, taps, norm2
  const auto dwo = st.take<half_t>((size_t)D * D), dwot = st.take<half_t>(ffn_outproj_weight_bytes() / 2);
  const auto dbo = st.take<float>(D);
  const auto dv = st.take<half_t>((size_t)(Mp + 128) * 3 * D);
  const auto dwT = st.take<float>((size_t)11 * D), dg2 = st.take<float>(D), dbe2 = st.take<float>(D);
  // the Q | K | V tail: the weight (f16 + its three images), bias, the blocked Q | K and the row-major V it writes
  const auto dwq = st.take<half_t>((size_t)3 * D * D), dwqt = st.take<half_t>(3 * ffn_outproj_weight_bytes() / 2);
  const auto dbq = st.take<float>((size_t)3 * D);
  const auto dqk = st.take<half_t>((size_t)Mp * 2 * D), dvo = st.take<half_t>((size_t)Mp * D);
  void* ws = op_ws(st);
  PF_HIP(hipMemsetAsync(dxr(ws), 0, (size_t)Mp * D * 4, stream_));
  fill_hostile_rows32(stream_, dxr(ws), D, M, Mp);                  // the residual rows behind M - 1 are never read (kernels.h)
  if (tail) { fill_sentinel(stream_, dqk(ws), (size_t)Mp * 2 * D); fill_sentinel(stream_, dvo(ws), (size_t)Mp * D); }
  fill_sentinel(stream_, dxo(ws), (size_t)Mp * D);
  fill_sentinel(stream_, dn16(ws), (size_t)Mp * D);
  upload_operand16(stream_, d32(ws), op ? op->ctx : x, M, D, dx16(ws), D, Mp);
  upload_f16(stream_, d32(ws), w1, F, D, dw1(ws), D);
  upload_f16(stream_, d32(ws), w2, D, F, dw2(ws), F);
  upload(stream_, db1(ws), b1, F);
  upload(stream_, db2(ws), b2, D);
  if (resid) upload(stream_, dxr(ws), resid, (size_t)M * D);
  launch_ffn_retile(stream_, dw1(ws), D, dw2(ws), F, dwt(ws));
  FfnFusedArgs f{};
  f.A = dx16(ws); f.lda = D; f.Wt = dwt(ws); f.b1 = db1(ws); f.b2 = db2(ws);
  f.M = M; f.resid = resid || !op ? dxr(ws) : nullptr; f.ldr = D; f.eps = 1e-12f;
  std::vector<float> wT;
  if (op) {
    upload_f16(stream_, d32(ws), op->wo, D, D, dwo(ws), D);
    launch_ffn_retile_out(stream_, dwo(ws), D, dwot(ws));
    fill_hostile_rows(stream_, dv(ws), 3 * D, 0, Mp + 128, 3 * D);      // as op_gemm_rc: hostile around the V slice
    half_t* vs = dv(ws) + (size_t)kVLead * 3 * D + 2 * D;
    upload_f16(stream_, d32(ws), op->v, M, D, vs, 3 * D);
    wT = fsmn_taps(op->fsmn_w, D, 11);
    upload(stream_, dwT(ws), wT.data(), wT.size());
    upload(stream_, dbo(ws), op->bo, D);
    upload(stream_, dg2(ws), op->ln2_gamma, D);
    upload(stream_, dbe2(ws), op->ln2_beta, D);
    f.ctx = dx16(ws); f.lda_c = D; f.Wot = dwot(ws); f.bo = dbo(ws);
    f.fsmn_v = vs; f.ldv = 3 * D; f.fsmn_wT = dwT(ws); f.T = op->T > 0 ? op->T : M;
    f.ln2_g = dg2(ws); f.ln2_b = dbe2(ws);
    f.A = nullptr;
  }
  if (tail) {
    PF_CHECK(op->bqkv && g, PF_ERR_INVALID_ARG, "attn_ffn_fused: the Q | K | V tail needs its bias and the LayerNorm in front of it");
    upload_f16(stream_, d32(ws), op->wqkv, 3 * D, D, dwq(ws), D);
    for (int part = 0; part < 3; ++part)
      launch_ffn_retile_out(stream_, dwq(ws) + (size_t)part * D * D, D, dwqt(ws) + (size_t)part * (ffn_outproj_weight_bytes() / 2));
    upload(stream_, dbq(ws), op->bqkv, (size_t)3 * D);
    f.Wqt = dwqt(ws); f.bq = dbq(ws); f.out_qk = dqk(ws); f.out_v = dvo(ws);
    f.ldvo = D; f.qscale = 1.0f / std::sqrt(128.0f);
  }
  if (x_out) { f.out_x = dxo(ws); f.ldx = D; }
  if (g) {
    upload(stream_, dg(ws), g, D);
    upload(stream_, dbe(ws), be, D);
    f.ln_g = dg(ws); f.ln_b = dbe(ws);
    if (n16_out) { f.out_n16 = dn16(ws); f.ldn16 = D; }
  }
  // (resid is a separate buffer: repeats compute the same result)
  op_timed(4.0 * M * (double)D * F + (op ? 2.0 * M * (double)D * D : 0.0), [&] { launch_ffn_fused(stream_, f); });
  if (f.out_x) check_guard(stream_, "ffn_fused: x", dxo(ws), kSentinel32, result_geom(Mp, M, D, D, M));
  if (f.out_n16) check_guard(stream_, "ffn_fused: the f16 LayerNorm result", dn16(ws), kSentinel16, result_geom(Mp, M, D, D, M));
  if (tail) {
    check_guard(stream_, "attn_ffn_fused: the blocked Q | K", dqk(ws), kSentinel16, result_geom(Mp, M, 2 * D, 2 * D, round_up(M, 64), true));
    check_guard(stream_, "attn_ffn_fused: V", dvo(ws), kSentinel16, result_geom(Mp, M, D, D, round_up(M, 64)));
  }
  if (x_out) download(stream_, x_out, (const float*)dxo(ws), (size_t)M * D);
  PF_HIP(hipStreamSynchronize(stream_));
  if (f.out_n16) download_f16(stream_, n16_out, dn16(ws), M, D, D);
  if (tail) {
    if (op->q_out) download_blocked16(stream_, op->q_out, dqk(ws), M, 2 * D, 0, D);
    if (op->k_out) download_blocked16(stream_, op->k_out, dqk(ws), M, 2 * D, D, D);
    if (op->v_out) download_f16(stream_, op->v_out, dvo(ws), M, D, D);
  }
}

// Encoder FSMN exactly as enc_layer() launches it: the f16 V slice of a [M, 3D] QKV buffer (row stride 3D).
void Engine::op_fsmn_enc(const float* v, const float* w, int B, int T, int D, int k, float* y) {
  PF_HIP(hipSetDevice(device_));
  PF_CHECK(D % 8 == 0 && B > 0 && T > 0, PF_ERR_INVALID_ARG, "fsmn_enc: bad shape");
  const size_t n = (size_t)B * T * D;
  const std::vector<float> wT = fsmn_taps(w, D, k);
  StageCarve st;
  const auto dv = st.take<float>(n);
  const auto dq = st.take<half_t>(((size_t)B * T + 128) * 3 * D);
  const auto dw = st.take<float>(wT.size()), dy = st.take<float>(n);
  void* ws = op_ws(st);
  PF_HIP(hipMemsetAsync(dq(ws), 0, dq.count * 2, stream_));
  upload(stream_, dw(ws), wT.data(), wT.size());
  half_t* vs = dq(ws) + 2 * D;
  upload_f16(stream_, dv(ws), v, (int64_t)B * T, D, vs, 3 * D);
  launch_fsmn_enc(stream_, vs, 3 * D, dw(ws), B, T, D, k, dy(ws));
  download(stream_, y, (const float*)dy(ws), n);
  PF_HIP(hipStreamSynchronize(stream_));
}

// Decoder FSMN exactly as the decoder launches it: x += (dwconv(tn*m) + tn*m)*m, m = (l < token_num[b]).
void Engine::op_fsmn_dec(const float* tn, const float* w, const int32_t* token_num, int B, int L, int D, int k, float* x) {
  PF_HIP(hipSetDevice(device_));
  PF_CHECK(D % 4 == 0 && B > 0 && L > 0, PF_ERR_INVALID_ARG, "fsmn_dec: bad shape");
  const size_t n = (size_t)B * L * D;
  const std::vector<float> wT = fsmn_taps(w, D, k);
  StageCarve st;
  const auto dt = st.take<float>(n), dx = st.take<float>(n), dw = st.take<float>(wT.size());
  const auto dnum = st.take<int32_t>(B);
  void* ws = op_ws(st);
  upload(stream_, dt(ws), tn, n);
  upload(stream_, dx(ws), (const float*)x, n);
  upload(stream_, dw(ws), wT.data(), wT.size());
  upload(stream_, dnum(ws), token_num, B);
  launch_fsmn_dec(stream_, dt(ws), dw(ws), dnum(ws), B, L, D, k, dx(ws));
  download(stream_, x, (const float*)dx(ws), n);
  PF_HIP(hipStreamSynchronize(stream_));
}

// what both decoder-FSMN ops upload: tn [B, L, D] with the rows at l >= num[b] left as the device buffer holds them (hostile)
static void upload_valid_rows(hipStream_t s, float* dev, const float* tn, const int32_t* num, int B, int L, int D) {
  for (int b = 0; b < B; ++b) upload(s, dev + (size_t)b * L * D, tn + (size_t)b * L * D, (size_t)std::min(std::max(num[b], 0), L) * D);
}
// ... and what both require afterwards: a row of x at l >= num[b] comes back with the bits it went in with
static void check_masked_rows(const char* op, const float* x_out, const float* x, const int32_t* num, int B, int L, int D) {
  for (int b = 0; b < B; ++b)
    for (int l = std::max(num[b], 0); l < L; ++l)
      PF_CHECK(std::memcmp(x_out + ((size_t)b * L + l) * D, x + ((size_t)b * L + l) * D, (size_t)D * 4) == 0, PF_ERR_DEVICE,
               std::string(op) + ": x changed at utterance " + std::to_string(b) + ", position " + std::to_string(l) + " >= token_num");
}

// The fused decoder FSMN + norm3 kernel (k_norm.hip fsmn_dec_ln_kernel<11 | 21>) alone, on a hostile host: the rows of tn at
// l >= token_num[b] hold a large finite pattern (the kernel must mask them, not multiply them by zero), x and xn16 sit in
// sentinel-guarded buffers, and a row of x at l >= token_num[b] must come back with the bits it went in with.
void Engine::op_fsmn_dec_ln(const float* tn, const float* taps, const int32_t* token_num, int B, int L, int k, const float* x, const float* gamma,
                            const float* beta, float* x_out, float* xn16_out) {
  PF_HIP(hipSetDevice(device_));
  constexpr int D = 512;
  PF_CHECK(B > 0 && L > 0 && (k == 11 || k == 21), PF_ERR_INVALID_ARG, "fsmn_dec_ln: B, L > 0 and k = 11 | 21");
  const int M = B * L;
  const int64_t Mp = (int64_t)M + 64;
  StageCarve st;
  const auto dt = st.take<float>((size_t)Mp * D), dx = st.take<float>((size_t)Mp * D);
  const auto dn16 = st.take<half_t>((size_t)Mp * D);
  const auto dw = st.take<float>((size_t)k * D), dg = st.take<float>(D), db = st.take<float>(D);
  const auto dnum = st.take<int32_t>(B);
  void* ws = op_ws(st);
  fill_hostile_rows32(stream_, dt(ws), D, 0, Mp);
  upload_valid_rows(stream_, dt(ws), tn, token_num, B, L, D);
  fill_sentinel(stream_, dx(ws), (size_t)Mp * D);
  fill_sentinel(stream_, dn16(ws), (size_t)Mp * D);
  upload(stream_, dx(ws), x, (size_t)M * D);
  upload(stream_, dw(ws), taps, (size_t)k * D);
  upload(stream_, dg(ws), gamma, D);
  upload(stream_, db(ws), beta, D);
  upload(stream_, dnum(ws), token_num, B);
  prof_begin("gemm_op", 0);                       // ("gemm_" classes record the kernel the launcher notes)
  const bool ran = launch_fsmn_dec_ln(stream_, dt(ws), dw(ws), dnum(ws), B, L, D, k, dx(ws), dg(ws), db(ws), dn16(ws));
  prof_end("gemm_op");
  PF_CHECK(ran, PF_ERR_UNSUPPORTED, "fsmn_dec_ln: the launcher declined the geometry");
  check_guard(stream_, "fsmn_dec_ln: x", dx(ws), kSentinel32, result_geom(Mp, M, D, D, M, false, false));
  check_guard(stream_, "fsmn_dec_ln: the f16 LayerNorm result", dn16(ws), kSentinel16, result_geom(Mp, M, D, D, M));
  download(stream_, x_out, (const float*)dx(ws), (size_t)M * D);
  PF_HIP(hipStreamSynchronize(stream_));
  check_masked_rows("fsmn_dec_ln", x_out, x, token_num, B, L, D);
  if (xn16_out) download_f16(stream_, xn16_out, dn16(ws), M, D, D);
}

// ---- the row kernels alone (k_norm.hip, the non-CIF half of k_misc.hip): thin wrappers, no arithmetic of their own.  Every result
// buffer is PF_OP_GUARD_ROWS rows longer at either end than the result (and as wide as the caller's row stride), holds the
// sentinel before the launch and goes back to the caller WHOLE: what the kernel wrote outside its result is the caller's to see.
namespace {
constexpr int kG = PF_OP_GUARD_ROWS;
}  // namespace

void Engine::op_layernorm_ex(const float* x, const float* g, const float* b, int64_t rows, int D, int ld16, int ld32, int posenc_T,
                             uint16_t* out16, float* out32) {
  PF_HIP(hipSetDevice(device_));
  PF_CHECK(rows > 0 && rows < (1 << 24) && D > 0 && D % 4 == 0 && D <= 2048, PF_ERR_INVALID_ARG, "layernorm_ex: bad shape");
  PF_CHECK(out16 || out32, PF_ERR_INVALID_ARG, "layernorm_ex: no output requested");
  PF_CHECK(!out16 || (ld16 >= D && ld16 % 4 == 0), PF_ERR_INVALID_ARG, "layernorm_ex: ld16 must be a multiple of 4, >= D");
  PF_CHECK(!out32 || (ld32 >= D && ld32 % 4 == 0), PF_ERR_INVALID_ARG, "layernorm_ex: ld32 must be a multiple of 4, >= D");
  PF_CHECK(posenc_T == 0 || (posenc_T > 0 && rows % posenc_T == 0 && D == mc_.feat_dim && out16 && !out32), PF_ERR_INVALID_ARG,
           "layernorm_ex: the position-encoding form takes [B, T, feat_dim] and writes f16 only");
  if (!out16) ld16 = 0;
  if (!out32) ld32 = 0;
  if (posenc_T) build_pe(posenc_T);                           // the table the encoder would use, by the call the encoder makes
  const size_t n16 = (size_t)(rows + 2 * kG) * ld16, n32 = (size_t)(rows + 2 * kG) * ld32;
  StageCarve st;
  const auto dx = st.take<float>((size_t)(rows + 2) * D), dg = st.take<float>(D), db = st.take<float>(D);
  const auto d16 = st.take<uint16_t>((size_t)(rows + 2 * kG) * std::max(ld16, 1));
  const auto d32 = st.take<float>((size_t)(rows + 2 * kG) * std::max(ld32, 1));
  void* ws = op_ws(st);
  fill_hostile_rows32(stream_, dx(ws), D, rows, rows + 2);          // the rows behind rows - 1 are never read
  upload(stream_, dx(ws), x, (size_t)rows * D);
  upload(stream_, dg(ws), g, D);
  upload(stream_, db(ws), b, D);
  if (out16) fill_sentinel(stream_, d16(ws), n16);
  if (out32) fill_sentinel(stream_, d32(ws), n32);
  half_t* o16 = out16 ? (half_t*)d16(ws) + (size_t)kG * ld16 : nullptr;
  float* o32 = out32 ? d32(ws) + (size_t)kG * ld32 : nullptr;
  if (posenc_T)
    launch_posenc_ln_tab(stream_, dx(ws), (int)(rows / posenc_T), posenc_T, D, std::sqrt((float)mc_.d_model), (const float*)ws_pe_.p, dg(ws), db(ws),
                         o16, ld16);
  else
    launch_layernorm(stream_, dx(ws), rows, D, dg(ws), db(ws), o16, ld16, o32, ld32);
  if (out16) download(stream_, out16, (const uint16_t*)d16(ws), n16);
  if (out32) download(stream_, out32, (const float*)d32(ws), n32);
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_layernorm_f16(const uint16_t* x, const float* g, const float* b, int64_t rows, int D, int in_place, uint16_t* out) {
  PF_HIP(hipSetDevice(device_));
  PF_CHECK(rows > 0 && rows < (1 << 24) && D > 0 && D % 8 == 0 && D <= 2048, PF_ERR_INVALID_ARG, "layernorm_f16: bad shape");
  const size_t cells = (size_t)(rows + 2 * kG) * D;
  StageCarve st;
  const auto dx = st.take<uint16_t>((size_t)rows * D);
  const auto dg = st.take<float>(D), db = st.take<float>(D);
  const auto dout = st.take<uint16_t>(cells);
  void* ws = op_ws(st);
  fill_sentinel(stream_, dout(ws), cells);
  uint16_t* dst = dout(ws) + (size_t)kG * D;
  uint16_t* src = in_place ? dst : dx(ws);
  upload(stream_, src, x, (size_t)rows * D);
  upload(stream_, dg(ws), g, D);
  upload(stream_, db(ws), b, D);
  launch_layernorm_f16(stream_, (half_t*)src, rows, D, dg(ws), db(ws), (half_t*)dst);
  download(stream_, out, (const uint16_t*)dout(ws), cells);
  PF_HIP(hipStreamSynchronize(stream_));
}

// The rows of tn at l >= len[b] hold a large finite pattern on the device: the kernel must mask them, not multiply them by zero.
void Engine::op_fsmn_dec_stream(const float* tn, const float* taps, const int32_t* len, const float* cache_in, int B, int L, int D, int k,
                                const float* x, float* x_out, float* cache_out) {
  PF_HIP(hipSetDevice(device_));
  PF_CHECK(B > 0 && L > 0 && D > 0 && k >= 2 && (int64_t)B * L * D < (1 << 28), PF_ERR_INVALID_ARG, "fsmn_dec_stream: bad shape");
  const int CW = k - 1, M = B * L;
  const size_t nx = (size_t)(M + 2 * kG) * D, nc = (size_t)((int64_t)B * D + 2 * kG) * CW;
  StageCarve st;
  const auto dt = st.take<float>((size_t)M * D), dw = st.take<float>((size_t)k * D);
  const auto dlen = st.take<int32_t>(B);
  const auto dc = st.take<float>((size_t)B * D * CW), dx = st.take<float>(nx), dco = st.take<float>(nc);
  void* ws = op_ws(st);
  fill_hostile_rows32(stream_, dt(ws), D, 0, M);
  upload_valid_rows(stream_, dt(ws), tn, len, B, L, D);
  upload(stream_, dw(ws), taps, (size_t)k * D);
  upload(stream_, dlen(ws), len, B);
  upload(stream_, dc(ws), cache_in, (size_t)B * D * CW);
  fill_sentinel(stream_, dx(ws), nx);
  fill_sentinel(stream_, dco(ws), nc);
  float* xd = dx(ws) + (size_t)kG * D;
  upload(stream_, xd, x, (size_t)M * D);
  launch_fsmn_dec_stream(stream_, dt(ws), dw(ws), dlen(ws), dc(ws), B, L, D, k, xd, dco(ws) + (size_t)kG * CW);
  download(stream_, x_out, (const float*)dx(ws), nx);
  download(stream_, cache_out, (const float*)dco(ws), nc);
  PF_HIP(hipStreamSynchronize(stream_));
}

// ---- the stand-alone FSMN memory blocks of k_misc.hip (tests/fsmn_ref.py).  Each operand lies in a buffer that holds a large
// finite pattern everywhere else (the Q | K columns beside V, kFsmnTailRows rows behind row B T - 1), each result in a guarded
// buffer that goes back whole; the launch is timed as class "gemm_op" so that the kernel the launcher noted can be read.
namespace {
constexpr int kFsmnTailRows = 16;                 // more than the longest half window (k = 21: 10 rows)
void fsmn_ex_shape(const char* op, int B, int T, int D, int k, int ldv, int col) {
  PF_CHECK(B > 0 && T > 0 && D > 0 && k > 0 && k < 64 && (int64_t)B * T * std::max(ldv, D) < (1 << 26), PF_ERR_INVALID_ARG,
           std::string(op) + ": bad shape");
  PF_CHECK(col >= 0 && ldv >= col + D, PF_ERR_INVALID_ARG, std::string(op) + ": the V columns [col, col + D) must lie inside a row of ldv cells");
}
}  // namespace

// one launch as class "gemm_op"; a launcher that refuses (it throws before it launches) leaves the class closed
template <class Fn> void Engine::fsmn_timed(Fn launch) {
  prof_begin("gemm_op", 0);
  try {
    launch();
  } catch (...) {
    prof_end("gemm_op");
    throw;
  }
  prof_end("gemm_op");
}

void Engine::op_fsmn_enc_ex(const uint16_t* v16, const float* taps, int B, int T, int D, int k, int ldv, int col, float* y_out) {
  PF_HIP(hipSetDevice(device_));
  fsmn_ex_shape("fsmn_enc_ex", B, T, D, k, ldv, col);
  const int64_t M = (int64_t)B * T, Mv = M + kFsmnTailRows;
  const size_t ny = (size_t)(M + 2 * kG) * D;
  StageCarve st;
  const auto dv = st.take<uint16_t>((size_t)Mv * ldv);
  const auto dw = st.take<float>((size_t)k * D), dy = st.take<float>(ny);
  void* ws = op_ws(st);
  {
    std::vector<uint16_t> img((size_t)Mv * ldv);
    for (size_t i = 0; i < img.size(); ++i) img[i] = hostile16_bits(i);
    for (int64_t m = 0; m < M; ++m) std::memcpy(&img[(size_t)m * ldv + col], v16 + (size_t)m * D, (size_t)D * 2);
    upload_sync(stream_, dv(ws), img);
  }
  upload(stream_, dw(ws), taps, (size_t)k * D);
  fill_sentinel(stream_, dy(ws), ny);
  fsmn_timed([&] { launch_fsmn_enc(stream_, (const half_t*)dv(ws) + col, ldv, dw(ws), B, T, D, k, dy(ws) + (size_t)kG * D); });
  download(stream_, y_out, (const float*)dy(ws), ny);
  PF_HIP(hipStreamSynchronize(stream_));
}

// form 0: what the pipeline launches — launch_fsmn_f32 on dense rows (ldv == D), launch_fsmn_f32_ld on strided ones (the fp32
// engine's V third; no mask);  1: launch_fsmn_f32 with fsmn_f32_kernel<0> forced (dense rows, no mask);  2: launch_fsmn_f32 with
// the result placed on the operand, which the launcher must refuse before anything runs.
void Engine::op_fsmn_f32_ex(const float* v, const float* taps, const float* mask, int B, int T, int D, int k, int ldv, int col, int form,
                            float* y_out) {
  PF_HIP(hipSetDevice(device_));
  fsmn_ex_shape("fsmn_f32_ex", B, T, D, k, ldv, col);
  PF_CHECK(form >= 0 && form <= 2 && D % 4 == 0, PF_ERR_INVALID_ARG, "fsmn_f32_ex: form 0 | 1 | 2, D a multiple of 4");
  const bool dense = ldv == D && col == 0;
  PF_CHECK(dense || (form == 0 && !mask), PF_ERR_UNSUPPORTED, "fsmn_f32_ex: only the unmasked launcher's-choice form takes a row stride");
  PF_CHECK(form != 1 || !mask, PF_ERR_INVALID_ARG, "fsmn_f32_ex: form 1 is the unmasked generic kernel");
  const int64_t M = (int64_t)B * T, Mv = M + kFsmnTailRows;
  const size_t ny = (size_t)(M + 2 * kG) * D;
  StageCarve st;
  const auto dv = st.take<float>((size_t)Mv * ldv), dw = st.take<float>((size_t)k * D), dm = st.take<float>((size_t)M);
  const auto dy = st.take<float>(ny);
  void* ws = op_ws(st);
  {
    std::vector<float> img((size_t)Mv * ldv);
    for (size_t i = 0; i < img.size(); ++i) img[i] = hostile32(i);
    for (int64_t m = 0; m < M; ++m) std::memcpy(&img[(size_t)m * ldv + col], v + (size_t)m * D, (size_t)D * 4);
    upload_sync(stream_, dv(ws), img);
  }
  upload(stream_, dw(ws), taps, (size_t)k * D);
  if (mask) upload(stream_, dm(ws), mask, (size_t)M);
  fill_sentinel(stream_, dy(ws), ny);
  float* yd = dy(ws) + (size_t)kG * D;
  const float* vd = dv(ws) + col;
  fsmn_timed([&] {
    if (form == 2) launch_fsmn_f32(stream_, vd, dw(ws), mask ? dm(ws) : nullptr, B, T, D, k, dv(ws));
    else if (dense) launch_fsmn_f32(stream_, vd, dw(ws), mask ? dm(ws) : nullptr, B, T, D, k, yd, form == 1);
    else launch_fsmn_f32_ld(stream_, vd, ldv, dw(ws), B, T, D, k, yd);
  });
  download(stream_, y_out, (const float*)dy(ws), ny);
  PF_HIP(hipStreamSynchronize(stream_));
}

// launch_fsmn_dec with upload_valid_rows: the rows of tn at l >= token_num[b] keep what the device buffer held, and that is
// `hostile`: 0 the large finite pattern, 1 NaN, 2 +-Inf.  A row of x at l >= token_num[b] must come back with its bits.
void Engine::op_fsmn_dec_ex(const float* tn, const float* taps, const int32_t* token_num, int B, int L, int D, int k, int hostile,
                            const float* x, float* x_out) {
  PF_HIP(hipSetDevice(device_));
  fsmn_ex_shape("fsmn_dec_ex", B, L, D, k, D, 0);
  PF_CHECK(D % 4 == 0 && hostile >= 0 && hostile <= 2, PF_ERR_INVALID_ARG, "fsmn_dec_ex: D a multiple of 4, hostile 0 | 1 | 2");
  const int64_t M = (int64_t)B * L, Mv = M + kFsmnTailRows;
  const size_t nx = (size_t)(M + 2 * kG) * D;
  StageCarve st;
  const auto dt = st.take<float>((size_t)Mv * D), dw = st.take<float>((size_t)k * D), dx = st.take<float>(nx);
  const auto dnum = st.take<int32_t>(B);
  void* ws = op_ws(st);
  {
    std::vector<float> img((size_t)Mv * D);
    for (size_t i = 0; i < img.size(); ++i)
      img[i] = hostile == 0 ? hostile32(i) : hostile == 1 ? std::nanf("") : ((i & 1u) ? -INFINITY : INFINITY);
    upload_sync(stream_, dt(ws), img);
  }
  upload_valid_rows(stream_, dt(ws), tn, token_num, B, L, D);
  upload(stream_, dw(ws), taps, (size_t)k * D);
  upload(stream_, dnum(ws), token_num, B);
  fill_sentinel(stream_, dx(ws), nx);
  float* xd = dx(ws) + (size_t)kG * D;
  upload(stream_, xd, x, (size_t)M * D);
  fsmn_timed([&] { launch_fsmn_dec(stream_, dt(ws), dw(ws), dnum(ws), B, L, D, k, xd); });
  download(stream_, x_out, (const float*)dx(ws), nx);
  PF_HIP(hipStreamSynchronize(stream_));
  check_masked_rows("fsmn_dec_ex", x_out + (size_t)kG * D, x, token_num, B, L, D);
}

// The table sits between two rows of the large finite pattern: an id clamped one row off returns them.
void Engine::op_embed_gather(const float* table, const int32_t* ids, int rows, int D, int vocab, float* out32, uint16_t* out16) {
  PF_HIP(hipSetDevice(device_));
  PF_CHECK(rows > 0 && D > 0 && D % 4 == 0 && vocab > 0, PF_ERR_INVALID_ARG, "embed_gather: bad shape");
  const size_t cells = (size_t)(rows + 2 * kG) * D;
  StageCarve st;
  const auto dt = st.take<float>((size_t)(vocab + 2) * D);
  const auto di = st.take<int32_t>(rows);
  const auto d32 = st.take<float>(cells);
  const auto d16 = st.take<uint16_t>(cells);
  void* ws = op_ws(st);
  fill_hostile_rows32(stream_, dt(ws), D, 0, 1);
  fill_hostile_rows32(stream_, dt(ws), D, vocab + 1, vocab + 2);
  upload(stream_, dt(ws) + D, table, (size_t)vocab * D);
  upload(stream_, di(ws), ids, rows);
  fill_sentinel(stream_, d32(ws), cells);
  fill_sentinel(stream_, d16(ws), cells);
  launch_embed_gather(stream_, dt(ws) + D, di(ws), rows, D, vocab, d32(ws) + (size_t)kG * D, out16 ? (half_t*)d16(ws) + (size_t)kG * D : nullptr);
  download(stream_, out32, (const float*)d32(ws), cells);
  if (out16) download(stream_, out16, (const uint16_t*)d16(ws), cells);
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_add_to_f16(const float* a, const float* b, int64_t rows, int D, uint16_t* out16) {
  PF_HIP(hipSetDevice(device_));
  PF_CHECK(rows > 0 && rows < (1 << 24) && D > 0 && D % 4 == 0, PF_ERR_INVALID_ARG, "add_to_f16: bad shape");
  const size_t n = (size_t)rows * D, cells = (size_t)(rows + 2 * kG) * D;
  StageCarve st;
  const auto da = st.take<float>(n), db = st.take<float>(n);
  const auto dout = st.take<uint16_t>(cells);
  void* ws = op_ws(st);
  upload(stream_, da(ws), a, n);
  upload(stream_, db(ws), b, n);
  fill_sentinel(stream_, dout(ws), cells);
  launch_add_to_f16(stream_, da(ws), db(ws), rows, D, (half_t*)dout(ws) + (size_t)kG * D);
  download(stream_, out16, (const uint16_t*)dout(ws), cells);
  PF_HIP(hipStreamSynchronize(stream_));
}

// dha goes up with its pad columns [V, ld_dha) as the caller filled them; logits and ids go up as the caller's, between the guards.
void Engine::op_seaco_merge(const float* dha, int ld_dha, const int64_t* dha_ids, int64_t rows, int V, int nobias, int copy_logits,
                            const float* logits_in, int ld_logits, const int64_t* ids_in, float* logits_out, int64_t* ids_out) {
  PF_HIP(hipSetDevice(device_));
  PF_CHECK(rows > 0 && rows < (1 << 20) && V > 0 && ld_dha >= V && ld_logits >= V, PF_ERR_INVALID_ARG, "seaco_merge: bad shape");
  StageCarve st;
  const auto dd = st.take<float>((size_t)rows * ld_dha);
  const auto ddi = st.take<int64_t>(rows);
  const auto dl = st.take<float>((size_t)(rows + 2 * kG) * ld_logits);
  const auto di = st.take<int64_t>((size_t)(rows + 2 * kG));
  void* ws = op_ws(st);
  upload(stream_, dd(ws), dha, (size_t)rows * ld_dha);
  upload(stream_, ddi(ws), dha_ids, rows);
  fill_sentinel(stream_, dl(ws), dl.count);
  fill_sentinel(stream_, (uint32_t*)di(ws), di.count * 2);
  float* lg = dl(ws) + (size_t)kG * ld_logits;
  int64_t* id = di(ws) + kG;
  upload(stream_, lg, logits_in, (size_t)rows * ld_logits);
  upload(stream_, id, ids_in, rows);
  launch_seaco_merge(stream_, dd(ws), ld_dha, ddi(ws), rows, V, nobias, copy_logits, lg, ld_logits, id);
  download(stream_, logits_out, (const float*)dl(ws), dl.count);
  download(stream_, ids_out, (const int64_t*)di(ws), di.count);
  PF_HIP(hipStreamSynchronize(stream_));
}

// The middle of a decoder layer in the three forms the engine can run it (include/paraformer_hip.h pf_op_dec_mid), on a
// hostile host: operand rows behind M - 1 hold the large finite pattern, x / q / tn / xn16 sit in sentinel-guarded buffers
// (q with a row stride of 520 halves), the bytes behind the split form's workspace are guarded, and a row of x at
// l >= token_num[b] must come back with the bits it went in with.
void Engine::op_dec_mid(const pf_dec_mid_desc& ds, float* x_out, float* q_out, float* tn_out, float* xn16_out, int32_t* ran_out) {
  PF_HIP(hipSetDevice(device_));
  constexpr int D = 512, F = 2048, K = 11, LDQ = 520;
  const int B = ds.B, L = ds.L, splits = ds.splits, form = ds.form;
  PF_CHECK(B > 0 && L > 0, PF_ERR_INVALID_ARG, "dec_mid: B and L must be positive");
  PF_CHECK(splits == 0 || splits == 1 || splits == 2 || splits == 3 || splits == 4 || splits == 8, PF_ERR_INVALID_ARG,
           "dec_mid: splits must be 0 (automatic) | 1 | 2 | 3 | 4 | 8");
  PF_CHECK(form == 0 || form == 1 || form == 2, PF_ERR_INVALID_ARG, "dec_mid: form must be 0, 1 or 2");
  const int M = B * L;
  const int64_t Mp = round_up(M, 256) + 128;
  const size_t wsb = ffn_dec_workspace_bytes(M, splits);
  StageCarve st;
  const auto d32 = st.take<float>((size_t)std::max<int64_t>((int64_t)M * D, (int64_t)F * D));   // the fp32 staging slot
  const auto da16 = st.take<half_t>((size_t)Mp * D), dw1 = st.take<half_t>((size_t)F * D);
  const auto dw2 = st.take<float>((size_t)D * F);
  const auto dimg = st.take<half_t>(ffn_dec_image_bytes() / 2);
  const auto dws = st.take<uint8_t>(wsb + kWsGuard);
  const auto db1 = st.take<float>(F), dgf = st.take<float>(F), dbf = st.take<float>(F);
  const auto dg2 = st.take<float>(D), db2 = st.take<float>(D), dg3 = st.take<float>(D), db3 = st.take<float>(D), dtap = st.take<float>((size_t)K * D);
  const auto dnum = st.take<int32_t>(B);
  const auto dx = st.take<float>((size_t)Mp * D);
  const auto dwq = st.take<half_t>((size_t)D * D), dwqt = st.take<half_t>(ffn_outproj_weight_bytes() / 2);
  const auto dbq = st.take<float>(D);
  const auto dq = st.take<half_t>((size_t)Mp * LDQ);
  const auto dtn = st.take<float>((size_t)Mp * D);
  const auto dxn = st.take<half_t>((size_t)Mp * D);
  void* ws = op_ws(st);
  uint32_t* behind_ws = (uint32_t*)(dws(ws) + wsb);
  fill_sentinel(stream_, behind_ws, kWsGuard / 4);
  fill_sentinel(stream_, dx(ws), (size_t)Mp * D);
  fill_sentinel(stream_, dq(ws), (size_t)Mp * LDQ);
  fill_sentinel(stream_, dtn(ws), (size_t)Mp * D);
  fill_sentinel(stream_, dxn(ws), (size_t)Mp * D);
  upload_operand16(stream_, d32(ws), ds.a, M, D, da16(ws), D, Mp);
  upload_f16(stream_, d32(ws), ds.w1, F, D, dw1(ws), D);
  upload_f16(stream_, d32(ws), ds.wq, D, D, dwq(ws), D);
  upload(stream_, dw2(ws), ds.w2, (size_t)D * F); upload(stream_, db1(ws), ds.b1, F);
  upload(stream_, dgf(ws), ds.gamma_f, F); upload(stream_, dbf(ws), ds.beta_f, F);
  upload(stream_, dg2(ws), ds.n2_gamma, D); upload(stream_, db2(ws), ds.n2_beta, D);
  upload(stream_, dg3(ws), ds.n3_gamma, D); upload(stream_, db3(ws), ds.n3_beta, D);
  upload(stream_, dtap(ws), ds.taps, (size_t)K * D); upload(stream_, dnum(ws), ds.token_num, B);
  upload(stream_, dx(ws), ds.x, (size_t)M * D); upload(stream_, dbq(ws), ds.bq, D);
  launch_ffn_dec_retile(stream_, dw1(ws), D, dw2(ws), dgf(ws), dbf(ws), db1(ws), dimg(ws));
  launch_ffn_retile_out(stream_, dwq(ws), D, dwqt(ws));
  const float qscale = 1.0f / std::sqrt(128.0f);
  FfnDecArgs f{};
  f.A = da16(ws); f.lda = D; f.img = dimg(ws); f.ws = dws(ws); f.M = M; f.splits = splits;
  f.eps_hidden = 1e-12f; f.eps = 1e-12f;
  const int32_t* num = dnum(ws);
  float* xd = dx(ws);
  float* tn = dtn(ws);
  half_t* xn = dxn(ws);
  half_t* q16 = dq(ws);
  bool ran = true;
  if (form == 0) {
    f.no_finish = true;
    prof_begin("gemm_op", 4.0 * M * (double)D * F);
    launch_ffn_dec(stream_, f);
    prof_end("gemm_op");
    // what launch_dec_mid must not use (kernels.h): of every share the partial rows and statistics of the masked positions and of
    // the rows behind M - 1 — overwritten with the hostile pattern between the two launches
    {
      const int S = splits > 0 ? splits : ffn_dec_splits(M);
      const int64_t Mq = round_up(M, 64);
      float* part = (float*)dws(ws);
      float* stats = part + (size_t)S * Mq * D;
      for (int sh = 0; sh < S; ++sh) {
        for (int b = 0; b <= B; ++b) {
          const int64_t r0 = b < B ? (int64_t)b * L + std::min(std::max(ds.token_num[b], 0), L) : M, r1 = b < B ? (int64_t)(b + 1) * L : Mq;
          fill_hostile_rows32(stream_, part + (size_t)sh * Mq * D, D, r0, r1);
          fill_hostile_rows32(stream_, stats + (size_t)sh * Mq * 2, 2, r0, r1);
        }
      }
    }
    DecMidArgs m{};
    m.ws = dws(ws); m.img = f.img; m.splits = splits; m.eps_hidden = 1e-12f;
    m.n2_g = dg2(ws); m.n2_b = db2(ws); m.eps2 = 1e-12f;
    m.fsmn_wT = dtap(ws); m.k = K; m.token_num = num; m.B = B; m.L = L; m.x = xd;
    m.n3_g = dg3(ws); m.n3_b = db3(ws);
    m.Wqt = dwqt(ws); m.bq = dbq(ws); m.qscale = qscale; m.q16 = q16; m.ldq = LDQ;
    prof_begin("gemm_op_mid", 2.0 * M * (double)D * D);
    ran = launch_dec_mid(stream_, m);
    prof_end("gemm_op_mid");
  } else {
    f.ln_g = dg2(ws); f.ln_b = db2(ws); f.n32 = tn; f.ldn32 = D;
    prof_begin("gemm_op", 4.0 * M * (double)D * F);
    launch_ffn_dec(stream_, f);
    prof_end("gemm_op");
    check_guard(stream_, "dec_mid: tn", tn, kSentinel32, result_geom(Mp, M, D, D, M));
    if (form == 1) {
      prof_begin("gemm_op_mid", 0);
      const bool fused = launch_fsmn_dec_ln(stream_, tn, dtap(ws), num, B, L, D, K, xd, dg3(ws), db3(ws), xn);
      prof_end("gemm_op_mid");
      PF_CHECK(fused, PF_ERR_UNSUPPORTED, "dec_mid: the fused FSMN + LayerNorm launch declined the geometry");
    } else {
      launch_fsmn_dec(stream_, tn, dtap(ws), num, B, L, D, K, xd);
      launch_layernorm(stream_, xd, M, D, dg3(ws), db3(ws), xn, D, nullptr, 0);
    }
    check_guard(stream_, "dec_mid: xn16", xn, kSentinel16, result_geom(Mp, M, D, D, M));
    Lin Lq;
    Lq.w = dwq(ws); Lq.bias = dbq(ws); Lq.N = D; Lq.K = D; Lq.Kpad = D;
    gemm("gemm_dec_q", Lq, xn, D, M, nullptr, 0, q16, LDQ, nullptr, 0, nullptr, 0, false, D, qscale);
  }
  if (ran_out) *ran_out = ran ? 1 : 0;
  if (!ran) return;
  check_guard(stream_, "dec_mid: x", xd, kSentinel32, result_geom(Mp, M, D, D, M, false, false));
  // (the q GEMM of forms 1 and 2 declares its destination padded to round_up(M, 256) rows, the fused kernel declares nothing)
  check_guard(stream_, "dec_mid: q", q16, kSentinel16, result_geom(Mp, M, D, LDQ, form == 0 ? (int64_t)M : round_up(M, 256)));
  check_guard(stream_, "dec_mid: the bytes behind ffn_dec_workspace_bytes", behind_ws, kSentinel32, untouched_geom(kWsGuard / 4));
  download(stream_, x_out, (const float*)xd, (size_t)M * D);
  PF_HIP(hipStreamSynchronize(stream_));
  download_f16(stream_, q_out, q16, M, D, LDQ);
  check_masked_rows("dec_mid", x_out, ds.x, ds.token_num, B, L, D);
  if (form != 0) {
    if (tn_out) download(stream_, tn_out, (const float*)tn, (size_t)M * D);
    PF_HIP(hipStreamSynchronize(stream_));
    if (xn16_out) download_f16(stream_, xn16_out, xn, M, D, D);
  }
}

// The (Bi)LSTM recurrence through the functions the heads call (lstm_recurrence16 / lstm_steps16 / lstm_ring_x3 / lstm_fp32_steps):
// xg [B, T3, ndir * 4D] fp32 gate inputs with the biases added, whh [ndir, 4D, D] fp32 (converted here as load_weights /
// timestamp_head_fp32 convert it), hout [B, T3, ndir * D].  hout is NaN-filled first: an element no form wrote stays visible.
void Engine::op_lstm(const float* xg, const float* whh, int B, int T3, int D, int ndir, int form, float* hout) {
  PF_CHECK(D == 512 && D == mc_.d_model, PF_ERR_UNSUPPORTED, "lstm: hidden size must be 512 and the engine's d_model");
  PF_CHECK(B > 0 && T3 > 0 && (ndir == 1 || ndir == 2), PF_ERR_INVALID_ARG, "lstm: bad shape");
  PF_CHECK(form >= 0 && form <= 4, PF_ERR_INVALID_ARG, "lstm: form must be 0..4");
  PF_HIP(hipSetDevice(device_));
  const size_t rows = (size_t)B * T3, nw = (size_t)ndir * 4 * D * D;
  StageCarve st;
  const auto dxg = st.take<float>(rows * ndir * 4 * D), dw32 = st.take<float>(nw);
  const auto dw16 = st.take<half_t>(nw * 2), dhs = st.take<half_t>((size_t)ndir * 4 * B * 2 * D);
  const auto dcs = st.take<float>((size_t)ndir * B * D), dho = st.take<float>(rows * ndir * D);
  const auto dsw = st.take<unsigned>(64);
  const auto dxd = st.take<float>(rows * 4 * D), dg = st.take<float>((size_t)B * 4 * D), dh = st.take<float>((size_t)B * D), dc = st.take<float>((size_t)B * D);
  void* ws = op_ws(st);
  float* xgd = dxg(ws); float* w32 = dw32(ws); half_t* w16 = dw16(ws);
  float* ho = dho(ws);
  unsigned* sw = dsw(ws);
  upload(stream_, xgd, xg, rows * ndir * 4 * D);
  upload(stream_, w32, whh, nw);
  PF_HIP(hipMemsetAsync(ho, 0xFF, rows * ndir * D * 4, stream_));
  LstmArgs a{};
  a.whh = w16; a.xg = xgd; a.hstate = dhs(ws); a.cstate = dcs(ws); a.hout = ho;
  a.B = B; a.T3 = T3; a.D = D; a.ndir = ndir;
  if (form <= 2) {
    launch_f32_to_f16(stream_, w32, (int64_t)ndir * 4 * D, D, D, w16, D);
    if (form == 1) { lstm_clear16(a); lstm_steps16(a); }
    else lstm_recurrence16(a, sw, form == 2);
  } else if (form == 3) {
    for (int d = 0; d < ndir; ++d)
      launch_split_x3(stream_, w32 + (size_t)d * 4 * D * D, 4 * D, D, D, w16 + (size_t)d * 4 * D * 2 * D, 2 * D, D, 0);
    a.cstate = nullptr;
    PF_CHECK(lstm_ring_x3(a, sw), PF_ERR_UNSUPPORTED, "lstm: the persistent recurrence does not fit on the device at this shape");
  } else {
    float* xd = dxd(ws);
    for (int d = 0; d < ndir; ++d) {                  // lstm_fp32's gate inputs are one direction's [B * T3, 4D]
      PF_HIP(hipMemcpy2DAsync(xd, (size_t)4 * D * 4, xgd + (size_t)d * 4 * D, (size_t)ndir * 4 * D * 4, (size_t)4 * D * 4, rows,
                              hipMemcpyDeviceToDevice, stream_));
      lstm_fp32_steps(xd, B, T3, w32 + (size_t)d * 4 * D * D, d == 1, dg(ws), dh(ws), dc(ws), ho, ndir * D, d * D);
    }
  }
  download(stream_, hout, (const float*)ho, rows * ndir * D);
  PF_HIP(hipStreamSynchronize(stream_));
  check_async_errors();
}

// The tail of the timestamp heads: alphas_raw = relu(sigmoid(hout w + b0) * smooth - noise) (launch_us_alpha), then alphas =
// alphas_raw * token_num / sum and the running integral peak (launch_us_peak, in place as the heads run it).
void Engine::op_us_peak(const float* hout, const float* w, const float* b0, float smooth, float noise, const int32_t* token_num, float thr,
                        int B, int T3, int W, float* alphas_raw, float* alphas, float* peak) {
  PF_CHECK(B > 0 && T3 > 0 && W > 0 && W % 4 == 0, PF_ERR_INVALID_ARG, "us_peak: bad shape");
  PF_HIP(hipSetDevice(device_));
  const size_t rows = (size_t)B * T3;
  StageCarve st;
  const auto dh = st.take<float>(rows * W), dw = st.take<float>(W), db = st.take<float>(1);
  const auto dn = st.take<int32_t>(B);
  const auto dal = st.take<float>(rows), dpk = st.take<float>(rows);
  void* ws = op_ws(st);
  float* al = dal(ws); float* pk = dpk(ws);
  upload(stream_, dh(ws), hout, rows * W);
  upload(stream_, dw(ws), w, W);
  upload(stream_, db(ws), b0, 1);
  upload(stream_, dn(ws), token_num, B);
  PF_HIP(hipMemsetAsync(al, 0xFF, rows * 4, stream_));
  PF_HIP(hipMemsetAsync(pk, 0xFF, rows * 4, stream_));
  launch_us_alpha(stream_, dh(ws), (int64_t)rows, W, dw(ws), db(ws), smooth, noise, al);
  download(stream_, alphas_raw, (const float*)al, rows);
  launch_us_peak(stream_, al, dn(ws), B, T3, thr, pk);
  download(stream_, alphas, (const float*)al, rows);
  download(stream_, peak, (const float*)pk, rows);
  PF_HIP(hipStreamSynchronize(stream_));
}

// The pipeline's vocabulary tail: log-probs y = (x - max) - log(sum exp(x - max)) and the reference's last-index
// arg-max over y (OfflineRecognizer.cs:139-152 scans the graph OUTPUT).  y == nullptr: ids only (mode 1).
void Engine::op_logsoftmax_argmax(const float* x, int64_t rows, int V, float* y, int64_t* ids) {
  PF_HIP(hipSetDevice(device_));
  if (rows == 0) return;
  const int ld = (int)round_up(V, 4);
  StageCarve st;
  const auto dx = st.take<float>((size_t)rows * ld); const auto did = st.take<int64_t>(rows);
  void* ws = op_ws(st);
  upload2d(stream_, dx(ws), ld, x, V, V, rows);
  launch_argmax(stream_, dx(ws), rows, V, ld, y ? 2 : 1, did(ws));
  if (y) download2d(stream_, y, V, (const float*)dx(ws), ld, V, rows);
  download(stream_, ids, (const int64_t*)did(ws), rows);
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_layernorm(const float* x, const float* g, const float* b, int64_t rows, int D, float* y) {
  PF_HIP(hipSetDevice(device_));
  if (rows == 0) return;
  StageCarve st;
  const auto dx = st.take<float>((size_t)rows * D), dg = st.take<float>(D), db = st.take<float>(D), dy = st.take<float>((size_t)rows * D);
  void* ws = op_ws(st);
  upload(stream_, dx(ws), x, (size_t)rows * D);
  upload(stream_, dg(ws), g, D);
  upload(stream_, db(ws), b, D);
  launch_layernorm(stream_, dx(ws), rows, D, dg(ws), db(ws), nullptr, 0, dy(ws), D);
  download(stream_, y, (const float*)dy(ws), (size_t)rows * D);
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_attention(const float* q, const float* k, const float* v, int B, int Lq, int Lk, int H, float* o) {
  PF_HIP(hipSetDevice(device_));
  const int Dm = H * 128;
  const int64_t nq = (int64_t)B * Lq, nk = (int64_t)B * Lk;
  StageCarve st;
  const auto din = st.take<float>((size_t)std::max(nq, nk) * Dm);          // the fp32 staging slot
  const auto dq = st.take<half_t>((size_t)(nq + 128) * Dm), dk = st.take<half_t>((size_t)(nk + 128) * Dm);
  const auto dv = st.take<half_t>((size_t)(nk + 128) * Dm), dout = st.take<half_t>((size_t)(nq + 128) * Dm);
  void* ws = op_ws(st);
  PF_HIP(hipMemsetAsync(dq(ws), 0, st.off - dq.off, stream_));
  upload_f16(stream_, din(ws), q, nq, Dm, dq(ws), Dm);
  upload_f16(stream_, din(ws), k, nk, Dm, dk(ws), Dm);
  upload_f16(stream_, din(ws), v, nk, Dm, dv(ws), Dm);
  AttnArgs a{};
  a.q = dq(ws); a.k = dk(ws); a.v = dv(ws); a.o = dout(ws);
  a.q_bstride = (int64_t)Lq * Dm; a.k_bstride = a.v_bstride = (int64_t)Lk * Dm; a.o_bstride = (int64_t)Lq * Dm;
  a.q_rstride = a.k_rstride = a.v_rstride = a.o_rstride = Dm;
  a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk;
  prof_begin("attn_op", 4.0 * B * (double)Lq * Lk * Dm);
  launch_attention(stream_, a);
  prof_end("attn_op");
  download_f16(stream_, o, dout(ws), nq, Dm, Dm);
}

// The attention kernels on caller data, launched as the pipeline launches them (packed / interleaved / blocked operands, shared
// K | V, output strides, forced workgroup form, range output), for the conformance tests.  Every device buffer is built on the
// host: operand buffers hold the NaN pattern of their type (0x7E00 / a quiet NaN) except the valid elements, with at least 256
// rows of slack behind each, so a read past the contract shows as a NaN in the result and never touches unmapped memory; the
// output buffer holds PF_ATTN_CANARY except what the kernel stores, and comes back whole.
void Engine::op_attention_ex(const float* q, const float* k, const float* v, int B, int Lq, int Lk, int H, const pf_attn_desc& ds, float* out,
                             void* raw, int64_t raw_bytes, float* range_out, int32_t* ran) {
  PF_HIP(hipSetDevice(device_));
  PF_CHECK(ds.struct_size == (int32_t)sizeof(pf_attn_desc), PF_ERR_INVALID_ARG, "pf_attn_desc.struct_size mismatch");
  PF_CHECK(B > 0 && Lq > 0 && Lk > 0 && H > 0, PF_ERR_INVALID_ARG, "attention_ex: empty input");
  const int Dm = H * 128, kind = ds.kind, layout = ds.layout, Bk = ds.shared_kv ? 1 : B;
  const int o_ld = ds.o_ld ? ds.o_ld : Dm;
  PF_CHECK(kind >= 0 && kind <= 2 && layout >= 0 && layout <= 3, PF_ERR_INVALID_ARG, "attention_ex: kind is 0..2, layout 0..3");
  PF_CHECK(o_ld >= Dm, PF_ERR_INVALID_ARG, "attention_ex: o_ld < heads * 128");
  PF_CHECK(layout != 1 || (Lq == Lk && !ds.shared_kv), PF_ERR_INVALID_ARG, "attention_ex: the packed layout is self-attention");
  PF_CHECK(layout != 3 || (Lq == Lk && !ds.shared_kv && kind == 0), PF_ERR_INVALID_ARG, "attention_ex: the blocked layout is f16 self-attention");
  PF_CHECK(layout != 2 || (ds.kv_off >= 0 && ds.kv_off % 8 == 0 && ds.ldkv % 8 == 0 && ds.ldkv >= ds.kv_off + 2 * Dm), PF_ERR_INVALID_ARG,
           "attention_ex: ldkv / kv_off");
  PF_CHECK(kind == 0 || (!ds.form && !range_out), PF_ERR_INVALID_ARG, "attention_ex: form and range belong to the f16 kernel");
  PF_CHECK(quant_scratch_bytes() >= 256 * 2 * sizeof(float), PF_ERR_UNSUPPORTED, "attention_ex: the range output is 256 pairs");
  const size_t es = kind == 0 ? 2 : 4;                         // operand element size
  const int64_t kSlack = 256;
  const int64_t nq = (int64_t)B * Lq, nk = (int64_t)Bk * Lk;
  // operand matrices: rows x ld elements each; q / k / v = (matrix, column offset)
  int64_t rows[3] = {0, 0, 0}, ld[3] = {0, 0, 0};
  int mat[3] = {0, 1, 2}, col[3] = {0, 0, 0};
  if (layout == 0) { rows[0] = nq + kSlack; rows[1] = rows[2] = nk + kSlack; ld[0] = ld[1] = ld[2] = Dm; }
  else if (layout == 1) { rows[0] = nq + kSlack; ld[0] = 3 * Dm; mat[1] = mat[2] = 0; col[1] = Dm; col[2] = 2 * Dm; }
  else if (layout == 2) { rows[0] = nq + kSlack; ld[0] = Dm; rows[1] = nk + kSlack; ld[1] = ds.ldkv; mat[2] = 1; col[1] = ds.kv_off; col[2] = ds.kv_off + Dm; }
  else { rows[0] = round_up(nq, 32) + kSlack; ld[0] = 2 * Dm; mat[1] = 0; col[1] = Dm; rows[2] = nk + kSlack; ld[2] = Dm; }
  const int64_t orow = kind == 2 ? 2 * (int64_t)o_ld : o_ld;   // output row in elements (kind 2: hi | lo')
  const size_t oes = kind == 1 ? 4 : 2;
  const size_t obytes = (size_t)(nq + kSlack) * orow * oes;
  PF_CHECK(raw_bytes == (int64_t)obytes, PF_ERR_INVALID_ARG, "attention_ex: raw_bytes must be " + std::to_string(obytes));
  StageCarve st;
  const Field<uint8_t> dm[3] = {st.take<uint8_t>((size_t)rows[0] * ld[0] * es), st.take<uint8_t>((size_t)rows[1] * ld[1] * es),
                                st.take<uint8_t>((size_t)rows[2] * ld[2] * es)};     // (f16 or fp32 by kind)
  const auto dout = st.take<uint8_t>(obytes);
  const auto drg = st.take<float>(quant_scratch_bytes() / 4);
  void* ws = op_ws(st);
  // host images
  std::vector<std::vector<uint16_t>> img16(3);
  std::vector<std::vector<float>> img32(3);
  const float qnan = std::numeric_limits<float>::quiet_NaN();
  for (int m = 0; m < 3; ++m) {
    if (kind == 0) img16[m].assign((size_t)rows[m] * ld[m], (uint16_t)0x7E00);
    else img32[m].assign((size_t)rows[m] * ld[m], qnan);
  }
  auto put = [&](int which, const float* src, int64_t n_rows) {
    const int m = mat[which];
    for (int64_t r = 0; r < n_rows; ++r)
      for (int c = 0; c < Dm; ++c) {
        const float x = src[(size_t)r * Dm + c];
        const size_t at = layout == 3 && which < 2 ? blocked_index(r, col[which] + c, 2 * Dm) : (size_t)r * ld[m] + col[which] + c;
        if (kind == 0) { const half_t hx = (half_t)x; std::memcpy(&img16[m][at], &hx, 2); }
        else img32[m][at] = x;
      }
  };
  put(0, q, nq); put(1, k, nk); put(2, v, nk);
  for (int m = 0; m < 3; ++m)
    upload(stream_, dm[m](ws), kind == 0 ? (const uint8_t*)img16[m].data() : (const uint8_t*)img32[m].data(), (size_t)rows[m] * ld[m] * es);
  std::vector<uint16_t> oimg(obytes / 2, (uint16_t)PF_ATTN_CANARY);
  upload(stream_, dout(ws), (const uint8_t*)oimg.data(), obytes);
  std::vector<float> rimg(quant_scratch_bytes() / 4, qnan);
  upload(stream_, drg(ws), rimg.data(), rimg.size());
  const int64_t q_bs = (int64_t)Lq * ld[mat[0]], k_bs = ds.shared_kv ? 0 : (int64_t)Lk * ld[mat[1]], v_bs = ds.shared_kv ? 0 : (int64_t)Lk * ld[mat[2]];
  *ran = 1;
  if (kind == 0) {
    AttnArgs a{};
    a.q = (half_t*)dm[mat[0]](ws) + col[0]; a.k = (half_t*)dm[mat[1]](ws) + col[1]; a.v = (half_t*)dm[mat[2]](ws) + col[2];
    a.q_bstride = q_bs; a.k_bstride = k_bs; a.v_bstride = v_bs;
    a.q_rstride = (int)ld[mat[0]]; a.k_rstride = (int)ld[mat[1]]; a.v_rstride = (int)ld[mat[2]];
    if (layout == 3) {
      a.q = a.k = (half_t*)dm[0](ws);
      a.qk_blocked = 1; a.blk_groups = 2 * Dm / 8; a.blk_brows = Lq; a.blk_kgrp = Dm / 8;
      a.q_rstride = a.k_rstride = 8;                        // ignored (alignment checks only)
    }
    a.o = (half_t*)dout(ws); a.o_bstride = (int64_t)Lq * o_ld; a.o_rstride = o_ld;
    a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk;
    a.force_nw = ds.form;
    a.range = range_out ? drg(ws) : nullptr;
    launch_attention(stream_, a);
  } else {
    const float* qd = (const float*)dm[mat[0]](ws) + col[0];
    const float* kd = (const float*)dm[mat[1]](ws) + col[1];
    const float* vd = (const float*)dm[mat[2]](ws) + col[2];
    if (kind == 1)
      launch_attention_f32(stream_, qd, q_bs, (int)ld[mat[0]], kd, k_bs, (int)ld[mat[1]], vd, v_bs, (int)ld[mat[2]], (float*)dout(ws),
                           (int64_t)Lq * o_ld, o_ld, B, H, Lq, Lk);
    else if (!launch_attention_f32_pair(stream_, qd, q_bs, (int)ld[mat[0]], kd, k_bs, (int)ld[mat[1]], vd, v_bs, (int)ld[mat[2]],
                                        (half_t*)dout(ws), (int64_t)Lq * 2 * o_ld, 2 * o_ld, o_ld, B, H, Lq, Lk))
      *ran = 0;
  }
  download(stream_, (uint8_t*)raw, (const uint8_t*)dout(ws), obytes);
  if (range_out) download(stream_, range_out, (const float*)drg(ws), (size_t)256 * 2);
  PF_HIP(hipStreamSynchronize(stream_));
  for (int64_t r = 0; r < nq; ++r)
    for (int c = 0; c < Dm; ++c) {
      float val;
      if (kind == 1) {
        val = ((const float*)raw)[(size_t)r * o_ld + c];
      } else {
        half_t hi, lo;
        std::memcpy(&hi, (const uint16_t*)raw + (size_t)r * orow + c, 2);
        val = (float)hi;
        if (kind == 2) {
          std::memcpy(&lo, (const uint16_t*)raw + (size_t)r * orow + o_ld + c, 2);
          val += (float)lo * (1.0f / 2048.0f);
        }
      }
      out[(size_t)r * Dm + c] = val;
    }
}

// The encoder's fused Q | K | V projection and its self-attention as enc_layer() launches them for long inputs: the persistent
// 256 x 192 kernel (Q scaled and K blocked, V row-major: k_gemm_qkv.hip) followed by the attention kernel reading that layout.
// x [B*T, K], w [1536, K] ([Q | K | V] rows), bias [1536] or null; outputs (each may be null) q / k / v / ctx [B*T, 512] as
// fp32 copies of the stored f16 values (q / k de-blocked on the host).
void Engine::op_qkv_attention(const float* x, const float* w, const float* bias, int B, int T, int K, float* q_out, float* k_out,
                              float* v_out, float* ctx_out) {
  PF_HIP(hipSetDevice(device_));
  const int D = 512, H = 4, N = 3 * D;
  const int M = B * T;
  PF_CHECK(M > 0 && K > 0, PF_ERR_INVALID_ARG, "qkv_attention: empty input");
  const int Kpad = (int)round_up(K, 64);
  PF_CHECK(gemm_qkvp_applicable(M, Kpad, Kpad, Kpad, D), PF_ERR_INVALID_ARG, "qkv_attention: shape not covered by the 256 x 192 kernel");
  const int64_t Mp = round_up(M, 256) + 128;
  StageCarve st;
  const auto d32 = st.take<float>((size_t)std::max<int64_t>((int64_t)M * K, (int64_t)N * K));   // the fp32 staging slot
  const auto dA = st.take<half_t>((size_t)Mp * Kpad), dW = st.take<half_t>((size_t)N * Kpad), dWp = st.take<half_t>((size_t)N * Kpad);
  const auto db = st.take<float>(N), dbp = st.take<float>(N);
  const auto dqk = st.take<half_t>((size_t)Mp * 2 * D), dv = st.take<half_t>((size_t)Mp * D), dc = st.take<half_t>((size_t)Mp * D);
  void* ws = op_ws(st);
  half_t* qk = dqk(ws);
  half_t* vb = dv(ws);
  fill_sentinel(stream_, qk, (size_t)Mp * 2 * D);
  fill_sentinel(stream_, vb, (size_t)Mp * D);
  upload_operand16(stream_, d32(ws), x, M, K, dA(ws), Kpad, Mp);
  upload_operand16(stream_, d32(ws), w, N, K, dW(ws), Kpad, N);
  if (bias) upload(stream_, db(ws), bias, N);
  launch_qkv_permute(stream_, dW(ws), Kpad, bias ? db(ws) : nullptr, dWp(ws), dbp(ws));
  const float qscale = 1.0f / std::sqrt((float)(D / H));
  prof_begin("gemm_op", 2.0 * M * (double)N * K);
  launch_gemm_qkvp(stream_, dA(ws), Kpad, dWp(ws), Kpad, dbp(ws), M, Kpad, qscale, qk, vb, D);
  prof_end("gemm_op");
  check_guard(stream_, "qkv_attention: the blocked Q | K", qk, kSentinel16, result_geom(Mp, M, 2 * D, 2 * D, round_up(M, 256), true));
  check_guard(stream_, "qkv_attention: V", vb, kSentinel16, result_geom(Mp, M, D, D, round_up(M, 256)));
  AttnArgs a{};
  a.q = qk; a.k = qk; a.qk_blocked = 1; a.blk_groups = 2 * D / 8; a.blk_brows = T; a.blk_kgrp = D / 8;
  a.v = vb; a.v_bstride = (int64_t)T * D; a.v_rstride = D;
  a.o = dc(ws); a.o_bstride = (int64_t)T * D; a.o_rstride = D;
  a.q_rstride = a.k_rstride = 8;                          // ignored (alignment checks only)
  a.B = B; a.H = H; a.Lq = T; a.Lk = T;
  prof_begin("attn_op", 4.0 * B * (double)T * T * D);
  launch_attention(stream_, a);
  prof_end("attn_op");
  if (q_out) download_blocked16(stream_, q_out, qk, M, 2 * D, 0, D);
  if (k_out) download_blocked16(stream_, k_out, qk, M, 2 * D, D, D);
  if (v_out) download_f16(stream_, v_out, vb, M, D, D);
  if (ctx_out) download_f16(stream_, ctx_out, dc(ws), M, D, D);
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_fsmn(const float* v, const float* w, const float* mask, int B, int T, int D, int k, float* y) {
  PF_HIP(hipSetDevice(device_));
  PF_CHECK(D % 4 == 0, PF_ERR_INVALID_ARG, "fsmn: D must be a multiple of 4");
  const size_t n = (size_t)B * T * D;
  if (n == 0) return;
  const std::vector<float> wT = fsmn_taps(w, D, k);
  StageCarve st;
  const auto dv = st.take<float>(n), dw = st.take<float>(wT.size()), dm = st.take<float>((size_t)B * T), dy = st.take<float>(n);
  void* ws = op_ws(st);
  upload(stream_, dv(ws), v, n);
  upload(stream_, dw(ws), wT.data(), wT.size());
  if (mask) upload(stream_, dm(ws), mask, (size_t)B * T);
  launch_fsmn_f32(stream_, dv(ws), dw(ws), mask ? dm(ws) : nullptr, B, T, D, k, dy(ws));
  download(stream_, y, (const float*)dy(ws), n);
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_cif(const float* H, const float* alphas, int B, int T, int D, float thr, int Lcap, float* E,
                    int32_t* fire_count, int32_t* token_num, int32_t* L_out) {
  PF_HIP(hipSetDevice(device_));
  PF_CHECK(D % 4 == 0 && B > 0 && T > 0, PF_ERR_INVALID_ARG, "cif: bad shape");
  const int T1 = T + 1;
  StageCarve st;
  const auto dH = st.take<float>((size_t)B * T * D);
  const CifCarve o_cif(Carve{st.off, st.align}, B, T1);             // the stage's arrays, in the order every arena keeps them
  const Field<float> da{o_cif.al, (size_t)B * T1};
  const auto dE = st.take<float>((size_t)B * std::max(Lcap, 1) * D);
  void* ws = op_ws(st);
  const CifPlan p = o_cif.plan(static_cast<char*>(ws));
  upload(stream_, dH(ws), H, (size_t)B * T * D);
  upload(stream_, da(ws), alphas, (size_t)B * T1);
  if (mc_.cif_cumsum) launch_cif_scan_cumsum(stream_, da(ws), B, T1, p);
  else launch_cif_scan(stream_, da(ws), B, T1, thr, p);
  int32_t L = 0;
  download(stream_, &L, (const int32_t*)p.max_count, 1);
  download(stream_, fire_count, (const int32_t*)p.fire_count, B);
  download(stream_, token_num, (const int32_t*)p.token_num, B);
  PF_HIP(hipStreamSynchronize(stream_));
  if (L_out) *L_out = L;
  PF_CHECK(L <= Lcap, PF_ERR_CAPACITY, "cif: Lcap " + std::to_string(Lcap) + " < L = " + std::to_string(L));
  if (Lcap == 0) return;
  if (mc_.cif_cumsum) launch_cif_gather_cumsum(stream_, dH(ws), da(ws), B, T, D, T1, p, Lcap, dE(ws));
  else launch_cif_gather(stream_, dH(ws), B, T, D, T1, p, Lcap, dE(ws));
  download(stream_, E, (const float*)dE(ws), (size_t)B * Lcap * D);
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_cif_alphas(const float* H, int B, int T, float* alphas) {
  PF_CHECK(H && alphas && B > 0 && T > 0, PF_ERR_INVALID_ARG, "cif_alphas: bad arguments");
  PF_CHECK(mc_.kind != "sensevoicesmall", PF_ERR_UNSUPPORTED, "cif_alphas: paraformer models only");
  PF_CHECK(!int8_mode_, PF_ERR_UNSUPPORTED, "cif_alphas: math_mode 0, 1 and 3 only (math_mode 2 runs math_mode 0's stage: ask an engine of that mode)");
  PF_HIP(hipSetDevice(device_));
  const int D = mc_.d_model, taps = mc_.cif_l_order + mc_.cif_r_order + 1;
  const int64_t M = (int64_t)B * T, Mp = round_up(M, 128) + 128;     // the pipeline's row padding (Engine::gemm: out_padded)
  PF_CHECK(M < (1ll << 31) / (taps * D), PF_ERR_INVALID_ARG, "cif_alphas: batch too large for 32-bit row indexing");
  StageCarve st;
  const auto dH = st.take<float>((size_t)M * D), da = st.take<float>((size_t)B * (T + 1));
  const auto dH16 = st.take<half_t>((size_t)Mp * D);
  const auto dcol = st.take<float>((size_t)Mp * taps * D), dconv = st.take<float>((size_t)Mp * D);   // (col: f16 in the f16 stage)
  void* ws = op_ws(st);
  upload(stream_, dH(ws), H, (size_t)M * D);
  PF_HIP(hipMemsetAsync(da(ws), 0xFF, (size_t)B * (T + 1) * 4, stream_));          // NaN: an alpha nobody wrote shows
  if (fp32_mode_) {
    cif_alpha_stage32(dH(ws), B, T, dcol(ws), dconv(ws), da(ws));
    x3a_src_ = nullptr;                                                                // (the operand lives in ws_tmp_)
  } else {
    launch_f32_to_f16(stream_, dH(ws), M, D, D, dH16(ws), D);
    cif_alpha_stage(dH16(ws), B, T, (half_t*)dcol(ws), dconv(ws), da(ws), nullptr);
  }
  download(stream_, alphas, (const float*)da(ws), (size_t)B * (T + 1));
  PF_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_encoder(const float* speech, int B, int T, float* H) {
  PF_HIP(hipSetDevice(device_));
  PF_CHECK(speech && H && B > 0 && T > 0, PF_ERR_INVALID_ARG, "encoder: bad arguments");
  const size_t n = (size_t)B * T * mc_.feat_dim;
  ensure(ws_speech_, n * 4);
  upload(stream_, (float*)ws_speech_.p, speech, n);
  encoder((const float*)ws_speech_.p, B, T);
  download(stream_, H, (const float*)H32_, (size_t)B * T * mc_.d_model);
  PF_HIP(hipStreamSynchronize(stream_));
}

}  // namespace pf

