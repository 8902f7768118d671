// vadnet.cpp — the FSMN-VAD model score on the host (vadnet.h): the loader (on pfw.h's reader), the float64 twins of k_vadnet.hip and
// the builder of the kernel's weight image.  Uses no device.
#include "vadnet.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "hostutil.h"
#include "pfw.h"

namespace pf {

namespace {

void bad(const std::string& m) { pfw_bad(kPfwVadModel, m); }

void build_image(VadModel& m) {
  std::vector<char>& img = m.image;
  img.clear();
  m.ldp = (int)round_up(m.proj_dim, 32);
  m.shift_off = add_floats(img, m.shift.data(), 1, m.input_dim, m.input_dim);
  m.scale_off = add_floats(img, m.scale.data(), 1, m.input_dim, m.input_dim);
  m.g_in1 = add_gemm(img, m.in1_w, &m.in1_b, m.affine_dim, m.input_dim);
  m.g_in2 = add_gemm(img, m.in2_w, &m.in2_b, m.linear_dim, m.affine_dim);
  for (const VadModel::Layer& L : m.layers) {
    m.g_lin.push_back(add_gemm(img, L.lin_w, nullptr, m.proj_dim, m.linear_dim));
    m.taps_off.push_back(add_floats(img, L.taps.data(), m.lorder, m.proj_dim, m.ldp));
    m.g_aff.push_back(add_gemm(img, L.aff_w, &L.aff_b, m.linear_dim, m.proj_dim));
  }
  m.g_out1 = add_gemm(img, m.out1_w, &m.out1_b, m.affine_dim, m.linear_dim);
  m.g_out2 = add_gemm(img, m.out2_w, &m.out2_b, m.output_dim, m.affine_dim);
  std::vector<float> sil((size_t)m.g_out2.Npad, 0.f);
  for (int32_t i : m.sil_ids) sil[(size_t)i] = 1.f;
  m.sil_off = add_floats(img, sil.data(), 1, m.g_out2.Npad, m.g_out2.Npad);
  int widest = std::max(m.g_in1.Kpad, m.ldp);
  for (const TileGemm* g : {&m.g_in1, &m.g_in2, &m.g_out1}) widest = std::max(widest, g->Npad);
  for (const TileGemm& g : m.g_aff) widest = std::max(widest, g.Npad);
  m.lds_ld = widest + 8;
}

std::shared_ptr<const VadModel> parse(const char* data, int64_t nbytes) {
  const PfwFrame fr = pfw_frame(data, nbytes, kPfwVadModel);
  const PfwIndex ix = pfw_index(data + 16, fr.header_len, fr.data_bytes, kPfwVadModel);
  const Json* jc = &ix.config;
  if (jc->str_or("kind", "") != "fsmnvad") bad("the container's kind is not \"fsmnvad\"");
  auto dim = [&](const char* k) { return jc->int_or(k, -1, INT32_MIN, INT32_MAX); };
  auto m = std::make_shared<VadModel>();
  const int64_t I = dim("input_dim"), A = dim("affine_dim"), L = dim("linear_dim"), P = dim("proj_dim"), O = dim("output_dim"),
                NL = dim("n_layers"), lorder = dim("lorder"), lstride = dim("lstride"), lfr_m = dim("lfr_m");
  if (I < 1 || A < 1 || L < 1 || P < 1 || O < 1 || NL < 1 || lorder < 1 || lstride < 1 || lfr_m < 1) bad("a dimension is missing or not positive");
  PF_CHECK(jc->int_or("rorder", 0, INT32_MIN, INT32_MAX) == 0, PF_ERR_UNSUPPORTED, "vad model: rorder > 0 (a look-ahead FSMN) is not supported");
  PF_CHECK(jc->int_or("lfr_n", 1, INT32_MIN, INT32_MAX) == 1, PF_ERR_UNSUPPORTED, "vad model: only lfr_n = 1 is supported");
  PF_CHECK(I <= kVadMaxWidth && A <= kVadMaxWidth && L <= kVadMaxWidth && O <= kVadMaxWidth && P <= kVadMaxProj && NL <= kVadMaxLayers &&
               lfr_m <= kVadMaxLfr && (lorder - 1) * lstride <= kVadMaxReach,
           PF_ERR_UNSUPPORTED,
           "vad model: a dimension is beyond the limits (input, affine, linear, output <= 512, proj <= 256, layers <= 8, lfr_m <= 16, "
           "(lorder - 1) * lstride <= 256)");
  if (I % lfr_m != 0) bad("input_dim is no multiple of lfr_m");
  m->input_dim = (int)I; m->affine_dim = (int)A; m->linear_dim = (int)L; m->proj_dim = (int)P; m->output_dim = (int)O;
  m->n_layers = (int)NL; m->lorder = (int)lorder; m->lstride = (int)lstride; m->lfr_m = (int)lfr_m;
  const Json* js = jc->get("sil_ids");
  if (!js || js->type != Json::Arr || js->arr.empty()) bad("sil_ids is missing or empty");
  for (const Json& s : js->arr) {
    if (s.type != Json::Num || !(s.num >= 0 && s.num < (double)O) || s.num != (double)(int64_t)s.num) bad("a silence id is outside [0, output_dim)");
    if (std::find(m->sil_ids.begin(), m->sil_ids.end(), (int32_t)s.num) != m->sil_ids.end()) bad("a silence id is listed twice");
    m->sil_ids.push_back((int32_t)s.num);
  }

  auto take = [&](const std::string& name, std::vector<int64_t> shape) { return pfw_take(ix, data + fr.data_off, name, shape, kPfwVadModel); };
  m->shift = take("cmvn.shift", {I});
  m->scale = take("cmvn.scale", {I});
  m->in1_w = take("in1.weight", {A, I}); m->in1_b = take("in1.bias", {A});
  m->in2_w = take("in2.weight", {L, A}); m->in2_b = take("in2.bias", {L});
  for (int l = 0; l < (int)NL; ++l) {
    const std::string p = "fsmn." + std::to_string(l) + ".";
    VadModel::Layer y;
    y.lin_w = take(p + "linear.weight", {P, L});
    y.taps = take(p + "taps", {lorder, P});
    y.aff_w = take(p + "affine.weight", {L, P});
    y.aff_b = take(p + "affine.bias", {L});
    m->layers.push_back(std::move(y));
  }
  m->out1_w = take("out1.weight", {A, L}); m->out1_b = take("out1.bias", {A});
  m->out2_w = take("out2.weight", {O, A}); m->out2_b = take("out2.bias", {O});
  build_image(*m);
  return m;
}

// Levels [t0, t0 + n) of one utterance or stream, the per-row code of both host twins.  frame(src): fbank row src of the stream,
// asked for src in [0, last] only (last: the newest frame the LFR window may touch).  hist [n_layers][reach * P]: per layer the p
// rows t0 - reach .. t0 - 1 (in), t0 + n - reach .. t0 + n - 1 (out); a row before frame 0 is never read.  z [n, output_dim].
template <class Frame>
void block64(const VadModel& m, Frame&& frame, int64_t last, int64_t t0, int64_t n, int n_mels, std::vector<std::vector<double>>& hist,
             std::vector<double>& z) {
  const int I = m.input_dim, left = (m.lfr_m - 1) / 2;
  const int64_t T = n;
  std::vector<double> a((size_t)T * I), b;
  for (int64_t t = 0; t < T; ++t)
    for (int j = 0; j < m.lfr_m; ++j) {
      const int64_t src = std::min<int64_t>(std::max<int64_t>(t0 + t - left + j, 0), last);
      const float* row = frame(src);
      for (int c = 0; c < n_mels; ++c) {
        const int col = j * n_mels + c;
        a[(size_t)t * I + col] = ((double)row[c] + (double)m.shift[(size_t)col]) * (double)m.scale[(size_t)col];
      }
    }
  affine64(a, T, I, m.in1_w, &m.in1_b, m.affine_dim, false, b);
  affine64(b, T, m.affine_dim, m.in2_w, &m.in2_b, m.linear_dim, true, a);
  const int P = m.proj_dim;
  const int64_t reach = (int64_t)(m.lorder - 1) * m.lstride;
  std::vector<double> p, f, w;
  for (size_t l = 0; l < m.layers.size(); ++l) {
    const VadModel::Layer& L = m.layers[l];
    affine64(a, T, m.linear_dim, L.lin_w, nullptr, P, false, p);
    w = hist[l];                                                 // the window: the history rows, then p
    w.insert(w.end(), p.begin(), p.end());
    f = p;
    for (int k = 0; k < m.lorder; ++k) {
      const int64_t d = (int64_t)(m.lorder - 1 - k) * m.lstride;
      for (int64_t t = std::max<int64_t>(d - t0, 0); t < T; ++t)  // d <= t0 + t on the absolute frame index
        for (int c = 0; c < P; ++c) f[(size_t)t * P + c] += (double)L.taps[(size_t)k * P + c] * w[(size_t)(reach + t - d) * P + c];
    }
    hist[l].assign(w.end() - (long)(reach * P), w.end());
    affine64(f, T, P, L.aff_w, &L.aff_b, m.linear_dim, true, a);
  }
  affine64(a, T, m.linear_dim, m.out1_w, &m.out1_b, m.affine_dim, false, b);
  affine64(b, T, m.affine_dim, m.out2_w, &m.out2_b, m.output_dim, false, z);
}

std::vector<std::vector<double>> fresh_hist(const VadModel& m) {
  return std::vector<std::vector<double>>((size_t)m.n_layers, std::vector<double>((size_t)(m.lorder - 1) * m.lstride * m.proj_dim, 0.0));
}

void logits64(const VadModel& m, const float* rows, int64_t T, int n_mels, std::vector<double>& z) {
  PF_CHECK(T >= 0 && n_mels >= 1 && (int64_t)n_mels * m.lfr_m == m.input_dim, PF_ERR_INVALID_ARG,
           "vad model: n_mels * lfr_m does not equal the model's input width");
  std::vector<std::vector<double>> hist = fresh_hist(m);
  block64(m, [&](int64_t src) { return rows + src * n_mels; }, T - 1, 0, T, n_mels, hist, z);
}

// the level of one frame from its logits r [output_dim]
int32_t level64(const VadModel& m, const double* r) {
  const int O = m.output_dim;
  double mx = r[0];
  for (int i = 1; i < O; ++i) mx = std::max(mx, r[i]);         // (a NaN makes the sums NaN below, whatever the maximum)
  double sum = 0.0, sil = 0.0;
  for (int i = 0; i < O; ++i) sum += std::exp(r[i] - mx);
  for (int32_t i : m.sil_ids) sil += std::exp(r[i] - mx);
  const double v = (1.0 - 2.0 * (sil / sum)) * 16384.0;
  return std::isfinite(v) ? (int32_t)std::nearbyint(v) : -16384;
}

}  // namespace

const std::vector<float>* VadModel::tensor(const std::string& name) const {
  if (name == "cmvn.shift") return &shift;
  if (name == "cmvn.scale") return &scale;
  if (name == "in1.weight") return &in1_w;
  if (name == "in1.bias") return &in1_b;
  if (name == "in2.weight") return &in2_w;
  if (name == "in2.bias") return &in2_b;
  if (name == "out1.weight") return &out1_w;
  if (name == "out1.bias") return &out1_b;
  if (name == "out2.weight") return &out2_w;
  if (name == "out2.bias") return &out2_b;
  for (size_t l = 0; l < layers.size(); ++l) {
    const std::string p = "fsmn." + std::to_string(l) + ".";
    if (name == p + "linear.weight") return &layers[l].lin_w;
    if (name == p + "taps") return &layers[l].taps;
    if (name == p + "affine.weight") return &layers[l].aff_w;
    if (name == p + "affine.bias") return &layers[l].aff_b;
  }
  return nullptr;
}

std::shared_ptr<const VadModel> vad_model_from_memory(const void* data, int64_t nbytes) {
  try {
    return parse(static_cast<const char*>(data), nbytes);
  } catch (const Error& e) {
    pfw_rethrow(kPfwVadModel, e);                     // a config field that is no integer in range
  }
}

std::shared_ptr<const VadModel> vad_model_load(const std::string& path) {
  std::vector<char> file;
  read_binary_file(path, file);
  return vad_model_from_memory(file.data(), (int64_t)file.size());
}

void host_vad_model_logits(const VadModel& m, const float* rows, int64_t T, int n_mels, double* logits) {
  std::vector<double> z;
  logits64(m, rows, T, n_mels, z);
  if (T > 0) std::memcpy(logits, z.data(), z.size() * 8);
}

void host_vad_model_levels(const VadModel& m, const float* rows, int64_t T, int n_mels, int32_t* levels) {
  std::vector<double> z;
  logits64(m, rows, T, n_mels, z);
  for (int64_t t = 0; t < T; ++t) levels[t] = level64(m, z.data() + (size_t)t * m.output_dim);
}

pf_vad_config vad_model_default() {
  pf_vad_config c = vad_default();
  c.floor_pct = -1;
  c.abs_level = 9830;
  return c;
}

// ---- streaming (paraformer_hip.h "Voice-activity endpointing, streaming, model score"; the schedule is tests/vadnet_stream_ref.py)
int64_t vad_stream_released(const VadModel& m, int64_t n, bool flushed) {
  const int64_t right = m.lfr_m - 1 - (m.lfr_m - 1) / 2;
  return flushed ? n : std::max<int64_t>(0, n - right);
}

void vad_stream_admit(int64_t count, int32_t flushed, int64_t n_new) {
  PF_CHECK(n_new >= 0, PF_ERR_INVALID_ARG, "vad model stream: negative frame count");
  PF_CHECK(count >= 0 && count <= PF_ENDPOINT_MAX_STREAM_FRAMES && (flushed | 1) == 1, PF_ERR_INVALID_ARG,
           "vad model stream: not a state block of this model");
  PF_CHECK(!(flushed && n_new > 0), PF_ERR_INVALID_ARG, "vad model stream: frames after a flush");
  PF_CHECK(count + n_new <= PF_ENDPOINT_MAX_STREAM_FRAMES, PF_ERR_CAPACITY,
           "vad model stream: more than PF_ENDPOINT_MAX_STREAM_FRAMES frames in one stream");
}

VadStreamLayout vad_stream_layout(const VadModel& m) {
  VadStreamLayout L;
  L.hist_floats = (int64_t)m.n_layers * (m.lorder - 1) * m.lstride * m.ldp;
  L.tail_floats = (int64_t)(m.lfr_m - 1) * (m.input_dim / m.lfr_m);
  L.bytes = round_up(4 * (L.hist_floats + L.tail_floats) + 8, 16);
  L.words_off = L.bytes - 8;
  return L;
}

namespace {
// the host twin's state: hist [n_layers][reach][proj] float64 | row tail [lfr_m - 1][n_mels] fp32 | count | flushed
struct HostStreamLayout { int64_t hist_doubles, tail_floats, words_off, bytes; };
HostStreamLayout host_stream_layout(const VadModel& m) {
  HostStreamLayout L;
  L.hist_doubles = (int64_t)m.n_layers * (m.lorder - 1) * m.lstride * m.proj_dim;
  L.tail_floats = (int64_t)(m.lfr_m - 1) * (m.input_dim / m.lfr_m);
  L.bytes = round_up(8 * L.hist_doubles + 4 * L.tail_floats + 8, 8);
  L.words_off = L.bytes - 8;
  return L;
}
}  // namespace

int64_t host_vad_stream_state_bytes(const VadModel& m) { return host_stream_layout(m).bytes; }

int64_t host_vad_model_stream(const VadModel& m, void* state, const float* rows, int64_t n_new, bool flush, int n_mels, int32_t* levels,
                              double* logits, int64_t cap) {
  PF_CHECK(n_mels >= 1 && (int64_t)n_mels * m.lfr_m == m.input_dim, PF_ERR_INVALID_ARG,
           "vad model: n_mels * lfr_m does not equal the model's input width");
  const HostStreamLayout L = host_stream_layout(m);
  char* sb = static_cast<char*>(state);
  int32_t words[2];
  std::memcpy(words, sb + L.words_off, 8);
  vad_stream_admit(words[0], words[1], n_new);
  const int64_t n = words[0], n1 = n + n_new;
  const bool fl = flush || words[1] != 0;
  const int64_t rel0 = vad_stream_released(m, n, words[1] != 0), rel1 = vad_stream_released(m, n1, fl), n_out = rel1 - rel0;
  PF_CHECK(n_out <= cap || (!levels && !logits), PF_ERR_CAPACITY,
           "vad model stream: capacity " + std::to_string(cap) + " < " + std::to_string(n_out) + " released levels");
  const int keep = m.lfr_m - 1, P = m.proj_dim;
  const int64_t reach = (int64_t)(m.lorder - 1) * m.lstride;
  std::vector<float> tail((size_t)L.tail_floats);
  if (L.tail_floats) std::memcpy(tail.data(), sb + 8 * L.hist_doubles, (size_t)L.tail_floats * 4);
  // frame f of the stream: the row tail holds frames n - keep .. n - 1, the new rows n .. n1 - 1
  auto frame = [&](int64_t f) { return f >= n ? rows + (f - n) * n_mels : tail.data() + (f - n + keep) * n_mels; };
  if (n_out > 0) {
    std::vector<std::vector<double>> hist = fresh_hist(m);
    for (int l = 0; l < m.n_layers; ++l)
      if (reach) std::memcpy(hist[(size_t)l].data(), sb + 8 * (size_t)l * reach * P, (size_t)reach * P * 8);
    std::vector<double> z;
    block64(m, frame, n1 - 1, rel0, n_out, n_mels, hist, z);
    for (int l = 0; l < m.n_layers; ++l)
      if (reach) std::memcpy(sb + 8 * (size_t)l * reach * P, hist[(size_t)l].data(), (size_t)reach * P * 8);
    if (logits) std::memcpy(logits, z.data(), z.size() * 8);
    if (levels)
      for (int64_t t = 0; t < n_out; ++t) levels[t] = level64(m, z.data() + (size_t)t * m.output_dim);
  }
  if (n_new > 0) {
    std::vector<float> nt((size_t)L.tail_floats, 0.f);
    for (int q = 0; q < keep; ++q) {
      const int64_t f = n1 - keep + q;
      if (f >= 0) std::memcpy(nt.data() + (size_t)q * n_mels, frame(f), (size_t)n_mels * 4);
    }
    if (L.tail_floats) std::memcpy(sb + 8 * L.hist_doubles, nt.data(), (size_t)L.tail_floats * 4);
    words[0] = (int32_t)n1;
  }
  if (flush) words[1] = 1;
  std::memcpy(sb + L.words_off, words, 8);
  return n_out;
}

pf_endpoint_config endpoint_model_default() {
  pf_endpoint_config c = endpoint_default();
  c.rise = -1;
  c.abs_level = 9830;
  return c;
}

}  // namespace pf
