// vadnet.cpp — the FSMN-VAD model score on the host (vadnet.h): the container loader, the float64 twins of k_vadnet.hip and
// the builder of the kernel's weight image.  Uses no device.
#include "vadnet.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

#include "hostutil.h"
#include "json.h"

namespace pf {

namespace {

constexpr int64_t kAlignBytes = 256;

struct RawTensor { const float* p; std::vector<int64_t> shape; int64_t numel; };

void bad(const std::string& m) { throw Error(PF_ERR_INVALID_ARG, "vad model: " + m); }

std::vector<float> take(const std::map<std::string, RawTensor>& ts, const std::string& name, std::vector<int64_t> shape) {
  auto it = ts.find(name);
  if (it == ts.end()) bad("tensor '" + name + "' is missing");
  if (it->second.shape != shape) bad("tensor '" + name + "' has the wrong shape");
  std::vector<float> v((size_t)it->second.numel);
  std::memcpy(v.data(), it->second.p, v.size() * 4);                 // (the file's data section need not be 4-aligned in memory)
  for (float x : v)
    if (!std::isfinite(x)) bad("tensor '" + name + "' holds a value that is not finite");
  return v;
}

}  // namespace

// W [N, K] -> the MFMA fragments of vadnet.h, bias [N] (or none) -> fp32 [Npad]
VadGemm add_gemm(std::vector<char>& img, const std::vector<float>& w, const std::vector<float>* bias, int N, int K) {
  VadGemm g;
  g.N = N; g.K = K; g.Npad = (int)round_up(N, 32); g.Kpad = (int)round_up(K, 16);
  g.w_off = round_up((int64_t)img.size(), kAlignBytes);
  const int64_t halves = (int64_t)g.Npad * g.Kpad;
  g.b_off = round_up(g.w_off + halves * 2, kAlignBytes);
  img.resize((size_t)(g.b_off + (int64_t)g.Npad * 4), 0);
  half_t* wt = reinterpret_cast<half_t*>(img.data() + g.w_off);
  const int KS = g.Kpad / 16;
  for (int nt = 0; nt < g.Npad / 32; ++nt)
    for (int ks = 0; ks < KS; ++ks)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int n = 32 * nt + (lane & 31), k = 16 * ks + 8 * (lane >> 5) + j;
          const float v = (n < N && k < K) ? w[(size_t)n * K + k] : 0.f;
          wt[(((int64_t)nt * KS + ks) * 64 + lane) * 8 + j] = (half_t)v;       // rounding point R0
        }
  float* b = reinterpret_cast<float*>(img.data() + g.b_off);
  for (int n = 0; n < g.Npad; ++n) b[n] = (bias && n < N) ? (*bias)[(size_t)n] : 0.f;
  return g;
}

int64_t add_floats(std::vector<char>& img, const float* src, int64_t rows, int64_t cols, int64_t ld) {
  const int64_t off = round_up((int64_t)img.size(), kAlignBytes);
  img.resize((size_t)(off + rows * ld * 4), 0);
  float* d = reinterpret_cast<float*>(img.data() + off);
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t c = 0; c < cols; ++c) d[r * ld + c] = src[r * cols + c];
  return off;
}

namespace {

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
  for (const VadGemm* g : {&m.g_in1, &m.g_in2, &m.g_out1}) widest = std::max(widest, g->Npad);
  for (const VadGemm& g : m.g_aff) widest = std::max(widest, g.Npad);
  m.lds_ld = widest + 8;
}

std::shared_ptr<const VadModel> parse(const char* data, int64_t nbytes) {
  if (!data || nbytes < 16) bad("image too small");
  if (std::memcmp(data, "PFW1", 4) != 0) bad("bad magic (expected a PFW1 container)");
  uint64_t hlen = 0;
  std::memcpy(&hlen, data + 8, 8);
  if (hlen > (uint64_t)nbytes - 16u) bad("truncated header");
  Json j = JsonParser(data + 16, (size_t)hlen).parse();
  const Json* jc = j.get("config");
  const Json* jt = j.get("tensors");
  if (!jc || jc->type != Json::Obj || !jt || jt->type != Json::Arr) bad("the header lacks config / tensors");
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

  const int64_t data_off = round_up((int64_t)(16 + hlen), kAlignBytes);
  const int64_t data_bytes = nbytes - data_off;
  if (data_bytes < 0) bad("truncated data section");
  std::map<std::string, RawTensor> ts;
  for (const Json& t : jt->arr) {
    if (t.type != Json::Obj) bad("a tensor entry is no object");
    const std::string name = t.str_or("name", "");
    if (t.str_or("dtype", "f32") != "f32") bad("tensor '" + name + "' is not f32");
    const int64_t off = t.int_or("offset", -1), nb = t.int_or("nbytes", -1);
    if (off < 0 || nb < 0 || off > data_bytes || nb > data_bytes - off) bad("the extent of tensor '" + name + "' lies outside the file");
    RawTensor r{reinterpret_cast<const float*>(data + data_off + off), {}, 1};
    const Json* sh = t.get("shape");
    if (!sh || sh->type != Json::Arr) bad("tensor '" + name + "' has no shape");
    for (const Json& d : sh->arr) {
      if (d.type != Json::Num || !(d.num >= 1.0 && d.num <= 1048576.0) || d.num != (double)(int64_t)d.num) bad("bad dimension in the shape of '" + name + "'");
      r.shape.push_back((int64_t)d.num);
      r.numel *= (int64_t)d.num;
      if (r.numel > ((int64_t)1 << 30)) bad("the shape of '" + name + "' overflows");
    }
    if (r.numel * 4 != nb) bad("shape / nbytes mismatch for '" + name + "'");
    ts[name] = r;
  }
  m->shift = take(ts, "cmvn.shift", {I});
  m->scale = take(ts, "cmvn.scale", {I});
  m->in1_w = take(ts, "in1.weight", {A, I}); m->in1_b = take(ts, "in1.bias", {A});
  m->in2_w = take(ts, "in2.weight", {L, A}); m->in2_b = take(ts, "in2.bias", {L});
  for (int l = 0; l < (int)NL; ++l) {
    const std::string p = "fsmn." + std::to_string(l) + ".";
    VadModel::Layer y;
    y.lin_w = take(ts, p + "linear.weight", {P, L});
    y.taps = take(ts, p + "taps", {lorder, P});
    y.aff_w = take(ts, p + "affine.weight", {L, P});
    y.aff_b = take(ts, p + "affine.bias", {L});
    m->layers.push_back(std::move(y));
  }
  m->out1_w = take(ts, "out1.weight", {A, L}); m->out1_b = take(ts, "out1.bias", {A});
  m->out2_w = take(ts, "out2.weight", {O, A}); m->out2_b = take(ts, "out2.bias", {O});
  build_image(*m);
  return m;
}

// y [T, N] = x [T, K] W^T + b in float64
void affine64(const std::vector<double>& x, int64_t T, int K, const std::vector<float>& w, const std::vector<float>* b, int N, bool relu,
              std::vector<double>& y) {
  y.assign((size_t)T * N, 0.0);
  for (int64_t t = 0; t < T; ++t)
    for (int n = 0; n < N; ++n) {
      double acc = 0.0;
      const float* wr = w.data() + (size_t)n * K;
      const double* xr = x.data() + (size_t)t * K;
      for (int k = 0; k < K; ++k) acc += xr[k] * (double)wr[k];
      if (b) acc += (double)(*b)[(size_t)n];
      y[(size_t)t * N + n] = (relu && acc < 0.0) ? 0.0 : acc;
    }
}

void logits64(const VadModel& m, const float* rows, int64_t T, int n_mels, std::vector<double>& z) {
  PF_CHECK(T >= 0 && n_mels >= 1 && (int64_t)n_mels * m.lfr_m == m.input_dim, PF_ERR_INVALID_ARG,
           "vad model: n_mels * lfr_m does not equal the model's input width");
  const int I = m.input_dim, left = (m.lfr_m - 1) / 2;
  std::vector<double> a((size_t)T * I), b;
  for (int64_t t = 0; t < T; ++t)
    for (int j = 0; j < m.lfr_m; ++j) {
      const int64_t src = std::min<int64_t>(std::max<int64_t>(t - left + j, 0), T - 1);
      for (int c = 0; c < n_mels; ++c) {
        const int col = j * n_mels + c;
        a[(size_t)t * I + col] = ((double)rows[src * n_mels + c] + (double)m.shift[(size_t)col]) * (double)m.scale[(size_t)col];
      }
    }
  affine64(a, T, I, m.in1_w, &m.in1_b, m.affine_dim, false, b);
  affine64(b, T, m.affine_dim, m.in2_w, &m.in2_b, m.linear_dim, true, a);
  const int P = m.proj_dim;
  std::vector<double> p, f;
  for (const VadModel::Layer& L : m.layers) {
    affine64(a, T, m.linear_dim, L.lin_w, nullptr, P, false, p);
    f = p;
    for (int k = 0; k < m.lorder; ++k) {
      const int64_t d = (int64_t)(m.lorder - 1 - k) * m.lstride;
      for (int64_t t = d; t < T; ++t)
        for (int c = 0; c < P; ++c) f[(size_t)t * P + c] += (double)L.taps[(size_t)k * P + c] * p[(size_t)(t - d) * P + c];
    }
    affine64(f, T, P, L.aff_w, &L.aff_b, m.linear_dim, true, a);
  }
  affine64(a, T, m.linear_dim, m.out1_w, &m.out1_b, m.affine_dim, false, b);
  affine64(b, T, m.affine_dim, m.out2_w, &m.out2_b, m.output_dim, false, z);
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
    if (e.code == PF_ERR_INVALID_ARG || e.code == PF_ERR_UNSUPPORTED) throw;
    throw Error(PF_ERR_INVALID_ARG, std::string("vad model: ") + e.what());      // a header that is no JSON, a number out of range
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
  const int O = m.output_dim;
  for (int64_t t = 0; t < T; ++t) {
    const double* r = z.data() + (size_t)t * O;
    double mx = r[0];
    for (int i = 1; i < O; ++i) mx = std::max(mx, r[i]);         // (a NaN makes the sums NaN below, whatever the maximum)
    double sum = 0.0, sil = 0.0;
    for (int i = 0; i < O; ++i) sum += std::exp(r[i] - mx);
    for (int32_t i : m.sil_ids) sil += std::exp(r[i] - mx);
    const double v = (1.0 - 2.0 * (sil / sum)) * 16384.0;
    levels[t] = std::isfinite(v) ? (int32_t)std::nearbyint(v) : -16384;
  }
}

pf_vad_config vad_model_default() {
  pf_vad_config c = vad_default();
  c.floor_pct = -1;
  c.abs_level = 9830;
  return c;
}

}  // namespace pf
