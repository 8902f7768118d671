// nnlm.cpp — the causal Transformer LM on the host (nnlm.h): the loader (on pfw.h's reader), the float64 twin of k_nnlm.hip,
// the fusion of LM scores into an n-best list and the builder of the kernel's weight image.  Uses no device.
#include "nnlm.h"

#include <algorithm>
#include <cmath>
#include <numeric>

#include "hostutil.h"
#include "pfw.h"

namespace pf {

namespace {

constexpr double kLnEps = 1e-12;                       // ESPnet's LayerNorm(nout, eps = 1e-12)

void bad(const std::string& m) { pfw_bad(kPfwNnlmModel, m); }

void build_image(NnlmModel& m) {
  std::vector<char>& img = m.image;
  img.clear();
  const int D = m.d_model, E = m.embed_dim;
  m.embed_off = 0;
  img.resize((size_t)m.vocab * E * 2, 0);
  {
    half_t* e = reinterpret_cast<half_t*>(img.data());
    for (size_t i = 0; i < m.embed.size(); ++i) e[i] = (half_t)m.embed[i];           // rounding point R0e
  }
  m.in = add_gemm(img, m.in_w, &m.in_b, D, E);
  m.in_g_off = add_floats(img, m.in_g.data(), 1, D, D);
  m.in_b_off = add_floats(img, m.in_beta.data(), 1, D, D);
  for (const NnlmModel::Layer& L : m.layers) {
    NnlmModel::LayerImg g;
    g.n1_g = add_floats(img, L.n1_g.data(), 1, D, D);
    g.n1_b = add_floats(img, L.n1_b.data(), 1, D, D);
    g.qkv = add_gemm(img, L.qkv_w, &L.qkv_b, 3 * D, D);
    g.out = add_gemm(img, L.out_w, &L.out_b, D, D);
    g.n2_g = add_floats(img, L.n2_g.data(), 1, D, D);
    g.n2_b = add_floats(img, L.n2_b.data(), 1, D, D);
    g.w1 = add_gemm(img, L.w1_w, &L.w1_b, m.ffn, D);
    g.w2 = add_gemm(img, L.w2_w, &L.w2_b, D, m.ffn);
    m.limg.push_back(g);
  }
  m.after_g_off = add_floats(img, m.after_g.data(), 1, D, D);
  m.after_b_off = add_floats(img, m.after_b.data(), 1, D, D);
  m.dec = add_gemm(img, m.dec_w, &m.dec_b, m.vocab, D);
}

std::shared_ptr<const NnlmModel> parse(const char* data, int64_t nbytes) {
  const PfwFrame fr = pfw_frame(data, nbytes, kPfwNnlmModel);
  const PfwIndex ix = pfw_index(data + 16, fr.header_len, fr.data_bytes, kPfwNnlmModel);
  const Json* jc = &ix.config;
  if (jc->str_or("kind", "") != "transformerlm") bad("the container's kind is not \"transformerlm\"");
  auto dim = [&](const char* k) { return jc->int_or(k, -1, INT32_MIN, INT32_MAX); };
  const int64_t V = dim("vocab"), E = dim("embed"), D = dim("d_model"), H = dim("heads"), F = dim("ffn"), NL = dim("n_layers");
  if (V < 1 || E < 1 || D < 1 || H < 1 || F < 1 || NL < 1) bad("a dimension is missing or not positive");
  PF_CHECK(D == kNnlmDModel && H == kNnlmHeads && E % 16 == 0 && E <= kNnlmMaxEmbed && F % 256 == 0 && F <= kNnlmMaxFfn &&
               NL <= kNnlmMaxLayers && V >= kNnlmMinVocab && V <= kNnlmMaxVocab,
           PF_ERR_UNSUPPORTED,
           "nnlm model: a dimension is beyond what the kernels are built for (d_model 512, heads 8, embed a multiple of 16 up to "
           "512, ffn a multiple of 256 up to 4096, layers 1 .. 24, vocab 2 .. 2^20)");
  auto m = std::make_shared<NnlmModel>();
  m->vocab = (int)V; m->embed_dim = (int)E; m->d_model = (int)D; m->heads = (int)H; m->ffn = (int)F; m->n_layers = (int)NL;
  const char* sec = data + fr.data_off;
  auto take = [&](const std::string& name, std::vector<int64_t> shape) { return pfw_take(ix, sec, name, shape, kPfwNnlmModel); };
  m->embed = take("embed.weight", {V, E});
  m->in_w = take("input.linear.weight", {D, E}); m->in_b = take("input.linear.bias", {D});
  m->in_g = take("input.norm.weight", {D}); m->in_beta = take("input.norm.bias", {D});
  for (int l = 0; l < (int)NL; ++l) {
    const std::string p = "layers." + std::to_string(l) + ".";
    NnlmModel::Layer y;
    y.n1_g = take(p + "norm1.weight", {D}); y.n1_b = take(p + "norm1.bias", {D});
    y.qkv_w = take(p + "attn.qkv.weight", {3 * D, D}); y.qkv_b = take(p + "attn.qkv.bias", {3 * D});
    y.out_w = take(p + "attn.out.weight", {D, D}); y.out_b = take(p + "attn.out.bias", {D});
    y.n2_g = take(p + "norm2.weight", {D}); y.n2_b = take(p + "norm2.bias", {D});
    y.w1_w = take(p + "ffn.w1.weight", {F, D}); y.w1_b = take(p + "ffn.w1.bias", {F});
    y.w2_w = take(p + "ffn.w2.weight", {D, F}); y.w2_b = take(p + "ffn.w2.bias", {D});
    m->layers.push_back(std::move(y));
  }
  m->after_g = take("after_norm.weight", {D}); m->after_b = take("after_norm.bias", {D});
  m->dec_w = take("decoder.weight", {V, D}); m->dec_b = take("decoder.bias", {V});
  build_image(*m);
  return m;
}

void norm64(const std::vector<double>& x, int T, int D, const std::vector<float>& g, const std::vector<float>& b, bool relu,
            std::vector<double>& y) {
  y.assign((size_t)T * D, 0.0);
  for (int t = 0; t < T; ++t) {
    const double* r = x.data() + (size_t)t * D;
    double mu = 0.0, var = 0.0;
    for (int c = 0; c < D; ++c) mu += r[c];
    mu /= D;
    for (int c = 0; c < D; ++c) var += (r[c] - mu) * (r[c] - mu);
    var /= D;
    const double inv = 1.0 / std::sqrt(var + kLnEps);
    for (int c = 0; c < D; ++c) {
      const double v = (r[c] - mu) * inv * (double)g[(size_t)c] + (double)b[(size_t)c];
      y[(size_t)t * D + c] = relu && v < 0.0 ? 0.0 : v;
    }
  }
}

}  // namespace

std::shared_ptr<const NnlmModel> nnlm_model_from_memory(const void* data, int64_t nbytes) {
  try {
    return parse(static_cast<const char*>(data), nbytes);
  } catch (const Error& e) {
    pfw_rethrow(kPfwNnlmModel, e);                    // a config field that is no integer in range
  }
}

std::shared_ptr<const NnlmModel> nnlm_model_load(const std::string& path) {
  std::vector<char> file;
  read_binary_file(path, file);
  return nnlm_model_from_memory(file.data(), (int64_t)file.size());
}

void nnlm_admit(const NnlmModel& m, const int32_t* ids, int n) {
  PF_CHECK(n >= 0 && n <= PF_NNLM_MAX_TOKENS, PF_ERR_INVALID_ARG, "nnlm: a hypothesis holds 0 .. PF_NNLM_MAX_TOKENS tokens");
  for (int i = 0; i < n; ++i) PF_CHECK(ids[i] >= 0 && ids[i] < m.vocab, PF_ERR_INVALID_ARG, "nnlm: a token id is outside the vocabulary");
}

void host_nnlm_logp(const NnlmModel& m, const int32_t* ids, int n, double* logp) {
  nnlm_admit(m, ids, n);
  const int D = m.d_model, H = m.heads, dh = D / H, E = m.embed_dim, V = m.vocab, T = n + 1;
  std::vector<double> e((size_t)T * E), x, xn, qkv, att, h, y;
  for (int t = 0; t < T; ++t) {
    const int id = t == 0 ? m.sos() : ids[t - 1];
    for (int c = 0; c < E; ++c) e[(size_t)t * E + c] = (double)m.embed[(size_t)id * E + c];
  }
  affine64(e, T, E, m.in_w, &m.in_b, D, false, y);
  norm64(y, T, D, m.in_g, m.in_beta, true, x);
  const double qs = 1.0 / std::sqrt((double)dh);
  std::vector<double> ctx((size_t)T * D), s((size_t)T);
  for (const NnlmModel::Layer& L : m.layers) {
    norm64(x, T, D, L.n1_g, L.n1_b, false, xn);
    affine64(xn, T, D, L.qkv_w, &L.qkv_b, 3 * D, false, qkv);
    for (int hd = 0; hd < H; ++hd)
      for (int t = 0; t < T; ++t) {
        double mx = -INFINITY;
        for (int u = 0; u <= t; ++u) {                             // strictly causal: the keys end at the query
          double a = 0.0;
          for (int c = 0; c < dh; ++c) a += qkv[(size_t)t * 3 * D + hd * dh + c] * qs * qkv[(size_t)u * 3 * D + D + hd * dh + c];
          s[(size_t)u] = a;
          mx = std::max(mx, a);
        }
        double sum = 0.0;
        for (int u = 0; u <= t; ++u) { s[(size_t)u] = std::exp(s[(size_t)u] - mx); sum += s[(size_t)u]; }
        for (int c = 0; c < dh; ++c) {
          double a = 0.0;
          for (int u = 0; u <= t; ++u) a += s[(size_t)u] * qkv[(size_t)u * 3 * D + 2 * D + hd * dh + c];
          ctx[(size_t)t * D + hd * dh + c] = a / sum;
        }
      }
    affine64(ctx, T, D, L.out_w, &L.out_b, D, false, att);
    for (size_t i = 0; i < x.size(); ++i) x[i] += att[i];
    norm64(x, T, D, L.n2_g, L.n2_b, false, xn);
    affine64(xn, T, D, L.w1_w, &L.w1_b, m.ffn, true, h);
    affine64(h, T, m.ffn, L.w2_w, &L.w2_b, D, false, y);
    for (size_t i = 0; i < x.size(); ++i) x[i] += y[i];
  }
  norm64(x, T, D, m.after_g, m.after_b, false, xn);
  std::vector<double> row((size_t)D), z;
  for (int t = 0; t < T; ++t) {                                    // the decoder one row at a time: [T, V] is never held
    std::copy(xn.begin() + (size_t)t * D, xn.begin() + (size_t)(t + 1) * D, row.begin());
    affine64(row, 1, D, m.dec_w, &m.dec_b, V, false, z);
    double mx = -INFINITY, sum = 0.0;
    for (int v = 0; v < V; ++v) mx = std::max(mx, z[(size_t)v]);
    for (int v = 0; v < V; ++v) sum += std::exp(z[(size_t)v] - mx);
    const int target = t < n ? ids[t] : m.sos();
    logp[t] = z[(size_t)target] - (mx + std::log(sum));
  }
}

void host_nnlm_fuse(const double* base, const double* lm_sum, const int32_t* n_tokens, int N, double weight, double bonus, double* score,
                    int32_t* order) {
  PF_CHECK(N >= 0 && weight == weight && bonus == bonus, PF_ERR_INVALID_ARG, "nnlm fuse: a negative count or a NaN weight");
  for (int i = 0; i < N; ++i) {
    PF_CHECK(n_tokens[i] >= 0, PF_ERR_INVALID_ARG, "nnlm fuse: a negative token count");
    score[i] = base[i] + weight * lm_sum[i] + bonus * (double)n_tokens[i];
    PF_CHECK(score[i] == score[i], PF_ERR_INVALID_ARG, "nnlm fuse: a score is NaN");
  }
  std::iota(order, order + N, 0);
  std::stable_sort(order, order + N, [&](int32_t a, int32_t b) { return score[a] > score[b]; });
}

}  // namespace pf
