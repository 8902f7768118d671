// punc.cpp — the CT-Transformer punctuation model on the host (punc.h): the loader (on pfw.h's reader), the float64 twins of
// k_punc.hip and of the text loop, and the builder of the kernel's weight image.  Uses no device.
#include "punc.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "hostutil.h"
#include "pfw.h"

namespace pf {

namespace {

constexpr double kLnEps = 1e-12;                       // FunASR's LayerNorm(nout, eps = 1e-12)

void bad(const std::string& m) { pfw_bad(kPfwPuncModel, m); }

// oracle/model.py sinusoidal_pe in its own float32 steps: positions 1 .. T, [sin || cos].  exp, sin and cos are taken in
// double and rounded once (tests/punc_ref.py does the same): numpy's float32 forms of them are not one function on every host.
void sinusoidal_pe(int T, int D, std::vector<float>& pe) {
  const int half = D / 2;
  const float inc = (float)(std::log(10000.0) / (double)(half - 1));
  std::vector<float> inv((size_t)half);
  for (int i = 0; i < half; ++i) inv[(size_t)i] = (float)std::exp((double)((float)i * (-inc)));
  pe.assign((size_t)T * D, 0.f);
  for (int t = 0; t < T; ++t)
    for (int i = 0; i < half; ++i) {
      const float st = (float)(t + 1) * inv[(size_t)i];
      pe[(size_t)t * D + i] = (float)std::sin((double)st);
      pe[(size_t)t * D + half + i] = (float)std::cos((double)st);
    }
}

void build_image(PuncModel& m) {
  std::vector<char>& img = m.image;
  img.clear();
  const int D = m.d_model;
  std::vector<float> pe;
  sinusoidal_pe(PF_PUNC_MAX_WINDOW, D, pe);
  m.pe_off = add_floats(img, pe.data(), PF_PUNC_MAX_WINDOW, D, D);
  m.embed_off = round_up((int64_t)img.size(), 256);
  img.resize((size_t)(m.embed_off + (int64_t)m.vocab * D * 2), 0);
  {
    half_t* e = reinterpret_cast<half_t*>(img.data() + m.embed_off);
    for (size_t i = 0; i < m.embed.size(); ++i) e[i] = (half_t)m.embed[i];           // rounding point R0e
  }
  std::vector<float> taps((size_t)m.kernel * D);
  for (const PuncModel::Layer& L : m.layers) {
    PuncModel::LayerImg g;
    g.n1_g = add_floats(img, L.n1_g.data(), 1, D, D);
    g.n1_b = add_floats(img, L.n1_b.data(), 1, D, D);
    g.qkv = add_gemm(img, L.qkv_w, &L.qkv_b, 3 * D, D);
    for (int c = 0; c < D; ++c)
      for (int j = 0; j < m.kernel; ++j) taps[(size_t)j * D + c] = L.fsmn[(size_t)c * m.kernel + j];
    g.taps = add_floats(img, taps.data(), m.kernel, D, D);
    g.out = add_gemm(img, L.out_w, &L.out_b, D, D);
    g.n2_g = add_floats(img, L.n2_g.data(), 1, D, D);
    g.n2_b = add_floats(img, L.n2_b.data(), 1, D, D);
    g.w1 = add_gemm(img, L.w1_w, &L.w1_b, m.ffn, D);
    g.w2 = add_gemm(img, L.w2_w, &L.w2_b, D, m.ffn);
    m.limg.push_back(g);
  }
  m.after_g_off = add_floats(img, m.after_g.data(), 1, D, D);
  m.after_b_off = add_floats(img, m.after_b.data(), 1, D, D);
  m.dec = add_gemm(img, m.dec_w, &m.dec_b, m.n_punc, D);
}

std::shared_ptr<const PuncModel> parse(const char* data, int64_t nbytes) {
  const PfwFrame fr = pfw_frame(data, nbytes, kPfwPuncModel);
  const PfwIndex ix = pfw_index(data + 16, fr.header_len, fr.data_bytes, kPfwPuncModel);
  const Json* jc = &ix.config;
  if (jc->str_or("kind", "") != "cttransformer") bad("the container's kind is not \"cttransformer\"");
  auto dim = [&](const char* k) { return jc->int_or(k, -1, INT32_MIN, INT32_MAX); };
  auto m = std::make_shared<PuncModel>();
  const int64_t V = dim("vocab"), D = dim("d_model"), H = dim("heads"), F = dim("ffn"), K = dim("kernel"), NL = dim("n_layers");
  if (V < 1 || D < 1 || H < 1 || F < 1 || K < 1 || NL < 1) bad("a dimension is missing or not positive");
  if (V > ((int64_t)1 << 24)) bad("the vocabulary is larger than 2^24 words");
  const Json* jp = jc->get("punc_list");
  if (!jp || jp->type != Json::Arr) bad("punc_list is missing");
  for (const Json& s : jp->arr) {
    if (s.type != Json::Str || s.str.empty()) bad("punc_list holds an entry that is no non-empty string");
    if (std::find(m->punc_list.begin(), m->punc_list.end(), s.str) != m->punc_list.end()) bad("punc_list names a mark twice");
    m->punc_list.push_back(s.str);
  }
  const int64_t P = (int64_t)m->punc_list.size();
  PF_CHECK(D == kPuncDModel && H == kPuncHeads && F % 256 == 0 && F <= kPuncMaxFfn && K % 2 == 1 && K <= kPuncMaxKernel &&
               NL <= kPuncMaxLayers && P >= 2 && P <= kPuncMaxClasses,
           PF_ERR_UNSUPPORTED,
           "punc model: a dimension is beyond what the kernels are built for (d_model 256, heads 8, ffn a multiple of 256 up to "
           "4096, kernel odd up to 31, layers 1 .. 8, classes 2 .. 32)");
  auto find = [&](const char* s) {
    auto it = std::find(m->punc_list.begin(), m->punc_list.end(), std::string(s));
    return it == m->punc_list.end() ? -1 : (int)(it - m->punc_list.begin());
  };
  m->id_unk = find("<unk>"); m->id_none = find("_"); m->id_comma = find("\xEF\xBC\x8C"); m->id_period = find("\xE3\x80\x82");
  m->id_question = find("\xEF\xBC\x9F"); m->id_pause = find("\xE3\x80\x81");
  if (m->id_unk < 0 || m->id_none < 0) bad("punc_list lacks \"<unk>\" or \"_\"");
  const int64_t se = dim("sentence_end_id");
  if (se < 0 || se >= P) bad("sentence_end_id is outside punc_list");
  m->vocab = (int)V; m->d_model = (int)D; m->heads = (int)H; m->ffn = (int)F; m->kernel = (int)K; m->n_layers = (int)NL;
  m->n_punc = (int)P; m->sentence_end_id = (int)se;
  {
    const int64_t causal = jc->int_or("causal", 0, INT32_MIN, INT32_MAX), shift = jc->int_or("sanm_shift", 0, INT32_MIN, INT32_MAX);
    if (causal != 0 && causal != 1) bad("causal is neither 0 nor 1");
    const int64_t left = (K - 1) / 2 + shift;
    if (left < 0 || left > K - 1) bad("sanm_shift moves the FSMN taps outside the kernel");
    PF_CHECK(causal ? left == K - 1 : shift == 0, PF_ERR_UNSUPPORTED,
             "punc model: a causal model takes all its FSMN taps from the left (sanm_shift = (kernel - 1) / 2), any other model none");
    m->causal = (int)causal; m->left = (int)left;
  }

  const char* sec = data + fr.data_off;
  auto take = [&](const std::string& name, std::vector<int64_t> shape) { return pfw_take(ix, sec, name, shape, kPfwPuncModel); };
  {
    auto it = ix.tensors.find("vocab");
    if (it == ix.tensors.end() || !it->second.u8 || it->second.shape.size() != 1) bad("the u8 tensor 'vocab' is missing");
    const std::string all(sec + it->second.offset, (size_t)it->second.numel);
    size_t pos = 0;
    while (pos <= all.size()) {
      size_t e = all.find('\n', pos);
      if (e == std::string::npos) e = all.size();
      m->words.push_back(all.substr(pos, e - pos));
      pos = e + 1;
    }
    if ((int64_t)m->words.size() != V) bad("'vocab' does not hold `vocab` words");
    m->word_id.reserve(m->words.size() * 2);
    for (size_t i = 0; i < m->words.size(); ++i) {
      if (m->words[i].empty()) bad("'vocab' holds an empty word");
      if (!m->word_id.emplace(m->words[i], (int32_t)i).second) bad("'vocab' holds a word twice");
    }
    auto u = m->word_id.find("<unk>");
    if (u == m->word_id.end()) bad("'vocab' lacks \"<unk>\"");
    m->unk_word = u->second;
  }
  m->embed = take("embed.weight", {V, D});
  for (int l = 0; l < (int)NL; ++l) {
    const std::string p = "layers." + std::to_string(l) + ".";
    PuncModel::Layer y;
    y.n1_g = take(p + "norm1.weight", {D}); y.n1_b = take(p + "norm1.bias", {D});
    y.qkv_w = take(p + "attn.qkv.weight", {3 * D, D}); y.qkv_b = take(p + "attn.qkv.bias", {3 * D});
    y.fsmn = take(p + "attn.fsmn.weight", {D, K});
    y.out_w = take(p + "attn.out.weight", {D, D}); y.out_b = take(p + "attn.out.bias", {D});
    y.n2_g = take(p + "norm2.weight", {D}); y.n2_b = take(p + "norm2.bias", {D});
    y.w1_w = take(p + "ffn.w1.weight", {F, D}); y.w1_b = take(p + "ffn.w1.bias", {F});
    y.w2_w = take(p + "ffn.w2.weight", {D, F}); y.w2_b = take(p + "ffn.w2.bias", {D});
    m->layers.push_back(std::move(y));
  }
  m->after_g = take("after_norm.weight", {D}); m->after_b = take("after_norm.bias", {D});
  m->dec_w = take("decoder.weight", {P, D}); m->dec_b = take("decoder.bias", {P});
  build_image(*m);
  return m;
}

void norm64(const std::vector<double>& x, int T, int D, const std::vector<float>& g, const std::vector<float>& b, std::vector<double>& y) {
  y.assign((size_t)T * D, 0.0);
  for (int t = 0; t < T; ++t) {
    const double* r = x.data() + (size_t)t * D;
    double mu = 0.0, var = 0.0;
    for (int c = 0; c < D; ++c) mu += r[c];
    mu /= D;
    for (int c = 0; c < D; ++c) var += (r[c] - mu) * (r[c] - mu);
    var /= D;
    const double inv = 1.0 / std::sqrt(var + kLnEps);
    for (int c = 0; c < D; ++c) y[(size_t)t * D + c] = (r[c] - mu) * inv * (double)g[(size_t)c] + (double)b[(size_t)c];
  }
}

bool one_byte(const std::string& text, const PuncWord& w) { return ((unsigned char)text[(size_t)w.begin] & 0x80) == 0; }

}  // namespace

std::shared_ptr<const PuncModel> punc_model_from_memory(const void* data, int64_t nbytes) {
  try {
    return parse(static_cast<const char*>(data), nbytes);
  } catch (const Error& e) {
    pfw_rethrow(kPfwPuncModel, e);                    // a config field that is no integer in range
  }
}

std::shared_ptr<const PuncModel> punc_model_load(const std::string& path) {
  std::vector<char> file;
  read_binary_file(path, file);
  return punc_model_from_memory(file.data(), (int64_t)file.size());
}

std::vector<PuncWord> host_punc_words(const PuncModel& m, const std::string& text) {
  std::vector<PuncWord> out;
  const size_t n = text.size();
  PF_CHECK(n < ((size_t)1 << 31), PF_ERR_CAPACITY, "punc: the text is longer than 2^31 bytes");
  auto emit = [&](size_t b, size_t e) {
    auto it = m.word_id.find(text.substr(b, e - b));
    out.push_back(PuncWord{it == m.word_id.end() ? m.unk_word : it->second, (int32_t)b, (int32_t)e});
  };
  size_t i = 0;
  while (i < n) {
    const unsigned char c = (unsigned char)text[i];
    if (c == 0x20 || (c >= 0x09 && c <= 0x0D)) { ++i; continue; }
    size_t e = i + 1;
    if (c < 0x80) {                                          // a maximal run of one-byte characters that are no whitespace
      while (e < n) {
        const unsigned char d = (unsigned char)text[e];
        if (d >= 0x80 || d == 0x20 || (d >= 0x09 && d <= 0x0D)) break;
        ++e;
      }
    } else {                                                 // one character: its lead byte and the continuation bytes behind it
      while (e < n && ((unsigned char)text[e] & 0xC0) == 0x80) ++e;
    }
    emit(i, e);
    i = e;
  }
  return out;
}

void host_punc_logits(const PuncModel& m, const int32_t* ids, int T, double* logits) {
  PF_CHECK(T >= 0 && T <= PF_PUNC_MAX_WINDOW, PF_ERR_INVALID_ARG, "punc: a window holds 0 .. PF_PUNC_MAX_WINDOW ids");
  if (T == 0) return;
  const int D = m.d_model, H = m.heads, dh = D / H, K = m.kernel, left = m.left;
  std::vector<float> pe;
  sinusoidal_pe(T, D, pe);
  std::vector<double> x((size_t)T * D), xn, qkv, att, h, y;
  const float scale = (float)std::sqrt((double)D);
  for (int t = 0; t < T; ++t) {
    PF_CHECK(ids[t] >= 0 && ids[t] < m.vocab, PF_ERR_INVALID_ARG, "punc: a word id is outside the vocabulary");
    for (int c = 0; c < D; ++c) {
      const float a = m.embed[(size_t)ids[t] * D + c] * scale;          // Mul, then Add: separate float32 roundings
      x[(size_t)t * D + c] = (double)(float)(a + pe[(size_t)t * D + c]);
    }
  }
  const double qs = 1.0 / std::sqrt((double)dh);
  std::vector<double> ctx((size_t)T * D), s((size_t)T);
  for (const PuncModel::Layer& L : m.layers) {
    norm64(x, T, D, L.n1_g, L.n1_b, xn);
    affine64(xn, T, D, L.qkv_w, &L.qkv_b, 3 * D, false, qkv);
    for (int hd = 0; hd < H; ++hd)
      for (int t = 0; t < T; ++t) {
        double mx = -INFINITY;
        bool nan = false;
        const int nk = m.causal ? t + 1 : T;                  // a causal model's keys end at the query
        for (int u = 0; u < nk; ++u) {
          double a = 0.0;
          for (int c = 0; c < dh; ++c) a += qkv[(size_t)t * 3 * D + hd * dh + c] * qs * qkv[(size_t)u * 3 * D + D + hd * dh + c];
          s[(size_t)u] = a;
          if (a != a) nan = true;
          mx = std::max(mx, a);
        }
        double sum = 0.0;
        for (int u = 0; u < nk; ++u) { s[(size_t)u] = nan ? NAN : std::exp(s[(size_t)u] - mx); sum += s[(size_t)u]; }
        for (int c = 0; c < dh; ++c) {
          double a = 0.0;
          for (int u = 0; u < nk; ++u) a += s[(size_t)u] * qkv[(size_t)u * 3 * D + 2 * D + hd * dh + c];
          ctx[(size_t)t * D + hd * dh + c] = a / sum;
        }
      }
    affine64(ctx, T, D, L.out_w, &L.out_b, D, false, att);
    for (int t = 0; t < T; ++t)
      for (int c = 0; c < D; ++c) {
        double f = qkv[(size_t)t * 3 * D + 2 * D + c];
        for (int j = 0; j < K; ++j) {
          const int u = t + j - left;
          if (u >= 0 && u < T) f += (double)L.fsmn[(size_t)c * K + j] * qkv[(size_t)u * 3 * D + 2 * D + c];
        }
        x[(size_t)t * D + c] += att[(size_t)t * D + c] + f;
      }
    norm64(x, T, D, L.n2_g, L.n2_b, xn);
    affine64(xn, T, D, L.w1_w, &L.w1_b, m.ffn, true, h);
    affine64(h, T, m.ffn, L.w2_w, &L.w2_b, D, false, y);
    for (size_t i = 0; i < x.size(); ++i) x[i] += y[i];
  }
  norm64(x, T, D, m.after_g, m.after_b, xn);
  affine64(xn, T, D, m.dec_w, &m.dec_b, m.n_punc, false, y);
  std::memcpy(logits, y.data(), y.size() * 8);
}

void host_punc_argmax(const PuncModel& m, const double* logits, int T, int32_t* p) {
  for (int t = 0; t < T; ++t) {
    double best = -INFINITY;
    int at = 0;
    for (int i = 0; i < m.n_punc; ++i)
      if (logits[(size_t)t * m.n_punc + i] >= best) { best = logits[(size_t)t * m.n_punc + i]; at = i; }
    p[t] = at;
  }
}

int host_punc_cut(const PuncModel& m, int32_t* p, int n, bool last) {
  if (n <= 0) return -1;
  if (last) {
    if (p[n - 1] == m.id_none || (m.id_comma >= 0 && p[n - 1] == m.id_comma) || (m.id_pause >= 0 && p[n - 1] == m.id_pause))
      p[n - 1] = m.sentence_end_id;
    return n - 1;
  }
  int cut = -1, comma = -1;
  for (int i = n - 2; i >= 2; --i) {
    if ((m.id_period >= 0 && p[i] == m.id_period) || (m.id_question >= 0 && p[i] == m.id_question)) { cut = i; break; }
    if (comma < 0 && m.id_comma >= 0 && p[i] == m.id_comma) comma = i;
  }
  const bool by_comma = cut < 0 && n > kPuncCommaWindow && comma >= 0;
  if (by_comma) cut = comma;
  // the hard cut: no cut, or a tail behind it that with the next mini-sentence would pass PF_PUNC_MAX_WINDOW
  if (n > kPuncHardWindow && (cut < 0 || n - 1 - cut > kPuncHardWindow)) return n - 1;
  if (by_comma) p[cut] = m.sentence_end_id;
  return cut;
}

void host_punc_ids(const PuncModel& m, const int32_t* ids, int64_t n, int32_t* punc_ids, std::vector<std::pair<int32_t, int32_t>>* windows) {
  std::vector<int32_t> win, p;
  std::vector<double> z;
  int64_t done = 0;
  const int64_t n_mini = (n + kPuncMini - 1) / kPuncMini;
  for (int64_t mi = 0; mi < n_mini; ++mi) {
    const int64_t b = mi * kPuncMini, e = std::min<int64_t>(n, b + kPuncMini);
    win.insert(win.end(), ids + b, ids + e);
    const int T = (int)win.size();
    z.assign((size_t)T * m.n_punc, 0.0);
    p.assign((size_t)T, 0);
    host_punc_logits(m, win.data(), T, z.data());
    host_punc_argmax(m, z.data(), T, p.data());
    const int cut = host_punc_cut(m, p.data(), T, mi == n_mini - 1);
    if (windows) windows->push_back({(int32_t)T, (int32_t)cut});
    for (int i = 0; i <= cut; ++i) punc_ids[done++] = p[(size_t)i];
    win.erase(win.begin(), win.begin() + (cut + 1));
  }
}

std::string host_punc_assemble(const PuncModel& m, const std::string& text, const std::vector<PuncWord>& words, const int32_t* punc_ids,
                               std::vector<int32_t>* sent_end) {
  std::string out;
  if (sent_end) sent_end->clear();
  for (size_t i = 0; i < words.size(); ++i) {
    const bool ascii = one_byte(text, words[i]);
    if (i > 0 && ascii && one_byte(text, words[i - 1])) out += ' ';
    out.append(text, (size_t)words[i].begin, (size_t)(words[i].end - words[i].begin));
    const int p = punc_ids[i];
    PF_CHECK(p >= 0 && p < m.n_punc, PF_ERR_INVALID_ARG, "punc: a punctuation id is outside punc_list");
    if (p != m.id_none && p != m.id_unk) {
      if (ascii && (p == m.id_comma || p == m.id_pause)) out += ',';
      else if (ascii && p == m.id_period) out += '.';
      else if (ascii && p == m.id_question) out += '?';
      else out += m.punc_list[(size_t)p];
    }
    const bool end = (m.id_period >= 0 && p == m.id_period) || (m.id_question >= 0 && p == m.id_question);
    if (sent_end && (end || i + 1 == words.size())) sent_end->push_back((int32_t)i + 1);
  }
  return out;
}

// ---- streaming (paraformer_hip.h "Punctuation, streaming"; the definition is tests/punc_stream_ref.py)
PuncStreamLayout punc_stream_layout(const PuncModel& m) {
  const int64_t kv = (int64_t)m.n_layers * kPuncStreamMaxContext * 2 * m.d_model * 2;
  return PuncStreamLayout{kv, kv + 16};
}

int64_t host_punc_stream_state_bytes(const PuncModel& m) { return (int64_t)m.n_layers * kPuncStreamMaxContext * 2 * m.d_model * 8 + 16; }

void punc_stream_admit(const PuncModel& m, int32_t count, const int32_t* ids, int n_new, int max_context, int flags) {
  PF_CHECK(m.causal == 1, PF_ERR_UNSUPPORTED, "punc stream: the model is not causal (header key causal = 1)");
  PF_CHECK(max_context >= 2 && max_context <= kPuncStreamMaxContext, PF_ERR_INVALID_ARG, "punc stream: max_context outside 2 .. 256");
  PF_CHECK(n_new >= 0 && (flags & ~1) == 0, PF_ERR_INVALID_ARG, "punc stream: a negative n_new or an unknown flag");
  PF_CHECK(count >= 0 && count <= kPuncStreamMaxContext && ((flags & 1) || count < max_context), PF_ERR_INVALID_ARG,
           "punc stream: the state block's count is outside its context (not a state of this model and max_context)");
  PF_CHECK(!(flags & 1) || (int64_t)count + n_new <= kPuncStreamMaxContext, PF_ERR_INVALID_ARG,
           "punc stream: without restarts a context holds at most 256 words");
  for (int i = 0; i < n_new; ++i)
    PF_CHECK(ids[i] >= 0 && ids[i] < m.vocab, PF_ERR_INVALID_ARG, "punc stream: a word id is outside the vocabulary");
}

void host_punc_stream_step(const PuncModel& m, void* state, const int32_t* ids, int n_new, bool flush, int max_context, int flags,
                           int32_t* marks, int32_t* mark_flags, double* logits, int32_t* flush_mark) {
  const int D = m.d_model, H = m.heads, dh = D / H, K = m.kernel, NL = m.n_layers, P = m.n_punc, C = kPuncStreamMaxContext;
  char* words_at = static_cast<char*>(state) + (size_t)NL * C * 2 * D * 8;
  int32_t words[4];
  std::memcpy(words, words_at, 16);
  punc_stream_admit(m, words[0], ids, n_new, max_context, flags);
  double* kv = static_cast<double*>(state);                      // k | v [n_layers, 256, 2, d_model]
  auto row = [&](int l, int t, int which) { return kv + (((size_t)l * C + t) * 2 + which) * D; };
  int n = words[0], last = words[1];
  std::vector<float> pe;
  sinusoidal_pe(C, D, pe);
  const float scale = (float)std::sqrt((double)D);
  const double qs = 1.0 / std::sqrt((double)dh);
  std::vector<double> x((size_t)D), xn, qkv, ctx((size_t)D), att, h, y, s((size_t)C);
  for (int w = 0; w < n_new; ++w) {
    const int t = n;                                             // the word's index in its context
    for (int c = 0; c < D; ++c) {
      const float a = m.embed[(size_t)ids[w] * D + c] * scale;
      x[(size_t)c] = (double)(float)(a + pe[(size_t)t * D + c]);
    }
    for (int l = 0; l < NL; ++l) {
      const PuncModel::Layer& L = m.layers[(size_t)l];
      norm64(x, 1, D, L.n1_g, L.n1_b, xn);
      affine64(xn, 1, D, L.qkv_w, &L.qkv_b, 3 * D, false, qkv);
      std::memcpy(row(l, t, 0), qkv.data() + D, (size_t)D * 8);
      std::memcpy(row(l, t, 1), qkv.data() + 2 * D, (size_t)D * 8);
      for (int hd = 0; hd < H; ++hd) {
        double mx = -INFINITY;
        bool nan = false;
        for (int u = 0; u <= t; ++u) {
          double a = 0.0;
          for (int c = 0; c < dh; ++c) a += qkv[(size_t)(hd * dh + c)] * qs * row(l, u, 0)[hd * dh + c];
          s[(size_t)u] = a;
          if (a != a) nan = true;
          mx = std::max(mx, a);
        }
        double sum = 0.0;
        for (int u = 0; u <= t; ++u) { s[(size_t)u] = nan ? NAN : std::exp(s[(size_t)u] - mx); sum += s[(size_t)u]; }
        for (int c = 0; c < dh; ++c) {
          double a = 0.0;
          for (int u = 0; u <= t; ++u) a += s[(size_t)u] * row(l, u, 1)[hd * dh + c];
          ctx[(size_t)(hd * dh + c)] = a / sum;
        }
      }
      affine64(ctx, 1, D, L.out_w, &L.out_b, D, false, att);
      for (int c = 0; c < D; ++c) {
        double f = row(l, t, 1)[c];
        for (int j = 0; j < K; ++j) {
          const int u = t - (K - 1) + j;                         // a tap before the context's first word is skipped
          if (u >= 0) f += (double)L.fsmn[(size_t)c * K + j] * row(l, u, 1)[c];
        }
        x[(size_t)c] += att[(size_t)c] + f;
      }
      norm64(x, 1, D, L.n2_g, L.n2_b, xn);
      affine64(xn, 1, D, L.w1_w, &L.w1_b, m.ffn, true, h);
      affine64(h, 1, m.ffn, L.w2_w, &L.w2_b, D, false, y);
      for (int c = 0; c < D; ++c) x[(size_t)c] += y[(size_t)c];
    }
    norm64(x, 1, D, m.after_g, m.after_b, xn);
    affine64(xn, 1, D, m.dec_w, &m.dec_b, P, false, y);
    if (logits) std::memcpy(logits + (size_t)w * P, y.data(), (size_t)P * 8);
    int32_t p = 0;
    host_punc_argmax(m, y.data(), 1, &p);
    int mf = 0;
    n = t + 1;
    last = p;
    if (!(flags & 1)) {
      if ((m.id_period >= 0 && p == m.id_period) || (m.id_question >= 0 && p == m.id_question)) { mf = 1; n = 0; }
      else if (n == max_context) { mf = 2; n = 0; }
    }
    marks[w] = p;
    mark_flags[w] = mf;
  }
  int fm = -1;
  if (flush) {
    if (n > 0) fm = punc_flush_mark(m, last);
    n = 0;
  }
  if (flush_mark) *flush_mark = fm;
  words[0] = n; words[1] = n > 0 ? last : 0;
  std::memcpy(words_at, words, 16);
}

}  // namespace pf
