// lm.cpp — the n-gram language model on the host: builder, ARPA reader, scorer (lm.h; the image is described in lm_dev.h).
#include "lm.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <unordered_map>

#include "lm_dev.h"

namespace pf {

namespace {

// the n-grams as a trie read left to right: node 0 is the empty context, a node of depth k a context of k tokens.  Only
// contexts (depth < O) are nodes; an n-gram of the full order is an arc out of its context node and nothing else.
struct LmTrie {
  std::unordered_map<uint64_t, int32_t> child;     // (node << 32 | token) -> node
  std::vector<int32_t> depth, fail, lnext;
  std::vector<float> logp, bo;
  std::vector<char> listed;
  int32_t find(int32_t u, int32_t c) const {
    auto it = child.find(((uint64_t)(uint32_t)u << 32) | (uint32_t)c);
    return it == child.end() ? -1 : it->second;
  }
  int32_t get(int32_t u, int32_t c) {
    const uint64_t k = ((uint64_t)(uint32_t)u << 32) | (uint32_t)c;
    auto it = child.find(k);
    if (it != child.end()) return it->second;
    const int32_t v = (int32_t)depth.size();
    child.emplace(k, v);
    depth.push_back(depth[(size_t)u] + 1);
    fail.push_back(0);
    lnext.push_back(0);
    logp.push_back(0.f);
    bo.push_back(0.f);
    listed.push_back(0);
    return v;
  }
  // the longest suffix of path(x) + c that is a node, x's own extension included
  int32_t step(int32_t x, int32_t c) const {
    for (;;) {
      const int32_t v = find(x, c);
      if (v >= 0) return v;
      if (x == 0) return 0;
      x = fail[(size_t)x];
    }
  }
};

struct RawArc { int32_t u, tok; float logp; int32_t next; };

}  // namespace

void lm_check_weights(float alpha, float beta, int flags) {
  if (!(alpha >= 0.f) || std::isinf(alpha) || !std::isfinite(beta)) throw Error(PF_ERR_INVALID_ARG, "lm: alpha is finite and >= 0, beta finite");
  if (flags & ~PF_LM_EOS) throw Error(PF_ERR_INVALID_ARG, "lm: unknown flag");
}

std::shared_ptr<const LmImage> lm_build(int order, const int64_t* n_ngrams, const int32_t* ids, const float* logp, const float* backoff,
                                        int V, int bos, int eos, int unk, float oov, const int32_t* transparent, int n_transparent) {
  if (order < 1 || order > PF_LM_ORDER_MAX) throw Error(PF_ERR_INVALID_ARG, "lm_build: the order is 1 .. PF_LM_ORDER_MAX");
  if (!n_ngrams || V < 2 || n_transparent < 0 || (n_transparent > 0 && !transparent)) throw Error(PF_ERR_INVALID_ARG, "lm_build: bad n_ngrams / V / transparent");
  int64_t total = 0, total_ids = 0;
  for (int k = 1; k <= order; ++k) {
    if (n_ngrams[k - 1] < 0) throw Error(PF_ERR_INVALID_ARG, "lm_build: a negative n-gram count");
    total += n_ngrams[k - 1];
    total_ids += n_ngrams[k - 1] * k;
  }
  if (total > 0 && (!ids || !logp || !backoff)) throw Error(PF_ERR_INVALID_ARG, "lm_build: null argument");
  // 12 bytes an arc at the least: refuse before anything of that size is made
  if (total > (int64_t)PF_LM_IMAGE_BYTES_MAX / 12) throw Error(PF_ERR_CAPACITY, "lm_build: an image over PF_LM_IMAGE_BYTES_MAX");
  for (int x : {bos, eos, unk})
    if (x != -1 && (x < 1 || x >= V)) throw Error(PF_ERR_INVALID_ARG, "lm_build: bos / eos / unk are -1 or ids in [1, V)");
  if (!std::isfinite(oov)) throw Error(PF_ERR_INVALID_ARG, "lm_build: a non-finite oov weight");
  for (int i = 0; i < n_transparent; ++i)
    if (transparent[i] < 0 || transparent[i] >= V) throw Error(PF_ERR_INVALID_ARG, "lm_build: a transparent id outside [0, V)");
  for (int64_t x = 0; x < total_ids; ++x)
    if (ids[x] < 1 || ids[x] >= V) throw Error(PF_ERR_INVALID_ARG, "lm_build: an id outside [1, V)");
  for (int64_t x = 0; x < total; ++x)
    if (!std::isfinite(logp[x])) throw Error(PF_ERR_INVALID_ARG, "lm_build: a non-finite log-probability");

  LmTrie t;
  t.depth.push_back(0); t.fail.push_back(0); t.lnext.push_back(0); t.logp.push_back(0.f); t.bo.push_back(0.f); t.listed.push_back(0);
  std::vector<RawArc> arcs;                          // every listed n-gram of order >= 2, as (context node, token)
  const int32_t* w = ids;
  int64_t x = 0;
  for (int k = 1; k <= order; ++k)
    for (int64_t i = 0; i < n_ngrams[k - 1]; ++i, ++x, w += k) {
      int32_t u = 0;
      for (int p = 0; p + 1 < k; ++p) u = t.get(u, w[p]);
      if (k < order) {
        const float b = backoff[x];
        if (std::isinf(b)) throw Error(PF_ERR_INVALID_ARG, "lm_build: an infinite back-off weight");
        const int32_t v = t.get(u, w[k - 1]);
        if (t.listed[(size_t)v]) throw Error(PF_ERR_INVALID_ARG, "lm_build: a duplicate n-gram");
        t.listed[(size_t)v] = 1;
        t.logp[(size_t)v] = logp[x];
        t.bo[(size_t)v] = b != b ? 0.f : b;          // listed without a back-off: +0, and g + 0 is g
      }
      if (k >= 2) arcs.push_back(RawArc{u, w[k - 1], logp[x], 0});
      else if (order == 1) {                         // the unigrams of an order-1 model are no nodes: keep them apart
        arcs.push_back(RawArc{0, w[0], logp[x], 0});
      }
    }
  // order 1: the "arcs" above are the unigrams; duplicates are found by the sort below, then they move to the dense table
  std::sort(arcs.begin(), arcs.end(), [](const RawArc& a, const RawArc& b) { return a.u != b.u ? a.u < b.u : a.tok < b.tok; });
  for (size_t i = 1; i < arcs.size(); ++i)
    if (arcs[i].u == arcs[i - 1].u && arcs[i].tok == arcs[i - 1].tok) throw Error(PF_ERR_INVALID_ARG, "lm_build: a duplicate n-gram");
  const int32_t start = (order > 1 && bos >= 0) ? t.get(0, bos) : 0;
  const size_t S = t.depth.size();

  // suffix links by depth: fail(v) the longest proper suffix of v's context that is a node; lnext(v) the longest suffix of it,
  // itself included, that is a LISTED n-gram (0: none) — the state a search is in after an n-gram that ends there
  std::vector<std::vector<std::pair<int32_t, int32_t>>> by_depth((size_t)order);       // (parent, token) of the nodes of a depth
  for (auto& kv : t.child) by_depth[(size_t)t.depth[(size_t)kv.second]].push_back({(int32_t)(kv.first >> 32), (int32_t)(uint32_t)kv.first});
  for (int d = 1; d < order; ++d)
    for (auto& pc : by_depth[(size_t)d]) {
      const int32_t v = t.find(pc.first, pc.second);
      const int32_t f = pc.first == 0 ? 0 : t.step(t.fail[(size_t)pc.first], pc.second);
      t.fail[(size_t)v] = f;
      t.lnext[(size_t)v] = t.listed[(size_t)v] ? v : t.lnext[(size_t)f];
    }
  std::vector<float> uni_logp((size_t)V, 0.f);
  std::vector<char> uni_listed((size_t)V, 0);
  if (order == 1) {
    for (auto& a : arcs) { uni_listed[(size_t)a.tok] = 1; uni_logp[(size_t)a.tok] = a.logp; }
    arcs.clear();
  } else {
    for (auto& pc : by_depth[1])
      if (pc.first == 0) {
        const int32_t v = t.find(0, pc.second);
        if (t.listed[(size_t)v]) { uni_listed[(size_t)pc.second] = 1; uni_logp[(size_t)pc.second] = t.logp[(size_t)v]; }
      }
    for (auto& a : arcs) {
      const int32_t v = t.depth[(size_t)a.u] + 1 < order ? t.find(a.u, a.tok) : -1;     // a listed child is the n-gram's own node
      a.next = v >= 0 ? t.lnext[(size_t)v] : t.lnext[(size_t)(a.u == 0 ? 0 : t.step(t.fail[(size_t)a.u], a.tok))];
    }
  }
  if (unk >= 0 && !uni_listed[(size_t)unk]) throw Error(PF_ERR_INVALID_ARG, "lm_build: unk is not a listed unigram");

  // the image
  auto up4 = [](size_t words) { return (words + 3) / 4 * 4; };
  const size_t off_uni = kLmHdrWords, off_st = off_uni + ((size_t)V + 1) * 4, off_key = off_st + S * 4, off_arc = off_key + up4(arcs.size());
  const size_t n_words = off_arc + up4(arcs.size() * 2);
  if (n_words * 4 > (size_t)PF_LM_IMAGE_BYTES_MAX) throw Error(PF_ERR_CAPACITY, "lm_build: an image of " + std::to_string(n_words * 4) + " bytes > PF_LM_IMAGE_BYTES_MAX");
  auto img = std::make_shared<LmImage>();
  img->words.assign(n_words, 0);
  int32_t* h = img->words.data();
  h[kLmHdrMagic] = kLmMagic; h[kLmHdrOrder] = order; h[kLmHdrV] = V; h[kLmHdrStates] = (int32_t)S; h[kLmHdrArcs] = (int32_t)arcs.size();
  h[kLmHdrStart] = start; h[kLmHdrEos] = eos; std::memcpy(&h[kLmHdrOovBits], &oov, 4);
  h[kLmHdrUni] = (int32_t)off_uni; h[kLmHdrState] = (int32_t)off_st; h[kLmHdrKey] = (int32_t)off_key; h[kLmHdrArc] = (int32_t)off_arc;
  LmUni* uni = (LmUni*)(h + off_uni);
  LmState* st = (LmState*)(h + off_st);
  int32_t* key = h + off_key;
  LmArc* arc = (LmArc*)(h + off_arc);
  auto uni_of = [&](int c) {
    const int32_t v = order > 1 ? t.find(0, c) : -1;
    return LmUni{c, uni_logp[(size_t)c], v >= 0 ? t.lnext[(size_t)v] : 0, 0};
  };
  for (int c = 0; c <= V; ++c) {                     // (entry V: what an id outside the table is)
    if (c >= 1 && c < V && uni_listed[(size_t)c]) uni[c] = uni_of(c);
    else if (unk >= 0) uni[c] = uni_of(unk);
    else uni[c] = LmUni{kLmOov, 0.f, 0, 0};
  }
  for (int i = 0; i < n_transparent; ++i) uni[transparent[i]] = LmUni{kLmTransparent, 0.f, 0, 0};
  for (size_t s = 0; s < S; ++s) st[s] = LmState{0, 0, t.fail[s], t.bo[s]};
  for (size_t i = 0; i < arcs.size(); ++i) {
    LmState& s = st[(size_t)arcs[i].u];
    if (s.count == 0) s.begin = (int32_t)i;
    ++s.count;
    key[i] = arcs[i].tok;
    arc[i] = LmArc{arcs[i].logp, arcs[i].next};
  }
  st[0].begin = 0; st[0].count = 0;                 // the empty context is the dense table: its arcs (the bigram-less unigrams) are not searched
  img->order = order; img->V = V; img->states = (int64_t)S; img->arcs = (int64_t)arcs.size();
  img->bos = bos; img->eos = eos; img->unk = unk;
  return img;
}

void lm_score(const LmImage& lm, const int32_t* ids, int n, float alpha, float beta, int flags, double* g_out, int32_t* state_out,
              double* g_pos, int32_t* state_pos) {
  lm_check_weights(alpha, beta, flags);
  if (n < 0 || (n > 0 && !ids)) throw Error(PF_ERR_INVALID_ARG, "lm_score: bad ids / n");
  const LmView v = lm_view(lm.words.data());
  double g = 0.0;
  int s = v.start;
  for (int p = 0; p < n; ++p) {
    s = lm_step(v, s, ids[p], (double)alpha, (double)beta, true, g);
    if (g_pos) g_pos[p] = g;
    if (state_pos) state_pos[p] = s;
  }
  if ((flags & PF_LM_EOS) && v.eos >= 0) s = lm_step(v, s, v.eos, (double)alpha, (double)beta, false, g);
  if (g_out) *g_out = g;
  if (state_out) *state_out = s;
}

// ------------------------------------------------------------------ ARPA text ---------------
namespace {
std::vector<std::string> split_ws(const std::string& line) {
  std::vector<std::string> out;
  size_t i = 0;
  while (i < line.size()) {
    while (i < line.size() && (line[i] == ' ' || line[i] == '\t' || line[i] == '\r')) ++i;
    size_t j = i;
    while (j < line.size() && line[j] != ' ' && line[j] != '\t' && line[j] != '\r') ++j;
    if (j > i) out.push_back(line.substr(i, j - i));
    i = j;
  }
  return out;
}
[[noreturn]] void arpa_fail(const std::string& path, int64_t line, const std::string& what) {
  throw Error(PF_ERR_INVALID_ARG, "lm_from_arpa: " + path + ":" + std::to_string(line) + ": " + what);
}
float arpa_value(const std::string& text, const std::string& path, int64_t line) {
  char* end = nullptr;
  const double v = std::strtod(text.c_str(), &end);
  if (end == text.c_str() || *end != 0 || !std::isfinite(v)) arpa_fail(path, line, "not a finite number: " + text);
  return (float)(v * 2.302585092994046);            // log10 -> natural log, then narrowed
}
}  // namespace

std::shared_ptr<const LmImage> lm_from_arpa(const std::string& path, const char* const* tokens, int n_tokens, float oov, int64_t* n_dropped) {
  if (n_tokens < 2 || !tokens) throw Error(PF_ERR_INVALID_ARG, "lm_from_arpa: a token table of at least two entries");
  std::unordered_map<std::string, int32_t> id_of;
  std::vector<int32_t> transparent;
  for (int i = 0; i < n_tokens; ++i) {
    if (!tokens[i]) throw Error(PF_ERR_INVALID_ARG, "lm_from_arpa: a null token");
    const std::string s(tokens[i]);
    id_of.emplace(s, i);                             // the first spelling wins, as IndexOf does
    if (s.size() >= 4 && s.compare(0, 2, "<|") == 0 && s.compare(s.size() - 2, 2, "|>") == 0) transparent.push_back(i);
  }
  std::ifstream f(path);
  if (!f) throw Error(PF_ERR_IO, "lm_from_arpa: cannot open " + path);
  std::vector<int64_t> declared, kept;
  std::vector<int32_t> ids;
  std::vector<float> logp, bo;
  std::string line;
  int64_t ln = 0, dropped = 0, in_section = 0;
  int k = 0;                                         // 0: before \data\; -1: the counts; k >= 1: inside \k-grams:
  bool ended = false;
  while (std::getline(f, line)) {
    ++ln;
    const std::vector<std::string> w = split_ws(line);
    if (w.empty()) continue;
    if (ended) arpa_fail(path, ln, "text after \\end\\");
    if (k == 0) {
      if (w.size() == 1 && w[0] == "\\data\\") k = -1;
      continue;                                      // a preamble before \data\ is allowed
    }
    if (w[0][0] == '\\') {
      if (k >= 1 && in_section != declared[(size_t)k - 1])
        arpa_fail(path, ln, std::to_string(in_section) + " " + std::to_string(k) + "-grams, " + std::to_string(declared[(size_t)k - 1]) + " declared");
      if (w.size() == 1 && w[0] == "\\end\\") {
        if ((k == -1 ? 0 : k) != (int)declared.size()) arpa_fail(path, ln, "\\end\\ before every declared section");
        ended = true;
        continue;
      }
      const int want = k == -1 ? 1 : k + 1;
      if (w.size() != 1 || w[0] != "\\" + std::to_string(want) + "-grams:" || want > (int)declared.size())
        arpa_fail(path, ln, "expected \\" + std::to_string(want) + "-grams: or \\end\\");
      k = want;
      in_section = 0;
      kept.push_back(0);
      continue;
    }
    if (k == -1) {                                   // ngram K=COUNT
      const std::string s = w.size() == 2 ? w[1] : "";
      const size_t eq = s.find('=');
      char* end = nullptr;
      if (w[0] != "ngram" || eq == std::string::npos || std::atoi(s.c_str()) != (int)declared.size() + 1)
        arpa_fail(path, ln, "expected ngram " + std::to_string(declared.size() + 1) + "=COUNT");
      const long long c = std::strtoll(s.c_str() + eq + 1, &end, 10);
      if (end == s.c_str() + eq + 1 || *end != 0 || c < 0) arpa_fail(path, ln, "bad count");
      if ((int)declared.size() >= PF_LM_ORDER_MAX) arpa_fail(path, ln, "an order above PF_LM_ORDER_MAX");
      declared.push_back((int64_t)c);
      continue;
    }
    if ((int)w.size() != k + 1 && (int)w.size() != k + 2) arpa_fail(path, ln, "expected a value, " + std::to_string(k) + " words and an optional back-off");
    const float lp = arpa_value(w[0], path, ln);
    const float b = (int)w.size() == k + 2 ? arpa_value(w[(size_t)k + 1], path, ln) : NAN;
    ++in_section;
    bool known = true;
    const size_t at = ids.size();
    for (int p = 0; p < k; ++p) {
      auto it = id_of.find(w[(size_t)p + 1]);
      if (it == id_of.end() || it->second < 1) { known = false; break; }
      ids.push_back(it->second);
    }
    if (!known) { ids.resize(at); ++dropped; continue; }
    logp.push_back(lp);
    bo.push_back(b);
    ++kept.back();
  }
  if (!ended) arpa_fail(path, ln, "truncated: no \\end\\");
  if (declared.empty()) arpa_fail(path, ln, "no ngram counts");
  auto special = [&](const char* s) {
    auto it = id_of.find(s);
    return it != id_of.end() && it->second >= 1 ? it->second : -1;
  };
  int unk = special("<unk>");
  if (unk >= 0) {                                    // an unk the file does not list as a unigram is none
    bool listed = false;
    for (int64_t i = 0; i < kept[0]; ++i) listed = listed || ids[(size_t)i] == unk;
    if (!listed) unk = -1;
  }
  if (n_dropped) *n_dropped = dropped;
  return lm_build((int)declared.size(), kept.data(), ids.data(), logp.data(), bo.data(), n_tokens, special("<s>"), special("</s>"), unk, oov,
                  transparent.data(), (int)transparent.size());
}

}  // namespace pf
