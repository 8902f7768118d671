// spk.cpp — the speaker labels on the host (spk.h): the loader of the CAM++ model (on pfw.h's reader), the builder of the
// image k_spk.hip reads, the window plan, the clustering and the segment labels.  Uses no device.
#include "spk.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "hostutil.h"
#include "pfw.h"

namespace pf {

namespace {

void bad(const std::string& m) { pfw_bad(kPfwSpkModel, m); }

int64_t add_bytes(std::vector<char>& img, const void* src, size_t n) {
  const int64_t off = round_up((int64_t)img.size(), 256);
  img.resize((size_t)off + n, 0);
  if (n) std::memcpy(img.data() + off, src, n);
  return off;
}

// a convolution's weights [N, cin, taps] as the matrix [N, taps * seg] (column tap * seg + c; seg >= cin, zeros between)
std::vector<float> taps_major(const std::vector<float>& w, int N, int cin, int taps, int seg, int extra = 0) {
  std::vector<float> out((size_t)N * ((size_t)taps * seg + extra), 0.f);
  const size_t K = (size_t)taps * seg + extra;
  for (int n = 0; n < N; ++n)
    for (int c = 0; c < cin; ++c)
      for (int k = 0; k < taps; ++k) out[(size_t)n * K + (size_t)k * seg + c] = w[((size_t)n * cin + c) * taps + k];
  return out;
}

void build_image(SpkModel& m) {
  std::vector<char>& img = m.image;
  img.clear();
  auto T = [&](const std::string& n) -> const std::vector<float>& { return m.tensors.at(n); };
  const int mc = m.m;
  int ci = 0;
  double head_flops = 0;                                   // per input frame: F positions per frame at each convolution
  auto conv = [&](const std::string& name, int cin, int sf, const std::string& shortcut, bool residual, int in, int out, int aux, int F_out,
                  bool to_frames = false) {
    SpkConvDesc& d = m.conv[ci++];
    std::vector<float> w = taps_major(T(name + ".weight"), mc, cin, 9, cin, shortcut.empty() ? 0 : cin);
    std::vector<float> b = T(name + ".bias");
    const int K = 9 * cin + (shortcut.empty() ? 0 : cin);
    if (!shortcut.empty()) {
      const std::vector<float>& ws = T(shortcut + ".weight");
      const std::vector<float>& bs = T(shortcut + ".bias");
      for (int n = 0; n < mc; ++n) {
        for (int c = 0; c < cin; ++c) w[(size_t)n * K + 9 * cin + c] = ws[(size_t)n * cin + c];
        b[(size_t)n] = (float)((double)b[(size_t)n] + (double)bs[(size_t)n]);
      }
    }
    d.g = add_gemm(img, w, &b, mc, K);
    d.cin = cin; d.sf = sf; d.shortcut = shortcut.empty() ? 0 : 1; d.residual = residual ? 1 : 0;
    d.in = in; d.out = out; d.aux = aux; d.to_frames = to_frames ? 1 : 0;
    head_flops += 2.0 * d.g.Npad * d.g.Kpad * F_out;
  };
  int F = m.n_mels;
  conv("head.conv1", 1, 1, "", false, -1, 0, -1, F);
  for (int layer = 1; layer <= 2; ++layer) {
    const std::string p = "head.layer" + std::to_string(layer) + ".";
    F /= 2;
    // the buffer rotation: the layer's input is in a; P, Q are the other two
    const int a = layer == 1 ? 0 : 1, P = layer == 1 ? 1 : 0, Q = 2;
    conv(p + "0.conv1", mc, 2, "", false, a, P, -1, F);
    conv(p + "0.conv2", mc, 1, p + "0.shortcut", false, P, Q, a, F);
    conv(p + "1.conv1", mc, 1, "", false, Q, a, -1, F);
    conv(p + "1.conv2", mc, 1, "", true, a, layer == 1 ? 1 : 0, Q, F);
  }
  F /= 2;
  conv("head.conv2", mc, 2, "", false, 0, -1, -1, F, true);

  m.tdnn = add_gemm(img, taps_major(T("tdnn.weight"), m.init, m.frame_w, 5, m.frame_ld), &T("tdnn.bias"), m.init, 5 * m.frame_ld);
  double tail_flops = 2.0 * m.tdnn.Npad * m.tdnn.Kpad;    // per output frame (two input frames)
  const int bnp = (int)round_up(m.bn, 16);
  for (int b = 0; b < 3; ++b) {
    std::vector<SpkLayerDev> layers;
    for (int l = 0; l < m.blocks[b]; ++l) {
      const std::string p = "block" + std::to_string(b + 1) + "." + std::to_string(l) + ".";
      SpkLayerDev d{};
      d.C = m.C0[b] + l * m.growth;
      d.scale_off = add_floats(img, T(p + "bn1.scale").data(), 1, d.C, d.C);
      d.shift_off = add_floats(img, T(p + "bn1.shift").data(), 1, d.C, d.C);
      d.lin1 = add_gemm(img, T(p + "linear1.weight"), &T(p + "linear1.bias"), m.bn, d.C);
      d.local = add_gemm(img, taps_major(T(p + "local.weight"), m.growth, m.bn, 3, bnp), nullptr, m.growth, 3 * bnp);
      d.cam1 = add_gemm(img, T(p + "cam1.weight"), &T(p + "cam1.bias"), m.bn / 2, m.bn);
      d.cam2 = add_gemm(img, T(p + "cam2.weight"), &T(p + "cam2.bias"), m.growth, m.bn / 2);
      tail_flops += 2.0 * ((double)d.lin1.Npad * d.lin1.Kpad + (double)d.local.Npad * d.local.Kpad);
      layers.push_back(d);
    }
    const std::string p = "transit" + std::to_string(b + 1) + ".";
    m.tr_scale_off[b] = add_floats(img, T(p + "bn.scale").data(), 1, m.C1[b], m.C1[b]);
    m.tr_shift_off[b] = add_floats(img, T(p + "bn.shift").data(), 1, m.C1[b], m.C1[b]);
    m.transit[b] = add_gemm(img, T(p + "weight"), nullptr, m.C1[b] / 2, m.C1[b]);
    tail_flops += 2.0 * m.transit[b].Npad * m.transit[b].Kpad;
    m.layers_off[b] = add_bytes(img, layers.data(), layers.size() * sizeof(SpkLayerDev));
  }
  m.out_scale_off = add_floats(img, T("out_bn.scale").data(), 1, m.c_out, m.c_out);
  m.out_shift_off = add_floats(img, T("out_bn.shift").data(), 1, m.c_out, m.c_out);
  m.dense = add_gemm(img, T("dense.weight"), &T("dense.bias"), m.embedding, 2 * m.c_out);
  m.flops_per_frame = head_flops + tail_flops / 2;
}

std::vector<int> int_list3(const Json& cfg, const char* key) {
  const Json* j = cfg.get(key);
  if (!j || j->type != Json::Arr || j->arr.size() != 3) bad(std::string(key) + " is no list of three integers");
  std::vector<int> out;
  for (const Json& v : j->arr) {
    if (v.type != Json::Num || v.num != (double)(int64_t)v.num || !(v.num >= 1 && v.num <= 1e6)) bad(std::string(key) + " holds a value that is no positive integer");
    out.push_back((int)v.num);
  }
  return out;
}

std::shared_ptr<const SpkModel> parse(const char* data, int64_t nbytes) {
  const PfwFrame fr = pfw_frame(data, nbytes, kPfwSpkModel);
  const PfwIndex ix = pfw_index(data + 16, fr.header_len, fr.data_bytes, kPfwSpkModel);
  const Json* jc = &ix.config;
  if (jc->str_or("kind", "") != "campplus") bad("the container's kind is not \"campplus\"");
  auto dim = [&](const char* k) { return jc->int_or(k, -1, INT32_MIN, INT32_MAX); };
  const int64_t n_mels = dim("n_mels"), mc = dim("m_channels"), I = dim("init_channels"), g = dim("growth"), bn = dim("bn_channels"),
                S = dim("seg_len"), E = dim("embedding");
  if (n_mels < 1 || mc < 1 || I < 1 || g < 1 || bn < 1 || S < 1 || E < 1) bad("a dimension is missing or not positive");
  const std::vector<int> blocks = int_list3(*jc, "blocks"), dil = int_list3(*jc, "dilations");
  bool ok = n_mels % 8 == 0 && n_mels <= kSpkMaxMels && mc % 8 == 0 && mc <= kSpkMaxM && mc * (n_mels / 8) <= kSpkMaxFrameWidth &&
            I <= kSpkMaxInit && bn <= kSpkMaxBn && bn % 2 == 0 && g <= kSpkMaxGrowth && S >= kSpkMinSegLen && E <= kSpkMaxEmbedding;
  auto m = std::make_shared<SpkModel>();
  int64_t C = I;
  for (int b = 0; b < 3 && ok; ++b) {
    ok = blocks[(size_t)b] <= kSpkMaxLayers && dil[(size_t)b] <= kSpkMaxDilation;
    m->blocks[b] = blocks[(size_t)b]; m->dilations[b] = dil[(size_t)b];
    m->C0[b] = (int)C;
    C += (int64_t)blocks[(size_t)b] * g;
    ok = ok && C % 2 == 0 && C <= kSpkMaxWidth;
    m->C1[b] = (int)C;
    m->ldx[b] = (int)round_up(C, 8);
    C /= 2;
  }
  PF_CHECK(ok, PF_ERR_UNSUPPORTED,
           "spk model: a dimension is beyond the limits (n_mels a multiple of 8 and <= 128; m_channels a multiple of 8 and <= 64; "
           "m_channels * n_mels / 8 <= 512; init_channels, bn_channels <= 128, bn_channels even; growth <= 64; blocks <= 64 layers; "
           "dilations <= 8; seg_len >= 4; every concatenated width even and <= 2048; embedding <= 512)");
  m->n_mels = (int)n_mels; m->m = (int)mc; m->init = (int)I; m->growth = (int)g; m->bn = (int)bn; m->seg_len = (int)std::min<int64_t>(S, 1 << 20);
  m->embedding = (int)E;
  m->c_out = (int)C;
  m->ldx[3] = (int)round_up(C, 8);
  m->frame_w = (int)(mc * (n_mels / 8));
  m->frame_ld = (int)round_up(m->frame_w, 16);

  auto take = [&](const std::string& name, std::vector<int64_t> shape) {
    m->tensors[name] = pfw_take(ix, data + fr.data_off, name, shape, kPfwSpkModel);
  };
  auto conv = [&](const std::string& p, int64_t cin, int64_t k) { take(p + ".weight", {mc, cin, k, k}); take(p + ".bias", {mc}); };
  conv("head.conv1", 1, 3);
  for (int layer = 1; layer <= 2; ++layer)
    for (int blk = 0; blk < 2; ++blk) {
      const std::string p = "head.layer" + std::to_string(layer) + "." + std::to_string(blk) + ".";
      conv(p + "conv1", mc, 3);
      conv(p + "conv2", mc, 3);
      if (blk == 0) conv(p + "shortcut", mc, 1);
    }
  conv("head.conv2", mc, 3);
  take("tdnn.weight", {I, m->frame_w, 5});
  take("tdnn.bias", {I});
  for (int b = 0; b < 3; ++b) {
    for (int l = 0; l < m->blocks[b]; ++l) {
      const std::string p = "block" + std::to_string(b + 1) + "." + std::to_string(l) + ".";
      const int64_t Cl = m->C0[b] + (int64_t)l * g;
      take(p + "bn1.scale", {Cl}); take(p + "bn1.shift", {Cl});
      take(p + "linear1.weight", {bn, Cl}); take(p + "linear1.bias", {bn});
      take(p + "local.weight", {g, bn, 3});
      take(p + "cam1.weight", {bn / 2, bn}); take(p + "cam1.bias", {bn / 2});
      take(p + "cam2.weight", {g, bn / 2}); take(p + "cam2.bias", {g});
    }
    const std::string p = "transit" + std::to_string(b + 1) + ".";
    take(p + "bn.scale", {m->C1[b]}); take(p + "bn.shift", {m->C1[b]});
    take(p + "weight", {m->C1[b] / 2, m->C1[b]});
  }
  take("out_bn.scale", {C}); take("out_bn.shift", {C});
  take("dense.weight", {E, 2 * C}); take("dense.bias", {E});
  build_image(*m);
  return m;
}

}  // namespace

const std::vector<float>* SpkModel::tensor(const std::string& name) const {
  auto it = tensors.find(name);
  return it == tensors.end() ? nullptr : &it->second;
}

std::shared_ptr<const SpkModel> spk_model_from_memory(const void* data, int64_t nbytes) {
  try {
    return parse(static_cast<const char*>(data), nbytes);
  } catch (const Error& e) {
    pfw_rethrow(kPfwSpkModel, e);                     // a config field that is no integer in range
  }
}

std::shared_ptr<const SpkModel> spk_model_load(const std::string& path) {
  std::vector<char> file;
  read_binary_file(path, file);
  return spk_model_from_memory(file.data(), (int64_t)file.size());
}

pf_spk_config spk_default() {
  pf_spk_config c{};
  c.struct_size = (int32_t)sizeof(pf_spk_config);
  c.win = 150; c.shift = 75; c.min_frames = 20; c.threshold = 0.5f; c.num_speakers = 0; c.min_cluster = 4;
  return c;
}

void spk_check_config(const pf_spk_config& c) {
  PF_CHECK(c.struct_size == (int32_t)sizeof(pf_spk_config), PF_ERR_INVALID_ARG, "pf_spk_config.struct_size mismatch");
  PF_CHECK(c.win >= 1 && c.win <= PF_SPK_MAX_FRAMES && c.shift >= 1 && c.min_frames >= 1 && c.min_frames <= c.win && c.num_speakers >= 0 &&
               c.min_cluster >= 0 && c.threshold == c.threshold,
           PF_ERR_INVALID_ARG,
           "pf_spk_config: win 1 .. PF_SPK_MAX_FRAMES, shift >= 1, min_frames 1 .. win, num_speakers >= 0, min_cluster >= 0, a threshold that is a number");
}

void host_spk_windows(const int32_t* seg, int32_t n_seg, const pf_spk_config& c, std::vector<int32_t>& win, int32_t* shift_used) {
  int64_t shift = c.shift;
  for (;;) {
    win.clear();
    for (int32_t i = 0; i < n_seg; ++i) {
      const int64_t b = seg[2 * i], e = seg[2 * i + 1], n = e - b;
      if (n < c.min_frames) continue;
      if (n <= c.win) { win.insert(win.end(), {i, (int32_t)b, (int32_t)e}); continue; }
      const int64_t k_end = (n - c.win) / shift;
      for (int64_t k = 0; k <= k_end; ++k) win.insert(win.end(), {i, (int32_t)(b + k * shift), (int32_t)(b + k * shift + c.win)});
      if (b + k_end * shift + c.win != e) win.insert(win.end(), {i, (int32_t)(e - c.win), (int32_t)e});
    }
    if ((int64_t)win.size() / 3 <= PF_SPK_MAX_WINDOWS) break;
    if (shift >= ((int64_t)1 << 30)) { win.resize((size_t)3 * PF_SPK_MAX_WINDOWS); break; }
    shift *= 2;
  }
  if (shift_used) *shift_used = (int32_t)std::min<int64_t>(shift, INT32_MAX);
}

void host_spk_cluster(const float* S, int32_t N, const pf_spk_config& c, int32_t* labels, int32_t* n_speakers) {
  if (n_speakers) *n_speakers = 0;
  if (N <= 0) return;
  const size_t n = (size_t)N;
  std::vector<double> sim(n * n, 0.0);
  for (size_t i = 0; i < n; ++i)
    for (size_t j = i + 1; j < n; ++j) {
      const float v = S[i * n + j];
      sim[i * n + j] = sim[j * n + i] = std::isfinite(v) ? (double)v : -2.0;
    }
  std::vector<int32_t> alive(n), size(n, 1), first(n), owner(n);
  for (size_t i = 0; i < n; ++i) alive[i] = first[i] = owner[i] = (int32_t)i;
  const double threshold = (double)c.threshold;
  // The pair of largest similarity, ties to the smallest first then second index, without rescanning every pair at every merge
  // (N^3 at 8192 windows): every live cluster i keeps its best partner nn[i] among the live j > i (the smallest such j on a
  // tie).  A merge of (i, j), i < j, changes only the similarities with i and removes those with j: row i is rescanned, a row
  // k < i whose partner was i or j is rescanned, any other row k < i takes i where it now beats its partner (or ties it with a
  // smaller index), and a row between i and j whose partner was j is rescanned.
  std::vector<char> live(n, 1);
  std::vector<int32_t> nn(n, -1);
  auto rescan = [&](size_t i) {
    nn[i] = -1;
    double best = -INFINITY;
    for (size_t j = i + 1; j < n; ++j)
      if (live[j] && sim[i * n + j] > best) { best = sim[i * n + j]; nn[i] = (int32_t)j; }
  };
  for (size_t i = 0; i < n; ++i) rescan(i);
  size_t n_alive = n;
  while (n_alive > 1 && !(c.num_speakers > 0 && (int64_t)n_alive <= c.num_speakers)) {
    double best = -INFINITY;
    size_t i = n, j = n;
    for (size_t a = 0; a < n; ++a)
      if (live[a] && nn[a] >= 0 && sim[a * n + (size_t)nn[a]] > best) { best = sim[a * n + (size_t)nn[a]]; i = a; j = (size_t)nn[a]; }
    if (c.num_speakers <= 0 && best < threshold) break;
    for (size_t k = 0; k < n; ++k) {
      if (!live[k] || k == i || k == j) continue;
      const double v = ((double)size[i] * sim[i * n + k] + (double)size[j] * sim[j * n + k]) / (double)(size[i] + size[j]);
      sim[i * n + k] = sim[k * n + i] = v;
    }
    size[i] += size[j];
    for (size_t w = 0; w < n; ++w)
      if (owner[w] == (int32_t)j) owner[w] = (int32_t)i;
    live[j] = 0;
    --n_alive;
    rescan(i);
    for (size_t k = 0; k < j; ++k) {
      if (!live[k] || k == i) continue;
      if (nn[k] == (int32_t)j || (k < i && nn[k] == (int32_t)i)) { rescan(k); continue; }
      if (k < i && nn[k] >= 0) {
        const double cur = sim[k * n + (size_t)nn[k]], v = sim[k * n + i];
        if (v > cur || (v == cur && (int32_t)i < nn[k])) nn[k] = (int32_t)i;
      }
    }
  }
  alive.clear();
  for (size_t i = 0; i < n; ++i)
    if (live[i]) alive.push_back((int32_t)i);
  if (c.num_speakers <= 0) {
    std::vector<int32_t> major, minor;
    for (int32_t cc : alive) (size[(size_t)cc] >= c.min_cluster ? major : minor).push_back(cc);
    if (!major.empty()) {
      for (int32_t cc : minor) {
        int32_t t = major[0];
        for (int32_t k : major)
          if (sim[(size_t)cc * n + (size_t)k] > sim[(size_t)cc * n + (size_t)t]) t = k;      // (ties stay with the smaller index)
        for (size_t w = 0; w < n; ++w)
          if (owner[w] == cc) owner[w] = t;
        first[(size_t)t] = std::min(first[(size_t)t], first[(size_t)cc]);
      }
      alive = major;
    }
  }
  std::sort(alive.begin(), alive.end(), [&](int32_t a, int32_t b) { return first[(size_t)a] < first[(size_t)b]; });
  std::vector<int32_t> label(n, -1);
  for (size_t k = 0; k < alive.size(); ++k) label[(size_t)alive[k]] = (int32_t)k;
  for (size_t w = 0; w < n; ++w) labels[w] = label[(size_t)owner[w]];
  if (n_speakers) *n_speakers = (int32_t)alive.size();
}

void host_spk_segment_labels(const int32_t* seg, int32_t n_seg, const int32_t* win_seg, const int32_t* win_label, int32_t N,
                             int32_t* out) {
  std::vector<int32_t> own((size_t)std::max(n_seg, 0), -1);
  for (int32_t i = 0; i < n_seg; ++i) {
    std::map<int32_t, int32_t> count;
    for (int32_t w = 0; w < N; ++w)
      if (win_seg[w] == i && win_label[w] >= 0) ++count[win_label[w]];
    int32_t best = -1, most = 0;
    for (const auto& kv : count)
      if (kv.second > most) { most = kv.second; best = kv.first; }       // (ascending labels: a tie stays with the lower)
    own[(size_t)i] = best;
  }
  for (int32_t i = 0; i < n_seg; ++i) {
    out[i] = own[(size_t)i];
    if (out[i] >= 0) continue;
    int64_t best_gap = INT64_MAX;
    for (int32_t j = 0; j < n_seg; ++j) {
      if (own[(size_t)j] < 0) continue;
      const int64_t gap = j < i ? (int64_t)seg[2 * i] - seg[2 * j + 1] : (int64_t)seg[2 * j] - seg[2 * i + 1];
      if (gap < best_gap) { best_gap = gap; out[i] = own[(size_t)j]; }
    }
  }
}

void host_spk_centroids(const float* emb, const int32_t* labels, int32_t N, int32_t E, int32_t K, float* out) {
  std::vector<double> acc((size_t)K * E, 0.0);
  std::vector<int64_t> cnt((size_t)K, 0);
  for (int32_t w = 0; w < N; ++w) {
    const int32_t k = labels[w];
    if (k < 0 || k >= K) continue;
    double n2 = 0;
    for (int32_t e = 0; e < E; ++e) n2 += (double)emb[(size_t)w * E + e] * emb[(size_t)w * E + e];
    ++cnt[(size_t)k];
    if (!(n2 > 0)) continue;
    const double inv = 1.0 / std::sqrt(n2);
    for (int32_t e = 0; e < E; ++e) acc[(size_t)k * E + e] += (double)emb[(size_t)w * E + e] * inv;
  }
  for (int32_t k = 0; k < K; ++k) {
    double n2 = 0;
    for (int32_t e = 0; e < E; ++e) {
      if (cnt[(size_t)k]) acc[(size_t)k * E + e] /= (double)cnt[(size_t)k];
      n2 += acc[(size_t)k * E + e] * acc[(size_t)k * E + e];
    }
    const double inv = n2 > 0 ? 1.0 / std::sqrt(n2) : 0.0;
    for (int32_t e = 0; e < E; ++e) out[(size_t)k * E + e] = (float)(acc[(size_t)k * E + e] * inv);
  }
}

}  // namespace pf
