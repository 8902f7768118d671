// pfw.cpp — the PFW1 container reader (pfw.h) and the builders of a row-tile weight image with the float64 twin of one of its
// products (tile_image.h).  Uses no device.
#include "pfw.h"

#include <cmath>
#include <cstring>

#include "tile_image.h"

namespace pf {

namespace {
constexpr int64_t kAlignBytes = 256;
constexpr int64_t kMaxDim = 2147483647, kMaxNumel = (int64_t)1 << 40;
}  // namespace

void pfw_bad(const PfwPolicy& p, const std::string& m) { throw Error(p.code, p.prefix + m); }

void pfw_rethrow(const PfwPolicy& p, const Error& e) {
  if (e.code == p.code || e.code == PF_ERR_UNSUPPORTED) throw e;
  pfw_bad(p, e.what());
}

PfwFrame pfw_frame(const char* first16, int64_t nbytes, const PfwPolicy& p) {
  if (!first16 || nbytes < 16) pfw_bad(p, "image too small");
  if (std::memcmp(first16, "PFW1", 4) != 0) pfw_bad(p, "bad magic (expected a PFW1 container)");
  uint64_t hlen = 0;
  std::memcpy(&hlen, first16 + 8, 8);
  if (hlen > (uint64_t)nbytes - 16u) pfw_bad(p, "truncated header");                // unsigned: a huge hlen cannot wrap
  PfwFrame f;
  f.header_len = (int64_t)hlen;
  f.data_off = round_up(16 + f.header_len, kAlignBytes);
  f.data_bytes = nbytes - f.data_off;
  if (f.data_bytes < 0) pfw_bad(p, "truncated data section");
  return f;
}

PfwIndex pfw_index(const char* header, int64_t header_len, int64_t data_bytes, const PfwPolicy& p) {
  try {
    PfwIndex ix;
    const Json j = JsonParser(header, (size_t)header_len).parse();
    const Json* jc = j.get("config");
    const Json* jt = j.get("tensors");
    if (!jc || jc->type != Json::Obj || !jt || jt->type != Json::Arr) pfw_bad(p, "the header lacks config / tensors");
    ix.config = *jc;
    for (const Json& t : jt->arr) {
      if (t.type != Json::Obj) pfw_bad(p, "a tensor entry is no object");
      const std::string name = t.str_or("name", "");
      const std::string dt = t.str_or("dtype", "f32");
      if (dt != "f32" && !(p.allow_u8 && dt == "u8"))
        pfw_bad(p, "tensor '" + name + "' has dtype '" + dt + (p.allow_u8 ? "' (f32 and u8 are supported)" : "' (f32 is supported)"));
      PfwEntry e;
      e.u8 = dt == "u8";
      e.offset = t.int_or("offset", -1);
      e.nbytes = t.int_or("nbytes", -1);
      if (e.offset < 0 || e.nbytes < 0 || e.offset > data_bytes || e.nbytes > data_bytes - e.offset || e.offset % p.offset_align != 0)
        pfw_bad(p, "the extent of tensor '" + name + "' lies outside the file or is misaligned");
      const Json* sh = t.get("shape");
      if (!sh || sh->type != Json::Arr) pfw_bad(p, "tensor '" + name + "' has no shape");
      e.numel = 1;
      for (const Json& d : sh->arr) {
        if (d.type != Json::Num || !(d.num >= 1.0 && d.num <= (double)kMaxDim) || d.num != (double)(int64_t)d.num)
          pfw_bad(p, "bad dimension in the shape of '" + name + "'");
        const int64_t n = (int64_t)d.num;
        if (e.numel > kMaxNumel / n) pfw_bad(p, "the shape of '" + name + "' overflows");       // before the product is formed
        e.numel *= n;
        e.shape.push_back(n);
      }
      if (e.numel * (e.u8 ? 1 : 4) != e.nbytes) pfw_bad(p, "shape / nbytes mismatch for '" + name + "'");
      ix.tensors[name] = std::move(e);
    }
    return ix;
  } catch (const Error& e) {
    pfw_rethrow(p, e);                                  // a header that is no JSON, a number out of range
  }
}

std::vector<float> pfw_take(const PfwIndex& ix, const char* data, const std::string& name, const std::vector<int64_t>& shape,
                            const PfwPolicy& p) {
  auto it = ix.tensors.find(name);
  if (it == ix.tensors.end()) pfw_bad(p, "tensor '" + name + "' is missing");
  if (it->second.u8) pfw_bad(p, "tensor '" + name + "' is not f32");
  if (it->second.shape != shape) pfw_bad(p, "tensor '" + name + "' has the wrong shape");
  std::vector<float> v((size_t)it->second.numel);
  std::memcpy(v.data(), data + it->second.offset, v.size() * 4);
  for (float x : v)
    if (!std::isfinite(x)) pfw_bad(p, "tensor '" + name + "' holds a value that is not finite");
  return v;
}

// ---- tile_image.h
TileGemm add_gemm(std::vector<char>& img, const std::vector<float>& w, const std::vector<float>* bias, int N, int K) {
  TileGemm g;
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

}  // namespace pf
