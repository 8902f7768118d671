// ctcbeam_bias_sanitize — pf::build_hotword_graph and pf::host_ctc_beam_hot (csrc/hostutil.cpp) as a stand-alone program,
// built by tests/test_ctcbeam_bias_cpu.py with AddressSanitizer + UBSan on the host code.
//   usage: ctcbeam_bias_sanitize <cases file>
// The file holds one case after the other as text:  T K W N cap H boost(uint32 bit pattern)  then blank_lp[0..T) as uint32 bit
// patterns, ids[0..T*K), val[0..T*K) as uint32 bit patterns, n[0..T), the H hot-word lengths and their ids.
// For every case one line goes to stdout:  S A n_hyp  then per hypothesis its length, its ids, matched and the uint64 bit
// patterns of score and loglik_sum; a case that is refused prints "error <code>".  Buffers are sized exactly, so an overrun is
// a report.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hostutil.h"

static bool read_f32(FILE* f, std::vector<float>& out) {
  for (auto& v : out) {
    uint32_t u;
    if (std::fscanf(f, "%" SCNu32, &u) != 1) return false;
    std::memcpy(&v, &u, 4);
  }
  return true;
}

static uint64_t bits(double d) {
  uint64_t u;
  std::memcpy(&u, &d, 8);
  return u;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int T, K, W, N, cap, H, cases = 0;
  uint32_t boost_bits;
  while (std::fscanf(f, "%d %d %d %d %d %d %" SCNu32, &T, &K, &W, &N, &cap, &H, &boost_bits) == 7) {
    float boost;
    std::memcpy(&boost, &boost_bits, 4);
    std::vector<float> lb((size_t)T), val((size_t)T * K);
    std::vector<int64_t> ids((size_t)T * K);
    std::vector<int32_t> n((size_t)T), hl((size_t)H);
    if (!read_f32(f, lb)) return 3;
    for (auto& v : ids) if (std::fscanf(f, "%" SCNd64, &v) != 1) return 3;
    if (!read_f32(f, val)) return 3;
    for (auto& v : n) if (std::fscanf(f, "%" SCNd32, &v) != 1) return 3;
    size_t total = 0;
    for (auto& v : hl) { if (std::fscanf(f, "%" SCNd32, &v) != 1) return 3; total += (size_t)(v > 0 ? v : 0); }
    std::vector<int32_t> hi(total);
    for (auto& v : hi) if (std::fscanf(f, "%" SCNd32, &v) != 1) return 3;
    const size_t Nn = (size_t)(N > 0 ? N : 0);
    std::vector<int64_t> out_ids(Nn * (size_t)(cap > 0 ? cap : 0));
    std::vector<int32_t> out_len(Nn), out_m(Nn);
    std::vector<double> out_score(Nn), out_ll(Nn);
    try {
      pf::HotwordGraph g;
      pf::build_hotword_graph(hi.data(), hl.data(), H, pf::hotword_vocab_bound(hi.data(), hl.data(), H), g);
      const int got = pf::host_ctc_beam_hot(lb.data(), 1, ids.data(), val.data(), n.data(), T, K, 0, W, N, hi.data(), hl.data(), H, boost,
                                            out_ids.data(), out_len.data(), out_score.data(), out_m.data(), out_ll.data(), cap);
      std::printf("%d %d %d", g.S, g.A, got);
      for (int i = 0; i < got; ++i) {
        std::printf(" %d", out_len[(size_t)i]);
        for (int p = 0; p < out_len[(size_t)i]; ++p) std::printf(" %" PRId64, out_ids[(size_t)i * cap + p]);
        std::printf(" %d %" PRIu64 " %" PRIu64, out_m[(size_t)i], bits(out_score[(size_t)i]), bits(out_ll[(size_t)i]));
      }
      std::printf("\n");
    } catch (const pf::Error& e) {
      std::printf("error %d\n", e.code);
    }
    ++cases;
  }
  std::fclose(f);
  std::printf("ok %d\n", cases);
  return 0;
}
