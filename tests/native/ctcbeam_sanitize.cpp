// ctcbeam_sanitize — pf::host_ctc_beam (csrc/hostutil.cpp) as a stand-alone program, built by tests/test_ctcbeam_cpu.py
// with AddressSanitizer + UBSan on the host code.
//   usage: ctcbeam_sanitize <cases file>
// The file holds one case after the other as text:  T K W N cap  then blank_lp[0..T) as uint32 bit patterns, ids[0..T*K),
// val[0..T*K) as uint32 bit patterns, n[0..T).
// For every case one line goes to stdout:  n_hyp  then per hypothesis its length, its ids and the score's uint64 bit
// pattern; a case the search refuses prints "error <code>".  Buffers are sized exactly, so an overrun is a report.
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

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int T, K, W, N, cap, cases = 0;
  while (std::fscanf(f, "%d %d %d %d %d", &T, &K, &W, &N, &cap) == 5) {
    std::vector<float> lb((size_t)T), val((size_t)T * K);
    std::vector<int64_t> ids((size_t)T * K);
    std::vector<int32_t> n((size_t)T);
    if (!read_f32(f, lb)) return 3;
    for (auto& v : ids) if (std::fscanf(f, "%" SCNd64, &v) != 1) return 3;
    if (!read_f32(f, val)) return 3;
    for (auto& v : n) if (std::fscanf(f, "%" SCNd32, &v) != 1) return 3;
    const size_t Nn = (size_t)(N > 0 ? N : 0);
    std::vector<int64_t> out_ids(Nn * (size_t)(cap > 0 ? cap : 0));
    std::vector<int32_t> out_len(Nn);
    std::vector<double> out_score(Nn);
    try {
      const int got = pf::host_ctc_beam(lb.data(), 1, ids.data(), val.data(), n.data(), T, K, 0, W, N, out_ids.data(), out_len.data(),
                                        out_score.data(), cap);
      std::printf("%d", got);
      for (int i = 0; i < got; ++i) {
        std::printf(" %d", out_len[(size_t)i]);
        for (int p = 0; p < out_len[(size_t)i]; ++p) std::printf(" %" PRId64, out_ids[(size_t)i * cap + p]);
        uint64_t u;
        std::memcpy(&u, &out_score[(size_t)i], 8);
        std::printf(" %" PRIu64, u);
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
