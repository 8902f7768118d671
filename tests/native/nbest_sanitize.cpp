// nbest_sanitize — pf::host_nbest (csrc/hostutil.cpp) as a stand-alone program, built by tests/test_topk_cpu.py with
// AddressSanitizer + UBSan on the host code.
//   usage: nbest_sanitize <cases file>
// The file holds one case after the other as text:  L K n_free N  then n[0..L)  then val[0..L*K) as uint32 bit patterns.
// For every case one line goes to stdout:  got  then per hypothesis its L ranks and the score's uint64 bit pattern; a
// case the enumerator refuses prints "error <code>".  Output buffers are sized exactly, so an overrun is a report.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hostutil.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int L, K, n_free, N, cases = 0;
  while (std::fscanf(f, "%d %d %d %d", &L, &K, &n_free, &N) == 4) {
    std::vector<int32_t> n((size_t)L);
    std::vector<float> val((size_t)L * K);
    for (auto& v : n) if (std::fscanf(f, "%" SCNd32, &v) != 1) return 3;
    for (auto& v : val) {
      uint32_t u;
      if (std::fscanf(f, "%" SCNu32, &u) != 1) return 3;
      std::memcpy(&v, &u, 4);
    }
    std::vector<int32_t> ranks((size_t)(N > 0 ? N : 0) * L);
    std::vector<double> scores((size_t)(N > 0 ? N : 0));
    try {
      const int got = pf::host_nbest(val.data(), n.data(), L, K, n_free, N, ranks.data(), scores.data());
      std::printf("%d", got);
      for (int i = 0; i < got; ++i) {
        for (int l = 0; l < L; ++l) std::printf(" %d", ranks[(size_t)i * L + l]);
        uint64_t u;
        std::memcpy(&u, &scores[(size_t)i], 8);
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
