// ctcalign_sanitize — pf::host_ctc_align (csrc/hostutil.cpp) as a stand-alone program, built by tests/test_ctcalign_cpu.py
// with AddressSanitizer + UBSan on the host code.
//   usage: ctcalign_sanitize <cases file>
// The file holds one case after the other as text:  T V ld U  then lp[0..T*ld) as uint32 bit patterns and y[0..U).
// For every case one line goes to stdout:  ok, the path score's uint32 and the log-likelihood's uint64 bit patterns, then per
// token first, last and the token score's uint32 bit pattern; a case the twin refuses prints "error <code>".  Buffers are
// sized exactly, so an overrun is a report.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hostutil.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int T, V, ld, U, cases = 0;
  while (std::fscanf(f, "%d %d %d %d", &T, &V, &ld, &U) == 4) {
    std::vector<float> lp((size_t)(T > 0 ? T : 0) * (size_t)(ld > 0 ? ld : 0));
    std::vector<int64_t> y((size_t)(U > 0 ? U : 0));
    for (auto& v : lp) {
      uint32_t u;
      if (std::fscanf(f, "%" SCNu32, &u) != 1) return 3;
      std::memcpy(&v, &u, 4);
    }
    for (auto& v : y) if (std::fscanf(f, "%" SCNd64, &v) != 1) return 3;
    std::vector<int32_t> first(y.size()), last(y.size());
    std::vector<float> tok(y.size());
    float path = 0.f;
    double ll = 0.0;
    try {
      const int ok = pf::host_ctc_align(lp.data(), ld, T, V, y.data(), U, &path, &ll, first.data(), last.data(), tok.data());
      uint32_t p32;
      uint64_t l64;
      std::memcpy(&p32, &path, 4);
      std::memcpy(&l64, &ll, 8);
      std::printf("%d %" PRIu32 " %" PRIu64, ok, p32, l64);
      for (size_t u = 0; u < y.size(); ++u) {
        uint32_t t32;
        std::memcpy(&t32, &tok[u], 4);
        std::printf(" %d %d %" PRIu32, first[u], last[u], t32);
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
