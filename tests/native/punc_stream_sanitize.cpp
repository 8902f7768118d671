// punc_stream_sanitize — the loader's two streaming header keys and the float64 stream twin (csrc/punc.cpp) as a stand-alone
// program, built with AddressSanitizer + UBSan on the host code (tests/test_punc_stream_cpu.py): every file named on the command
// line is loaded; a refusal prints its status code, a causal model runs a fixed stream of 300 ids through
// host_punc_stream_step in calls of 0, 1, 7 and 64 words with max_context 50 and a final flush and prints marks, flags and the
// flush mark, a model that is not causal prints the status the stream twin refuses it with.
//   usage: punc_stream_sanitize <file> [<file> ...]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "hostutil.h"
#include "punc.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  for (int i = 1; i < argc; ++i) {
    try {
      std::shared_ptr<const pf::PuncModel> m = pf::punc_model_load(argv[i]);
      std::vector<char> state((size_t)pf::host_punc_stream_state_bytes(*m), 0);
      std::vector<int32_t> ids(300), marks(300), flags(300);
      for (int k = 0; k < 300; ++k) ids[(size_t)k] = (int32_t)((k * 37 + 11) % m->vocab);
      const int calls[4] = {0, 1, 7, 64};
      int at = 0, fm = -2;
      try {
        for (int c = 0; at < 300; ++c) {
          const int n = std::min(calls[c % 4], 300 - at);
          pf::host_punc_stream_step(*m, state.data(), ids.data() + at, n, at + n == 300, 50, 0, marks.data() + at, flags.data() + at,
                                    nullptr, &fm);
          at += n;
        }
      } catch (const pf::Error& e) {
        std::printf("model %d stream refused %d\n", m->causal, e.code);
        continue;
      }
      std::printf("ok %d %d %d|", m->causal, m->left, fm);
      for (int32_t e : marks) std::printf(" %d", e);
      std::printf("|");
      for (int32_t e : flags) std::printf(" %d", e);
      std::printf("\n");
    } catch (const pf::Error& e) {
      std::printf("refused %d\n", e.code);
    }
  }
  return 0;
}
