// vadnet_sanitize — the FSMN-VAD container loader and float64 twins (csrc/vadnet.cpp) as a stand-alone program, built with
// AddressSanitizer + UBSan on the host code (tests/test_vadnet_cpu.py): every file named on the command line is loaded; a
// refusal prints its status code, a model prints its dimensions and the levels of a fixed input.
//   usage: vadnet_sanitize <n_mels> <file> [<file> ...]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hostutil.h"
#include "vadnet.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int n_mels = std::atoi(argv[1]);
  for (int i = 2; i < argc; ++i) {
    try {
      std::shared_ptr<const pf::VadModel> m = pf::vad_model_load(argv[i]);
      const int T = 37;
      std::vector<float> rows((size_t)T * n_mels);
      for (size_t k = 0; k < rows.size(); ++k) rows[k] = (float)((((uint32_t)k * 2654435761u) >> 24) % 13u) * 0.5f - 4.f;
      std::vector<int32_t> lev((size_t)T);
      std::vector<double> z((size_t)T * m->output_dim);
      pf::host_vad_model_logits(*m, rows.data(), T, n_mels, z.data());
      pf::host_vad_model_levels(*m, rows.data(), T, n_mels, lev.data());
      std::printf("ok %d %d %d %zu", m->input_dim, m->output_dim, m->n_layers, m->image.size());
      for (int32_t e : lev) std::printf(" %d", e);
      std::printf("\n");
    } catch (const pf::Error& e) {
      std::printf("refused %d\n", e.code);
    }
  }
  return 0;
}
