// nnlm_sanitize — the Transformer LM container loader, the float64 twin and the fusion (csrc/nnlm.cpp) as a stand-alone program,
// built with AddressSanitizer + UBSan on the host code (tests/test_nnlm_cpu.py): every file named on the command line is loaded;
// a refusal prints its status code, a model prints its dimensions, the logp of a fixed hypothesis and a fused order.
//   usage: nnlm_sanitize <file> [<file> ...]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "hostutil.h"
#include "nnlm.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  for (int i = 1; i < argc; ++i) {
    try {
      std::shared_ptr<const pf::NnlmModel> m = pf::nnlm_model_load(argv[i]);
      std::vector<int32_t> ids;
      for (int t = 0; t < 9; ++t) ids.push_back((7 * t + 3) % m->vocab);
      std::vector<double> logp(ids.size() + 1);
      pf::host_nnlm_logp(*m, ids.data(), (int)ids.size(), logp.data());
      pf::host_nnlm_logp(*m, ids.data(), 0, logp.data() + ids.size());            // the empty hypothesis: the eos row alone
      const double base[4] = {1.0, 2.0, 2.0, -1.0}, lm[4] = {0.0, -2.0, -2.0, 8.0};
      const int32_t n[4] = {1, 2, 2, 3};
      double score[4];
      int32_t order[4];
      pf::host_nnlm_fuse(base, lm, n, 4, 0.5, 0.0, score, order);
      std::printf("ok %d %d %d %zu %d%d%d%d|", m->vocab, m->embed_dim, m->n_layers, m->image.size(), order[0], order[1], order[2], order[3]);
      for (double v : logp) std::printf(" %.17g", v);
      std::printf("\n");
    } catch (const pf::Error& e) {
      std::printf("refused %d\n", e.code);
    }
  }
  return 0;
}
