// spk_sanitize — the speaker model's container loader and the host half of the speaker labels (csrc/spk.cpp) as a stand-alone
// program, built with AddressSanitizer + UBSan on the host code (tests/test_spk_cpu.py): every file named on the command line
// is loaded; a refusal prints its status code, a model prints its dimensions and the size of its device image.  Then the window
// plan, the clustering, the segment labels and the centroids run once on fixed inputs and print their results.
//   usage: spk_sanitize <file> [<file> ...]
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "hostutil.h"
#include "spk.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  for (int i = 1; i < argc; ++i) {
    try {
      std::shared_ptr<const pf::SpkModel> m = pf::spk_model_load(argv[i]);
      std::printf("ok %d %d %d %d %d %d %d %zu\n", m->n_mels, m->m, m->init, m->growth, m->bn, m->embedding, m->c_out, m->image.size());
    } catch (const pf::Error& e) {
      std::printf("refused %d\n", e.code);
    }
  }
  const pf_spk_config c = pf::spk_default();
  const int32_t seg[] = {0, 19, 30, 50, 100, 250, 300, 451, 500, 724, 800, 1025, 2000, 2010};
  std::vector<int32_t> win;
  int32_t shift = 0;
  pf::host_spk_windows(seg, 7, c, win, &shift);
  const int N = (int)(win.size() / 3);
  std::vector<float> S((size_t)N * N), emb((size_t)N * 3);
  for (int i = 0; i < N; ++i) {
    for (int j = 0; j < N; ++j) S[(size_t)i * N + j] = (i % 2 == j % 2) ? 0.9f - 0.01f * (float)((i + j) % 5) : 0.1f;
    emb[(size_t)i * 3] = (float)(i % 2); emb[(size_t)i * 3 + 1] = (float)(1 - i % 2); emb[(size_t)i * 3 + 2] = 0.1f * (float)i;
  }
  std::vector<int32_t> labels((size_t)N), wseg((size_t)N), out(7);
  int32_t K = 0;
  pf_spk_config c2 = c;
  c2.min_cluster = 2;
  pf::host_spk_cluster(S.data(), N, c2, labels.data(), &K);
  for (int i = 0; i < N; ++i) wseg[(size_t)i] = win[3 * (size_t)i];
  pf::host_spk_segment_labels(seg, 7, wseg.data(), labels.data(), N, out.data());
  std::vector<float> cent((size_t)K * 3);
  pf::host_spk_centroids(emb.data(), labels.data(), N, 3, K, cent.data());
  std::printf("plan %d %d %d |", N, (int)shift, (int)K);
  for (int32_t l : labels) std::printf(" %d", l);
  std::printf(" |");
  for (int32_t l : out) std::printf(" %d", l);
  std::printf("\n");
  pf::host_spk_cluster(nullptr, 0, c, nullptr, &K);
  return 0;
}
