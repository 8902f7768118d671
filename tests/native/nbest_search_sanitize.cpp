// nbest_search_sanitize — pf::host_nbest_search (csrc/hostutil.cpp) with pf::lm_build (csrc/lm.cpp) as a stand-alone program, built
// by tests/test_nbest_search_cpu.py with AddressSanitizer + UBSan on the host code.
//   usage: nbest_search_sanitize <commands file>
// The file holds one command after the other as whitespace-separated text; a float is its uint32 bit pattern:
//   M order V bos eos unk oov n_transparent ids..  count[0..order)  then per n-gram (1-grams first): its ids, logp, back-off
//       builds the model the commands that follow may use        -> "M order states arcs bytes"
//   N L K token_num W N H boost alpha beta flags use_lm  ids[L*K] val[L*K] n[L] hot-word lengths[H] and their ids
//                                                                -> "N n_hyp" then for ALL N slots: ranks[L] matched score loglik lm
// A command that is refused prints "error <code>".  Buffers are sized exactly, so an overrun is a report.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "hostutil.h"
#include "lm.h"

static bool rd_f32(FILE* f, float& v) {
  uint32_t u;
  if (std::fscanf(f, "%" SCNu32, &u) != 1) return false;
  std::memcpy(&v, &u, 4);
  return true;
}
static bool rd_f32s(FILE* f, std::vector<float>& out) {
  for (auto& v : out) if (!rd_f32(f, v)) return false;
  return true;
}
static bool rd_i32s(FILE* f, std::vector<int32_t>& out) {
  for (auto& v : out) if (std::fscanf(f, "%" SCNd32, &v) != 1) return false;
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
  std::shared_ptr<const pf::LmImage> lm;
  char cmd[8];
  int done = 0;
  while (std::fscanf(f, "%7s", cmd) == 1) {
    try {
      if (cmd[0] == 'M') {
        int order, V, bos, eos, unk, ntr;
        float oov;
        if (std::fscanf(f, "%d %d %d %d %d", &order, &V, &bos, &eos, &unk) != 5 || !rd_f32(f, oov) || std::fscanf(f, "%d", &ntr) != 1) return 3;
        std::vector<int32_t> tr((size_t)ntr);
        if (!rd_i32s(f, tr)) return 3;
        std::vector<int64_t> cnt((size_t)(order > 0 ? order : 0));
        size_t total = 0, total_ids = 0;
        for (size_t k = 0; k < cnt.size(); ++k) {
          if (std::fscanf(f, "%" SCNd64, &cnt[k]) != 1) return 3;
          total += (size_t)cnt[k];
          total_ids += (size_t)cnt[k] * (k + 1);
        }
        std::vector<int32_t> ids(total_ids);
        std::vector<float> lp(total), bo(total);
        size_t at = 0, x = 0;
        for (size_t k = 0; k < cnt.size(); ++k)
          for (int64_t i = 0; i < cnt[k]; ++i, ++x) {
            for (size_t p = 0; p <= k; ++p) if (std::fscanf(f, "%" SCNd32, &ids[at++]) != 1) return 3;
            if (!rd_f32(f, lp[x]) || !rd_f32(f, bo[x])) return 3;
          }
        lm.reset();
        lm = pf::lm_build(order, cnt.data(), ids.data(), lp.data(), bo.data(), V, bos, eos, unk, oov, tr.data(), ntr);
        std::printf("M %d %" PRId64 " %" PRId64 " %zu\n", lm->order, lm->states, lm->arcs, lm->bytes());
      } else if (cmd[0] == 'N') {
        int L, K, tn, W, N, H, flags, use_lm;
        float boost, alpha, beta;
        if (std::fscanf(f, "%d %d %d %d %d %d", &L, &K, &tn, &W, &N, &H) != 6 || !rd_f32(f, boost) || !rd_f32(f, alpha) || !rd_f32(f, beta) ||
            std::fscanf(f, "%d %d", &flags, &use_lm) != 2)
          return 3;
        const size_t cells = (size_t)(L > 0 ? L : 0) * (size_t)(K > 0 ? K : 0);
        std::vector<float> val(cells);
        std::vector<int64_t> ids(cells);
        std::vector<int32_t> n((size_t)(L > 0 ? L : 0)), hl((size_t)H);
        for (auto& v : ids) if (std::fscanf(f, "%" SCNd64, &v) != 1) return 3;
        if (!rd_f32s(f, val) || !rd_i32s(f, n) || !rd_i32s(f, hl)) return 3;
        size_t total = 0;
        for (auto v : hl) total += (size_t)(v > 0 ? v : 0);
        std::vector<int32_t> hi(total);
        if (!rd_i32s(f, hi)) return 3;
        const size_t Nn = (size_t)(N > 0 ? N : 0);
        std::vector<int32_t> out_ranks(Nn * n.size()), out_m(Nn);
        std::vector<double> out_score(Nn), out_ll(Nn), out_lm(Nn);
        if (use_lm && !lm) return 4;
        const int got = pf::host_nbest_search(ids.data(), val.data(), n.data(), L, K, tn, W, N, hi.data(), hl.data(), H, boost,
                                              use_lm ? lm.get() : nullptr, alpha, beta, flags, out_ranks.data(), out_score.data(),
                                              out_ll.data(), out_lm.data(), out_m.data());
        std::printf("N %d", got);
        for (size_t i = 0; i < Nn; ++i) {
          for (size_t l = 0; l < n.size(); ++l) std::printf(" %d", out_ranks[i * n.size() + l]);
          std::printf(" %d %" PRIu64 " %" PRIu64 " %" PRIu64, out_m[i], bits(out_score[i]), bits(out_ll[i]), bits(out_lm[i]));
        }
        std::printf("\n");
      } else {
        return 5;
      }
    } catch (const pf::Error& e) {
      std::printf("error %d\n", e.code);
    }
    ++done;
  }
  std::fclose(f);
  std::printf("ok %d\n", done);
  return 0;
}
