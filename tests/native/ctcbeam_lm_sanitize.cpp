// ctcbeam_lm_sanitize — pf::lm_build, pf::lm_from_arpa, pf::lm_score (csrc/lm.cpp) and pf::host_ctc_beam_lm (csrc/hostutil.cpp)
// as a stand-alone program, built by tests/test_ctcbeam_lm_cpu.py with AddressSanitizer + UBSan on the host code.
//   usage: ctcbeam_lm_sanitize <commands file>
// The file holds one command after the other as whitespace-separated text; a float is its uint32 bit pattern:
//   M order V bos eos unk oov n_transparent ids..  count[0..order)  then per n-gram (1-grams first): its ids, logp, back-off
//       builds the model the commands that follow use            -> "M order states arcs bytes"
//   A arpa_path tokens_path oov     (tokens_path: one token per line)  -> "A order states arcs bytes dropped"
//   S alpha beta flags n ids..                                   -> "S g state" then per position "g state" (g: uint64 bits)
//   B T K W N cap H boost alpha beta flags  blank_lp[T] ids[T*K] val[T*K] n[T] hot-word lengths[H] and their ids
//                                                                -> "B n_hyp" then per hypothesis len ids.. matched score loglik lm
// A command that is refused prints "error <code>".  Buffers are sized exactly, so an overrun is a report.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
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
      } else if (cmd[0] == 'A') {
        char path[1024], tpath[1024];
        float oov;
        if (std::fscanf(f, "%1023s %1023s", path, tpath) != 2 || !rd_f32(f, oov)) return 3;
        std::vector<std::string> toks;
        std::ifstream tf(tpath);
        for (std::string line; std::getline(tf, line);) toks.push_back(line);
        std::vector<const char*> ptr;
        for (auto& t : toks) ptr.push_back(t.c_str());
        int64_t dropped = -1;
        lm.reset();
        lm = pf::lm_from_arpa(path, ptr.data(), (int)ptr.size(), oov, &dropped);
        std::printf("A %d %" PRId64 " %" PRId64 " %zu %" PRId64 "\n", lm->order, lm->states, lm->arcs, lm->bytes(), dropped);
      } else if (cmd[0] == 'S') {
        float alpha, beta;
        int flags, n;
        if (!rd_f32(f, alpha) || !rd_f32(f, beta) || std::fscanf(f, "%d %d", &flags, &n) != 2) return 3;
        std::vector<int32_t> ids((size_t)(n > 0 ? n : 0)), st(ids.size());
        if (!rd_i32s(f, ids)) return 3;
        std::vector<double> gp(ids.size());
        double g = 0;
        int32_t s = 0;
        if (!lm) return 4;
        pf::lm_score(*lm, ids.data(), n, alpha, beta, flags, &g, &s, gp.data(), st.data());
        std::printf("S %" PRIu64 " %d", bits(g), s);
        for (size_t p = 0; p < ids.size(); ++p) std::printf(" %" PRIu64 " %d", bits(gp[p]), st[p]);
        std::printf("\n");
      } else if (cmd[0] == 'B') {
        int T, K, W, N, cap, H, flags;
        float boost, alpha, beta;
        if (std::fscanf(f, "%d %d %d %d %d %d", &T, &K, &W, &N, &cap, &H) != 6 || !rd_f32(f, boost) || !rd_f32(f, alpha) || !rd_f32(f, beta) ||
            std::fscanf(f, "%d", &flags) != 1)
          return 3;
        std::vector<float> lb((size_t)T), val((size_t)T * K);
        std::vector<int64_t> ids((size_t)T * K);
        std::vector<int32_t> n((size_t)T), hl((size_t)H);
        if (!rd_f32s(f, lb)) return 3;
        for (auto& v : ids) if (std::fscanf(f, "%" SCNd64, &v) != 1) return 3;
        if (!rd_f32s(f, val) || !rd_i32s(f, n) || !rd_i32s(f, hl)) return 3;
        size_t total = 0;
        for (auto v : hl) total += (size_t)(v > 0 ? v : 0);
        std::vector<int32_t> hi(total);
        if (!rd_i32s(f, hi)) return 3;
        const size_t Nn = (size_t)(N > 0 ? N : 0);
        std::vector<int64_t> out_ids(Nn * (size_t)(cap > 0 ? cap : 0));
        std::vector<int32_t> out_len(Nn), out_m(Nn);
        std::vector<double> out_score(Nn), out_ll(Nn), out_lm(Nn);
        if (!lm) return 4;
        const int got = pf::host_ctc_beam_lm(lb.data(), 1, ids.data(), val.data(), n.data(), T, K, 0, W, N, hi.data(), hl.data(), H, boost,
                                             out_ids.data(), out_len.data(), out_score.data(), out_m.data(), out_ll.data(), cap, *lm, alpha,
                                             beta, flags, out_lm.data());
        std::printf("B %d", got);
        for (int i = 0; i < got; ++i) {
          std::printf(" %d", out_len[(size_t)i]);
          for (int p = 0; p < out_len[(size_t)i]; ++p) std::printf(" %" PRId64, out_ids[(size_t)i * cap + p]);
          std::printf(" %d %" PRIu64 " %" PRIu64 " %" PRIu64, out_m[(size_t)i], bits(out_score[(size_t)i]), bits(out_ll[(size_t)i]),
                      bits(out_lm[(size_t)i]));
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
