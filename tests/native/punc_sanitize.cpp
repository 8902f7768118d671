// punc_sanitize — the punctuation container loader and float64 twins (csrc/punc.cpp) as a stand-alone program, built with
// AddressSanitizer + UBSan on the host code (tests/test_punc_cpu.py): every file named on the command line is loaded; a
// refusal prints its status code, a model prints its dimensions, the punctuated form of a fixed text and its punc_ids.
//   usage: punc_sanitize <file> [<file> ...]
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "hostutil.h"
#include "punc.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string text = "\xE4\xB8\x81\xE4\xB8\x83 wb \xE4\xB8\x88\xE4\xB8\x89  hello \xF0\x9F\x98\x80\xE4\xB8\x8A\xE4\xB8\x8B wc wd\t\xE4\xB8\x81";
  for (int i = 1; i < argc; ++i) {
    try {
      std::shared_ptr<const pf::PuncModel> m = pf::punc_model_load(argv[i]);
      const std::vector<pf::PuncWord> w = pf::host_punc_words(*m, text);
      std::vector<int32_t> ids, p(w.size());
      for (const pf::PuncWord& x : w) ids.push_back(x.id);
      for (int rep = 0; rep < 2; ++rep) ids.insert(ids.end(), ids.begin(), ids.end());       // 4 x the text: three windows
      p.resize(ids.size());
      std::vector<std::pair<int32_t, int32_t>> wins;
      pf::host_punc_ids(*m, ids.data(), (int64_t)ids.size(), p.data(), &wins);
      std::vector<int32_t> sent;
      const std::string out = pf::host_punc_assemble(*m, text, w, p.data(), &sent);
      std::printf("ok %d %d %d %zu %zu %zu|%s|", m->vocab, m->n_punc, m->n_layers, m->image.size(), wins.size(), sent.size(), out.c_str());
      for (int32_t e : p) std::printf(" %d", e);
      std::printf("\n");
    } catch (const pf::Error& e) {
      std::printf("refused %d\n", e.code);
    }
  }
  return 0;
}
