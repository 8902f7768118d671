// pfw_sanitize — the PFW1 container reader (csrc/pfw.cpp) as a stand-alone program, built with AddressSanitizer + UBSan on
// the host code (tests/test_pfw_cpu.py): every file named on the command line is framed and indexed under each of the three
// caller policies (the recogniser's weights, the VAD model, the punctuation model), and every byte of every indexed tensor
// is read, so an extent that the reader let through although it leaves the file is a sanitizer report.  One line per file,
// one word per policy: "ok" or the status code of the refusal.
//   usage: pfw_sanitize <file> [<file> ...]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pfw.h"

static std::vector<char> slurp(const char* path) {
  std::vector<char> v;
  if (FILE* f = std::fopen(path, "rb")) {
    char buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
  }
  return v;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const pf::PfwPolicy* policies[3] = {&pf::kPfwWeights, &pf::kPfwVadModel, &pf::kPfwPuncModel};
  unsigned long long sum = 0;
  for (int i = 1; i < argc; ++i) {
    const std::vector<char> file = slurp(argv[i]);
    // an exact-size copy on the heap: one byte past the image is poisoned, whatever the vector's capacity was
    char* image = new char[file.size() ? file.size() : 1];
    for (size_t k = 0; k < file.size(); ++k) image[k] = file[k];
    for (int p = 0; p < 3; ++p) {
      try {
        const pf::PfwFrame fr = pf::pfw_frame(file.empty() ? nullptr : image, (int64_t)file.size(), *policies[p]);
        const pf::PfwIndex ix = pf::pfw_index(image + 16, fr.header_len, fr.data_bytes, *policies[p]);
        for (const auto& kv : ix.tensors)
          for (int64_t k = 0; k < kv.second.nbytes; ++k) sum += (unsigned char)image[fr.data_off + kv.second.offset + k];
        std::printf("ok%s", p < 2 ? " " : "\n");
      } catch (const pf::Error& e) {
        std::printf("%d%s", e.code, p < 2 ? " " : "\n");
      }
    }
    delete[] image;
  }
  std::fprintf(stderr, "checksum %llu\n", sum);
  return 0;
}
