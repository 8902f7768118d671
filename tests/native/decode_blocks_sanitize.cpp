// csrc/decode_blocks.h under AddressSanitizer + UBSan: every block layout over a grid of dimensions that includes the awkward
// ones (B = 0, cap = 0, odd row counts), and copy_rows_padded.
//   (a) words() is the formula HostBatchOut carried by hand before the layouts had one definition (restated below)
//   (b) every field starts at a multiple of its element size
//   (c) fields do not overlap and end within bytes(): a distinct pattern is written through every field of a heap buffer of
//       exactly bytes() and read back (an out-of-bounds field is AddressSanitizer's to report)
//   (d) copy_rows_padded for dst_cap <, ==, > src_cap and dst_cap == 0, the fill value, int32 -> int64
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "decode_blocks.h"

using namespace pf;

static int g_checks = 0;
#define REQUIRE(cond)                                                                  \
  do {                                                                                 \
    ++g_checks;                                                                        \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

// the formulas as they stood in shards.h
static size_t ctc_words(int B, int cap) { return (size_t)B * cap + ((size_t)B * cap * 12 + (size_t)B * 4 + 7) / 8; }
static size_t topk_words(int64_t rows, int K) { return (size_t)rows * K + ((size_t)rows * K * 4 + (size_t)rows * 4 + 7) / 8; }
static size_t beam_words(int B, int N, int cap) { return (size_t)B * N + ((size_t)B * N * cap * 4 + (size_t)B * N * 4 + (size_t)B * 4 + 7) / 8; }
static size_t beam_hot_words(int B, int N) { return (size_t)B * N + ((size_t)B * N * 4 + 7) / 8; }
static size_t align_words(int B, int H, int cap) { return (size_t)B * H + ((size_t)B * H * 12 + (size_t)B * H * cap * 12 + 7) / 8; }

// one field of a block over `buf`: aligned, filled with a pattern of its own (phase 0) or compared with it (phase 1)
struct Walker {
  char* buf; size_t bytes; int phase; unsigned tag = 0; size_t prev_end = 0;
  template <class T> void operator()(const Field<T>& f, size_t want_count) {
    ++tag;
    REQUIRE(f.off % sizeof(T) == 0);
    REQUIRE(f.count == want_count);
    REQUIRE(f.off >= prev_end);                        // declaration order is memory order
    REQUIRE(f.off + f.count * sizeof(T) <= bytes);
    prev_end = f.off + f.count * sizeof(T);
    T* p = f((void*)buf);
    REQUIRE((const void*)f((const void*)buf) == (const void*)p);
    for (size_t i = 0; i < f.count; ++i) {
      const T v = (T)(tag * 1000 + i % 997);
      if (phase == 0) p[i] = v;
      else REQUIRE(p[i] == v);
    }
  }
};

template <class Blk, class Visit> static void check_block(const Blk& k, size_t want_words, Visit visit) {
  REQUIRE(k.begin == 0);
  REQUIRE(k.words() == want_words);
  REQUIRE(k.bytes() <= k.words() * 8 && k.bytes() + 8 > k.words() * 8);
  char* buf = (char*)std::malloc(k.bytes() ? k.bytes() : 1);   // malloc: 16-byte aligned, and ASan guards byte bytes()
  for (int phase = 0; phase < 2; ++phase) {
    Walker w{buf, k.bytes(), phase};
    visit(w);
    if (phase) REQUIRE(w.prev_end == k.bytes());       // the last field ends the block
  }
  std::free(buf);
}

// a block behind something else in a workspace: it begins 8-aligned, keeps its shape, and leaves the cursor past words() * 8
template <class Blk, class... Dims> static void check_placed(Dims... dims) {
  for (size_t lead : {(size_t)0, (size_t)1, (size_t)3, (size_t)8}) {
    Cursor c;
    c.take<int32_t>(lead);
    const Blk k(c, (size_t)dims...);
    const Blk z = block_at_zero<Blk>(dims...);
    REQUIRE(k.begin % 8 == 0 && k.begin >= lead * 4 && k.begin < lead * 4 + 8);
    REQUIRE(k.bytes() == z.bytes() && k.words() == z.words());
    REQUIRE(c.off == k.begin + k.words() * 8);
  }
}

static void blocks() {
  const int Bs[] = {0, 1, 3}, NHs[] = {1, 5}, caps[] = {0, 1, 7}, Ks[] = {1, 8}, rowss[] = {1, 3, 21};
  for (int B : Bs)
    for (int cap : caps) {
      const size_t n = (size_t)B * cap;
      const CtcBlock k = block_at_zero<CtcBlock>(B, cap);
      check_block(k, ctc_words(B, cap), [&](Walker& w) { w(k.ids, n); w(k.first, n); w(k.last, n); w(k.score, n); w(k.n, (size_t)B); });
      check_placed<CtcBlock>(B, cap);
    }
  for (int rows : rowss)
    for (int K : Ks) {
      const size_t n = (size_t)rows * K;
      const TopkBlock k = block_at_zero<TopkBlock>(rows, K);
      check_block(k, topk_words(rows, K), [&](Walker& w) { w(k.ids, n); w(k.val, n); w(k.n, (size_t)rows); });
      REQUIRE(k.bytes() == n * 12 + (size_t)rows * 4);
      check_placed<TopkBlock>(rows, K);
    }
  for (int B : Bs)
    for (int N : NHs) {
      const size_t hyp = (size_t)B * N;
      const BeamHotBlock h = block_at_zero<BeamHotBlock>(B, N);
      check_block(h, beam_hot_words(B, N), [&](Walker& w) { w(h.loglik, hyp); w(h.matched, hyp); });
      check_placed<BeamHotBlock>(B, N);
      for (int cap : caps) {
        const BeamBlock k = block_at_zero<BeamBlock>(B, N, cap);
        check_block(k, beam_words(B, N, cap), [&](Walker& w) { w(k.score, hyp); w(k.ids, hyp * cap); w(k.len, hyp); w(k.n_hyp, (size_t)B); });
        check_placed<BeamBlock>(B, N, cap);
        const AlignBlock a = block_at_zero<AlignBlock>(B, N, cap);   // H takes N's values
        check_block(a, align_words(B, N, cap), [&](Walker& w) {
          w(a.loglik, hyp); w(a.path, hyp); w(a.ok, hyp); w(a.len, hyp); w(a.first, hyp * cap); w(a.last, hyp * cap); w(a.tok, hyp * cap);
        });
        check_placed<AlignBlock>(B, N, cap);
      }
    }
  // the "take" step on its own: mixed element sizes, each field aligned to its own
  Cursor c;
  const Field<int32_t> a = c.take<int32_t>(3);
  const Field<double> d = c.take<double>(2);
  const Field<int32_t> e = c.take<int32_t>(0);
  const Field<int64_t> f = c.take<int64_t>(1);
  REQUIRE(a.off == 0 && d.off == 16 && e.off == 32 && f.off == 32 && c.off == 40);
}

template <class D, class S> static void rows_case(size_t dst_cap, size_t src_cap, size_t rows, D fill) {
  std::vector<S> src(rows * src_cap);
  for (size_t i = 0; i < src.size(); ++i) src[i] = (S)((i % 2 ? -1 : 1) * (S)(i + 1));
  // heap buffers of the exact size: a write past a row's end of the last row is AddressSanitizer's to report
  D* dst = (D*)std::malloc(rows * dst_cap * sizeof(D) ? rows * dst_cap * sizeof(D) : 1);
  for (size_t i = 0; i < rows * dst_cap; ++i) dst[i] = (D)77;
  copy_rows_padded(dst, dst_cap, src.data(), src_cap, rows, fill);
  for (size_t r = 0; r < rows; ++r)
    for (size_t p = 0; p < dst_cap; ++p) REQUIRE(dst[r * dst_cap + p] == (p < src_cap ? (D)src[r * src_cap + p] : fill));
  std::free(dst);
}

static void rows() {
  for (size_t nrows : {(size_t)0, (size_t)1, (size_t)3})
    for (size_t src_cap : {(size_t)0, (size_t)1, (size_t)7})
      for (size_t dst_cap : {(size_t)0, (size_t)1, (size_t)6, (size_t)7, (size_t)8, (size_t)19}) {
        rows_case<int64_t, int64_t>(dst_cap, src_cap, nrows, -1);
        rows_case<int32_t, int32_t>(dst_cap, src_cap, nrows, -1);
        rows_case<float, float>(dst_cap, src_cap, nrows, 0.f);
        rows_case<int64_t, int32_t>(dst_cap, src_cap, nrows, -1);      // the beam ids widen
      }
  // a negative int32 widens by value, not by bit pattern
  const int32_t s[2] = {-5, 2147483647};
  int64_t d[3] = {0, 0, 0};
  copy_rows_padded(d, 3, s, 2, 1, (int64_t)-1);
  REQUIRE(d[0] == -5 && d[1] == 2147483647LL && d[2] == -1);
  // a null destination is skipped
  copy_rows_padded((int64_t*)nullptr, 4, s, 2, 1, (int64_t)-1);
}

int main() {
  blocks();
  rows();
  std::printf("ok %d checks\n", g_checks);
  return 0;
}
