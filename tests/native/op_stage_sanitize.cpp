// The host-only part of csrc/op_stage.h under AddressSanitizer + UBSan: the kit the stand-alone ops stage their buffers and check
// their results with.  No test before this one showed that the guard rule FIRES.
//   (a) blocked_index is a bijection of [0, Mp) x [0, Kp) onto [0, Mp * Kp) and equals the formula restated here
//   (b) the hostile patterns are finite, large, never equal in neighbouring cells, and have the bit formulas restated here
//   (c) the typed carve: 256-aligned fields in declaration order, no overlap, total = the sum of the rounded sizes; a pattern
//       written through every field of a heap buffer of exactly that size reads back (an out-of-bounds field is ASan's to report)
//   (d) the guard rule against a brute-force restatement over a grid of geometries, row-major and blocked: a clean image passes,
//       one unwritten cell inside / one written cell beyond N / one written guard-row cell is reported AS THAT CELL, a written
//       cell of the declared padding is not; must_write = false; the before-image form; the two-sentinel byte rule
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "op_stage.h"

using namespace pf;

static long g_checks = 0;
#define REQUIRE(cond)                                                                  \
  do {                                                                                 \
    ++g_checks;                                                                        \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

static int64_t up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// ---- (a)
static void test_blocked_index() {
  for (int Mp : {32, 64, 96})
    for (int Kp : {8, 64, 72, 512}) {
      std::vector<char> seen((size_t)Mp * Kp, 0);
      for (int m = 0; m < Mp; ++m)
        for (int k = 0; k < Kp; ++k) {
          const size_t want = (((size_t)(m / 32) * (Kp / 8) + k / 8) * 32 + m % 32) * 8 + k % 8;
          const size_t got = blocked_index(m, k, Kp);
          REQUIRE(got == want);
          REQUIRE(got < seen.size());
          REQUIRE(!seen[got]);
          seen[got] = 1;
        }
    }
}

// ---- (b)
static void test_hostile() {
  for (size_t i = 0; i < 70000; ++i) {
    const uint16_t b16 = (uint16_t)(0x7800u | ((i * 37u) & 0x3FFu) | ((i & 1u) << 15));
    REQUIRE(hostile16_bits(i) == b16);
    const _Float16 h = hostile16(i);
    uint16_t back;
    std::memcpy(&back, &h, 2);
    REQUIRE(back == b16);
    const float f = (float)h;
    REQUIRE(std::isfinite(f) && std::fabs(f) >= 32768.0f && std::fabs(f) <= 65504.0f);
    REQUIRE(hostile16_bits(i) != hostile16_bits(i + 1));
    const float w = std::ldexp(1.0f + (float)((i * 37u) & 0x3FFu) / 1024.0f, 100) * ((i & 1u) ? -1.0f : 1.0f);
    REQUIRE(hostile32(i) == w && std::isfinite(w) && std::fabs(w) >= std::ldexp(1.0f, 100) && std::fabs(w) < std::ldexp(1.0f, 101));
    REQUIRE(hostile32(i) != hostile32(i + 1));
    const int32_t v = ((i & 1u) ? -1 : 1) * ((1 << 30) + (int32_t)((i * 37u) & 0xFFFFu));
    REQUIRE(hostile_i32(i) == v && std::abs((int64_t)v) >= (1 << 30));
    REQUIRE(hostile_i32(i) != hostile_i32(i + 1));
  }
  REQUIRE(kSentinel32 == 0x7FC5A5A5u && kSentinel16 == 0x7E5Au && kSentinel8[0] == 0x5A && kSentinel8[1] == 0xA5 && kPoison16 == 0x7A5Au);
  float s;
  std::memcpy(&s, &kSentinel32, 4);
  REQUIRE(std::isnan(s));
}

// ---- (c)
struct Walker {
  char* buf; size_t bytes, align; int phase; unsigned tag = 0; size_t prev_end = 0, rounded = 0;
  template <class T> void operator()(const Field<T>& f, size_t want_count) {
    ++tag;
    REQUIRE(f.off % align == 0);
    REQUIRE(f.count == want_count);
    REQUIRE(f.off == prev_end);                         // declaration order is memory order, nothing between two fields
    prev_end = f.off + (size_t)up((int64_t)(f.count * sizeof(T)), (int64_t)align);
    rounded += prev_end - f.off;
    REQUIRE(prev_end <= bytes);
    T* p = f((void*)buf);
    REQUIRE((const void*)f((const void*)buf) == (const void*)p);
    for (size_t i = 0; i < f.count; ++i) {
      const T v = (T)(tag * 1000 + i % 97);
      if (phase == 0) p[i] = v;
      else REQUIRE(p[i] == v);
    }
  }
};
static void test_carve() {
  for (size_t align : {(size_t)256, (size_t)512})
    for (size_t n : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)1000}) {
      StageCarve st{0, align};
      const auto a = st.take<float>(n);
      const auto b = st.take<uint8_t>(n + 3);
      const auto c = st.take<_Float16>(2 * n + 1);
      const auto d = st.take<int64_t>(n);
      const auto e = st.take<double>(1);
      std::vector<char> heap(st.off);                   // exactly the carved size
      for (int phase = 0; phase < 2; ++phase) {
        Walker w{heap.data(), heap.size(), align, phase};
        w(a, n); w(b, n + 3); w(c, 2 * n + 1); w(d, n); w(e, 1);
        REQUIRE(w.prev_end == st.off && w.rounded == st.off);
      }
    }
}

// ---- (d) the rule restated cell by cell: every offending cell, in no particular order
template <class U>
static bool brute_ok(const std::vector<U>& after, const std::vector<U>* before, U sentinel, const GuardGeom& g, int64_t* bad_m, int64_t* bad_n) {
  for (int64_t m = 0; m < g.rows; ++m)
    for (int64_t n = 0; n < g.ld; ++n) {
      size_t i = (size_t)(m * g.ld + n);
      if (g.blocked) i = (((size_t)(m / 32) * (g.N / 8) + n / 8) * 32 + m % 32) * 8 + n % 8;
      const bool inside = m < g.M && n < g.N, padding = !inside && n < g.N && m < g.guard_row;
      const U was = before ? (*before)[i] : sentinel;
      const bool bad = inside ? (g.must_write && after[i] == sentinel) : (!padding && after[i] != was);
      if (bad) { *bad_m = m; *bad_n = n; return false; }
    }
  return true;
}

template <class U>
static void guard_cases(U sentinel, U value) {
  for (int M : {1, 31, 33})
    for (int N : {4, 64})
      for (int blocked = 0; blocked < 2; ++blocked)
        for (int ld : {N, N + 4})
          for (int64_t guard : {(int64_t)M, up(M, 64), up(M, 256)}) {
            if (blocked && (ld != N || N % 8)) continue;           // the blocked layout has ld == N, N % 8 == 0
            const int64_t rows = up(M, 256) + 32;                  // a whole number of 32-row blocks, guard rows behind every guard
            const GuardGeom g{rows, ld, M, N, guard, blocked != 0, true};
            auto at = [&](int64_t m, int64_t n) { return blocked ? blocked_index(m, n, N) : (size_t)(m * ld + n); };
            std::vector<U> clean((size_t)rows * ld, sentinel);
            for (int m = 0; m < M; ++m)
              for (int n = 0; n < N; ++n) clean[at(m, n)] = value;
            int64_t bm = -1, bn = -1;
            REQUIRE(!guard_scan<U>(clean.data(), nullptr, sentinel, g));
            REQUIRE(brute_ok<U>(clean, nullptr, sentinel, g, &bm, &bn));
            auto expect = [&](std::vector<U> img, int64_t m, int64_t n, GuardFault why) {
              const GuardHit h = guard_scan<U>(img.data(), nullptr, sentinel, g);
              REQUIRE(h.fault == why && h.m == m && h.n == n);
              REQUIRE(!brute_ok<U>(img, nullptr, sentinel, g, &bm, &bn) && bm == m && bn == n);
              const std::string msg = guard_message("op: buffer", g, h);
              REQUIRE(msg.find("op: buffer") == 0 && msg.find(std::to_string(M) + " x " + std::to_string(N)) != std::string::npos &&
                      msg.find("ld " + std::to_string(ld)) != std::string::npos &&
                      msg.find("cell (" + std::to_string(m) + ", " + std::to_string(n) + ")") != std::string::npos &&
                      msg.find(guard_reason(why)) != std::string::npos && guard_reason(why)[0] != 0);
            };
            std::vector<U> img = clean;
            img[at(M - 1, N / 2)] = sentinel;                      // one unwritten cell inside
            expect(img, M - 1, N / 2, GuardFault::not_written);
            if (ld > N) {
              img = clean;
              img[at(M / 2, N + 1)] = value;                       // one written cell in a column beyond N
              expect(img, M / 2, N + 1, GuardFault::column_written);
              img = clean;
              img[at(rows - 1, ld - 1)] = value;                   // ... also in a guard row: still the column's fault
              expect(img, rows - 1, ld - 1, GuardFault::column_written);
            }
            img = clean;
            img[at(guard, 1)] = value;                             // the first guard row
            expect(img, guard, 1, GuardFault::row_written);
            img = clean;
            img[at(rows - 1, N - 1)] = value;                      // the last one
            expect(img, rows - 1, N - 1, GuardFault::row_written);
            if (guard > M) {
              img = clean;
              img[at(M, 0)] = value; img[at(guard - 1, N - 1)] = value;   // the declared padding [M, guard_row) may be written
              REQUIRE(!guard_scan<U>(img.data(), nullptr, sentinel, g));
              REQUIRE(brute_ok<U>(img, nullptr, sentinel, g, &bm, &bn));
            }
            // must_write = false accepts sentinel cells inside, and still guards the rest
            GuardGeom loose = g;
            loose.must_write = false;
            std::vector<U> none((size_t)rows * ld, sentinel);
            REQUIRE(!guard_scan<U>(none.data(), nullptr, sentinel, loose));
            none[at(guard, 0)] = value;
            REQUIRE(guard_scan<U>(none.data(), nullptr, sentinel, loose).fault == GuardFault::row_written);
            // the before-image form: a guard cell whose bits changed to another non-sentinel value is reported, an unchanged image is not
            std::vector<U> before((size_t)rows * ld);
            for (size_t i = 0; i < before.size(); ++i) before[i] = (U)(value + 1 + i % 5);
            std::vector<U> after = before;
            for (int m = 0; m < M; ++m)
              for (int n = 0; n < N; ++n) after[at(m, n)] = value;
            REQUIRE(!guard_scan<U>(after.data(), before.data(), sentinel, g));
            REQUIRE(brute_ok<U>(after, &before, sentinel, g, &bm, &bn));
            after[at(guard + 1, 2)] = (U)(before[at(guard + 1, 2)] + 1);
            REQUIRE(after[at(guard + 1, 2)] != sentinel);
            const GuardHit h = guard_scan<U>(after.data(), before.data(), sentinel, g);
            REQUIRE(h.fault == GuardFault::row_written && h.m == guard + 1 && h.n == 2);
            REQUIRE(!brute_ok<U>(after, &before, sentinel, g, &bm, &bn) && bm == guard + 1 && bn == 2);
          }
}

static void test_bytes_rule() {
  const int64_t M = 5, N = 12, ld = 16;
  std::vector<uint8_t> a0((size_t)(M + 2) * ld, kSentinel8[0]), a1((size_t)(M + 2) * ld, kSentinel8[1]);
  for (int64_t m = 0; m < M; ++m)
    for (int64_t n = 0; n < N; ++n) a0[(size_t)(m * ld + n)] = a1[(size_t)(m * ld + n)] = (uint8_t)(m * 16 + n);
  a0[0] = a1[0] = kSentinel8[0];                                   // a code may equal one run's sentinel
  a0[1] = a1[1] = kSentinel8[1];
  REQUIRE(!bytes_written_scan(a0.data(), a1.data(), ld, M, N));
  auto b0 = a0, b1 = a1;
  b0[(size_t)(3 * ld + 7)] = kSentinel8[0]; b1[(size_t)(3 * ld + 7)] = kSentinel8[1];   // written by neither run
  GuardHit h = bytes_written_scan(b0.data(), b1.data(), ld, M, N);
  REQUIRE(h.fault == GuardFault::not_written && h.m == 3 && h.n == 7);
  b0 = a0; b1 = a1;
  b1[(size_t)(4 * ld + 11)] ^= 1;                                   // differs between the runs
  h = bytes_written_scan(b0.data(), b1.data(), ld, M, N);
  REQUIRE(h.fault == GuardFault::runs_differ && h.m == 4 && h.n == 11);
  REQUIRE(guard_reason(GuardFault::runs_differ)[0] != 0);
}

int main() {
  test_blocked_index();
  test_hostile();
  test_carve();
  guard_cases<uint8_t>(kSentinel8[0], 0x11);
  guard_cases<uint16_t>(kSentinel16, 0x3C00);
  guard_cases<uint32_t>(kSentinel32, 0x3F800000u);
  test_bytes_rule();
  std::printf("ok %ld checks\n", g_checks);
  return 0;
}
