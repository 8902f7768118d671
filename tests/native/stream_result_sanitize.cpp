// csrc/stream_result.cpp under AddressSanitizer + UBSan: build_stream_result over result blocks filled by hand through the
// block views of decode_blocks.h — the host half of Recognizer::Forward without an engine.  Every case has B = 2 with
// unequal streams (a wrong row offset reads the other stream's data), every block is exactly words() long (an over-read is
// AddressSanitizer's to report), cells the builder must not read hold a canary, and the expected values are literals.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <utility>
#include <vector>

#include "hostutil.h"
#include "stream_result.h"

using namespace pf;

static int g_checks = 0;
#define REQUIRE(cond)                                                                  \
  do {                                                                                 \
    ++g_checks;                                                                        \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

template <class T, class U> static bool is(const std::vector<T>& v, std::initializer_list<U> want) {
  return v.size() == want.size() && std::equal(v.begin(), v.end(), want.begin(), [](const T& a, const U& b) { return a == (T)b; });
}
static bool is(const TsList& v, std::initializer_list<std::pair<int, int>> want) {
  if (v.size() != want.size()) return false;
  size_t i = 0;
  for (auto& w : want) {
    if (v[i].size() != 2 || v[i][0] != w.first || v[i][1] != w.second) return false;
    ++i;
  }
  return true;
}
template <class T> struct same { using type = T; };        // (keeps the list out of the deduction of T)
template <class T> static void put(T* dst, std::initializer_list<typename same<T>::type> v) { std::copy(v.begin(), v.end(), dst); }
template <class T> static void fill(const Field<T>& f, void* base, T v) { std::fill(f(base), f(base) + f.count, v); }
static uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static float from_bits(uint32_t u) { float x; std::memcpy(&x, &u, 4); return x; }

static const int kCanary = -77;

// a forward of two streams and L positions: ids 100 .. (stream 0), 200 .. (stream 1)
static HostBatchOut forward(int L, int dflags) {
  HostBatchOut r;
  r.B = 2; r.L = L; r.V = 1000; r.T = L; r.decode_flags = dflags;
  for (int b = 0; b < 2; ++b)
    for (int l = 0; l < L; ++l) r.ids.push_back(100 * (b + 1) + l);
  r.token_num = {L, L}; r.fire_count = {L, L};
  return r;
}
// a stream that has been through an earlier call: every field the builder must reset holds something
static StreamResult used() {
  StreamResult s;
  s.Tokens = {9, 9, 9}; s.Scores = {9.f}; s.AltIds = {9}; s.AltVal = {9.f}; s.AltK = 9; s.Alternatives.resize(2);
  s.AlignTs = {9, 9}; s.AlignTok = {9.f}; s.AlignPath = 9.f; s.AlignLoglik = 9.0; s.AlignOk = 9; s.AlignN = 9;
  return s;
}
static StreamResult build(const HostBatchOut& r, const ResultPlan& p, int b) {
  StreamResult s = used();
  build_stream_result(r, p, b, s);
  return s;
}
static bool no_extras(const StreamResult& s) {
  return s.AltIds.empty() && s.AltVal.empty() && s.AltK == 0 && s.Alternatives.empty() && s.AlignTs.empty() && s.AlignTok.empty() &&
         s.AlignPath == 0.f && s.AlignLoglik == 0.0 && s.AlignOk == 0 && s.AlignN == -1;
}

static void plain_and_scores() {
  HostBatchOut r = forward(3, 0);
  ResultPlan p;
  p.ms_frame = 60;
  StreamResult s = used();
  s.Timestamps = {{7, 8}};                             // what an earlier call left: appended to, not replaced
  build_stream_result(r, p, 1, s);
  REQUIRE(is(s.Tokens, {200, 201, 202}));
  REQUIRE(is(s.Timestamps, {{7, 8}, {0, 0}, {0, 0}, {0, 0}}));
  REQUIRE(s.Scores.empty() && no_extras(s));
  REQUIRE(is(build(r, p, 0).Tokens, {100, 101, 102}));
  // want_scores on and off over the same forward
  r.decode_flags = p.dflags = PF_DECODE_SCORES;
  r.scores = {-0.5f, -1.5f, -2.5f, -3.5f, -4.5f, -5.5f};
  p.want_scores = true;
  REQUIRE(is(build(r, p, 1).Scores, {-3.5f, -4.5f, -5.5f}));
  REQUIRE(is(build(r, p, 0).Scores, {-0.5f, -1.5f, -2.5f}));
  p.want_scores = false;
  REQUIRE(build(r, p, 1).Scores.empty());
}

static void peak_row() {
  // a timestamp model: P = 3 * T floats per stream; the entries are time_stamp_lfr6's on the stream's own row and ids
  HostBatchOut r = forward(3, 0);
  const int P = 12;
  r.peak_len = P;
  r.cif_peak.assign(2 * P, 0.f);
  for (int i : {1, 4, 9}) r.cif_peak[(size_t)i] = 1.f;
  for (int i : {2, 5, 8}) r.cif_peak[(size_t)P + i] = 1.f;
  ResultPlan p;
  p.ms_frame = 60;
  for (int b = 0; b < 2; ++b) {
    const StreamResult s = build(r, p, b);
    const TsList want = time_stamp_lfr6(r.cif_peak.data() + (size_t)b * P, P, s.Tokens);
    REQUIRE(want.size() == 2 && s.Timestamps == want);
  }
  REQUIRE(!(build(r, p, 0).Timestamps == build(r, p, 1).Timestamps));
}

// the collapse of stream 0: three runs (inside the prompt rows, across their end, behind them), of stream 1: two
static HostBatchOut ctc_forward(int cap, int dflags) {
  HostBatchOut r = forward(12, dflags);
  r.scores.assign(24, -9.f);
  r.ctc_cap = cap;
  const CtcBlock k = r.ctc_block();
  r.ctc.assign(k.words(), 0);
  void* q = r.ctc.data();
  fill(k.ids, q, (int64_t)kCanary); fill(k.first, q, kCanary); fill(k.last, q, kCanary); fill(k.score, q, (float)kCanary);
  put(k.n(q), {3, 2});
  put(k.ids(q), {(int64_t)5, 6, 7}); put(k.first(q), {0, 3, 6}); put(k.last(q), {2, 5, 11}); put(k.score(q), {-0.25f, -0.5f, -0.75f});
  put(k.ids(q) + cap, {(int64_t)8, 9}); put(k.first(q) + cap, {4, 7}); put(k.last(q) + cap, {6, 9}); put(k.score(q) + cap, {-1.25f, -1.5f});
  return r;
}

static void ctc_collapse() {
  ResultPlan p;
  p.dflags = PF_DECODE_CTC | PF_DECODE_SCORES; p.sensevoice = true; p.ms_frame = 60;
  for (int cap : {3, 12}) {                            // the kernel's cap is L; n_max and a larger one read the same
    const HostBatchOut r = ctc_forward(cap, p.dflags);
    const StreamResult s0 = build(r, p, 0), s1 = build(r, p, 1);
    REQUIRE(is(s0.Tokens, {5, 6, 7}) && is(s0.Scores, {-0.25f, -0.5f, -0.75f}));
    REQUIRE(is(s0.Timestamps, {{0, 0}, {0, 120}, {120, 480}}));      // frames 0-2 | 3-5 | 6-11 behind four prompt rows of 60 ms
    REQUIRE(is(s1.Tokens, {8, 9}) && is(s1.Scores, {-1.25f, -1.5f}));
    REQUIRE(is(s1.Timestamps, {{0, 180}, {180, 360}}));
    REQUIRE(no_extras(s0) && no_extras(s1));
  }
  HostBatchOut r = ctc_forward(12, p.dflags);
  r.ctc_block().n(r.ctc.data())[1] = 0;                // n[b] = 0: nothing, not the per-frame ids
  StreamResult s = build(r, p, 1);
  REQUIRE(s.Tokens.empty() && s.Scores.empty() && s.Timestamps.empty());
  REQUIRE(is(build(r, p, 0).Tokens, {5, 6, 7}));
  r.ctc.clear(); r.ctc_cap = 0;                        // a forward that left no block: n = 0 for every stream
  for (int b = 0; b < 2; ++b) {
    s = build(r, p, b);
    REQUIRE(s.Tokens.empty() && s.Scores.empty() && s.Timestamps.empty());
  }
}

static void ctc_topk_peak_frame() {
  // per collapsed token the alternatives of ONE frame of its run: the first whose log-prob has the token's score's bits
  const int L = 6, K = 2;
  const float nan1 = from_bits(0x7fc00001u);
  ResultPlan p;
  p.dflags = PF_DECODE_CTC | PF_DECODE_SCORES | PF_DECODE_TOPK; p.sensevoice = true; p.ms_frame = 60;
  HostBatchOut r = forward(L, p.dflags);
  r.scores = {-0.5f, -0.5f, -0.125f, -0.5f, -0.5f, -0.5f,          // stream 0: the token's score sits at frame 2 only
              -0.75f, -0.5f, -0.5f, -0.375f, -1.f, nan1};            // stream 1
  r.ctc_cap = L;
  const CtcBlock c = r.ctc_block();
  r.ctc.assign(c.words(), 0);
  void* q = r.ctc.data();
  fill(c.first, q, kCanary); fill(c.last, q, kCanary);
  put(c.n(q), {1, 3});
  put(c.ids(q), {(int64_t)5}); put(c.first(q), {0}); put(c.last(q), {5}); put(c.score(q), {-0.125f});
  put(c.ids(q) + L, {(int64_t)6, 7, 8}); put(c.first(q) + L, {0, 3, 4}); put(c.last(q) + L, {2, 3, 5});
  put(c.score(q) + L, {-0.5f, -0.25f, nan1});          // at frames 1 and 2 | at no frame of the run | a NaN of frame 5's bits
  r.topk_k = K;
  const TopkBlock t = r.topk_block();
  r.topk.assign(t.words(), 0);
  for (int row = 0; row < 2 * L; ++row)
    for (int j = 0; j < K; ++j) {
      t.ids(r.topk.data())[row * K + j] = 1000 + 10 * row + j;
      t.val(r.topk.data())[row * K + j] = -(float)row - 0.5f * j;
    }
  const StreamResult s0 = build(r, p, 0), s1 = build(r, p, 1);
  REQUIRE(s0.AltK == 2 && is(s0.AltIds, {1020, 1021}) && is(s0.AltVal, {-2.f, -2.5f}));
  REQUIRE(s1.AltK == 2 && is(s1.AltIds, {1070, 1071, 1090, 1091, 1110, 1111}));    // rows 6 + 1 (the first of two), 6 + 3 (first), 6 + 5
  REQUIRE(is(s1.AltVal, {-7.f, -7.5f, -9.f, -9.5f, -11.f, -11.5f}));
  REQUIRE(is(s1.Tokens, {6, 7, 8}) && s1.Scores.size() == 3 && bits(s1.Scores[2]) == 0x7fc00001u);
  REQUIRE(s0.Alternatives.empty() && s1.Alternatives.empty());
}

// paraformer, L = 2, K = 2: the lists of stream 0 (ids 10 11 | 20 21) and stream 1 (30 31 | 40 41), exactly representable values
static HostBatchOut topk_forward(int dflags) {
  HostBatchOut r = forward(2, dflags);
  r.scores = {-0.125f, -0.25f, -0.125f, -0.25f};
  r.token_num = {1, 2};                                // stream 0: only its first position is its own
  r.topk_k = 2;
  const TopkBlock t = r.topk_block();
  r.topk.assign(t.words(), 0);
  void* q = r.topk.data();
  put(t.ids(q), {(int64_t)10, 11, 20, 21, 30, 31, 40, 41});
  put(t.val(q), {-0.125f, -0.75f, -0.25f, -0.375f, -0.125f, -1.f, -0.25f, -0.5f});
  put(t.n(q), {2, 2, 2, 2});
  return r;
}
static bool plain_alt(const Alternative& a) {
  return !a.ctc && a.ts.empty() && std::isnan(a.loglik) && a.hot_tokens == 0 && std::isnan(a.loglik_sum) && std::isnan(a.lm_sum);
}

static void nbest_lists() {
  ResultPlan p;
  p.dflags = PF_DECODE_TOPK | PF_DECODE_SCORES; p.nbest = 3; p.ms_frame = 60;
  HostBatchOut r = topk_forward(p.dflags);
  for (int pass = 0; pass < 2; ++pass) {               // the host enumeration; then a search that was planned but left no block
    const StreamResult s0 = build(r, p, 0), s1 = build(r, p, 1);
    REQUIRE(s1.AltK == 2 && is(s1.AltIds, {30, 31, 40, 41}) && is(s1.AltVal, {-0.125f, -1.f, -0.25f, -0.5f}));
    REQUIRE(is(s0.AltIds, {10, 11, 20, 21}));
    REQUIRE(s1.Alternatives.size() == 3);              // n_free = min(L, token_num) = 2: ranks 00, 01, 10
    REQUIRE(is(s1.Alternatives[0].ids, {30, 40}) && s1.Alternatives[0].score == -0.375);
    REQUIRE(is(s1.Alternatives[1].ids, {30, 41}) && s1.Alternatives[1].score == -0.625);
    REQUIRE(is(s1.Alternatives[2].ids, {31, 40}) && s1.Alternatives[2].score == -1.25);
    REQUIRE(s0.Alternatives.size() == 2);              // n_free = 1: position 1 keeps rank 0, so 00 and 10 are all there is
    REQUIRE(is(s0.Alternatives[0].ids, {10, 20}) && s0.Alternatives[0].score == -0.375);
    REQUIRE(is(s0.Alternatives[1].ids, {11, 20}) && s0.Alternatives[1].score == -1.0);
    for (auto& a : s1.Alternatives) REQUIRE(plain_alt(a));
    p.search_on = true;
  }
  r.token_num[0] = -3;                                 // max(token_num, 0): no free position, the arg-max alone
  REQUIRE(build(r, p, 0).Alternatives.size() == 1);
  // the device search: N = 3 rank vectors per stream in ITS order, stream 1 found two
  r.nbs_n = 3;
  const NbestSearchBlock k = r.nbs_block();
  r.nbs.assign(k.words(), 0);
  void* q = r.nbs.data();
  fill(k.ranks, q, kCanary); fill(k.matched, q, kCanary);
  put(k.n_hyp(q), {3, 2});
  put(k.ranks(q), {0, 0, 1, 1, 0, 1}); put(k.ranks(q) + 3 * 2, {1, 0, 0, 1});
  put(k.score(q), {-1.0, -1.5, -1.75, -2.0, -3.0, 77.0}); put(k.loglik(q), {-0.5, -0.75, -1.0, -1.5, -2.5, 77.0});
  put(k.lm_sum(q), {-0.25, -0.25, -0.25, -0.5, -0.75, 77.0}); put(k.matched(q), {0, 0, 0, 1, 0, kCanary});
  const StreamResult s0 = build(r, p, 0), s1 = build(r, p, 1);
  REQUIRE(s0.Alternatives.size() == 3 && s1.Alternatives.size() == 2);
  REQUIRE(is(s0.Alternatives[0].ids, {10, 20}) && is(s0.Alternatives[1].ids, {11, 21}) && is(s0.Alternatives[2].ids, {10, 21}));
  REQUIRE(s0.Alternatives[2].score == -1.75 && s0.Alternatives[2].loglik_sum == -1.0 && s0.Alternatives[2].lm_sum == -0.25);
  const Alternative& a = s1.Alternatives[0];
  REQUIRE(is(a.ids, {31, 40}) && a.score == -2.0 && a.loglik_sum == -1.5 && a.lm_sum == -0.5 && a.hot_tokens == 1 && !a.ctc);
  const Alternative& c = s1.Alternatives[1];
  REQUIRE(is(c.ids, {30, 41}) && c.score == -3.0 && c.loglik_sum == -2.5 && c.lm_sum == -0.75 && c.hot_tokens == 0);
  REQUIRE(is(s1.AltIds, {30, 31, 40, 41}));
  p.sensevoice = true;                                 // SenseVoice offers K alone
  REQUIRE(build(r, p, 1).Alternatives.empty() && build(r, p, 1).AltK == 2);
  // L == 0: no list, no search, whatever the plan says
  p.sensevoice = false;
  HostBatchOut z = forward(0, p.dflags);
  z.topk_k = 2; z.nbs_n = 3;
  for (int b = 0; b < 2; ++b) {
    const StreamResult s = build(z, p, b);
    REQUIRE(s.Tokens.empty() && s.Timestamps.empty() && s.Scores.empty() && no_extras(s));
  }
}

// the beam search of N = 3 labelings, cap 4: stream 0 found three (lengths 1, 0, 4), stream 1 two (2, 3)
static HostBatchOut beam_forward(int dflags, bool hot, bool lm) {
  HostBatchOut r = forward(5, dflags);
  r.scores.assign(10, -9.f);
  r.beam_n = 3; r.beam_cap = 4;
  const BeamBlock k = r.beam_block();
  r.beam.assign(k.words(), 0);
  void* q = r.beam.data();
  fill(k.ids, q, kCanary); fill(k.len, q, kCanary);
  put(k.n_hyp(q), {3, 2});
  put(k.len(q), {1, 0, 4, 2, 3});
  put(k.score(q), {-0.5, -1.0, -1.25, -1.5, -2.5, 77.0});
  put(k.ids(q), {5}); put(k.ids(q) + 2 * 4, {1, 2, 3, 4}); put(k.ids(q) + 3 * 4, {7, 8}); put(k.ids(q) + 4 * 4, {7, 8, 9});
  if (hot || lm) {
    r.beam_biased = hot;
    const BeamHotBlock h = r.beam_hot_block();
    r.beam_hot.assign(h.words(), 0);
    put(h.loglik(r.beam_hot.data()), {-0.25, -0.75, -1.0, -3.5, -2.25, 77.0});
    if (hot) put(h.matched(r.beam_hot.data()), {1, 0, 3, 2, 0, kCanary});
  }
  if (lm) {
    const BeamLmBlock l = r.beam_lm_block();
    r.beam_lm.assign(l.words(), 0);
    put(l.lm_sum(r.beam_lm.data()), {-0.125, -0.25, -0.375, -0.625, -0.875, 77.0});
  }
  return r;
}

static void beam_lists() {
  ResultPlan p;
  p.dflags = PF_DECODE_CTC_BEAM | PF_DECODE_SCORES; p.sensevoice = true; p.ms_frame = 60;
  for (int form = 0; form < 4; ++form) {               // plain | hot only | LM only | both
    const bool hot = form & 1, lm = form & 2;
    p.hot_on = hot; p.lm_on = lm;
    const HostBatchOut r = beam_forward(p.dflags, hot, lm);
    const StreamResult s0 = build(r, p, 0), s1 = build(r, p, 1);
    REQUIRE(is(s1.Tokens, {200, 201, 202, 203, 204}) && s1.AltK == 0);
    REQUIRE(s0.Alternatives.size() == 3 && s1.Alternatives.size() == 2);        // n_hyp[1] < N
    REQUIRE(is(s0.Alternatives[0].ids, {5}) && s0.Alternatives[1].ids.empty() && is(s0.Alternatives[2].ids, {1, 2, 3, 4}));
    REQUIRE(s0.Alternatives[2].score == -1.25);
    const Alternative& a = s1.Alternatives[0];
    const Alternative& c = s1.Alternatives[1];
    REQUIRE(a.ctc && c.ctc && is(a.ids, {7, 8}) && is(c.ids, {7, 8, 9}) && a.score == -1.5 && c.score == -2.5);
    REQUIRE(a.ts.empty() && std::isnan(a.loglik) && c.ts.empty() && std::isnan(c.loglik));
    REQUIRE(a.hot_tokens == (hot ? 2 : 0) && c.hot_tokens == 0 && s0.Alternatives[2].hot_tokens == (hot ? 3 : 0));
    if (hot || lm) REQUIRE(a.loglik_sum == -3.5 && c.loglik_sum == -2.25);
    else REQUIRE(std::isnan(a.loglik_sum) && std::isnan(c.loglik_sum));
    if (lm) REQUIRE(a.lm_sum == -0.625 && c.lm_sum == -0.875 && s0.Alternatives[0].lm_sum == -0.125);
    else REQUIRE(std::isnan(a.lm_sum) && std::isnan(c.lm_sum));
  }
  p.hot_on = p.lm_on = false;
  HostBatchOut r = beam_forward(p.dflags, false, false);
  r.beam.clear();                                      // a forward that left no block: no hypotheses
  REQUIRE(build(r, p, 0).Alternatives.empty() && build(r, p, 1).Alternatives.empty());
}

// H jobs per stream, cap 3 (own targets) or 4 (beside the beam); every job's cells hold the canary until a case writes them
static void lay_align(HostBatchOut& r, int H, int cap) {
  r.align_h = H; r.align_cap = cap;
  const AlignBlock k = r.align_block();
  r.align.assign(k.words(), 0);
  void* q = r.align.data();
  fill(k.first, q, kCanary); fill(k.last, q, kCanary); fill(k.tok, q, (float)kCanary); fill(k.len, q, -1);
}
static void job(HostBatchOut& r, int j, int ok, int len, double loglik, float path, std::initializer_list<int> first,
                std::initializer_list<int> last, std::initializer_list<float> tok) {
  const AlignBlock k = r.align_block();
  void* q = r.align.data();
  k.ok(q)[j] = ok; k.len(q)[j] = len; k.loglik(q)[j] = loglik; k.path(q)[j] = path;
  put(k.first(q) + (size_t)j * r.align_cap, first); put(k.last(q) + (size_t)j * r.align_cap, last); put(k.tok(q) + (size_t)j * r.align_cap, tok);
}

static void own_targets() {
  ResultPlan p;
  p.dflags = PF_DECODE_ALIGN | PF_DECODE_SCORES; p.sensevoice = true; p.ms_frame = 60; p.any_target = true;
  HostBatchOut r = forward(12, p.dflags);
  r.scores.assign(24, -9.f);
  lay_align(r, 1, 3);
  job(r, 0, 1, 2, -0.75, -0.875f, {4, 6}, {5, 9}, {-0.5f, -0.25f});             // stream 1 has no target: len = -1
  StreamResult s0 = build(r, p, 0), s1 = build(r, p, 1);
  REQUIRE(s0.AlignN == 2 && s0.AlignOk == 1 && s0.AlignPath == -0.875f && s0.AlignLoglik == -0.75);
  REQUIRE(is(s0.AlignTs, {0, 120, 120, 360}) && is(s0.AlignTok, {-0.5f, -0.25f}));
  REQUIRE(no_extras(s1) && is(s1.Tokens, {200, 201, 202, 203, 204, 205, 206, 207, 208, 209, 210, 211}));
  p.any_target = false;                                // no stream of the batch had one: job 0 is nobody's own
  REQUIRE(no_extras(build(r, p, 0)) && no_extras(build(r, p, 1)));
  p.any_target = true;
  const float ninf = -std::numeric_limits<float>::infinity();
  job(r, 1, 0, 3, -(double)std::numeric_limits<float>::infinity(), ninf, {}, {}, {});   // not ok: no times, the fields still set
  s1 = build(r, p, 1);
  REQUIRE(s1.AlignN == 3 && s1.AlignOk == 0 && s1.AlignPath == ninf && s1.AlignLoglik == (double)ninf);
  REQUIRE(s1.AlignTs.empty() && s1.AlignTok.empty());
  r.align.clear();                                     // a forward that left no block: H = 0
  REQUIRE(no_extras(build(r, p, 0)) && no_extras(build(r, p, 1)));
}

static void align_beside_beam() {
  ResultPlan p;
  p.dflags = PF_DECODE_ALIGN | PF_DECODE_CTC_BEAM | PF_DECODE_SCORES; p.sensevoice = true; p.ms_frame = 60; p.any_target = true;
  HostBatchOut r = beam_forward(p.dflags, false, false);        // lengths: stream 0: 1 0 4, stream 1: 2 3
  lay_align(r, 4, 4);                                  // H = a_hc + N: the own target, then one job per labeling
  job(r, 0, 1, 1, -0.5, -0.5f, {4}, {4}, {-0.5f});
  job(r, 1, 0, 1, -1.5, -1.5f, {}, {}, {});           // stream 0's first labeling: not ok
  job(r, 2, 1, 0, -1.75, -1.75f, {}, {}, {});
  job(r, 3, 1, 4, -2.0, -2.0f, {4, 5, 6, 7}, {4, 5, 6, 9}, {-0.125f, -0.125f, -0.125f, -0.125f});
  job(r, 5, 1, 2, -1.25, -1.25f, {4, 5}, {4, 7}, {-0.25f, -0.25f});              // stream 1 (own job 4: no target), labeling 0
  job(r, 6, 1, 2, -2.25, -2.25f, {4, 5}, {4, 7}, {-0.25f, -0.25f});              // labeling 1 has 3 ids: a_len != b_len
  StreamResult s0 = build(r, p, 0), s1 = build(r, p, 1);
  REQUIRE(s0.AlignN == 1 && is(s0.AlignTs, {0, 60}) && s1.AlignN == -1);
  REQUIRE(s0.Alternatives.size() == 3 && s1.Alternatives.size() == 2);
  REQUIRE(s0.Alternatives[0].loglik == -1.5 && s0.Alternatives[0].ts.empty());
  REQUIRE(s0.Alternatives[1].loglik == -1.75 && s0.Alternatives[1].ts.empty() && s0.Alternatives[1].ids.empty());
  REQUIRE(s0.Alternatives[2].loglik == -2.0 && is(s0.Alternatives[2].ts, {0, 60, 60, 120, 120, 180, 180, 360}));
  REQUIRE(s1.Alternatives[0].loglik == -1.25 && is(s1.Alternatives[0].ts, {0, 60, 60, 240}));
  REQUIRE(s1.Alternatives[1].loglik == -2.25 && s1.Alternatives[1].ts.empty());
  // no own job (no target in the batch): H = N, the labelings' jobs begin at 0
  p.any_target = false;
  lay_align(r, 3, 4);
  job(r, 3, 1, 2, -1.25, -1.25f, {8, 9}, {8, 9}, {-0.25f, -0.25f});
  s1 = build(r, p, 1);
  REQUIRE(s1.AlignN == -1 && s1.Alternatives[0].loglik == -1.25 && is(s1.Alternatives[0].ts, {240, 300, 300, 360}));
  // H smaller than a_hc + N: no labeling gets times or a log-likelihood; the own job is still read
  p.any_target = true;
  s1 = build(r, p, 1);
  REQUIRE(s1.AlignN == 2 && is(s1.AlignTs, {240, 300, 300, 360}));
  REQUIRE(s1.Alternatives.size() == 2);
  for (auto& a : s1.Alternatives) REQUIRE(a.ts.empty() && std::isnan(a.loglik));
}

int main() {
  try {
    plain_and_scores();
    peak_row();
    ctc_collapse();
    ctc_topk_peak_frame();
    nbest_lists();
    beam_lists();
    own_targets();
    align_beside_beam();
  } catch (const Error& e) {
    std::printf("FAILED: pf::Error %d: %s\n", e.code, e.what());
    return 1;
  }
  REQUIRE(frame_ms(60, 0, 3).size() == 2 && frame_ms(60, 0, 3)[0] == 0 && frame_ms(60, 0, 3)[1] == 0 && frame_ms(60, 4, 4)[1] == 60);
  std::printf("ok %d checks\n", g_checks);
  return 0;
}
