// stream_result.h — what a GetResults leaves in a stream, and the host arithmetic that builds it from the result blocks of one
// forward (decode_blocks.h).  Host-only: no engine, no lease, no device call — tests/native/stream_result_sanitize.cpp runs
// it without a GPU.  A new decoding extra is a field of StreamResult and lines in build_stream_result.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

#include "decode_blocks.h"

namespace pf {

// One timestamp, the reference's int[]: {begin_ms, end_ms} — or several pairs in a row where DecodeMulti merges word pieces
// (OfflineRecognizer.cs:350-395).  Up to six ints live inside the object: a std::vector per token cost one heap allocation when
// Forward pushes it, one when DecodeMulti copies it and a free each — 0.4 ms of host time per 32 x 30 s GetResults (round 6).
class TsVec {
 public:
  TsVec() = default;
  TsVec(std::initializer_list<int32_t> l) { append(l.begin(), l.end()); }
  TsVec(const int32_t* a, const int32_t* b) { append(a, b); }
  const int32_t* data() const { return n_ <= kInline ? inl_ : big_.data(); }
  size_t size() const { return n_; }
  const int32_t* begin() const { return data(); }
  const int32_t* end() const { return data() + n_; }
  int32_t operator[](size_t i) const { return data()[i]; }
  void append(const int32_t* a, const int32_t* b) {
    const size_t k = (size_t)(b - a);
    if (n_ > kInline) big_.insert(big_.end(), a, b);
    else if (n_ + k <= kInline) std::copy(a, b, inl_ + n_);
    else { big_.assign(inl_, inl_ + n_); big_.insert(big_.end(), a, b); }
    n_ += (uint32_t)k;
  }
  bool operator==(const TsVec& o) const { return n_ == o.n_ && std::equal(begin(), end(), o.begin()); }
 private:
  static constexpr uint32_t kInline = 6;
  uint32_t n_ = 0;
  int32_t inl_[kInline] = {0, 0, 0, 0, 0, 0};
  std::vector<int32_t> big_;
};
using TsList = std::vector<TsVec>;

// OfflineRecognizerResultEntity (Model/OfflineRecognizerResultEntity.cs:9-29)
struct ResultEntity {
  std::string Text;
  int TextLen = 0;                              // UTF-16 length, as C# string.Length
  std::vector<std::string> Tokens;
  TsList Timestamps;
};

// One entry of a stream's n-best list (Recognizer::SetNBest): the ids of every position, the float64 sum of their log-probs
// and what DecodeMulti makes of them
struct Alternative {
  std::vector<int64_t> ids;
  double score = 0;
  bool ctc = false;            // a labeling of the CTC beam search (SetCtcBeam): its own length, score = log of the summed alignments
  // with SetAlign beside SetCtcBeam: the labeling's own forced alignment — [begin, end] ms per id (flat, 2 per id; empty without
  // it or when the alignment is not ok) and the log of the sum over ALL of its alignments (NaN without it)
  std::vector<int32_t> ts;
  double loglik = std::nan("");
  // with SetHotwordBoost beside SetCtcBeam: the hot-word tokens the labeling completed (score = loglik_sum + boost * these) and
  // the unbiased log of the alignments the search summed (0 / NaN without it)
  int hot_tokens = 0;
  double loglik_sum = std::nan("");
  // with SetLm beside SetCtcBeam: the weighted LM score of the labeling, score = (loglik_sum + boost * hot_tokens) + lm_sum (NaN
  // without it; loglik_sum is then filled with or without hot words)
  double lm_sum = std::nan("");
  ResultEntity res;
};
// time_stamp_lfr6_onnx (OfflineRecognizer.cs:200-302); throws PF_ERR_RECOGNITION where the C#
// would throw inside Forward's try block.
TsList time_stamp_lfr6(const float* us_cif_peak, int n, const std::vector<int64_t>& tokens);

// The fields Recognizer::Forward writes into a stream (Stream derives from this)
struct StreamResult {
  std::vector<int64_t> Tokens{0, 0};                          // OfflineStream.cs:26
  TsList Timestamps;
  std::vector<float> Scores;                                  // of the last GetResults (Recognizer::SetDecode); empty without a flag
  // of the last GetResults (Recognizer::SetNBest); empty without it.  TokenAlternatives: AltK (id, log-prob) pairs per entry
  // of Tokens, [n_tokens, AltK], slots past a position's count -1 / -inf
  std::vector<int64_t> AltIds;
  std::vector<float> AltVal;
  int AltK = 0;
  std::vector<Alternative> Alternatives;
  // CTC forced alignment (Recognizer::SetAlign) of the last GetResults: [begin, end] ms per target id (flat), the token scores,
  // the Viterbi score, the log-likelihood, ok; AlignN = -1 when that GetResults aligned nothing for this stream
  std::vector<int32_t> AlignTs; std::vector<float> AlignTok;
  float AlignPath = 0.f; double AlignLoglik = 0.0; int AlignOk = 0, AlignN = -1;
};

// What a GetResults call knows before its forward runs (Recognizer::configure_engine)
struct ResultPlan {
  int dflags = 0;              // the engine's decode flags of this forward (PF_DECODE_*)
  bool sensevoice = false;
  int nbest = 0;               // SetNBest's N
  int ms_frame = 0;            // a frame = lfr_n x 10 ms
  bool want_scores = false;    // Scores = the arg-max log-probs (with PF_DECODE_CTC they are the collapsed tokens' instead)
  bool search_on = false;      // the n-best list comes from the device search (r.nbs), not from host_nbest
  bool hot_on = false;         // the beam search ran biased: r.beam_hot's matched / loglik
  bool lm_on = false;          // the beam search ran fused: r.beam_lm's lm_sum, r.beam_hot's loglik
  bool any_target = false;     // a stream of the batch has an align target: job 0 of every stream is its own
};

// [begin, end] ms of the frames first .. last of a SenseVoice row: the prompt rows in front carry no audio, so a run inside
// them gets {0, 0}
constexpr int kPromptRows = 4;
inline TsVec frame_ms(int ms_frame, int first, int last) {
  return {ms_frame * std::max(first - kPromptRows, 0), ms_frame * std::max(last + 1 - kPromptRows, 0)};
}

// Stream b of the forward whose results are r -> s (every field of StreamResult; Timestamps is appended to, as the
// reference does — RemoveChunk decides what stays).  A block the forward did not leave is empty: no CTC tokens, no
// hypotheses, no alignment jobs; without r.nbs (or with L == 0) the n-best list is the host enumeration's.
void build_stream_result(const HostBatchOut& r, const ResultPlan& p, int b, StreamResult& s);

}  // namespace pf
