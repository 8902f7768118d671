// stream_result.cpp — see stream_result.h.
#include "stream_result.h"

#include <array>
#include <cstring>

#include "hostutil.h"

namespace pf {

TsList time_stamp_lfr6(const float* us_cif_peak, int n, const std::vector<int64_t>& tokens_in) {
  // float32 arithmetic throughout, (int)(t*1000) truncation (quirk Q10)
  const int START_END_THRESHOLD = 5, MAX_TOKEN_DURATION = 30;
  volatile float tr0 = 10.0f * 6;
  volatile float tr1 = tr0 / 1000;
  const float TIME_RATE = tr1 / 3;
  const float total_offset = -1.5f;
  const int num_frames = n;
  if (tokens_in.empty()) throw Error(PF_ERR_RECOGNITION, "Sequence contains no elements");   // tokens.Last()
  std::vector<int64_t> tokens(tokens_in);
  if (tokens.back() == 2) tokens.pop_back();
  std::vector<float> fire;
  for (int i = 0; i < n; ++i)
    if ((double)us_cif_peak[i] > (double)1.0f - 1e-4) fire.push_back((float)i + total_offset);
  if (fire.empty()) throw Error(PF_ERR_RECOGNITION, "Index was out of range (no CIF fire)");   // fire_place[0]
  std::vector<std::array<float, 2>> tl;
  std::vector<bool> nc;
  if (fire[0] > (float)START_END_THRESHOLD) {
    tl.push_back({0.0f, fire[0] * TIME_RATE});
    nc.push_back(false);
  }
  const int nf = (int)fire.size();
  for (int i = 0; i < nf - 1; ++i) {
    if (i >= (int)tokens.size()) throw Error(PF_ERR_RECOGNITION, "Index was outside the bounds of the array");
    nc.push_back(tokens[i] != 1);
    if (i == nf - 2 || MAX_TOKEN_DURATION < 0 || fire[i + 1] - fire[i] < (float)MAX_TOKEN_DURATION) {
      tl.push_back({fire[i] * TIME_RATE, fire[i + 1] * TIME_RATE});
    } else {
      const float split = fire[i] + (float)MAX_TOKEN_DURATION;
      tl.push_back({fire[i] * TIME_RATE, split * TIME_RATE});
      tl.push_back({split * TIME_RATE, fire[i + 1] * TIME_RATE});
      nc.push_back(false);
    }
  }
  if ((float)num_frames - fire.back() > (float)START_END_THRESHOLD) {
    const float end = ((float)num_frames + fire.back()) / 2;
    if (tl.empty()) throw Error(PF_ERR_RECOGNITION, "Sequence contains no elements");
    tl.back()[1] = end * TIME_RATE;
    tl.push_back({end * TIME_RATE, (float)num_frames * TIME_RATE});
    nc.push_back(false);
  } else {
    if (tl.empty()) throw Error(PF_ERR_RECOGNITION, "Sequence contains no elements");
    tl.back()[1] = (float)num_frames * TIME_RATE;
  }
  nc.push_back(true);
  TsList out;
  const size_t m = std::min(nc.size(), tl.size());
  for (size_t i = 0; i < m; ++i) {
    if (!nc[i]) continue;
    volatile float a = tl[i][0] * 1000, b = tl[i][1] * 1000;
    out.push_back({(int32_t)a, (int32_t)b});
  }
  return out;
}

// [begin, end] ms of `len` aligned tokens, flat (2 per token)
static void append_frame_ms(std::vector<int32_t>& out, int ms_frame, const int32_t* first, const int32_t* last, int len) {
  for (int k = 0; k < len; ++k) {
    const TsVec t = frame_ms(ms_frame, first[k], last[k]);
    out.insert(out.end(), t.begin(), t.end());
  }
}

void build_stream_result(const HostBatchOut& r, const ResultPlan& p, int b, StreamResult& s) {
  const int L = r.L, P = r.peak_len, dflags = p.dflags;
  const size_t r0 = (size_t)b * L;                                 // the stream's first row of [B, L]
  // the collapsed hypothesis (PF_DECODE_CTC): n tokens at row b of the block
  const bool ctc = (dflags & PF_DECODE_CTC) != 0;
  const CtcBlock cb = r.ctc_block();
  const bool have_ctc = ctc && !r.ctc.empty();
  const size_t co = (size_t)b * r.ctc_cap;
  const int64_t* c_ids = have_ctc ? cb.ids(r.ctc.data()) + co : nullptr;
  const int32_t* c_first = have_ctc ? cb.first(r.ctc.data()) + co : nullptr;
  const int32_t* c_last = have_ctc ? cb.last(r.ctc.data()) + co : nullptr;
  const float* c_score = have_ctc ? cb.score(r.ctc.data()) + co : nullptr;
  const int c_n = have_ctc ? cb.n(r.ctc.data())[b] : 0;

  s.Tokens.assign(r.ids.begin() + r0, r.ids.begin() + r0 + L);                                       // :187
  s.Scores.clear();
  if (p.want_scores) s.Scores.assign(r.scores.begin() + r0, r.scores.begin() + r0 + L);
  s.Timestamps.reserve(s.Timestamps.size() + (size_t)L);
  if (ctc) {
    // the collapsed hypothesis instead of the per-frame ids: one [begin, end] pair per token from its first / last frame
    s.Tokens.assign(c_ids, c_ids + c_n);
    s.Scores.assign(c_score, c_score + c_n);
    for (int k = 0; k < c_n; ++k) s.Timestamps.push_back(frame_ms(p.ms_frame, c_first[k], c_last[k]));
  } else if (P > 0) {
    // :172-183: the peak row and ALL L arg-max ids go to time_stamp_lfr6_onnx
    TsList ts = time_stamp_lfr6(r.cif_peak.data() + (size_t)b * P, P, s.Tokens);
    for (auto& t2 : ts) s.Timestamps.push_back(t2);
  } else {
    for (int l = 0; l < L; ++l) s.Timestamps.push_back({0, 0});                                      // :151,:188
  }

  s.AltIds.clear(); s.AltVal.clear(); s.AltK = 0; s.Alternatives.clear();
  const int K = (dflags & PF_DECODE_TOPK) ? r.topk_k : 0;
  if (K > 0 && L > 0) {
    const TopkBlock tb = r.topk_block();
    const int64_t* k_ids = tb.ids(r.topk.data()) + r0 * K;        // the stream's lists [L, K]
    const float* k_val = tb.val(r.topk.data()) + r0 * K;
    s.AltK = K;
    if (ctc) {
      // per collapsed token: the alternatives of the run's peak frame — the first frame whose log-prob is the token's
      // score bit for bit
      const float* sc = r.scores.data() + r0;
      for (int k = 0; k < c_n; ++k) {
        int t = c_first[k];
        for (int u = c_first[k]; u <= c_last[k]; ++u)
          if (std::memcmp(&sc[u], &c_score[k], 4) == 0) { t = u; break; }
        s.AltIds.insert(s.AltIds.end(), k_ids + (size_t)t * K, k_ids + (size_t)(t + 1) * K);
        s.AltVal.insert(s.AltVal.end(), k_val + (size_t)t * K, k_val + (size_t)(t + 1) * K);
      }
    } else {
      s.AltIds.assign(k_ids, k_ids + (size_t)L * K);
      s.AltVal.assign(k_val, k_val + (size_t)L * K);
    }
    if (p.nbest > 1 && !p.sensevoice) {
      // the n-best list: rank vectors over the top-k lists, from the device search (its fused order) or the host enumeration
      const int Ns = (p.search_on && !r.nbs.empty()) ? r.nbs_n : 0;
      std::vector<int32_t> h_ranks;
      std::vector<double> h_score;
      const int32_t* ranks;
      int got;
      const NbestSearchBlock nb = r.nbs_block();
      const size_t x0 = (size_t)b * Ns;
      if (Ns > 0) {
        got = nb.n_hyp(r.nbs.data())[b];
        ranks = nb.ranks(r.nbs.data()) + x0 * L;
      } else {
        h_ranks.resize((size_t)p.nbest * L); h_score.resize((size_t)p.nbest);
        const int n_free = std::min(L, std::max(r.token_num[(size_t)b], 0));   // the list varies only below an utterance's own count
        got = host_nbest(k_val, tb.n(r.topk.data()) + r0, L, K, n_free, p.nbest, h_ranks.data(), h_score.data());
        ranks = h_ranks.data();
      }
      s.Alternatives.resize((size_t)got);
      for (int i = 0; i < got; ++i) {
        Alternative& a = s.Alternatives[(size_t)i];
        if (Ns > 0) {
          const void* q = r.nbs.data();
          a.score = nb.score(q)[x0 + i]; a.loglik_sum = nb.loglik(q)[x0 + i]; a.lm_sum = nb.lm_sum(q)[x0 + i]; a.hot_tokens = nb.matched(q)[x0 + i];
        } else {
          a.score = h_score[(size_t)i];
        }
        a.ids.resize((size_t)L);
        for (int l = 0; l < L; ++l) a.ids[(size_t)l] = k_ids[(size_t)l * K + ranks[(size_t)i * L + l]];
      }
    }
  }

  // forced alignments (PF_DECODE_ALIGN): job 0 is the stream's own target when any stream of the batch has one, then the
  // beam's hypotheses
  const int H = ((dflags & PF_DECODE_ALIGN) && !r.align.empty()) ? r.align_h : 0;
  const int a_hc = (H > 0 && p.any_target) ? 1 : 0;
  const AlignBlock ab = r.align_block();
  const void* ap = r.align.data();
  const size_t a_cap = (size_t)r.align_cap;

  // the beam search's labelings (PF_DECODE_CTC_BEAM) behind whatever the top-k branch listed.  (The forward that leaves
  // r.beam also leaves r.beam_hot when it ran biased or fused and r.beam_lm when it ran fused: Engine::queue_ctc_beam.)
  const bool have_beam = (dflags & PF_DECODE_CTC_BEAM) && !r.beam.empty();
  const int Nb = have_beam ? r.beam_n : 0;
  const BeamBlock bb = r.beam_block();
  const BeamHotBlock hb = r.beam_hot_block();
  const BeamLmBlock lb = r.beam_lm_block();
  for (int i = 0; i < (Nb > 0 ? bb.n_hyp(r.beam.data())[b] : 0); ++i) {
    const size_t x = (size_t)b * Nb + i;
    const int b_len = bb.len(r.beam.data())[x];
    const int32_t* b_ids = bb.ids(r.beam.data()) + x * r.beam_cap;
    Alternative a;
    a.score = bb.score(r.beam.data())[x];
    a.ctc = true;
    if (p.hot_on) { a.hot_tokens = hb.matched(r.beam_hot.data())[x]; a.loglik_sum = hb.loglik(r.beam_hot.data())[x]; }
    if (p.lm_on) { a.lm_sum = lb.lm_sum(r.beam_lm.data())[x]; a.loglik_sum = hb.loglik(r.beam_hot.data())[x]; }
    a.ids.assign(b_ids, b_ids + b_len);
    if (H >= a_hc + Nb) {
      const size_t j = (size_t)b * H + a_hc + i;
      a.loglik = ab.loglik(ap)[j];
      if (ab.ok(ap)[j] && ab.len(ap)[j] == b_len) append_frame_ms(a.ts, p.ms_frame, ab.first(ap) + j * a_cap, ab.last(ap) + j * a_cap, b_len);
    }
    s.Alternatives.push_back(std::move(a));
  }

  s.AlignTs.clear(); s.AlignTok.clear(); s.AlignPath = 0.f; s.AlignLoglik = 0.0; s.AlignOk = 0; s.AlignN = -1;
  if (a_hc && ab.len(ap)[(size_t)b * H] >= 0) {
    const size_t j = (size_t)b * H;
    const int n = ab.len(ap)[j];
    s.AlignN = n; s.AlignOk = ab.ok(ap)[j]; s.AlignPath = ab.path(ap)[j]; s.AlignLoglik = ab.loglik(ap)[j];
    if (s.AlignOk) {
      append_frame_ms(s.AlignTs, p.ms_frame, ab.first(ap) + j * a_cap, ab.last(ap) + j * a_cap, n);
      s.AlignTok.assign(ab.tok(ap) + j * a_cap, ab.tok(ap) + j * a_cap + n);
    }
  }
}

}  // namespace pf
