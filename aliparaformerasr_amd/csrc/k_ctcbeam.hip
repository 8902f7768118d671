// k_ctcbeam.hip — CTC prefix beam search over the per-frame top-k lists (PF_DECODE_CTC_BEAM).
//
// The definition is tests/ctcbeam_ref.py, the host twin host_ctc_beam (hostutil.cpp).  Per utterance a beam of at most W
// entries (prefix, pb, pnb) in float64; per frame every entry proposes one "stay" candidate (index i*(K+1)) and one
// extension per listed non-blank id (index i*(K+1)+1+r); an extension whose prefix already sits in the beam is folded
// into that entry's stay candidate; the W best totals stay, ties to the smaller candidate index.
//
// One workgroup per utterance, the frame loop inside the kernel; 256 threads when the W*(K+1) <= 576 candidates fit, else
// 1024, so that a thread owns ONE candidate through a frame: its pb' / pnb' stay in registers, only the totals go to
// LDS, where every live candidate counts the candidates ordered before it ((total, index) is a total order, so that
// count is its slot in the new beam: no sort, no atomics).  With one wave per SIMD nothing hides an LDS read's latency,
// so the two scans over LDS (merge test, rank count) read one value per step and are unrolled: eight loads in flight.
// The beam is double-buffered in LDS; the next frame's list and blank log-prob are loaded before the current frame is
// worked on.
//
// A prefix is a chain of nodes (parent, token) in a global workspace; the node made for the extension that lands in
// slot r at frame t is 1 + t*W + r, so no counter is needed.  Node identity is NOT prefix identity: a prefix that left
// the beam and was made again hangs off a new node while a descendant of the old one may still be in the beam.  The
// merge test therefore compares token sequences: a 64-bit hash of the sequence is the filter, then both chains are
// walked until they meet in one node (the usual case: at once; chains of different length never meet).
//
// Hot words (kBias; the definition is tests/ctcbeam_bias_ref.py): a beam entry also carries its state in the
// hot-word automaton and the tokens m its prefix has matched.  An extension looks its (state, token) up in the table the host
// compiled (hostutil.cpp build_hotword_graph) — one read, issued before the merge scan and independent of it; a stay
// candidate inherits.  The select orders by key = total + boost * (m + pending depth) while pb / pnb stay unbiased, and after
// the last frame one more rank-by-count over (total + boost * m, beam rank) gives the output order.  The kBias = false form
// is the kernel as it was: every addition sits behind `if constexpr (kBias)`.
//
// Language model (kLm; the definition is tests/ctcbeam_lm_ref.py): a beam entry also carries its state in the
// back-off automaton lm.cpp compiled and g, the weighted LM score of its prefix.  An extension takes one step of lm_dev.h — a
// back-off walk with one bounded search of a sorted arc list per level — issued, like the hot-word read, before the merge scan;
// a stay candidate inherits.  g is one more term of the select key and of the final score, pb / pnb stay unfused, and the
// finish shares the biased form's rank-by-count pass.  The kLm = false forms are the kernel as it was.
#include <type_traits>

#include "kernels.h"
#include "lm_dev.h"

namespace pf {

namespace {

constexpr int kBeamW = PF_NBEST_MAX;                          // 64
constexpr int kBeamCand = kBeamW * (PF_TOPK_MAX + 1);         // 576
constexpr double kNegInf = -__builtin_huge_val();

struct BeamBuf {
  double pb[kBeamW], pnb[kBeamW];
  unsigned long long hash[kBeamW];
  int node[kBeamW], par[kBeamW], tok[kBeamW], len[kBeamW];
};

__device__ inline double beam_lse(double a, double b) {
  if (a == kNegInf) return b;
  if (b == kNegInf) return a;
  const double m = a > b ? a : b;
  return m + log1p(exp(-fabs(a - b)));
}

__device__ inline unsigned long long beam_hash(unsigned long long h, int c) {
  h = (h ^ ((unsigned long long)(unsigned)c + 0x9E3779B97F4A7C15ull)) * 0x100000001B3ull;
  return h ^ (h >> 29);
}

// the token sequences that end in nodes a and b (node 0 is the empty one): stepping back in lockstep, equal sequences meet
// in one node or spell the same tokens down to node 0 together
__device__ inline bool beam_same_prefix(const int32_t* npar, const int32_t* ntok, int a, int b) {
  while (a != b) {
    if (a <= 0 || b <= 0) return false;
    if (ntok[a] != ntok[b]) return false;
    a = npar[a];
    b = npar[b];
  }
  return true;
}

}  // namespace

// what the biased form reads and writes beyond the unbiased one; an empty argument in the kBias = false form
struct BeamHotArgs {
  const int32_t* tok_col;   // [V]: column of a hot-word token, -1 elsewhere
  const int32_t* table;     // [S, A]: next state | completed length << 16 | depth of the next state << 24
  int V, A;
  double boost;
  int32_t* out_matched;     // [B, N]
  double* out_loglik;       // [B, N]
};
struct BeamNoArgs {};
// the same for the language model: the image, the weights widened, whether finish takes the end-of-sentence step
struct BeamLmArgs {
  const int32_t* image;
  double alpha, beta;
  int eos;
  double* out_lm;           // [B, N]
  double* out_loglik;       // [B, N] (the biased form's own pointer when both are on)
};
struct BeamLmOnlyArgs { BeamLmArgs lm; };
struct BeamHotLmArgs : BeamHotArgs { BeamLmArgs lm; };
// what a candidate carries for the language model (its LM state and g), and the kernel's view of the image; empty without one
template <bool kLm> struct BeamLmCand { int ls = 0; double g = 0.0; };
template <> struct BeamLmCand<false> {};
template <bool kBias, bool kLm>
using BeamExtraArgs = std::conditional_t<kLm, std::conditional_t<kBias, BeamHotLmArgs, BeamLmOnlyArgs>, std::conditional_t<kBias, BeamHotArgs, BeamNoArgs>>;

template <int kBeamThreads, bool kBias, bool kLm>
__global__ __launch_bounds__(kBeamThreads) void ctc_beam_kernel(const float* blank_lp, int64_t blank_stride, const int64_t* ids,
                                                                const float* val, const int32_t* n, const int32_t* len, int T,
                                                                int K, int blank, int W, int N, int cap, int32_t* node_par,
                                                                int32_t* node_tok, int32_t* out_ids, int32_t* out_len,
                                                                double* out_score, int32_t* n_hyp,
                                                                BeamExtraArgs<kBias, kLm> hot) {
  __shared__ BeamBuf bm[2];
  __shared__ double c_tot[kBeamCand];
  __shared__ double m_val[kBeamW];                 // what the frame's merged extensions add to entry q's stay candidate
  __shared__ double f_val[2][PF_TOPK_MAX], f_lb[2];
  __shared__ int f_id[2][PF_TOPK_MAX], f_n[2];
  // kBias: per beam entry the automaton state (with its depth in the top byte, as the table packs it) and the matched tokens,
  // double-buffered like the beam; the output order of the final pass
  __shared__ int h_st[kBias ? 2 : 1][kBias ? kBeamW : 1], h_m[kBias ? 2 : 1][kBias ? kBeamW : 1], h_ord[kBias || kLm ? kBeamW : 1];
  // kLm: per beam entry the LM state and g of its prefix, double-buffered alike
  __shared__ int l_st[kLm ? 2 : 1][kLm ? kBeamW : 1];
  __shared__ double l_g[kLm ? 2 : 1][kLm ? kBeamW : 1];

  const int b = blockIdx.x, tid = threadIdx.x;
  const int nb = min(max(len[b], 0), T);
  const int64_t row0 = (int64_t)b * T;
  const int K1 = K + 1;
  int32_t* npar = node_par + (int64_t)b * ((int64_t)T * W + 1);
  int32_t* ntok = node_tok + (int64_t)b * ((int64_t)T * W + 1);
  [[maybe_unused]] std::conditional_t<kLm, LmView, BeamNoArgs> lv{};
  if constexpr (kLm) lv = lm_view(hot.lm.image);

  if (tid == 0) {
    bm[0].pb[0] = 0.0; bm[0].pnb[0] = kNegInf; bm[0].hash[0] = 0x243F6A8885A308D3ull;
    bm[0].node[0] = 0; bm[0].par[0] = -1; bm[0].tok[0] = -1; bm[0].len[0] = 0;
    npar[0] = -1; ntok[0] = -1;
    if constexpr (kBias) { h_st[0][0] = 0; h_m[0][0] = 0; }
    if constexpr (kLm) { l_st[0][0] = lv.start; l_g[0][0] = 0.0; }
  }
  if (tid < kBeamW) m_val[tid] = kNegInf;
  int n_nx = 0;                                    // n of frame t + 1, known one frame ahead so that its list can be prefetched
  if (nb > 0) {
    const int n0 = min(max(n[row0], 0), K);
    if (tid < n0) { f_id[0][tid] = (int)ids[row0 * K + tid]; f_val[0][tid] = (double)val[row0 * K + tid]; }
    if (tid == 0) { f_n[0] = n0; f_lb[0] = (double)blank_lp[row0 * blank_stride]; }
    if (nb > 1) n_nx = min(max(n[row0 + 1], 0), K);
  }
  __syncthreads();

  int nbeam = 1;
  bool bad = false;
  for (int t = 0; t < nb; ++t) {
    const int cur = t & 1, nxt = cur ^ 1;
    const BeamBuf& B0 = bm[cur];
    BeamBuf& B1 = bm[nxt];
    // frame t + 1's list and blank value, and frame t + 2's count
    int r_id = -1, n_nx2 = 0;
    double r_val = kNegInf, r_lb = 0.0;
    if (t + 1 < nb) {
      const int64_t row = row0 + t + 1;
      if (tid < n_nx) { r_id = (int)ids[row * K + tid]; r_val = (double)val[row * K + tid]; }
      if (tid == 0) r_lb = (double)blank_lp[row * blank_stride];
      if (t + 2 < nb) n_nx2 = min(max(n[row + 1], 0), K);
    }
    const int nt = f_n[cur];
    const double lb = f_lb[cur];
    if (nt == 0 || lb != lb) { bad = true; break; }             // wave- and block-uniform: both come from LDS

    const int NC = nbeam * K1;                     // <= kBeamThreads by the launcher's choice
    const int j = tid;
    const int i = j / K1, s = j - i * K1;
    // 1. the candidate; an extension that meets a beam entry leaves its value in m_val
    double pb1 = kNegInf, pnb1 = kNegInf;
    int st1 = 0, m1 = 0;                           // kBias: the candidate's automaton state and matched tokens
    [[maybe_unused]] BeamLmCand<kLm> lc;           // kLm: its LM state and g
    if (j < NC) {
      const double pb = B0.pb[i], pnb = B0.pnb[i];
      const double tot = beam_lse(pb, pnb);
      const int e = B0.tok[i], li = B0.len[i];
      if (s == 0) {
        pb1 = tot + lb;
        if constexpr (kBias) { st1 = h_st[cur][i]; m1 = h_m[cur][i]; }
        if constexpr (kLm) { lc.ls = l_st[cur][i]; lc.g = l_g[cur][i]; }
        if (li > 0)
          for (int r = 0; r < nt; ++r)
            if (f_id[cur][r] == e) pnb1 = pnb + f_val[cur][r];
      } else if (s - 1 < nt) {
        const int c = f_id[cur][s - 1];
        if (c != blank && c >= 0) {
          const double base = (li > 0 && c == e) ? pb : tot;
          if (base != kNegInf) {
            if constexpr (kBias) {                 // issued ahead of the scan below, which does not depend on it
              const int col = c < hot.V ? hot.tok_col[c] : -1;
              const int e = col >= 0 ? hot.table[(h_st[cur][i] & 0xFFFF) * hot.A + col] : 0;
              st1 = e & (int)0xFF00FFFF;
              m1 = h_m[cur][i] + ((e >> 16) & 0xFF);
            }
            if constexpr (kLm) {                   // the back-off walk, likewise independent of the scan
              lc.g = l_g[cur][i];
              lc.ls = lm_step(lv, l_st[cur][i], c, hot.lm.alpha, hot.lm.beta, true, lc.g);
            }
            const double value = base + f_val[cur][s - 1];
            const unsigned long long h = beam_hash(B0.hash[i], c);
            const int me = B0.node[i];
            // the scan itself is branch-free; the hash is only a filter, so a second entry with the same hash (never
            // seen) sends the thread through every entry
            int hit = -1, seen = 0, last = -1;
#pragma unroll 8
            for (int q = 0; q < nbeam; ++q) {
              const bool m = B0.hash[q] == h;
              last = m ? q : last;
              seen += m;
            }
            if (seen == 1) {
              if (B0.tok[last] == c && beam_same_prefix(npar, ntok, B0.par[last], me)) hit = last;
            } else if (seen > 1) {
              for (int q = 0; q < nbeam; ++q)
                if (B0.hash[q] == h && B0.tok[q] == c && beam_same_prefix(npar, ntok, B0.par[q], me)) hit = q;
            }
            if (hit >= 0) m_val[hit] = value;                    // at most one extension meets one entry
            else pnb1 = value;
          }
        }
      }
    }
    __syncthreads();
    // 2. totals
    double my = kNegInf, key = kNegInf;            // the unbiased total decides who lives, the key who ranks where
    if (j < NC) {
      if (s == 0) pnb1 = beam_lse(pnb1, m_val[i]);
      my = beam_lse(pb1, pnb1);
      if constexpr (kBias) key = my + hot.boost * (double)(m1 + (int)((unsigned)st1 >> 24));
      else key = my;
      if constexpr (kLm) key = key + lc.g;
      c_tot[j] = key;
    }
    __syncthreads();
    // 3. the slot of a candidate is the number of candidates ordered before it
    if (tid < kBeamW) m_val[tid] = kNegInf;
    int rank = 0, nlive = 0;
#pragma unroll 8
    for (int k = 0; k < NC; ++k) {
      const double tk = c_tot[k];
      nlive += tk > kNegInf;
      rank += (tk > key) || (tk == key && k < j);
    }
    if (j < NC && my > kNegInf && rank < W) {
      const int r = rank;
      B1.pb[r] = pb1; B1.pnb[r] = pnb1;
      if constexpr (kBias) { h_st[nxt][r] = st1; h_m[nxt][r] = m1; }
      if constexpr (kLm) { l_st[nxt][r] = lc.ls; l_g[nxt][r] = lc.g; }
      if (s == 0) {
        B1.hash[r] = B0.hash[i]; B1.node[r] = B0.node[i]; B1.par[r] = B0.par[i]; B1.tok[r] = B0.tok[i]; B1.len[r] = B0.len[i];
      } else {
        const int c = f_id[cur][s - 1];
        const int node = 1 + t * W + r;
        npar[node] = B0.node[i]; ntok[node] = c;
        B1.hash[r] = beam_hash(B0.hash[i], c); B1.node[r] = node; B1.par[r] = B0.node[i]; B1.tok[r] = c; B1.len[r] = B0.len[i] + 1;
      }
    }
    nbeam = min(W, nlive);
    if (t + 1 < nb) {
      if (tid < n_nx) { f_id[nxt][tid] = r_id; f_val[nxt][tid] = r_val; }
      if (tid == 0) { f_n[nxt] = n_nx; f_lb[nxt] = r_lb; }
    }
    n_nx = n_nx2;
    __syncthreads();
  }

  // the first N entries, ids by walking the chain back; every slot is written
  const BeamBuf& F = bm[nb & 1];
  const int nh = bad ? 0 : min(N, nbeam);
  int src = tid;                                   // the beam entry that output slot tid shows
  if constexpr (kBias || kLm) {
    // finish: score = total + boost * m (the pending part is revoked); a slot is again a count, over (score, beam rank)
    const int fb = nb & 1;
    double sc = kNegInf;
    if constexpr (!kLm) {
      if (tid < nbeam && !bad) sc = beam_lse(F.pb[tid], F.pnb[tid]) + hot.boost * (double)h_m[fb][tid];
    } else if (tid < nbeam && !bad) {              // + g_final: the end-of-sentence step where asked for; kept for the output
      sc = beam_lse(F.pb[tid], F.pnb[tid]);
      if constexpr (kBias) sc = sc + hot.boost * (double)h_m[fb][tid];
      double gf = l_g[fb][tid];
      if (hot.lm.eos && lv.eos >= 0) lm_step(lv, l_st[fb][tid], lv.eos, hot.lm.alpha, hot.lm.beta, false, gf);
      l_g[fb][tid] = gf;
      sc = sc + gf;
    }
    if (tid < kBeamW) c_tot[tid] = sc;
    __syncthreads();
    if (tid < nbeam && !bad) {
      int rank = 0;
      for (int q = 0; q < nbeam; ++q) {
        const double tq = c_tot[q];
        rank += (tq > sc) || (tq == sc && q < tid);
      }
      h_ord[rank] = tid;
    }
    __syncthreads();
    if (tid < nh) src = h_ord[tid];
  }
  if (tid < N) {
    const int64_t o = (int64_t)b * N + tid;
    if (tid < nh) {
      const int L = F.len[src];
      int node = F.node[src];
      for (int p = L - 1; p >= 0; --p) {
        if (p < cap) out_ids[o * cap + p] = ntok[node];
        node = npar[node];
      }
      out_len[o] = L;
      const double ll = beam_lse(F.pb[src], F.pnb[src]);
      if constexpr (kLm) {                          // score = (ll + boost * m) + g_final, as finish ranked it
        double sc = ll;
        if constexpr (kBias) {
          const int m = h_m[nb & 1][src];
          sc = ll + hot.boost * (double)m;
          hot.out_matched[o] = m;
        }
        const double gf = l_g[nb & 1][src];
        out_score[o] = sc + gf;
        hot.lm.out_lm[o] = gf;
        hot.lm.out_loglik[o] = ll;
      } else if constexpr (kBias) {
        const int m = h_m[nb & 1][src];
        out_score[o] = ll + hot.boost * (double)m;
        hot.out_matched[o] = m;
        hot.out_loglik[o] = ll;
      } else {
        out_score[o] = ll;
      }
    } else {
      out_len[o] = 0;
      out_score[o] = kNegInf;
      if constexpr (kLm) {
        if constexpr (kBias) hot.out_matched[o] = 0;
        hot.lm.out_lm[o] = 0.0;
        hot.lm.out_loglik[o] = kNegInf;
      } else if constexpr (kBias) { hot.out_matched[o] = 0; hot.out_loglik[o] = kNegInf; }
    }
  }
  for (int x = tid; x < N * cap; x += kBeamThreads) {
    const int h = x / cap, p = x - h * cap;
    int L = 0;
    if (h < nh) {
      if constexpr (kBias || kLm) L = F.len[h_ord[h]];
      else L = F.len[h];
    }
    if (p >= L) out_ids[(int64_t)b * N * cap + x] = -1;
  }
  if (tid == 0) n_hyp[b] = nh;
}

void launch_ctc_beam(hipStream_t s, const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val,
                     const int32_t* n, const int32_t* len, int B, int T, int K, int blank, int W, int N, int cap, int32_t* node_par,
                     int32_t* node_tok, int32_t* out_ids, int32_t* out_len, double* out_score, int32_t* n_hyp) {
  PF_CHECK(N >= 1 && N <= W && W <= kBeamW && K >= 1 && K <= PF_TOPK_MAX && T >= 0 && cap >= 0 && blank_stride >= 1,
           PF_ERR_INVALID_ARG, "ctc_beam: 1 <= N <= W <= 64, 1 <= K <= 8");
  if (B == 0) return;
  if (W * (K + 1) <= 256)
    hipLaunchKernelGGL((ctc_beam_kernel<256, false, false>), dim3((unsigned)B), dim3(256), 0, s, blank_lp, blank_stride, ids, val, n, len, T,
                       K, blank, W, N, cap, node_par, node_tok, out_ids, out_len, out_score, n_hyp, BeamNoArgs{});
  else
    hipLaunchKernelGGL((ctc_beam_kernel<1024, false, false>), dim3((unsigned)B), dim3(1024), 0, s, blank_lp, blank_stride, ids, val, n, len,
                       T, K, blank, W, N, cap, node_par, node_tok, out_ids, out_len, out_score, n_hyp, BeamNoArgs{});
  PF_HIP(hipGetLastError());
}

void launch_ctc_beam_hot(hipStream_t s, const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val,
                         const int32_t* n, const int32_t* len, int B, int T, int K, int blank, int W, int N, int cap,
                         int32_t* node_par, int32_t* node_tok, const int32_t* tok_col, int V, const int32_t* table, int A, float boost,
                         int32_t* out_ids, int32_t* out_len, double* out_score, int32_t* out_matched, double* out_loglik,
                         int32_t* n_hyp) {
  PF_CHECK(N >= 1 && N <= W && W <= kBeamW && K >= 1 && K <= PF_TOPK_MAX && T >= 0 && cap >= 0 && blank_stride >= 1,
           PF_ERR_INVALID_ARG, "ctc_beam: 1 <= N <= W <= 64, 1 <= K <= 8");
  PF_CHECK(tok_col && table && V >= 1 && A >= 1 && boost > 0.f && boost <= 3.4028234e38f, PF_ERR_INVALID_ARG,
           "ctc_beam_hot: a compiled hot-word table and a finite boost > 0");
  if (B == 0) return;
  const BeamHotArgs hot{tok_col, table, V, A, (double)boost, out_matched, out_loglik};
  if (W * (K + 1) <= 256)
    hipLaunchKernelGGL((ctc_beam_kernel<256, true, false>), dim3((unsigned)B), dim3(256), 0, s, blank_lp, blank_stride, ids, val, n, len, T,
                       K, blank, W, N, cap, node_par, node_tok, out_ids, out_len, out_score, n_hyp, hot);
  else
    hipLaunchKernelGGL((ctc_beam_kernel<1024, true, false>), dim3((unsigned)B), dim3(1024), 0, s, blank_lp, blank_stride, ids, val, n, len,
                       T, K, blank, W, N, cap, node_par, node_tok, out_ids, out_len, out_score, n_hyp, hot);
  PF_HIP(hipGetLastError());
}

// the fused forms: the language model alone (tok_col == nullptr) or together with a hot-word set
void launch_ctc_beam_lm(hipStream_t s, const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val,
                        const int32_t* n, const int32_t* len, int B, int T, int K, int blank, int W, int N, int cap, int32_t* node_par,
                        int32_t* node_tok, const int32_t* tok_col, int V, const int32_t* table, int A, float boost,
                        const int32_t* lm_image, float alpha, float beta, int lm_flags, int32_t* out_ids, int32_t* out_len,
                        double* out_score, int32_t* out_matched, double* out_loglik, double* out_lm, int32_t* n_hyp) {
  PF_CHECK(N >= 1 && N <= W && W <= kBeamW && K >= 1 && K <= PF_TOPK_MAX && T >= 0 && cap >= 0 && blank_stride >= 1,
           PF_ERR_INVALID_ARG, "ctc_beam: 1 <= N <= W <= 64, 1 <= K <= 8");
  PF_CHECK(lm_image && out_lm && out_loglik && alpha >= 0.f && alpha <= 3.4028234e38f && beta >= -3.4028234e38f && beta <= 3.4028234e38f,
           PF_ERR_INVALID_ARG, "ctc_beam_lm: a compiled model, alpha finite and >= 0, beta finite");
  if (B == 0) return;
  const BeamLmArgs lm{lm_image, (double)alpha, (double)beta, (lm_flags & PF_LM_EOS) != 0, out_lm, out_loglik};
  const bool big = W * (K + 1) > 256;
  if (tok_col) {
    PF_CHECK(table && out_matched && V >= 1 && A >= 1 && boost > 0.f && boost <= 3.4028234e38f, PF_ERR_INVALID_ARG,
             "ctc_beam_hot: a compiled hot-word table and a finite boost > 0");
    BeamHotLmArgs x;
    (BeamHotArgs&)x = BeamHotArgs{tok_col, table, V, A, (double)boost, out_matched, out_loglik};
    x.lm = lm;
    if (!big)
      hipLaunchKernelGGL((ctc_beam_kernel<256, true, true>), dim3((unsigned)B), dim3(256), 0, s, blank_lp, blank_stride, ids, val, n, len,
                         T, K, blank, W, N, cap, node_par, node_tok, out_ids, out_len, out_score, n_hyp, x);
    else
      hipLaunchKernelGGL((ctc_beam_kernel<1024, true, true>), dim3((unsigned)B), dim3(1024), 0, s, blank_lp, blank_stride, ids, val, n,
                         len, T, K, blank, W, N, cap, node_par, node_tok, out_ids, out_len, out_score, n_hyp, x);
  } else {
    const BeamLmOnlyArgs x{lm};
    if (!big)
      hipLaunchKernelGGL((ctc_beam_kernel<256, false, true>), dim3((unsigned)B), dim3(256), 0, s, blank_lp, blank_stride, ids, val, n, len,
                         T, K, blank, W, N, cap, node_par, node_tok, out_ids, out_len, out_score, n_hyp, x);
    else
      hipLaunchKernelGGL((ctc_beam_kernel<1024, false, true>), dim3((unsigned)B), dim3(1024), 0, s, blank_lp, blank_stride, ids, val, n,
                         len, T, K, blank, W, N, cap, node_par, node_tok, out_ids, out_len, out_score, n_hyp, x);
  }
  PF_HIP(hipGetLastError());
}

}  // namespace pf
