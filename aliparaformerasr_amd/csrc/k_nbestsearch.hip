// k_nbestsearch.hip — position-synchronous beam search over paraformer's per-position top-k lists, with optional hot-word and
// n-gram LM shallow fusion (paraformer_hip.h "N-best search").
//
// The definition is tests/nbest_search_ref.py, the host twin host_nbest_search (hostutil.cpp).  Per utterance a beam of at most
// W entries (a, g, LM state, hot-word state, m) in float64; at a free position l every entry i proposes one candidate per
// listed rank r < n[l]: a' = a + val[l, r], one lm_step and one hot-word table read on ids[l, r], key = (a' + boost * (m' + d'))
// + g'.  No candidate is discarded and none is merged (the ids of a list are distinct, so distinct candidates spell distinct
// sequences); the W best by key stay, ties to the smaller candidate index.
//
// One workgroup per utterance, the position loop inside the kernel; 256 threads when W * K <= 256, else 512, so that a thread
// owns ONE candidate through a position.  Candidates are numbered i * n[l] + r — the order of i * K + r without its holes — so
// that every slot below nbeam * n[l] is live and -inf needs no second meaning.  The LM walk and the table read are issued first,
// the key goes to LDS, and every candidate counts the candidates ordered before it: (key, index) is a total order, so the count
// is its slot in the new beam — no sort, no atomics (the scheme of k_ctcbeam.hip).  The beam is double-buffered in LDS; a
// survivor writes the other buffer and one back-pointer (parent slot << 8 | r) per (l, slot) into a global workspace [B, L, W].
// The next position's list is loaded before the current one is worked on.  The positions at and past n_free take rank 0: a
// running add per entry that the LM and the hot words do not see.  Finish: the end-of-sentence step where asked for, one more
// rank-by-count over (score, beam rank), then N threads walk their chains back and write ranks[b, i, 0 .. L).
//
// Arithmetic: alpha * x and boost * integer are exact products of widened floats, every + one rounded float64 addition in the
// definition's order (a fused multiply-add of an exact product rounds the same), nothing transcendental: kernel, twin and
// definition agree bit for bit, ties included.  The kBias = false / kLm = false forms leave the additions out behind
// `if constexpr`.
#include <type_traits>

#include "kernels.h"
#include "lm_dev.h"

namespace pf {

namespace {

constexpr int kNbW = PF_NBEST_MAX;                            // 64
constexpr int kNbCand = kNbW * PF_TOPK_MAX;                   // 512
constexpr double kNbNegInf = -__builtin_huge_val();

struct NbNoView {};

template <int kThreads, bool kBias, bool kLm>
__global__ __launch_bounds__(kThreads) void nbest_search_kernel(NbestSearchArgs p) {
  __shared__ double b_a[2][kNbW];                  // the beam: the acoustic sum of the entry's ranks so far
  __shared__ double c_key[kNbCand];
  __shared__ double f_val[2][PF_TOPK_MAX];
  __shared__ int f_id[2][PF_TOPK_MAX];
  __shared__ int h_ord[kNbW];
  __shared__ int s_bad;
  // kBias: per entry the automaton state (with its depth in the top byte, as the table packs it) and the matched tokens
  __shared__ int h_st[kBias ? 2 : 1][kBias ? kNbW : 1], h_m[kBias ? 2 : 1][kBias ? kNbW : 1];
  // kLm: per entry the LM state and g of its sequence
  __shared__ int l_st[kLm ? 2 : 1][kLm ? kNbW : 1];
  __shared__ double l_g[kLm ? 2 : 1][kLm ? kNbW : 1];

  const int b = blockIdx.x, tid = threadIdx.x;
  const int L = p.L, K = p.K, W = p.W, N = p.N;
  const int n_free = min(L, max(p.token_num[b], 0));
  const int64_t row0 = (int64_t)b * L;
  int32_t* bp = p.bp + row0 * W;
  [[maybe_unused]] std::conditional_t<kLm, LmView, NbNoView> lv{};
  if constexpr (kLm) lv = lm_view(p.lm_image);

  if (tid == 0) {
    s_bad = 0;
    b_a[0][0] = 0.0;
    if constexpr (kBias) { h_st[0][0] = 0; h_m[0][0] = 0; }
    if constexpr (kLm) { l_st[0][0] = lv.start; l_g[0][0] = 0.0; }
  }
  __syncthreads();
  // no hypothesis exists when a position lists nothing or a listed value is NaN or +inf (their sums would not order)
  {
    bool bad = L == 0;
    for (int x = tid; x < L * K; x += kThreads) {
      const int l = x / K, r = x - l * K;
      const int nl = min(max(p.n[row0 + l], 0), K);
      if (r == 0 && nl == 0) bad = true;
      if (r < nl) {
        const float v = p.val[(row0 + l) * K + r];
        if (v != v || v == __builtin_huge_valf()) bad = true;
      }
    }
    if (bad) s_bad = 1;                            // (every writer stores the same value)
  }
  int n_cur = 0, n_nx = 0;                         // n of position l and l + 1: known ahead so that the lists can be prefetched
  if (n_free > 0) {
    n_cur = min(max(p.n[row0], 0), K);
    if (tid < n_cur) { f_id[0][tid] = (int)p.ids[row0 * K + tid]; f_val[0][tid] = (double)p.val[row0 * K + tid]; }
    if (n_free > 1) n_nx = min(max(p.n[row0 + 1], 0), K);
  }
  __syncthreads();
  const bool bad = s_bad != 0;

  int nbeam = 1;
  if (!bad) {
    for (int l = 0; l < n_free; ++l) {
      const int cur = l & 1, nxt = cur ^ 1;
      // position l + 1's list, and position l + 2's count
      int r_id = -1, n_nx2 = 0;
      double r_val = kNbNegInf;
      if (l + 1 < n_free) {
        const int64_t row = row0 + l + 1;
        if (tid < n_nx) { r_id = (int)p.ids[row * K + tid]; r_val = (double)p.val[row * K + tid]; }
        if (l + 2 < n_free) n_nx2 = min(max(p.n[row + 1], 0), K);
      }
      const int nl = n_cur;                        // >= 1: the scan above found no empty position
      const int NC = nbeam * nl;                   // <= W * K <= kThreads by the launcher's choice
      const int j = tid;
      const int i = j / nl, r = j - i * nl;
      double a1 = 0.0, key = 0.0;
      [[maybe_unused]] int st1 = 0, m1 = 0, ls1 = 0;
      [[maybe_unused]] double g1 = 0.0;
      if (j < NC) {
        const int c = f_id[cur][r];
        if constexpr (kLm) {                       // the back-off walk and the table read first: the longest latencies
          g1 = l_g[cur][i];
          ls1 = lm_step(lv, l_st[cur][i], c, p.alpha, p.beta, true, g1);
        }
        if constexpr (kBias) {
          const int col = c >= 0 && c < p.V ? p.tok_col[c] : -1;
          const int e = col >= 0 ? p.table[(h_st[cur][i] & 0xFFFF) * p.A + col] : 0;
          st1 = e & (int)0xFF00FFFF;
          m1 = h_m[cur][i] + ((e >> 16) & 0xFF);
        }
        a1 = b_a[cur][i] + f_val[cur][r];
        key = a1;
        if constexpr (kBias) key = key + p.boost * (double)(m1 + (int)((unsigned)st1 >> 24));
        if constexpr (kLm) key = key + g1;
        c_key[j] = key;
      }
      __syncthreads();
      // the slot of a candidate is the number of candidates ordered before it
      if (j < NC) {
        int rank = 0;
#pragma unroll 8
        for (int k = 0; k < NC; ++k) {
          const double tk = c_key[k];
          rank += (tk > key) || (tk == key && k < j);
        }
        if (rank < W) {
          b_a[nxt][rank] = a1;
          if constexpr (kBias) { h_st[nxt][rank] = st1; h_m[nxt][rank] = m1; }
          if constexpr (kLm) { l_st[nxt][rank] = ls1; l_g[nxt][rank] = g1; }
          bp[(int64_t)l * W + rank] = (i << 8) | r;
        }
      }
      nbeam = min(W, NC);
      if (l + 1 < n_free && tid < n_nx) { f_id[nxt][tid] = r_id; f_val[nxt][tid] = r_val; }
      n_cur = n_nx;
      n_nx = n_nx2;
      __syncthreads();
    }
  }

  // the tail and the finish: thread tid is beam entry tid
  const int fb = n_free & 1;
  const int nh = bad ? 0 : min(N, nbeam);
  double a = 0.0, sc = kNbNegInf;
  [[maybe_unused]] double gf = 0.0;
  if (tid < nbeam && !bad) {
    a = b_a[fb][tid];
    for (int l = n_free; l < L; ++l) a = a + (double)p.val[(row0 + l) * K];
    sc = a;
    if constexpr (kBias) sc = sc + p.boost * (double)h_m[fb][tid];
    if constexpr (kLm) {
      gf = l_g[fb][tid];
      if (p.lm_eos && lv.eos >= 0) lm_step(lv, l_st[fb][tid], lv.eos, p.alpha, p.beta, false, gf);
      l_g[fb][tid] = gf;
      sc = sc + gf;
    }
    b_a[fb][tid] = a;
    c_key[tid] = sc;
  }
  __syncthreads();
  if (tid < nbeam && !bad) {
    int rank = 0;
    for (int q = 0; q < nbeam; ++q) {
      const double tq = c_key[q];
      rank += (tq > sc) || (tq == sc && q < tid);
    }
    h_ord[rank] = tid;
  }
  __syncthreads();
  if (tid < N) {
    const int64_t o = (int64_t)b * N + tid;
    int32_t* ranks = p.out_ranks + o * L;
    if (tid < nh) {
      int slot = h_ord[tid];
      p.out_score[o] = c_key[slot];
      p.out_loglik[o] = b_a[fb][slot];
      if constexpr (kLm) p.out_lm[o] = l_g[fb][slot];
      else p.out_lm[o] = 0.0;
      if constexpr (kBias) p.out_matched[o] = h_m[fb][slot];
      else p.out_matched[o] = 0;
      for (int l = L - 1; l >= n_free; --l) ranks[l] = 0;
      for (int l = n_free - 1; l >= 0; --l) {
        const int v = bp[(int64_t)l * W + slot];
        ranks[l] = v & 0xFF;
        slot = v >> 8;
      }
    } else {
      p.out_score[o] = kNbNegInf;
      p.out_loglik[o] = kNbNegInf;
      p.out_lm[o] = 0.0;
      p.out_matched[o] = 0;
      for (int l = 0; l < L; ++l) ranks[l] = -1;
    }
  }
  if (tid == 0) p.n_hyp[b] = nh;
}

template <bool kBias, bool kLm>
void nbest_search_launch(hipStream_t s, const NbestSearchArgs& a, int B) {
  if (a.W * a.K <= 256) hipLaunchKernelGGL((nbest_search_kernel<256, kBias, kLm>), dim3((unsigned)B), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((nbest_search_kernel<512, kBias, kLm>), dim3((unsigned)B), dim3(512), 0, s, a);
}

}  // namespace

void launch_nbest_search(hipStream_t s, const NbestSearchArgs& a, int B) {
  PF_CHECK(a.N >= 1 && a.N <= a.W && a.W <= kNbW && a.K >= 1 && a.K <= PF_TOPK_MAX && a.L >= 0 && B >= 0, PF_ERR_INVALID_ARG,
           "nbest_search: 1 <= N <= W <= 64, 1 <= K <= 8");
  PF_CHECK(a.token_num && a.out_ranks && a.out_score && a.out_loglik && a.out_lm && a.out_matched && a.n_hyp && (a.L == 0 || a.bp),
           PF_ERR_INVALID_ARG, "nbest_search: null argument");
  const bool bias = a.tok_col != nullptr, lm = a.lm_image != nullptr;
  if (bias)
    PF_CHECK(a.table && a.V >= 1 && a.A >= 1 && a.boost > 0.0 && a.boost <= 3.4028234663852886e38, PF_ERR_INVALID_ARG,
             "nbest_search: a compiled hot-word table and a finite boost > 0");
  if (lm)
    PF_CHECK(a.alpha >= 0.0 && a.alpha <= 3.4028234663852886e38 && a.beta >= -3.4028234663852886e38 && a.beta <= 3.4028234663852886e38,
             PF_ERR_INVALID_ARG, "nbest_search: alpha finite and >= 0, beta finite");
  if (B == 0) return;
  if (lm) {
    if (bias) nbest_search_launch<true, true>(s, a, B);
    else nbest_search_launch<false, true>(s, a, B);
  } else {
    if (bias) nbest_search_launch<true, false>(s, a, B);
    else nbest_search_launch<false, false>(s, a, B);
  }
  PF_HIP(hipGetLastError());
}

}  // namespace pf
