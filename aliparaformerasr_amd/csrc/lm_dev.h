// lm_dev.h — one step of the back-off n-gram LM over the image lm.cpp compiles (paraformer_hip.h "CTC language model"; the
// definition is tests/ctcbeam_lm_ref.py).  The layout is private to lm.cpp, the host twin and the two kernels that include
// this header (k_lm.hip, k_ctcbeam.hip); host and device run the same text.
//
// The image is a run of 16-byte aligned sections behind a header of kLmHdrWords int32 words:
//   uni [V + 1] LmUni   the dense lookup of the empty context (state 0).  tok > 0: the id the token is scored as (itself, or
//                       the model's unk for an id that is no listed unigram), logp / next of that unigram; tok == kLmOov: no
//                       listed unigram and no unk; tok == kLmTransparent: the token is skipped.  Entry V stands for every id
//                       outside [0, V)
//   state [S]  LmState  every other context: its arcs key[begin .. begin + count), sorted by token; the state it backs off to
//                       (the longest proper suffix that is a state: always a shorter context, so a walk ends after at most
//                       order - 1 levels) and the weight (+0 for a context listed without one, or not listed at all: g + 0 is g)
//   key   [A]  int32    the arcs' tokens, one sorted run per state
//   arc   [A]  LmArc    logp of context + token, and the state the search is in afterwards: the longest suffix of
//                       context + token that is a listed n-gram of order < O, worked out by the builder
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PF_LM_FN __host__ __device__ inline
#else
#define PF_LM_FN inline
#endif

#ifndef PF_LM_ORDER_MAX
#define PF_LM_ORDER_MAX 8
#endif

namespace pf {

constexpr int32_t kLmMagic = 0x314D4C50;
constexpr int32_t kLmOov = -1, kLmTransparent = -2;
enum { kLmHdrMagic = 0, kLmHdrOrder, kLmHdrV, kLmHdrStates, kLmHdrArcs, kLmHdrStart, kLmHdrEos, kLmHdrOovBits, kLmHdrUni, kLmHdrState,
       kLmHdrKey, kLmHdrArc, kLmHdrWords = 16 };   // the four section offsets count int32 words

struct alignas(16) LmUni { int32_t tok; float logp; int32_t next, pad; };
struct alignas(16) LmState { int32_t begin, count, bo_state; float bo; };
struct alignas(8) LmArc { float logp; int32_t next; };

struct LmView {
  const LmUni* uni;
  const LmState* st;
  const int32_t* key;
  const LmArc* arc;
  int V, start, eos;
  double oov;
};

PF_LM_FN LmView lm_view(const int32_t* img) {
  LmView v;
  v.uni = (const LmUni*)(img + img[kLmHdrUni]);
  v.st = (const LmState*)(img + img[kLmHdrState]);
  v.key = img + img[kLmHdrKey];
  v.arc = (const LmArc*)(img + img[kLmHdrArc]);
  v.V = img[kLmHdrV];
  v.start = img[kLmHdrStart];
  v.eos = img[kLmHdrEos];
  v.oov = (double)__builtin_bit_cast(float, img[kLmHdrOovBits]);
  return v;
}

// the place of `tok` in the sorted run key[lo .. lo + n), or -1.  An 8-ary search: the seven pivots of a level are independent
// loads, so a run of 25 000 arcs costs four dependent trips to memory and one last look at no more than eight neighbours.
PF_LM_FN int lm_find(const int32_t* key, int lo, int n, int tok) {
  while (n > 8) {
    int cnt = 0;                                   // pivots p_k = n * k / 8; the keys ascend, so key[p_k] <= tok holds for k <= cnt
#pragma unroll
    for (int k = 1; k < 8; ++k) cnt += key[lo + (int)(((unsigned)n * (unsigned)k) >> 3)] <= tok;
    const int a = (int)(((unsigned)n * (unsigned)cnt) >> 3), b = (int)(((unsigned)n * (unsigned)(cnt + 1)) >> 3);
    lo += a;
    n = b - a;                                     // <= n / 8 + 1 < n
  }
  int hit = -1;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (k < n && key[lo + k] == tok) hit = lo + k;
  return hit;
}

// One token of the definition: g takes the alpha-weighted back-offs and the log-probability in the walk's order, then the
// bonus; returns the next state.  alpha * x is the exact product of two widened floats, every + one float64 addition, so a
// fused multiply-add rounds alike.  bonus = false is the end-of-sentence step.
PF_LM_FN int lm_step(const LmView& v, int state, int c, double alpha, double beta, bool bonus, double& g) {
  const LmUni u = v.uni[c >= 0 && c < v.V ? c : v.V];
  if (u.tok == kLmTransparent) return state;
  int next = 0;
  if (u.tok == kLmOov) {
    g = g + alpha * v.oov;
  } else {
    int s = state;
    bool found = false;
    for (int lvl = 0; lvl < PF_LM_ORDER_MAX && s != 0; ++lvl) {
      const LmState st = v.st[s];
      const int a = lm_find(v.key, st.begin, st.count, u.tok);
      if (a >= 0) {
        const LmArc arc = v.arc[a];
        g = g + alpha * (double)arc.logp;
        next = arc.next;
        found = true;
        break;
      }
      g = g + alpha * (double)st.bo;
      s = st.bo_state;
    }
    if (!found) {
      g = g + alpha * (double)u.logp;
      next = u.next;
    }
  }
  if (bonus) g = g + beta;
  return next;
}

}  // namespace pf
