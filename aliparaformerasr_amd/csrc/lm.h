// lm.h — the back-off n-gram language model of the CTC beam search (paraformer_hip.h "CTC language model"; the definition is
// tests/ctcbeam_lm_ref.py): the builder that compiles a model into the flat image of lm_dev.h, the ARPA reader, the host scorer.
// Host-only: no HIP header beyond common.h.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "common.h"

namespace pf {

struct LmImage {
  std::vector<int32_t> words;        // the image (lm_dev.h); what an engine uploads, byte for byte
  int order = 0, V = 0;
  int64_t states = 0, arcs = 0;      // states: the empty context included; arcs: the listed n-grams of order >= 2
  int bos = -1, eos = -1, unk = -1;
  size_t bytes() const { return words.size() * 4; }
};

// order O, n_ngrams [O], and per listed n-gram in the order (all 1-grams, all 2-grams, ...): its k ids in `ids`, its natural-log
// probability and its back-off weight (NaN: listed without one; ignored at order O).  PF_ERR_INVALID_ARG: a duplicate n-gram, an
// id outside [1, V), a non-finite weight, an unk that is no listed unigram; PF_ERR_CAPACITY: an image over PF_LM_IMAGE_BYTES_MAX.
std::shared_ptr<const LmImage> lm_build(int order, const int64_t* n_ngrams, const int32_t* ids, const float* logp, const float* backoff,
                                        int V, int bos, int eos, int unk, float oov, const int32_t* transparent, int n_transparent);
// ARPA text against a token table; *n_dropped: the n-grams left out because a word is not in the table (or is id 0)
std::shared_ptr<const LmImage> lm_from_arpa(const std::string& path, const char* const* tokens, int n_tokens, float oov, int64_t* n_dropped);
// g and the state after ids[0 .. n), from the start state; g_pos / state_pos [n] optional: after every token.  PF_LM_EOS in
// flags adds the end-of-sentence step to *g (not to g_pos).
void lm_score(const LmImage& lm, const int32_t* ids, int n, float alpha, float beta, int flags, double* g, int32_t* state, double* g_pos,
              int32_t* state_pos);
void lm_check_weights(float alpha, float beta, int flags);       // PF_ERR_INVALID_ARG unless alpha >= 0, both finite, flags known

}  // namespace pf

// the C handle: a reference to an immutable image (an engine that installs the model takes a reference of its own)
struct pf_lm {
  std::shared_ptr<const pf::LmImage> p;
};
