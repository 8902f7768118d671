// punc.h — the CT-Transformer punctuation model (paraformer_hip.h "Punctuation"; the definition is tests/punc_ref.py): the
// loader of a `.pfw` of kind "cttransformer", the float64 host twins (words, logits, the cut rule, the text loop, the
// assembly) and the builder of the weight image k_punc.hip reads.  Host-only: no HIP header beyond common.h.
#pragma once
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "tile_image.h"

namespace pf {

// limits of the loader (PF_ERR_UNSUPPORTED beyond them).  The row kernel keeps a [64, 256] fp32 tile and two [64, 264] f16
// tiles in LDS and walks the FFN in slices of 256 hidden channels; the attention kernel holds one head of 32 channels in
// two k-steps of the 32x32x16 MFMA.  Both are written for d_model = 256 = 8 heads of 32; ffn is a multiple of 256.
constexpr int kPuncDModel = 256, kPuncHeads = 8, kPuncHeadDim = 32, kPuncMaxFfn = 4096, kPuncMaxKernel = 31, kPuncMaxLayers = 8,
              kPuncMaxClasses = 32, kPuncMini = 20, kPuncCommaWindow = 200, kPuncHardWindow = 492;

struct PuncModel {
  int vocab = 0, d_model = 0, heads = 0, ffn = 0, kernel = 0, n_layers = 0, n_punc = 0, sentence_end_id = 0;
  int unk_word = 0;                                         // the vocabulary index of "<unk>"
  // causal = 1 (header key `causal`): the streaming form, every layer attends to keys j <= i.  left: the FSMN taps before the
  // word, (kernel - 1) / 2 + the header's `sanm_shift`; a causal model has all its taps there (left = kernel - 1)
  int causal = 0, left = 0;
  int id_unk = -1, id_none = -1, id_comma = -1, id_period = -1, id_question = -1, id_pause = -1;   // "<unk>" "_" "，" "。" "？" "、"; -1: not listed
  std::vector<std::string> punc_list, words;
  std::unordered_map<std::string, int32_t> word_id;
  std::vector<float> embed, after_g, after_b, dec_w, dec_b;
  struct Layer { std::vector<float> n1_g, n1_b, qkv_w, qkv_b, fsmn, out_w, out_b, n2_g, n2_b, w1_w, w1_b, w2_w, w2_b; };
  std::vector<Layer> layers;
  // the device image: what an engine uploads, byte for byte (offsets in bytes, each 256-aligned)
  std::vector<char> image;
  int64_t pe_off = 0;                   // fp32 [PF_PUNC_MAX_WINDOW, d_model]: sinusoidal_pe, positions 1 .. 512
  int64_t embed_off = 0;                // f16 [vocab, d_model] (rounding point R0e)
  struct LayerImg { int64_t n1_g, n1_b, taps, n2_g, n2_b; TileGemm qkv, out, w1, w2; };   // taps fp32 [kernel, d_model]
  std::vector<LayerImg> limg;
  int64_t after_g_off = 0, after_b_off = 0;
  TileGemm dec;
};

// PF_ERR_INVALID_ARG: not a PFW1 container (pfw.h) of kind "cttransformer", a missing tensor, a
// wrong shape, a non-finite value, a vocabulary that is not `vocab` distinct non-empty words or lacks "<unk>", a punc_list
// without "<unk>" / "_", a sentence_end_id outside the list.  PF_ERR_UNSUPPORTED: d_model != 256, heads != 8, ffn no
// multiple of 256 or above 4096, an even kernel or one above 31, more than 8 layers, fewer than 2 or more than 32 classes.
std::shared_ptr<const PuncModel> punc_model_from_memory(const void* data, int64_t nbytes);
std::shared_ptr<const PuncModel> punc_model_load(const std::string& path);

// ---- the host twins (plain C++, float64 from the fp32 weights)
struct PuncWord { int32_t id; int32_t begin, end; };            // the vocabulary id and the byte span in the text
std::vector<PuncWord> host_punc_words(const PuncModel& m, const std::string& text);
// the network on ONE window of T ids (0 <= T <= PF_PUNC_MAX_WINDOW, ids in [0, vocab)): logits [T, n_punc].  A causal model
// masks the keys behind the query and takes its FSMN taps from the left alone (tests/punc_stream_ref.py)
void host_punc_logits(const PuncModel& m, const int32_t* ids, int T, double* logits);
void host_punc_argmax(const PuncModel& m, const double* logits, int T, int32_t* p);      // ties to the larger index
// steps 3 - 7 of the text loop and the last-window edits on one window's p [n] (edited in place); returns cut
int host_punc_cut(const PuncModel& m, int32_t* p, int n, bool last);
// the loop over one text: punc_ids [n].  windows (optional): per forward its length and its cut
void host_punc_ids(const PuncModel& m, const int32_t* ids, int64_t n, int32_t* punc_ids, std::vector<std::pair<int32_t, int32_t>>* windows);
// the output text from the words of `text` and their punc_ids; sent_end (optional): one past the last word of each sentence
std::string host_punc_assemble(const PuncModel& m, const std::string& text, const std::vector<PuncWord>& words, const int32_t* punc_ids,
                               std::vector<int32_t>* sent_end);

// ---- streaming (paraformer_hip.h "Punctuation, streaming"; the definition is tests/punc_stream_ref.py).  Causal models only.
constexpr int kPuncStreamMaxContext = 256, kPuncStreamDefaultContext = 200;
// the device form's state block (k_punc_stream.hip): f16 k | v [n_layers, 256, 2, 256], then int32 {count, the newest word's
// mark, 0, 0}; all zero = a fresh stream.  The host twin's: the same with float64 k | v.
struct PuncStreamLayout { int64_t words_off, bytes; };
PuncStreamLayout punc_stream_layout(const PuncModel& m);
int64_t host_punc_stream_state_bytes(const PuncModel& m);
// what both forms check before anything changes: a causal model, max_context in [2, 256], n_new >= 0, ids in the vocabulary,
// a count in [0, 256] and, with bit 0 of flags (no restarts), count + n_new <= 256
void punc_stream_admit(const PuncModel& m, int32_t count, const int32_t* ids, int n_new, int max_context, int flags);
// one call of ONE stream in float64: n_new words in order, then the flush.  marks / mark_flags [n_new] (bit 0: sentence end,
// bit 1: forced restart), logits [n_new, n_punc] optional, *flush_mark: -1 without a flush or for an empty context
void host_punc_stream_step(const PuncModel& m, void* state, const int32_t* ids, int n_new, bool flush, int max_context, int flags,
                           int32_t* marks, int32_t* mark_flags, double* logits, int32_t* flush_mark);
// the flush's edit of the newest word's mark
inline int punc_flush_mark(const PuncModel& m, int last) {
  return (last == m.id_none || (m.id_comma >= 0 && last == m.id_comma) || (m.id_pause >= 0 && last == m.id_pause)) ? m.sentence_end_id : last;
}

}  // namespace pf

// the C handle: a reference to an immutable model (an engine that attaches it takes a reference of its own)
struct pf_punc_model {
  std::shared_ptr<const pf::PuncModel> p;
};
