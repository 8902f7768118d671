// nnlm.h — the causal Transformer LM that rescores n-best lists (paraformer_hip.h "Neural LM rescoring"; the definition is
// tests/nnlm_ref.py): the loader of a `.pfw` of kind "transformerlm", the float64 host twin of k_nnlm.hip, the fusion of LM
// scores into a list and the builder of the weight image the kernels read.  Host-only: no HIP header beyond common.h.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "tile_image.h"

namespace pf {

// limits of the loader (PF_ERR_UNSUPPORTED beyond them).  The row kernel keeps a [32, 512] fp32 tile and two [32, 520] f16
// tiles in LDS and walks the FFN in slices of 256 hidden channels; the attention kernel holds one head of 64 channels in four
// k-steps of the 32x32x16 MFMA and a sequence's keys (at most 256) in LDS.
constexpr int kNnlmDModel = 512, kNnlmHeads = 8, kNnlmMaxEmbed = 512, kNnlmMaxFfn = 4096, kNnlmMaxLayers = 24, kNnlmMinVocab = 2,
              kNnlmMaxVocab = 1 << 20;

struct NnlmModel {
  int vocab = 0, embed_dim = 0, d_model = 0, heads = 0, ffn = 0, n_layers = 0;
  int sos() const { return vocab - 1; }                     // sos = eos = V - 1
  std::vector<float> embed, in_w, in_b, in_g, in_beta, after_g, after_b, dec_w, dec_b;
  struct Layer { std::vector<float> n1_g, n1_b, qkv_w, qkv_b, out_w, out_b, n2_g, n2_b, w1_w, w1_b, w2_w, w2_b; };
  std::vector<Layer> layers;
  // the device image: what an engine uploads, byte for byte (offsets in bytes, each 256-aligned)
  std::vector<char> image;
  int64_t embed_off = 0;                // f16 [vocab, embed_dim] (rounding point R0e)
  TileGemm in;
  int64_t in_g_off = 0, in_b_off = 0;
  struct LayerImg { int64_t n1_g, n1_b, n2_g, n2_b; TileGemm qkv, out, w1, w2; };
  std::vector<LayerImg> limg;
  int64_t after_g_off = 0, after_b_off = 0;
  TileGemm dec;
};

// PF_ERR_INVALID_ARG: not a PFW1 container (pfw.h) of kind "transformerlm", a missing tensor, a wrong shape, a non-finite
// value, a dimension that is missing or not positive.  PF_ERR_UNSUPPORTED: d_model != 512, heads != 8, an embedding width that
// is no multiple of 16 or above 512, ffn no multiple of 256 or above 4096, more than 24 layers, a vocabulary outside 2 .. 2^20.
std::shared_ptr<const NnlmModel> nnlm_model_from_memory(const void* data, int64_t nbytes);
std::shared_ptr<const NnlmModel> nnlm_model_load(const std::string& path);

// what both forms check before anything runs: 0 <= n <= PF_NNLM_MAX_TOKENS, every id in [0, vocab)
void nnlm_admit(const NnlmModel& m, const int32_t* ids, int n);
// the network on ONE hypothesis y_1 .. y_n in float64: logp [n + 1], logp[t] = log P(target_t | sos, y_1 .. y_t) with the
// targets y_1 .. y_n, eos
void host_nnlm_logp(const NnlmModel& m, const int32_t* ids, int n, double* logp);
// score'[i] = base[i] + weight * lm_sum[i] + bonus * n_tokens[i] in float64; order [N]: the indices stable-sorted by score'
// descending (ties keep their order).  A NaN anywhere is refused (PF_ERR_INVALID_ARG): a sort over NaN has no order.
void host_nnlm_fuse(const double* base, const double* lm_sum, const int32_t* n_tokens, int N, double weight, double bonus, double* score,
                    int32_t* order);

}  // namespace pf

// the C handle: a reference to an immutable model (an engine that attaches it takes a reference of its own)
struct pf_nnlm_model {
  std::shared_ptr<const pf::NnlmModel> p;
};
