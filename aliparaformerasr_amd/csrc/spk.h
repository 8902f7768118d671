// spk.h — the speaker labels of long-audio recognition (paraformer_hip.h "Speaker labels"; the definition is tests/spk_ref.py):
// the loader of a `.pfw` of kind "campplus", the builder of the weight image k_spk.hip reads, and the host half of the
// feature: the window plan, the clustering, the segment labels.  Host-only: no HIP header beyond common.h.
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "tile_image.h"

namespace pf {

// limits of the loader (PF_ERR_UNSUPPORTED beyond them), each from what k_spk.hip is built for:
//   n_mels % 8 == 0 and <= 128           the three frequency halvings are exact; the first launch keeps a window's column means in LDS
//   m_channels % 8 == 0 and <= 64        a tap of the head's gather is whole 16-byte chunks; one wave owns all of a convolution's
//                                        output channels and the [64, 10 m + 8] tile
//   m_channels * n_mels / 8 <= 512       the TDNN's [131, K + 8] input tile
//   init_channels <= 128, bn_channels <= 128 (and even)     one 32-row block of W per wave and product
//   growth <= 64                         the mask tile [64, growth]
//   exactly three blocks of 1 .. 64 layers, dilation 1 .. 8 (the zero rows around the bottleneck tile)
//   seg_len >= 4                         a window of PF_SPK_MAX_FRAMES has at most 64 segments: one tile of context rows
//   every concatenated width even (a transit halves it) and <= 2048; embedding <= 512
constexpr int kSpkMaxMels = 128, kSpkMaxM = 64, kSpkMaxFrameWidth = 512, kSpkMaxInit = 128, kSpkMaxBn = 128, kSpkMaxGrowth = 64,
              kSpkMaxLayers = 64, kSpkMaxDilation = 8, kSpkMinSegLen = 4, kSpkMaxWidth = 2048, kSpkMaxEmbedding = 512;

// what the kernels read of one layer / convolution, as it lies in the image (plain data)
struct SpkLayerDev { TileGemm lin1, local, cam1, cam2; int64_t scale_off, shift_off; int32_t C, pad; };
// a head convolution: K = 9 cin (+ cin: the fused 1x1 shortcut over `aux`); in / out / aux name the three activation buffers
struct SpkConvDesc { TileGemm g; int32_t cin, sf, shortcut, residual, in, out, aux, to_frames; };

struct SpkModel {
  int n_mels = 0, m = 0, init = 0, growth = 0, bn = 0, seg_len = 0, embedding = 0;
  int blocks[3] = {0, 0, 0}, dilations[3] = {0, 0, 0};
  int C0[3] = {0, 0, 0}, C1[3] = {0, 0, 0}, ldx[4] = {0, 0, 0, 0};   // widths into / behind each block; row strides of the X buffers
  int frame_w = 0, frame_ld = 0;                                      // m * n_mels / 8 and that padded to 16
  int c_out = 0;                                                      // the frames' width: C1[2] / 2
  std::map<std::string, std::vector<float>> tensors;                  // as loaded, by container name
  // the device image: what an engine uploads, byte for byte (offsets in bytes, each 256-aligned)
  std::vector<char> image;
  SpkConvDesc conv[10];
  TileGemm tdnn, transit[3], dense;
  int64_t layers_off[3] = {0, 0, 0};                                  // SpkLayerDev [blocks[b]]
  int64_t tr_scale_off[3] = {0, 0, 0}, tr_shift_off[3] = {0, 0, 0}, out_scale_off = 0, out_shift_off = 0;
  double flops_per_frame = 0;                                         // padded multiply-adds * 2 per input frame, for the profile
  const std::vector<float>* tensor(const std::string& name) const;
};

// PF_ERR_INVALID_ARG: not a PFW1 container (pfw.h) of kind "campplus", a u8 tensor, a missing tensor, a wrong shape, a value
// that is not finite, blocks / dilations that are no lists of three.  PF_ERR_UNSUPPORTED: a dimension beyond the limits above.
std::shared_ptr<const SpkModel> spk_model_from_memory(const void* data, int64_t nbytes);
std::shared_ptr<const SpkModel> spk_model_load(const std::string& path);

pf_spk_config spk_default();
void spk_check_config(const pf_spk_config& c);                         // PF_ERR_INVALID_ARG on a value outside its range
// the window plan of ONE stream: seg [n_seg, 2] frame pairs -> win [*, 3] (segment, begin, end), the shift used
void host_spk_windows(const int32_t* seg, int32_t n_seg, const pf_spk_config& c, std::vector<int32_t>& win, int32_t* shift_used);
// average-linkage agglomeration over S [N, N] fp32 (tests/spk_ref.py cluster) -> labels [N], the number of speakers
void host_spk_cluster(const float* S, int32_t N, const pf_spk_config& c, int32_t* labels, int32_t* n_speakers);
// the label per segment from its windows' (win_seg [N], win_label [N])
void host_spk_segment_labels(const int32_t* seg, int32_t n_seg, const int32_t* win_seg, const int32_t* win_label, int32_t N,
                             int32_t* out);
// speaker k's centroid: the L2-normalised mean of its windows' L2-normalised embeddings, out [K, E]
void host_spk_centroids(const float* emb, const int32_t* labels, int32_t N, int32_t E, int32_t K, float* out);

}  // namespace pf

// the C handle: a reference to an immutable model (an engine that attaches it takes a reference of its own)
struct pf_spk_model {
  std::shared_ptr<const pf::SpkModel> p;
};
