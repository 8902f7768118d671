// vadnet.h — the FSMN-VAD model score of the voice-activity segmentation (paraformer_hip.h "Voice-activity segmentation, model
// score"; the definition is tests/vadnet_ref.py): the loader of a `.pfw` of kind "fsmnvad", the float64 host twins and the
// builder of the weight image k_vadnet.hip reads.  Host-only: no HIP header beyond common.h.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "tile_image.h"

namespace pf {

// limits of the loader (PF_ERR_UNSUPPORTED beyond them): two [64, widest + 8] f16 tiles must fit the 160 KB of LDS
constexpr int kVadMaxWidth = 512, kVadMaxProj = 256, kVadMaxLayers = 8, kVadMaxReach = 256, kVadMaxLfr = 16;

struct VadModel {
  int input_dim = 0, affine_dim = 0, linear_dim = 0, proj_dim = 0, output_dim = 0, n_layers = 0, lorder = 0, lstride = 0, lfr_m = 0;
  std::vector<int32_t> sil_ids;
  std::vector<float> shift, scale, in1_w, in1_b, in2_w, in2_b, out1_w, out1_b, out2_w, out2_b;
  struct Layer { std::vector<float> lin_w, taps, aff_w, aff_b; };      // taps [lorder, proj]
  std::vector<Layer> layers;
  // the device image: what an engine uploads, byte for byte (offsets in bytes, each 256-aligned)
  std::vector<char> image;
  TileGemm g_in1, g_in2, g_out1, g_out2;
  std::vector<TileGemm> g_lin, g_aff;
  std::vector<int64_t> taps_off;        // fp32 [lorder, ldp] per layer
  int64_t shift_off = 0, scale_off = 0, sil_off = 0;   // fp32 [input_dim] each; fp32 [g_out2.Npad]: 1 on a silence id, else 0
  int ldp = 0;                          // row stride of the p rows: proj_dim padded to 32
  int lds_ld = 0;                       // row stride (halves) of the kernel's LDS tiles: the widest operand + 8
  const std::vector<float>* tensor(const std::string& name) const;     // by its container name; nullptr: no such tensor
};

// PF_ERR_INVALID_ARG: not a PFW1 container (pfw.h) of kind "fsmnvad", a u8 tensor, a missing tensor, a
// wrong shape, a non-finite value, a silence id outside [0, output_dim).  PF_ERR_UNSUPPORTED: rorder > 0, lfr_n != 1, a
// dimension beyond the limits above.
std::shared_ptr<const VadModel> vad_model_from_memory(const void* data, int64_t nbytes);
std::shared_ptr<const VadModel> vad_model_load(const std::string& path);
// the CPU twins for ONE utterance, float64 from the fp32 weights.  rows [T, n_mels]; logits [T, output_dim]
void host_vad_model_logits(const VadModel& m, const float* rows, int64_t T, int n_mels, double* logits);
void host_vad_model_levels(const VadModel& m, const float* rows, int64_t T, int n_mels, int32_t* levels);
pf_vad_config vad_model_default();      // vad_default() with floor_pct = -1, abs_level = 9830

// ---- streaming (paraformer_hip.h "Voice-activity endpointing, streaming, model score"; the schedule is tests/vadnet_stream_ref.py)
// the levels a stream of n received frames has released: max(0, n - right), all n once flushed
int64_t vad_stream_released(const VadModel& m, int64_t n, bool flushed);
// what both forms check about ONE stream's state words and its new frames before anything changes (as endpoint_admit)
void vad_stream_admit(int64_t count, int32_t flushed, int64_t n_new);
// the device form's state block (k_vadnet_stream.hip): fp32 history [n_layers, reach, ldp] | fp32 row tail [lfr_m - 1, n_mels] |
// int32 count | int32 flushed in the block's last 8 bytes (words_off); all zero = a fresh stream
struct VadStreamLayout { int64_t hist_floats = 0, tail_floats = 0, words_off = 0, bytes = 0; };
VadStreamLayout vad_stream_layout(const VadModel& m);
// The host twin for ONE stream, float64, on block64, the per-row code of host_vad_model_logits: n_new rows [n_new, n_mels], then
// the flush.  state: host_vad_stream_state_bytes bytes, in / out, all zero = fresh (its layout is the twin's own: float64 history, the
// row tail, and count | flushed in the last 8 bytes).  levels [cap]
// / logits [cap, output_dim]: either may be null.  Returns the released count; PF_ERR_CAPACITY when cap is below it (nothing
// changed), otherwise as vad_stream_admit.
int64_t host_vad_stream_state_bytes(const VadModel& m);
int64_t host_vad_model_stream(const VadModel& m, void* state, const float* rows, int64_t n_new, bool flush, int n_mels, int32_t* levels,
                              double* logits, int64_t cap);
pf_endpoint_config endpoint_model_default();   // endpoint_default() with rise = -1, abs_level = 9830

}  // namespace pf

// the C handle: a reference to an immutable model (an engine that attaches it takes a reference of its own)
struct pf_vad_model {
  std::shared_ptr<const pf::VadModel> p;
};
