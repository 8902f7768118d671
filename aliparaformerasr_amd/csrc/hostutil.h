// hostutil.h — host-side file/config helpers shared by the engine and the recognizer mirror.
#pragma once
#include <string>
#include <vector>

#include "common.h"
#include "json.h"

namespace pf {

std::string read_text_file(const std::string& path);          // throws PF_ERR_IO
bool file_exists(const std::string& path);
void read_binary_file(const std::string& path, std::vector<char>& out);

// LoadCmvn (AliParaformerAsr/WavFrontend.cs:112-153)
void parse_mvn_text(const std::string& text, std::vector<float>& shift, std::vector<float>& scale);

// ReadTokens (AliParaformerAsr/Utils/PreloadHelper.cs:120-141): File.ReadAllLines semantics
std::vector<std::string> read_lines(const std::string& path);
std::vector<std::string> split_lines(const std::string& text);

// ConfEntity subset consumed on the path (AliParaformerAsr/Model/ConfEntity.cs,
// FrontendConfEntity.cs) with the reference defaults.
struct ConfEntity {
  std::string model = "paraformer";
  bool use_itn = false;
  int fs = 16000;
  std::string window = "hamming";
  int n_mels = 80;
  int frame_length = 25, frame_shift = 10;
  float dither = 1.0f;
  int lfr_m = 7, lfr_n = 6;
  bool snip_edges = false;
};
// LoadConf (AliParaformerAsr/OfflineRecognizer.cs:55-71): ".json" -> json, ".yaml" -> yaml,
// anything else / missing file -> defaults.
ConfEntity load_conf(const std::string& path);
ConfEntity conf_from_yaml(const std::string& text);
ConfEntity conf_from_json(const std::string& text);

// ---- Examples harness (AliParaformerAsr.Examples/Utils/AudioHelper.cs) -------------------------------
// IsAudioByHeader restricted to what this build decodes: RIFF....WAVE in the first 16 bytes (:286-340)
bool is_wav_header(const std::string& path);
// AudioFileReader semantics for RIFF/WAVE (NAudio converts every PCM width to IEEE float): interleaved
// samples, PCM8 -> b/128-1, PCM16 -> /32768, PCM24 -> /8388608, PCM32 -> /2147483648, float32 as is.
struct WavData { std::vector<float> samples; int sample_rate = 0, channels = 0; double duration_ms = 0; };
WavData decode_wav_file(const std::string& path);
// decode_wav_file's header walk without the sample loop (pf_host_wav_info): format = pf_pcm_format, the payload's place in the file
struct WavInfo { int format = 0, sample_rate = 0, channels = 0; size_t data_offset = 0, data_bytes = 0; double duration_ms = 0; };
WavInfo wav_info(const std::vector<char>& file, const std::string& path);
WavInfo wav_info_file(const std::string& path);                 // the same, reading only the header region of the file
// the sample loop on memory: n values of `format` (pf_pcm_format) -> float
int pcm_bytes_per_value(int format);                           // throws PF_ERR_INVALID_ARG for an unknown format
void pcm_decode(const void* data, size_t n_values, int format, float* out);
// PCM intake (paraformer_hip.h "PCM intake"): what GetFileSample does to n_values interleaved values of `d` for an engine at
// rate fs — validated (PF_ERR_INVALID_ARG) and sized here, carried out by pcm_to_samples on the host or k_pcm.hip on the device
struct PcmPlan { bool resample = false, downmix = false; int bytes_per_value = 0; int64_t n_mono = 0, n_out = 0; double ratio = 1.0; };
PcmPlan pcm_plan(const pf_pcm_desc& d, int fs, int64_t n_values);
std::vector<float> pcm_to_samples(const void* data, int64_t n_values, const pf_pcm_desc& d, int fs);
// Resample(sourceData, sourceSampleRate, targetSampleRate, sourceChannels) (:223-279): stereo -> mono
// average first, then linear interpolation in double precision; target length = Round(n / ratio) (banker's)
std::vector<float> resample_linear(const std::vector<float>& src, int sr_in, int sr_out, int channels);
// GetFileSample (:12-32): missing file -> float[1]{0}; resampled (and down-mixed) ONLY when the rate is not
// 16 kHz — a 16 kHz stereo file is handed over interleaved, exactly as upstream does.
std::vector<float> get_file_sample(const std::string& path, double* duration_ms);

// ---- n-best list of one utterance from its per-position top-k lists (paraformer_hip.h "Top-k and n-best") ----------
// val / n: [L, K] / [L] as launch_topk leaves them.  A hypothesis is a rank vector r[0..L) with r[l] < n[l] and r[l] == 0 for
// l >= n_free; its score is the float64 sum of val[l, r[l]] added from l = 0 up.  Listed by descending score, ties to the
// lexicographically smaller rank vector; at most N (1 .. 64).  out_ranks [N, L], out_scores [N]; returns how many exist.
// Exact: a best-first walk in which every vector has ONE parent (its last non-zero rank lowered by one), which never scores
// lower and never sorts later, so the heap always holds the next hypothesis.  PF_ERR_INVALID_ARG for a ranked value that is
// NaN or +inf (their sums would not order).
int host_nbest(const float* val, const int32_t* n, int L, int K, int n_free, int N, int32_t* out_ranks, double* out_scores);

// ---- CTC prefix beam search of one utterance (paraformer_hip.h "CTC beam search"; the definition is tests/ctcbeam_ref.py) ----
// The host twin of k_ctcbeam.hip: blank_lp[t * blank_stride], ids / val [T, K], n [T] -> the N best of a beam of width W
// (1 <= N <= W <= 64).  out_ids [N, cap] (-1 past a hypothesis' length), out_len [N] (0), out_score [N] (-inf): every slot is
// written.  Returns the number of hypotheses: 0 when a frame has n[t] == 0 or a NaN blank log-prob.  PF_ERR_CAPACITY when a
// hypothesis is longer than cap (cap >= T always suffices).  Prefixes are back-pointer chains compared by token sequence.
int host_ctc_beam(const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val, const int32_t* n, int T, int K,
                  int blank, int W, int N, int64_t* out_ids, int32_t* out_len, double* out_score, int cap);

// ---- hot-word boosting inside the beam search (paraformer_hip.h "CTC hot words"; the definition is tests/ctcbeam_bias_ref.py) ----
// The context graph of a hot-word set, compiled into a deterministic table: a trie over the set with Aho-Corasick failure
// links folded in.  State 0 is the root.  From state u on token c: col = tok_col[c] (-1: not a hot-word token: root, nothing
// completes), e = table[u * A + col]: e & 0xFFFF the next state, (e >> 16) & 0xFF the length of the hot word that completes
// (then the next state is the root), e >> 24 the depth of the next state.  depth[u] is the length of the pending partial match in u.
// n words, word i = lens[i] ids at ids[sum of lens before i]; an empty word is dropped, a duplicate harmless.
// PF_ERR_INVALID_ARG for an id outside [1, V); PF_ERR_CAPACITY for a word longer than PF_HOTWORD_LEN_MAX, more than
// PF_HOTWORD_STATES_MAX states or a table over PF_HOTWORD_TABLE_BYTES_MAX.
struct HotwordGraph {
  int S = 0, A = 0;                 // states (trie nodes, root included), distinct hot-word tokens
  std::vector<int32_t> tok_col;     // [V]
  std::vector<int32_t> table;       // [S, A]
  std::vector<int32_t> depth;       // [S]
  bool empty() const { return A == 0; }
};
void build_hotword_graph(const int32_t* ids, const int32_t* lens, int n, int V, HotwordGraph& g);
// host_ctc_beam with the biased select and finish of the definition: out_score = lse(pb, pnb) + boost * matched in the
// re-ordered list, out_matched [N] (0), out_loglik [N] (-inf) next to it.  boost is widened to float64; with boost == 0 or a
// set without a non-empty word this IS host_ctc_beam (matched 0, loglik = score).
int hotword_vocab_bound(const int32_t* ids, const int32_t* lens, int n);   // one past the largest id; ids are below 2^24
int host_ctc_beam_hot(const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val, const int32_t* n, int T, int K,
                      int blank, int W, int N, const int32_t* hw_ids, const int32_t* hw_lens, int n_hw, float boost,
                      int64_t* out_ids, int32_t* out_len, double* out_score, int32_t* out_matched, double* out_loglik, int cap);

// host_ctc_beam_hot with a language model fused in (paraformer_hip.h "CTC language model"; the definition is
// tests/ctcbeam_lm_ref.py): score = (lse(pb, pnb) + boost * matched) + lm_sum in the re-ordered list, out_lm [N] (0) next to
// out_loglik.  A set that does not bias (boost == 0, no non-empty word) is allowed: matched 0.
struct LmImage;
int host_ctc_beam_lm(const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val, const int32_t* n, int T, int K,
                     int blank, int W, int N, const int32_t* hw_ids, const int32_t* hw_lens, int n_hw, float boost, int64_t* out_ids,
                     int32_t* out_len, double* out_score, int32_t* out_matched, double* out_loglik, int cap, const LmImage& lm, float alpha,
                     float beta, int lm_flags, double* out_lm);

// ---- n-best search of one paraformer utterance (paraformer_hip.h "N-best search"; the definition is tests/nbest_search_ref.py) ----
// The host twin of k_nbestsearch.hip: the top-k block ids / val [L, K], n [L] and token_num -> the N best of a position-synchronous
// beam of width W (1 <= N <= W <= 64), optionally biased by a hot-word set (boost > 0 and a non-empty word) and fused with a
// model (lm != nullptr).  out_ranks [N, L] (-1), out_score / out_loglik [N] (-inf), out_lm [N] (0), out_matched [N] (0): every
// slot is written; all but out_ranks are optional.  Returns the number of hypotheses: 0 when L == 0, some n[l] == 0 or a listed
// value is NaN or +inf (no throw).  Bit-equal to the definition and the kernel: it runs lm_step and the same table.
int host_nbest_search(const int64_t* ids, const float* val, const int32_t* n, int L, int K, int token_num, int W, int N,
                      const int32_t* hw_ids, const int32_t* hw_lens, int n_hw, float boost, const LmImage* lm, float alpha, float beta,
                      int lm_flags, int32_t* out_ranks, double* out_score, double* out_loglik, double* out_lm, int32_t* out_matched);

// ---- CTC forced alignment of one utterance and one target (paraformer_hip.h "CTC forced alignment"; tests/ctcalign_ref.py) ----
// The host twin of k_ctcalign.hip: lp [T, ld] log-prob rows (V read per row), y [U] ids in [1, V) (PF_ERR_INVALID_ARG
// otherwise; U > PF_ALIGN_MAX_TOKENS is PF_ERR_CAPACITY).  *path_score: the float32 Viterbi score, *loglik: the float64 log of
// the summed alignments; first / last / tok_score [U] (-1 / -1 / 0 when not ok).  Returns ok = path_score > -inf.
int host_ctc_align(const float* lp, int64_t ld, int T, int V, const int64_t* y, int U, float* path_score, double* loglik,
                   int32_t* first, int32_t* last, float* tok_score);

// ---- voice-activity segmentation (paraformer_hip.h "Voice-activity segmentation"; the definition is tests/vad_ref.py) ----
// The host twins of k_vad.hip.  vad_default: the stated defaults.  vad_check: cfg (null = the defaults) validated against the
// constraints of the header (PF_ERR_INVALID_ARG), returned by value.
pf_vad_config vad_default();
pf_vad_config vad_check(const pf_vad_config* cfg, int lfr_n);
void host_vad_levels(const float* rows, int64_t T, int n_mels, int32_t* out);
// steps 2-6 over ONE utterance's levels: all segments in order (PF_ERR_CAPACITY above PF_VAD_MAX_FRAMES / PF_VAD_MAX_SEGMENTS)
std::vector<int32_t> host_vad_segments(const int32_t* levels, int T, int n_mels, const pf_vad_config& c);
// the batch plan of long-audio recognition: batch / row per segment; returns the number of batches
int host_long_plan(const int32_t* len, int n, int batch_max, int64_t frame_budget, int32_t* batch, int32_t* row);

// ---- streaming endpointing (paraformer_hip.h "Voice-activity endpointing, streaming"; the definition is tests/endpoint_ref.py) ----
// endpoint_default / endpoint_check: as vad_default / vad_check.  endpoint_admit: what both forms check about ONE stream's
// call before anything changes (a block the detector cannot have left, frames after a flush: PF_ERR_INVALID_ARG; too many frames:
// PF_ERR_CAPACITY).
pf_endpoint_config endpoint_default();
pf_endpoint_config endpoint_check(const pf_endpoint_config* cfg, int lfr_n);
void endpoint_admit(const int32_t* state, int n_new);
// The host twin of k_endpoint.hip for ONE stream, one frame at a time: n_new levels, then the flush.  state
// [PF_ENDPOINT_STATE_INTS] in / out; returns every event as (b, e, kind) triples; *in_speech / *open_begin as the header says.
std::vector<int32_t> host_endpoint_update(int32_t* state, const int32_t* levels, int n_new, int flush, int n_mels,
                                          const pf_endpoint_config& c, int32_t* in_speech, int32_t* open_begin);

// UTF-8 <-> code points
std::vector<uint32_t> utf8_decode(const std::string& s);
std::string utf8_encode(uint32_t cp);
std::string utf8_encode(const std::vector<uint32_t>& cps);
int utf16_length(const std::string& utf8);   // C# string.Length

}  // namespace pf
