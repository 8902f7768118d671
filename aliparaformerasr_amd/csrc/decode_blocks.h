// decode_blocks.h — the packed blocks the decoding extras (Engine::set_decode) leave on the device, described once for the
// device side (the kernels' output pointers over a workspace) and the host side (HostBatchOut's vectors after the one copy).
// Host-only: no HIP header.
//
// A block is a run of fields; Cursor::take is the only place where offsets are added up, and it aligns every field to its
// element size.  The same step lays out the scratch that follows a block in its workspace.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pf {

// `count` elements of T at byte offset `off` of whatever base address the layout is put over
template <class T> struct Field {
  size_t off = 0, count = 0;
  T* operator()(void* base) const { return (T*)((char*)base + off); }
  const T* operator()(const void* base) const { return (const T*)((const char*)base + off); }
};

struct Cursor {
  size_t off = 0;
  template <class T> Field<T> take(size_t count) {
    off = (off + sizeof(T) - 1) / sizeof(T) * sizeof(T);
    const Field<T> f{off, count};
    off += count * sizeof(T);
    return f;
  }
};

// begins 8-aligned, and the cursor leaves it past words() * 8 bytes: what the device-to-host copy of a block moves
struct Block {
  size_t begin, end = 0;
  explicit Block(Cursor& c) : begin(c.take<int64_t>(0).off) {}
  size_t bytes() const { return end - begin; }             // up to the end of the last field
  size_t words() const { return (bytes() + 7) / 8; }       // int64 words (the size of HostBatchOut's vectors)
 protected:
  // lay(c, field, count, field, count, ...): the fields in memory order
  void lay(Cursor& c) { end = c.off; c.off = begin + words() * 8; }
  template <class T, class... Rest> void lay(Cursor& c, Field<T>& f, size_t count, Rest&&... rest) { f = c.take<T>(count); lay(c, rest...); }
};

// CTC collapse (k_ctc.hip): ids [B, cap] int64 | first [B, cap] | last [B, cap] int32 | score [B, cap] fp32 | n [B] int32
struct CtcBlock : Block {
  Field<int64_t> ids; Field<int32_t> first, last; Field<float> score; Field<int32_t> n;
  CtcBlock(Cursor& c, size_t B, size_t cap) : Block(c) { lay(c, ids, B * cap, first, B * cap, last, B * cap, score, B * cap, n, B); }
};

// top-k alternatives (k_topk.hip): ids [rows, K] int64 | val [rows, K] fp32 | n [rows] int32
struct TopkBlock : Block {
  Field<int64_t> ids; Field<float> val; Field<int32_t> n;
  TopkBlock(Cursor& c, size_t rows, size_t K) : Block(c) { lay(c, ids, rows * K, val, rows * K, n, rows); }
};

// CTC prefix beam search (k_ctcbeam.hip): score [B, N] float64 | ids [B, N, cap] int32 | len [B, N] | n_hyp [B]
struct BeamBlock : Block {
  Field<double> score; Field<int32_t> ids, len, n_hyp;
  BeamBlock(Cursor& c, size_t B, size_t N, size_t cap) : Block(c) { lay(c, score, B * N, ids, B * N * cap, len, B * N, n_hyp, B); }
};

// the biased search's extras: loglik_sum [B, N] float64 | matched [B, N] int32
struct BeamHotBlock : Block {
  Field<double> loglik; Field<int32_t> matched;
  BeamHotBlock(Cursor& c, size_t B, size_t N) : Block(c) { lay(c, loglik, B * N, matched, B * N); }
};

// the fused search's extra (language model): lm_sum [B, N] float64; loglik_sum travels in BeamHotBlock (matched 0 without a set)
struct BeamLmBlock : Block {
  Field<double> lm_sum;
  BeamLmBlock(Cursor& c, size_t B, size_t N) : Block(c) { lay(c, lm_sum, B * N); }
};

// n-best search over paraformer's top-k lists (k_nbestsearch.hip): score [B, N] | loglik_sum [B, N] | lm_sum [B, N] float64 |
// ranks [B, N, L] | matched [B, N] | n_hyp [B] int32
struct NbestSearchBlock : Block {
  Field<double> score, loglik, lm_sum; Field<int32_t> ranks, matched, n_hyp;
  NbestSearchBlock(Cursor& c, size_t B, size_t N, size_t L) : Block(c) {
    lay(c, score, B * N, loglik, B * N, lm_sum, B * N, ranks, B * N * L, matched, B * N, n_hyp, B);
  }
};

// CTC forced alignment (k_ctcalign.hip): loglik [B, H] float64 | path_score [B, H] fp32 | ok [B, H] | len [B, H] int32 |
// first [B, H, cap] | last [B, H, cap] int32 | tok_score [B, H, cap] fp32
struct AlignBlock : Block {
  Field<double> loglik; Field<float> path; Field<int32_t> ok, len, first, last; Field<float> tok;
  AlignBlock(Cursor& c, size_t B, size_t H, size_t cap) : Block(c) {
    lay(c, loglik, B * H, path, B * H, ok, B * H, len, B * H, first, B * H * cap, last, B * H * cap, tok, B * H * cap);
  }
};

// one stream's carried CIF pair (k_cif_stream.hip, online_cif_step in online.cpp): hidden [D] fp32, the carried frame already
// divided by the carried integrate | integrate [G] fp32, ONE COPY per kCifStreamGroup channels, G = ceil(D / kCifStreamGroup)
// (every workgroup of the kernel walks one group of channels and owns that group's copy: no workgroup reads a cell another
// writes; all copies hold the same bits), padded to a multiple of four cells that nobody writes.  A zero-filled block is the
// constructor's state.
constexpr size_t kCifStreamGroup = 256;
struct CifStreamBlock : Block {
  Field<float> hidden, integrate; size_t groups;
  CifStreamBlock(Cursor& c, size_t D) : Block(c), groups((D + kCifStreamGroup - 1) / kCifStreamGroup) { lay(c, hidden, D, integrate, (groups + 3) / 4 * 4); }
};

// a block on its own, from offset 0: the layout of a host vector
template <class Blk, class... Dims> Blk block_at_zero(Dims... dims) {
  Cursor c;
  return Blk(c, (size_t)dims...);
}

// rows of a [rows, src_cap] matrix into a [rows, dst_cap] one: the first min(dst_cap, src_cap) entries of each row (converted:
// the beam's int32 ids widen to int64), `fill` behind them.  A null dst is skipped.
template <class D, class S> void copy_rows_padded(D* dst, size_t dst_cap, const S* src, size_t src_cap, size_t rows, D fill) {
  if (!dst) return;
  const size_t k = std::min(dst_cap, src_cap);
  for (size_t r = 0; r < rows; ++r) {
    std::copy(src + r * src_cap, src + r * src_cap + k, dst + r * dst_cap);
    std::fill(dst + r * dst_cap + k, dst + (r + 1) * dst_cap, fill);
  }
}

struct HostBatchOut { // results of a forward, host side
  int B = 0, L = 0, V = 0, T = 0;
  std::vector<int64_t> ids;        // [B, L]
  std::vector<int32_t> token_num;  // [B]
  std::vector<int32_t> fire_count; // [B]
  std::vector<float> cif_peak;     // [B, peak_len] us_cif_peak (timestamp models), else empty
  int peak_len = 0;
  std::vector<float> logits;       // [B, L, V] host copy (per-thread result slots only)
  bool has_logits = false;
  // decoding extras (Engine::set_decode), empty without the flag: one block each, as the kernel leaves it; *_block() lays it out
  int decode_flags = 0;
  std::vector<float> scores;       // [B, L] log-prob of ids[b, l]
  std::vector<int64_t> ctc, topk, beam, beam_hot, align;   // beam_hot: empty when the search ran unbiased and unfused
  std::vector<int64_t> beam_lm;    // empty when the search ran without a language model; loglik_sum then sits in beam_hot
  bool beam_biased = false;        // a hot-word set biased the search: beam_hot's matched means something
  std::vector<int64_t> nbs;        // empty when the forward ran no n-best search (Engine::set_nbest_search)
  int ctc_cap = 0, topk_k = 0, beam_n = 0, beam_cap = 0, align_h = 0, align_cap = 0, nbs_n = 0;
  CtcBlock ctc_block() const { return block_at_zero<CtcBlock>(B, ctc_cap); }
  TopkBlock topk_block() const { return block_at_zero<TopkBlock>((size_t)B * L, topk_k); }
  BeamBlock beam_block() const { return block_at_zero<BeamBlock>(B, beam_n, beam_cap); }
  BeamHotBlock beam_hot_block() const { return block_at_zero<BeamHotBlock>(B, beam_n); }
  BeamLmBlock beam_lm_block() const { return block_at_zero<BeamLmBlock>(B, beam_n); }
  NbestSearchBlock nbs_block() const { return block_at_zero<NbestSearchBlock>(B, nbs_n, L); }
  AlignBlock align_block() const { return block_at_zero<AlignBlock>(B, align_h, align_cap); }
};

}  // namespace pf
