// op_stage.h — the staging kit of the stand-alone operator entry points (Engine::op_*, engine_ops.cpp / engine_int8.cpp): what an
// op does around its launch and none of its arithmetic.  Carve a workspace, upload, put a hostile pattern behind the operands,
// sentinel-fill the outputs, check what was written, copy the result back.
//
// The first part is host-only (no HIP header: tests/native/op_stage_sanitize.cpp includes it alone): the sentinels, the hostile
// patterns, the blocked activation layout, the guard rule and the typed carve.  The second part (uploads, fills, the check on a
// device buffer, downloads) is compiled where common.h came first.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "decode_blocks.h"

namespace pf {

// ---- sentinels: what an output buffer holds before the launch (NaN payloads no kernel computes; the byte outputs run twice)
constexpr uint32_t kSentinel32 = 0x7FC5A5A5u;                 // as an int32 no row / column sum or dz word either
constexpr uint16_t kSentinel16 = 0x7E5Au;
constexpr uint8_t kSentinel8[2] = {0x5A, 0xA5};
constexpr uint16_t kPoison16 = 0x7A5Au;                       // 52 032 as f16; two of them are 2.8e35 as an fp32 word

// ---- hostile patterns: large finite values for the cells a contract only calls readable, never the same in neighbouring cells
inline uint16_t hostile16_bits(size_t i) {                    // +-32768 .. +-65504 as f16
  return (uint16_t)(0x7800u | (uint16_t)((i * 37u) & 0x3FFu) | (uint16_t)((i & 1u) << 15));
}
inline _Float16 hostile16(size_t i) {
  const uint16_t bits = hostile16_bits(i);
  _Float16 h;
  std::memcpy(&h, &bits, 2);
  return h;
}
inline float hostile32(size_t i) {                            // +-2^100 .. 2^101
  return std::ldexp(1.0f + (float)((i * 37u) & 0x3FFu) / 1024.0f, 100) * ((i & 1u) ? -1.0f : 1.0f);
}
inline int32_t hostile_i32(size_t i) { return ((i & 1u) ? -1 : 1) * ((1 << 30) + (int32_t)((i * 37u) & 0xFFFFu)); }

// ---- the blocked activation layout: element (m, k) of a matrix of Kp columns (Kp % 8 == 0; 32-row blocks of 8-column groups)
inline size_t blocked_index(int64_t m, int64_t k, int64_t Kp) {
  return (((size_t)(m >> 5) * (size_t)(Kp >> 3) + (size_t)(k >> 3)) * 32 + (size_t)(m & 31)) * 8 + (size_t)(k & 7);
}

// ---- the guard rule.  A buffer of rows x ld cells held `before` (or the sentinel everywhere) at the launch and holds `after`
// now.  Inside [0, M) x [0, N) every cell must have been written (must_write: it no longer holds the sentinel); a cell in a
// column [N, ld) or in a row at or beyond guard_row keeps its bits; rows [M, guard_row) x [0, N) are the padding a kernel
// declares writable.  blocked: the blocked activation layout (ld == N).
struct GuardGeom {
  int64_t rows, ld, M, N, guard_row;
  bool blocked, must_write;
};
enum class GuardFault { none, not_written, column_written, row_written, runs_differ };
struct GuardHit {
  GuardFault fault = GuardFault::none;
  int64_t m = 0, n = 0;
  explicit operator bool() const { return fault != GuardFault::none; }
};
inline const char* guard_reason(GuardFault f) {
  return f == GuardFault::not_written ? "was not written"
       : f == GuardFault::column_written ? "was written: a column beyond N"
       : f == GuardFault::row_written ? "was written: a row the kernel's contract (kernels.h) calls never written"
       : f == GuardFault::runs_differ ? "differs between two runs" : "";
}
// the first offending cell in row order; U = uint8_t / uint16_t / uint32_t; before == nullptr: the sentinel everywhere
template <class U>
GuardHit guard_scan(const U* after, const U* before, U sentinel, const GuardGeom& g) {
  for (int64_t m = 0; m < g.rows; ++m)
    for (int64_t n = 0; n < g.ld; ++n) {
      const size_t i = g.blocked ? blocked_index(m, n, g.N) : (size_t)(m * g.ld + n);
      if (m < g.M && n < g.N) {
        if (g.must_write && after[i] == sentinel) return GuardHit{GuardFault::not_written, m, n};
      } else if ((n >= g.N || m >= g.guard_row) && after[i] != (before ? before[i] : sentinel)) {
        return GuardHit{n >= g.N ? GuardFault::column_written : GuardFault::row_written, m, n};
      }
    }
  return GuardHit{};
}
// "<what> (M x N, ld L): cell (m, n) <reason>"; row0: the buffer's row that the image's row 0 is
inline std::string guard_message(const std::string& what, const GuardGeom& g, const GuardHit& h, int64_t row0 = 0) {
  return what + " (" + std::to_string(g.M) + " x " + std::to_string(g.N) + ", ld " + std::to_string(g.ld) + "): cell (" +
         std::to_string(row0 + h.m) + ", " + std::to_string(h.n) + ") " + guard_reason(h.fault);
}
// the two runs of a byte output (a byte has no value a code cannot take): the first cell of [0, M) x [0, N) that holds its run's
// sentinel after both (not_written: neither run wrote it) or that differs between the runs (runs_differ)
inline GuardHit bytes_written_scan(const uint8_t* a0, const uint8_t* a1, int64_t ld, int64_t M, int64_t N) {
  for (int64_t m = 0; m < M; ++m)
    for (int64_t n = 0; n < N; ++n) {
      const size_t i = (size_t)(m * ld + n);
      if (a0[i] == kSentinel8[0] && a1[i] == kSentinel8[1]) return GuardHit{GuardFault::not_written, m, n};
      if (a0[i] != a1[i]) return GuardHit{GuardFault::runs_differ, m, n};
    }
  return GuardHit{};
}

// ---- the typed carve: fields of one allocation in declaration order, each starting at a multiple of `align` (Carve's rounding,
// Field's typed pointers).  An op names a buffer's element type once: `const auto dA = st.take<half_t>(n)` before the allocation
// exists, `dA(ws)` after it.
struct StageCarve {
  size_t off = 0, align = 256;
  template <class T> Field<T> take(size_t count) {
    const Field<T> f{off, count};
    off += (count * sizeof(T) + align - 1) / align * align;
    return f;
  }
};

// ---- `const auto done = at_exit([&] { ... });`: what an op undoes on every way out (state a launch helper left on the engine)
template <class F> struct AtExit {
  F f;
  ~AtExit() { f(); }
};
template <class F> AtExit<F> at_exit(F f) { return AtExit<F>{f}; }

}  // namespace pf

// ------------------------------------------------------------------ the device-facing part -------
#ifdef PF_HIP
#include "kernels.h"

namespace pf {

// ---- uploads (host -> device on stream s).  The plain forms are asynchronous: the source lives until the op's next
// synchronisation.  A form that builds its image on the host waits for its copy.
template <class T> void upload(hipStream_t s, T* dst, const T* src, size_t count) {
  if (count) PF_HIP(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, s));
}
template <class T> void upload_sync(hipStream_t s, T* dst, const std::vector<T>& h) {
  upload(s, dst, h.data(), h.size());
  PF_HIP(hipStreamSynchronize(s));
}
// rows x width cells between two row strides (in cells)
template <class T> void upload2d(hipStream_t s, T* dst, size_t ld_dst, const T* src, size_t ld_src, size_t width, size_t rows) {
  PF_HIP(hipMemcpy2DAsync(dst, ld_dst * sizeof(T), src, ld_src * sizeof(T), width * sizeof(T), rows, hipMemcpyHostToDevice, s));
}
// the dense fp32 host matrix [rows, cols] as f16 with row stride ld, through the fp32 staging slot (waits: the slot is reused)
inline void upload_f16(hipStream_t s, float* slot, const float* src, int64_t rows, int cols, half_t* dst, int ld) {
  upload(s, slot, src, (size_t)rows * cols);
  launch_f32_to_f16(s, slot, rows, cols, cols, dst, ld);
  PF_HIP(hipStreamSynchronize(s));
}
// rows [row0, row1) of a row-major f16 matrix: columns [0, cols) hostile (index (row) * 131 + c), [cols, ld) zero
inline void fill_hostile_rows(hipStream_t s, half_t* base, int ld, int64_t row0, int64_t row1, int cols) {
  if (row1 <= row0) return;
  std::vector<half_t> h((size_t)(row1 - row0) * ld, (half_t)0.f);
  for (int64_t r = 0; r < row1 - row0; ++r)
    for (int c = 0; c < cols; ++c) h[(size_t)r * ld + c] = hostile16((size_t)(row0 + r) * 131 + c);
  upload_sync(s, base + (size_t)row0 * ld, h);
}
// rows [row0, row1) of a row-major fp32 matrix [*, ld]: hostile, indexed from the start of the filled range
inline void fill_hostile_rows32(hipStream_t s, float* base, int ld, int64_t row0, int64_t row1) {
  if (row1 <= row0) return;
  std::vector<float> h((size_t)(row1 - row0) * ld);
  for (size_t i = 0; i < h.size(); ++i) h[i] = hostile32(i);
  upload_sync(s, base + (size_t)row0 * ld, h);
}
// an f16 GEMM operand [Mp, ld] of the fp32 host matrix [M, K]: the K pad columns zero (that IS the contract), rows [M, Mp) hostile
inline void upload_operand16(hipStream_t s, float* slot, const float* src, int M, int K, half_t* dst, int ld, int64_t Mp) {
  PF_HIP(hipMemsetAsync(dst, 0, (size_t)Mp * ld * 2, s));
  fill_hostile_rows(s, dst, ld, M, Mp, K);
  upload_f16(s, slot, src, M, K, dst, ld);
}
// the same operand in the blocked activation layout (Kp columns), laid out on the host: independent of the kernels' index arithmetic
inline void upload_blocked16(hipStream_t s, const float* src, int M, int K, half_t* dst, int Kp, int64_t Mp) {
  std::vector<half_t> img((size_t)Mp * Kp, (half_t)0.f);
  for (int64_t m = 0; m < Mp; ++m)
    for (int k = 0; k < K; ++k) img[blocked_index(m, k, Kp)] = m < M ? (half_t)src[(size_t)m * K + k] : hostile16((size_t)m * 131 + k);
  upload_sync(s, dst, img);
}
// device image [rows, ld] of the host matrix src [m, n] (dense rows; null: nothing inside), hostile everywhere else (indexed
// over the whole image)
inline void upload_hostile32(hipStream_t s, float* dev, int64_t rows, int ld, const float* src, int m, int n) {
  std::vector<float> h((size_t)rows * ld);
  for (size_t i = 0; i < h.size(); ++i) h[i] = hostile32(i);
  if (src)
    for (int r = 0; r < m; ++r) std::memcpy(&h[(size_t)r * ld], src + (size_t)r * n, (size_t)n * 4);
  upload_sync(s, dev, h);
}
// [k, D] taps of the [D, k] FSMN weight, as the pipeline keeps them
inline std::vector<float> fsmn_taps(const float* w, int D, int k) {
  std::vector<float> wT((size_t)D * k);
  for (int c = 0; c < D; ++c)
    for (int j = 0; j < k; ++j) wT[(size_t)j * D + c] = w[(size_t)c * k + j];
  return wT;
}

// ---- sentinel fill of `count` cells of 2 or 4 bytes
template <class T> void fill_sentinel(hipStream_t s, T* p, size_t count) {
  static_assert(sizeof(T) == 2 || sizeof(T) == 4, "sentinel cells are 16 or 32 bits wide");
  if (sizeof(T) == 4) PF_HIP(hipMemsetD32Async((hipDeviceptr_t)p, (int)kSentinel32, count, s));
  else PF_HIP(hipMemsetD16Async((hipDeviceptr_t)p, kSentinel16, count, s));
}

// ---- the guard rule on a device buffer: download g.rows x g.ld cells, scan, throw PF_ERR_DEVICE naming `what` ("op: buffer"),
// M x N, ld, the cell and the reason.  Returns the image.  before: what the buffer held at the launch (null: the sentinel).
template <class U>
std::vector<U> check_guard(hipStream_t s, const std::string& what, const void* dev, U sentinel, const GuardGeom& g,
                           const std::vector<typename std::common_type<U>::type>* before = nullptr, int64_t row0 = 0) {
  std::vector<U> h((size_t)(g.rows * g.ld));
  if (!h.empty()) PF_HIP(hipMemcpyAsync(h.data(), dev, h.size() * sizeof(U), hipMemcpyDeviceToHost, s));
  PF_HIP(hipStreamSynchronize(s));
  if (const GuardHit hit = guard_scan<U>(h.data(), before ? before->data() : nullptr, sentinel, g))
    throw Error(PF_ERR_DEVICE, guard_message(what, g, hit, row0));
  return h;
}
// the usual geometries: a sentinel-filled result [rows, ld] of which [M, N] is written and rows from guard_row on are not
inline GuardGeom result_geom(int64_t rows, int M, int N, int ld, int64_t guard_row, bool blocked = false, bool must_write = true) {
  return GuardGeom{rows, ld, M, N, guard_row, blocked, must_write};
}
// `cells` sentinel cells that nothing may have touched (the bytes behind a workspace, a buffer a form does not use)
inline GuardGeom untouched_geom(int64_t rows, int64_t ld = 1) { return GuardGeom{rows, ld, 0, ld, 0, false, false}; }

// ---- downloads (device -> host on stream s; asynchronous unless they convert)
template <class T> void download(hipStream_t s, T* dst, const T* src, size_t count) {
  if (count) PF_HIP(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, s));
}
template <class T> void download2d(hipStream_t s, T* dst, size_t ld_dst, const T* src, size_t ld_src, size_t width, size_t rows) {
  PF_HIP(hipMemcpy2DAsync(dst, ld_dst * sizeof(T), src, ld_src * sizeof(T), width * sizeof(T), rows, hipMemcpyDeviceToHost, s));
}
// [M, N] of a row-major f16 matrix with row stride ld as the caller's dense fp32 (waits)
inline void download_f16(hipStream_t s, float* out, const half_t* dev, int64_t M, int N, int ld) {
  std::vector<half_t> h((size_t)M * ld);
  download(s, h.data(), dev, h.size());
  PF_HIP(hipStreamSynchronize(s));
  for (int64_t m = 0; m < M; ++m)
    for (int n = 0; n < N; ++n) out[(size_t)m * N + n] = (float)h[(size_t)m * ld + n];
}
// columns [c0, c0 + n) of rows [0, M) of a blocked f16 matrix of Np columns as the caller's row-major fp32 [M, n] (waits)
inline void download_blocked16(hipStream_t s, float* out, const half_t* dev, int M, int Np, int c0, int n) {
  std::vector<half_t> h((size_t)round_up(M, 32) * Np);
  download(s, h.data(), dev, h.size());
  PF_HIP(hipStreamSynchronize(s));
  for (int m = 0; m < M; ++m)
    for (int c = 0; c < n; ++c) out[(size_t)m * n + c] = (float)h[blocked_index(m, c0 + c, Np)];
}

}  // namespace pf
#endif  // PF_HIP
