// pfw.h — the one reader of the PFW1 container (`.pfw`: the recogniser's weights, the FSMN-VAD model, the punctuation
// model, the speaker model; the writer is weights.py pack_pfw).  Host-only: no HIP header beyond common.h, no device call; the caller brings
// the bytes (a file, host memory, or the header copied back from a device-resident image).
//
//   bytes 0 .. 3 "PFW1" | 4 .. 7 version | 8 .. 15 header length (u64) | 16 .. the header, JSON {"config": {..}, "tensors": [..]}
//   | zeros up to the next multiple of 256 | the data section: tensor i at its `offset`, `nbytes` long
//
// Every check is made here, once, with arithmetic that cannot overflow: the magic; the header length, compared unsigned
// against nbytes - 16; a data section that starts inside the image; `config` an object and `tensors` an array; every entry an
// object with dtype "f32" or "u8", offset and nbytes non-negative integers with [offset, offset + nbytes) inside the data
// section, a `shape` array whose dimensions are integers in 1 .. 2^31 - 1 and whose product, checked BEFORE each
// multiplication, stays at or below 2^40 elements, and numel * element size == nbytes.  (Both bounds are far above anything
// real: the widest tensors the converter or a test writes are the recogniser's vocabulary projection and embedding,
// [8404, 512] = 4.3e6 elements; and since nbytes must lie inside the file, a shape is never larger than the file that holds it.)
// A header that is no JSON, or a number where an integer belongs, is refused with the same code.
//
// What differs per caller is the policy, nothing else: the status code and message prefix of a refusal, whether u8 tensors
// are accepted, and the alignment demanded of every offset (the recogniser reads fp32 tensors in place on the device, 16
// bytes at a time; the two models copy them out).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "json.h"

namespace pf {

struct PfwPolicy { int code; const char* prefix; bool allow_u8; int64_t offset_align; };
constexpr PfwPolicy kPfwWeights{PF_ERR_FORMAT, "weights: ", true, 16};
constexpr PfwPolicy kPfwVadModel{PF_ERR_INVALID_ARG, "vad model: ", false, 1};
constexpr PfwPolicy kPfwPuncModel{PF_ERR_INVALID_ARG, "punc model: ", true, 1};
constexpr PfwPolicy kPfwSpkModel{PF_ERR_INVALID_ARG, "spk model: ", false, 1};

[[noreturn]] void pfw_bad(const PfwPolicy& p, const std::string& m);      // throws Error(p.code, p.prefix + m)
// an Error on its way out of a loader: p.code and PF_ERR_UNSUPPORTED pass as they are, anything else (a JSON error from
// the header or from a config field) is recoded to p.code with the prefix in front
[[noreturn]] void pfw_rethrow(const PfwPolicy& p, const Error& e);

// the framing, from the first 16 bytes and the size of the whole image
struct PfwFrame { int64_t header_len = 0, data_off = 0, data_bytes = 0; };        // the header is at 16; data_off is a multiple of 256
PfwFrame pfw_frame(const char* first16, int64_t nbytes, const PfwPolicy& p);

// the index, from the header text and the size of the data section; offsets are relative to the data section
struct PfwEntry { int64_t offset = 0, nbytes = 0, numel = 0; std::vector<int64_t> shape; bool u8 = false; };
struct PfwIndex { Json config; std::map<std::string, PfwEntry> tensors; };
PfwIndex pfw_index(const char* header, int64_t header_len, int64_t data_bytes, const PfwPolicy& p);

// the named f32 tensor of exactly this shape, copied out of the data section (which need not be 4-aligned in memory);
// refused when it is missing, u8, of another shape, or holds a value that is not finite
std::vector<float> pfw_take(const PfwIndex& ix, const char* data, const std::string& name, const std::vector<int64_t>& shape,
                            const PfwPolicy& p);

}  // namespace pf
