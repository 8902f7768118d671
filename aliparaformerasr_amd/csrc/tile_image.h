// tile_image.h — the weight image the row-tile kernels read (k_vadnet.hip, k_punc.hip through tile_rows.h): the descriptor
// of one matrix product, the builders that append to an image, and the float64 host twin of a product.  The bodies are in
// pfw.cpp.  Host-only: no HIP header beyond common.h.
#pragma once
#include <vector>

#include "common.h"

namespace pf {

// one matrix product of a device image: W [N, K] fp32 as f16 fragments of the 32x32x16 MFMA, rows padded to Npad (a
// multiple of 32) and columns to Kpad (a multiple of 16) with zeros: halves [Npad / 32][Kpad / 16][64 lanes][8], lane
// (r = lane & 31, h = lane >> 5) holding W[32 nt + r][16 ks + 8 h + j]; bias fp32 [Npad] (zeros where the product has none)
struct TileGemm { int64_t w_off = 0, b_off = 0; int N = 0, K = 0, Npad = 0, Kpad = 0; };

// the builders of such an image: both append at the next 256-byte boundary and return the offset(s).  add_gemm rounds the
// weights to f16 (rounding point R0 of both kernels); add_floats copies fp32 rows [rows, cols] to a row stride of ld
TileGemm add_gemm(std::vector<char>& img, const std::vector<float>& w, const std::vector<float>* bias, int N, int K);
int64_t add_floats(std::vector<char>& img, const float* src, int64_t rows, int64_t cols, int64_t ld);

// the host twin of one product: y [T, N] = x [T, K] W^T + b (b may be null) in float64, optional ReLU
void affine64(const std::vector<double>& x, int64_t T, int K, const std::vector<float>& w, const std::vector<float>* b, int N, bool relu,
              std::vector<double>& y);

}  // namespace pf
