// k_consensus.hip — consensus (minimum-Bayes-risk) choice and per-token confidence inside n-best lists.
//
// The definition is tests/consensus_ref.py, the host twin host_consensus (hostutil.cpp).  A LIST is N <= 64 hypotheses of up to
// 255 int32 ids with float64 weights p.  D[i][j] is the unit-cost Levenshtein distance, risk_i = sum_j p_j D[i][j] (float64,
// j ascending, product and sum rounded separately), the winner w is the first i of minimal risk, m_j is the match mask of the
// canonical alignment of h_j to h_w (diagonal before up before left on the way back) and conf[t] = sum_j p_j m_j[t].  Every
// value is an integer or a float64 sum in a fixed order: the results are bit for bit the definition's.
//
// TWO LAUNCHES, the boundary between them the only dependence between workgroups; no atomics.
//
// 1. consensus_dist: ONE WAVE PER UNORDERED PAIR, four waves per workgroup that never need each other (no barrier).  A list of
//    N hypotheses is N (N - 1) / 2 + 1 work items: its pairs in row order and one item that zeroes its diagonal (so N = 1 is no
//    special case); a wave finds its list by bisection in the item offsets and peels the pair index off row by row.
//    The LONGER sequence of the pair lies along the lanes, FOUR COLUMNS PER LANE, its ids in registers; the shorter one goes
//    to the wave's 1 KB of LDS and the wave walks its rows in SKEWED order: at step s lane l updates row s - l + 1, so the cell
//    to its left (the last column of lane l - 1, same row) was finished one step earlier and arrives through ONE __shfl_up,
//    and the diagonal cell is the value that arrived the step before.  A lane keeps the previous row of its four columns in
//    registers; the row's id comes from LDS (each lane another row: no broadcast is possible in the skew).  ceil(n_long / 4) +
//    n_short - 1 steps, each four min-plus cells per lane.  Lanes beyond the length compute cells nobody reads and load
//    nothing.  The distance is read off the lane that owns the last column and stored to D[i][j] and D[j][i].
//    Min-plus over integers is not a matrix product: the matrix cores have no part here.
//
// 2. consensus_pick: ONE WORKGROUP PER LIST, four waves.  Lane i < N sums risk_i over its row of D; wave 0 reduces the key
//    (risk, index) through shfl_xor.  Then the waves share out j = wave, wave + 4, ..: h_w lies in LDS for all, h_j along the
//    lanes as above (never swapped: the preferences of the way back are not symmetric), and next to each cell the wave
//    records two bits, "the diagonal step explains this cell" and "the up step does": one byte per lane and row, 16 KB per
//    wave.  The way back is at most 510 dependent byte reads, wave-uniform; a lane collects the match bits of rows 4 lane ..
//    4 lane + 3 and leaves them in LDS.  After a barrier thread t < n_w adds p_j over the j whose bit is set, j ascending.
//
// Nothing at or beyond a list's extent is read or stored: ids are loaded under `column < length`, D only inside the list's
// N x N block, conf is the list's own 256 cells (those from n_w on are stored as 0).
#include "kernels.h"

namespace pf {

namespace {

constexpr int kConsWaves = 4, kConsThreads = 64 * kConsWaves, kConsRows = 256;
// consensus_pick's LDS: direction bytes [waves][256 rows][64 lanes] | h_w | h_j per wave | masks [64][64] | p [64] | the winner
constexpr size_t kPickDirBytes = (size_t)kConsWaves * kConsRows * 64;
constexpr size_t kPickLdsBytes = kPickDirBytes + kConsRows * 4 + (size_t)kConsWaves * kConsRows * 4 + 64 * 64 + 64 * 8 + 16;

// the lane's four ids of a sequence of n (columns 4 lane + 1 .. 4 lane + 4 of the table); nothing is loaded at or beyond n
__device__ __forceinline__ void load4(const int32_t* __restrict__ y, int n, int lane, int32_t (&v)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = 4 * lane + k < n ? y[4 * lane + k] : 0;
}

// one skewed step of the lane's four cells of row a (x = the row's id): prev = the row above, diag = the cell above the left
// boundary, lf = the left boundary.  Returns the two direction bits per cell (bit 2k: diagonal admissible, bit 2k + 1: up)
__device__ __forceinline__ uint32_t cell4(int32_t x, const int32_t (&y)[4], int32_t (&prev)[4], int32_t diag, int32_t lf) {
  uint32_t bits = 0;
  int32_t left = lf, dg = diag;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int32_t sub = dg + (x != y[k] ? 1 : 0), up = prev[k] + 1;
    const int32_t c = min(min(sub, up), left + 1);
    bits |= (c == sub ? 1u : 0u) << (2 * k) | (c == up ? 2u : 0u) << (2 * k);
    dg = prev[k];
    prev[k] = c;
    left = c;
  }
  return bits;
}

}  // namespace

__global__ __launch_bounds__(kConsThreads) void consensus_dist_kernel(ConsensusLaunch a) {
  __shared__ int32_t rows_lds[kConsWaves][kConsRows];
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const int64_t item = (int64_t)blockIdx.x * kConsWaves + wave;
  if (item >= a.item_off[a.L]) return;                 // wave-uniform
  int lo = 0, hi = a.L - 1;                            // the list: the last l with item_off[l] <= item
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.item_off[mid] <= item) lo = mid; else hi = mid - 1;
  }
  const int h0 = a.hyp_off[lo], N = a.hyp_off[lo + 1] - h0;
  int32_t* D = a.D + a.d_off[lo];
  int p = (int)(item - a.item_off[lo]);
  if (p == N * (N - 1) / 2) {                          // the list's diagonal
    if (lane < N) D[lane * N + lane] = 0;
    return;
  }
  int i = 0;
  while (p >= N - 1 - i) { p -= N - 1 - i; ++i; }
  const int j = i + 1 + p;
  const int ni = a.len[h0 + i], nj = a.len[h0 + j];
  const bool i_long = ni >= nj;
  const int nl = i_long ? ni : nj, ns = i_long ? nj : ni;
  const int32_t* yl = a.ids + a.id_off[h0 + (i_long ? i : j)];
  const int32_t* ys = a.ids + a.id_off[h0 + (i_long ? j : i)];
  int dist = nl;                                       // an empty shorter sequence
  if (ns > 0) {
    int32_t* xs = rows_lds[wave];
    for (int t = lane; t < ns; t += 64) xs[t] = ys[t];
    __builtin_amdgcn_wave_barrier();
    int32_t y[4], prev[4];
    load4(yl, nl, lane, y);
#pragma unroll
    for (int k = 0; k < 4; ++k) prev[k] = 4 * lane + 1 + k;
    int32_t diag = 4 * lane;
    const int steps = (nl + 3) / 4 + ns - 1;
    for (int s = 0; s < steps; ++s) {
      const int r = s - lane + 1;                      // this lane's row
      int32_t lf = __shfl_up(prev[3], 1);
      if (lane == 0) lf = r;
      if (r >= 1 && r <= ns) {
        cell4(xs[r - 1], y, prev, diag, lf);
        diag = lf;
      }
    }
    const int32_t last = (nl - 1) & 3;
    const int32_t v = last == 0 ? prev[0] : last == 1 ? prev[1] : last == 2 ? prev[2] : prev[3];
    dist = __shfl(v, (nl - 1) >> 2);
  }
  if (lane == 0) { D[i * N + j] = dist; D[j * N + i] = dist; }
}

// Every float64 product and sum below is rounded on its own.  The compiler contracts a * b + c into one fused operation by
// default, and __dmul_rn / __dadd_rn do not stop it (they are plain operators inlined from a header compiled with contraction
// on), so the kernel writes plain operators and switches contraction off for its whole body.
__global__ __launch_bounds__(kConsThreads) void consensus_pick_kernel(ConsensusLaunch a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char cp_lds[];
  uint8_t* dir_all = reinterpret_cast<uint8_t*>(cp_lds);
  int32_t* xw = reinterpret_cast<int32_t*>(cp_lds + kPickDirBytes);
  int32_t* yj_all = xw + kConsRows;
  uint8_t* mask = reinterpret_cast<uint8_t*>(yj_all + kConsWaves * kConsRows);          // [j][lane]: rows 4 lane .. 4 lane + 3
  double* ps = reinterpret_cast<double*>(mask + 64 * 64);
  int* win = reinterpret_cast<int*>(ps + 64);

  const int l = (int)blockIdx.x, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int h0 = a.hyp_off[l], N = a.hyp_off[l + 1] - h0;
  const int32_t* D = a.D + a.d_off[l];

  // risk (the product rounded, then added), and the winner on the key (risk, index)
  if (wave == 0) {
    double risk = __builtin_huge_val();
    if (lane < N) {
      ps[lane] = a.p[h0 + lane];
      risk = 0.0;
      for (int j = 0; j < N; ++j) {
        const double term = a.p[h0 + j] * (double)D[lane * N + j];
        risk = risk + term;
      }
      a.risk[h0 + lane] = risk;
    }
    int idx = lane < N ? lane : 64;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double r2 = __shfl_xor(risk, d);
      const int i2 = __shfl_xor(idx, d);
      if (r2 < risk || (r2 == risk && i2 < idx)) { risk = r2; idx = i2; }
    }
    if (lane == 0) { *win = idx; a.winner[l] = idx; }
  }
  __syncthreads();
  const int w = *win;
  const int nw = a.len[h0 + w];
  const int32_t* hw = a.ids + a.id_off[h0 + w];
  for (int t = tid; t < nw; t += kConsThreads) xw[t] = hw[t];
  __syncthreads();

  uint8_t* dir = dir_all + (size_t)wave * kConsRows * 64;
  int32_t* yj = yj_all + wave * kConsRows;
  for (int j = wave; j < N; j += kConsWaves) {         // wave-uniform
    const int nj = a.len[h0 + j];
    const int32_t* hj = a.ids + a.id_off[h0 + j];
    uint32_t mm = 0;
    if (nw > 0 && nj > 0) {
      int32_t y[4], prev[4];
      load4(hj, nj, lane, y);
#pragma unroll
      for (int k = 0; k < 4; ++k) { prev[k] = 4 * lane + 1 + k; if (4 * lane + k < nj) yj[4 * lane + k] = y[k]; }
      int32_t diag = 4 * lane;
      const int steps = (nj + 3) / 4 + nw - 1;
      for (int s = 0; s < steps; ++s) {
        const int r = s - lane + 1;
        int32_t lf = __shfl_up(prev[3], 1);
        if (lane == 0) lf = r;
        if (r >= 1 && r <= nw) {
          dir[(r - 1) * 64 + lane] = (uint8_t)cell4(xw[r - 1], y, prev, diag, lf);
          diag = lf;
        }
      }
      __builtin_amdgcn_wave_barrier();
      // the way back from (nw, nj), the same walk in every lane; a border ends it (forced up steps match nothing)
      int r = nw, c = nj;
      while (r > 0 && c > 0) {
        const uint32_t b = (uint32_t)dir[(r - 1) * 64 + ((c - 1) >> 2)] >> (2 * ((c - 1) & 3));
        if (b & 1u) {
          if (xw[r - 1] == yj[c - 1] && ((r - 1) >> 2) == lane) mm |= 1u << ((r - 1) & 3);
          --r; --c;
        } else if (b & 2u) {
          --r;
        } else {
          --c;
        }
      }
      __builtin_amdgcn_wave_barrier();                 // the next j overwrites dir and yj
    }
    mask[j * 64 + lane] = (uint8_t)mm;
  }
  __syncthreads();
  double conf = 0.0;
  if (tid < nw)
    for (int j = 0; j < N; ++j)
      if ((mask[j * 64 + (tid >> 2)] >> (tid & 3)) & 1) conf = conf + ps[j];
  a.conf[(int64_t)l * kConsRows + tid] = conf;
}

void launch_consensus_dist(hipStream_t s, const ConsensusLaunch& a, int64_t items) {
  PF_CHECK(a.L >= 1 && a.L <= PF_CONSENSUS_MAX_LISTS && items >= a.L, PF_ERR_INVALID_ARG, "consensus: bad shape");
  hipLaunchKernelGGL(consensus_dist_kernel, dim3((unsigned)((items + kConsWaves - 1) / kConsWaves)), dim3(kConsThreads), 0, s, a);
  PF_HIP(hipGetLastError());
}

void launch_consensus_pick(hipStream_t s, const ConsensusLaunch& a) {
  PF_CHECK(a.L >= 1 && a.L <= PF_CONSENSUS_MAX_LISTS, PF_ERR_INVALID_ARG, "consensus: bad shape");
  static DeviceOnce once;
  once.run([] { set_max_lds((const void*)consensus_pick_kernel, (int)kPickLdsBytes); });
  hipLaunchKernelGGL(consensus_pick_kernel, dim3((unsigned)a.L), dim3(kConsThreads), kPickLdsBytes, s, a);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
