// k_spk_cluster.hip — the speaker clustering on the device: exactly the average-linkage agglomeration
// host_spk_cluster (spk.cpp) performs, on the fp32 cosines launch_spk_affinity left on the device.  Same labels, same number
// of speakers, same merge order, and merge heights that are bit for bit the host's doubles.
//
// Two launches per group of streams (a group's work matrices stay within 2 GiB; the engine forms the groups):
//
//   spk_cluster_prep   grid (ceil(nmax / 64), streams), 256 threads.  A workgroup owns a band of 64 rows and walks the 64 x 64
//                      tiles of the upper triangle from its diagonal tile to the right.  Per tile: one coalesced read of S,
//                      widened to fp64 (-2.0 for a cell that is not finite), one coalesced store into sim[row][col], the tile
//                      turned in LDS (65-column pitch) and one coalesced store into sim[col][row].  The lower triangle and the
//                      diagonal of S are never read.  Wave y holds rows y, y + 4, ..; a lane keeps each row's running best over
//                      its columns (ascending, strict >, so the smallest column on a tie), and sixteen wave reductions on
//                      (value, column) at the band's end give every row's first best partner nn0 / its value bv0.
//
//   spk_cluster_merge  grid (streams), 1024 threads: ONE workgroup walks all of a stream's merges.  Only __syncthreads orders
//                      the steps; there is no grid barrier, nothing is shared between workgroups, no atomic is waited on.
//                      Per-cluster state in LDS, 16 bytes per window (128 KB at 8192): the best value bv (double: the arg-max
//                      never gathers from global memory), the best partner nn, the size (0: dead), the union-find parent and
//                      the rescan list, 16 bits each.  Per merge, four barriers:
//                        (a) arg-max of bv over the rows on (value descending, row ascending): strided fold, wave butterfly,
//                            16 partials through LDS; the stop rule;
//                        (b) threads strided over k form (size_i sim[i][k] + size_j sim[j][k]) / (size_i + size_j) — two
//                            products, a sum, a quotient, each rounded on its own — and store it into row i and column i; the
//                            thread of a k > i folds row i's new best partner, the thread of a k < i applies the host's
//                            partner maintenance to row k: onto the rescan list when its partner was i or j, else take i
//                            where it beats (or ties with a smaller index) the cached best; a row between i and j whose
//                            partner was j goes onto the list as well;
//                        (c) one thread updates size, parent, row i's partner and appends (i, j, best) to the trace;
//                        (d) the waves drain the list, one row per wave: lanes stride the live columns beyond the row.
//                      Then, in the same kernel: the minor-cluster rule (one wave per minor cluster), the roots by pointer
//                      jumping, each cluster's earliest window by an LDS minimum, the labels as the rank of that window (a flag
//                      per window and a block prefix count; no sort), labels and n_speakers.
//
// Every loop is bounded by n: at most n - 1 merges, at most n rows on a list, 14 jumping rounds.  A stream is a grid index and
// reads and writes only its own slices, so its result does not depend on what else is in the call.
// No fused multiply-add may be formed: contraction is off for this file (the pragma below and -ffp-contract=off in the
// Makefile), and the quotient is the IEEE-rounded fp64 division.
#include <climits>

#include "kernels.h"

namespace pf {

#pragma clang fp contract(off)

namespace {

constexpr int kClThreads = 1024, kClWaves = kClThreads / 64, kClPerThread = PF_SPK_MAX_WINDOWS / kClThreads;
constexpr int kClNone = INT_MAX;                       // "no row / no partner" in a (value, index) pair: loses every tie
constexpr unsigned short kClNone16 = 0xFFFF;
constexpr int kClJumpRounds = 14;                      // 2^14 > the deepest parent chain (PF_SPK_MAX_WINDOWS links)
static_assert(PF_SPK_MAX_WINDOWS % kClThreads == 0 && PF_SPK_MAX_WINDOWS < kClNone16 && (1 << kClJumpRounds) > PF_SPK_MAX_WINDOWS,
              "the 16-bit indices, the per-thread share and the jumping rounds are sized for PF_SPK_MAX_WINDOWS");

__device__ __forceinline__ double cl_neg_inf() { return -__builtin_huge_val(); }
__device__ __forceinline__ double cl_widen(float v) {
  return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u ? -2.0 : (double)v;
}
// (value descending, index ascending)
__device__ __forceinline__ bool cl_better(double v, int a, double bv, int ba) { return v > bv || (v == bv && a < ba); }
__device__ __forceinline__ void cl_wave_best(double& v, int& a, int from = 32) {
  for (int off = from; off; off >>= 1) {
    const double ov = __shfl_xor(v, off);
    const int oa = __shfl_xor(a, off);
    if (cl_better(ov, oa, v, a)) { v = ov; a = oa; }
  }
}
// the workgroup's best pair in every thread; pv / pa: kClWaves cells nobody else uses until the next barrier but one
__device__ __forceinline__ void cl_block_best(double& v, int& a, double* pv, int* pa) {
  cl_wave_best(v, a);
  if ((threadIdx.x & 63) == 0) { pv[threadIdx.x >> 6] = v; pa[threadIdx.x >> 6] = a; }
  __syncthreads();
  v = pv[threadIdx.x & (kClWaves - 1)];
  a = pa[threadIdx.x & (kClWaves - 1)];
  cl_wave_best(v, a, kClWaves / 2);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ the work matrix
__global__ __launch_bounds__(256) void spk_cluster_prep_kernel(SpkClusterLaunch a) {
  __shared__ double tile[64][65];
  const int s = blockIdx.y, n = a.n[s], ti = blockIdx.x;
  if (ti * 64 >= n) return;
  const float* __restrict__ S = a.S + a.soff[s];
  double* __restrict__ sim = a.sim + (a.soff[s] - a.sim_first);
  const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
  double bv[16];
  int bk[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { bv[r] = cl_neg_inf(); bk[r] = kClNone; }
  for (int tj = ti; tj * 64 < n; ++tj) {
    const int col = tj * 64 + x;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = ti * 64 + y + 4 * r;
      double d = 0.0;
      if (row < n && col < n && col >= row) {
        if (col > row) {
          d = cl_widen(S[(long long)row * n + col]);
          if (d > bv[r]) { bv[r] = d; bk[r] = col; }
        }
        sim[(long long)row * n + col] = d;                       // (the diagonal: 0.0, never read)
      }
      tile[y + 4 * r][x] = d;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {                               // cell (srow, scol) of the tile into sim[scol][srow]
      const int srow = ti * 64 + x, scol = tj * 64 + y + 4 * r;
      if (srow < n && scol < n && scol > srow) sim[(long long)scol * n + srow] = tile[x][y + 4 * r];
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = ti * 64 + y + 4 * r;
    cl_wave_best(bv[r], bk[r]);
    if (x == 0 && row < n) {
      a.nn0[a.woff[s] + row] = bk[r] == kClNone ? -1 : bk[r];
      a.bv0[a.woff[s] + row] = bv[r];
    }
  }
}

// ------------------------------------------------------------------------------------------------ the walk
__global__ __launch_bounds__(kClThreads) void spk_cluster_merge_kernel(SpkClusterLaunch a) {
  extern __shared__ __align__(16) char cl_lds[];
  __shared__ double part_v[2][kClWaves];
  __shared__ int part_a[2][kClWaves];
  __shared__ int wave_total[kClWaves];
  __shared__ int n_list;
  const int s = blockIdx.x, n = a.n[s], tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (n <= 0) {
    if (tid == 0) a.n_speakers[s] = 0;
    return;
  }
  const int np = (a.nmax + 3) & ~3;
  double* bv = (double*)cl_lds;                                  // [np]; after the walk: first [np] | rank [np] as int
  unsigned short* nn = (unsigned short*)(bv + np);
  unsigned short* size = nn + np;
  unsigned short* parent = size + np;
  unsigned short* list = parent + np;
  double* __restrict__ sim = a.sim + (a.soff[s] - a.sim_first);
  const long long w0 = a.woff[s], m0 = a.moff[s];
  int32_t* merges = a.merges ? a.merges + 2 * m0 : nullptr;
  double* heights = a.heights ? a.heights + m0 : nullptr;

  for (int k = tid; k < n; k += kClThreads) {
    const int p = a.nn0[w0 + k];
    nn[k] = p < 0 ? kClNone16 : (unsigned short)p;
    bv[k] = a.bv0[w0 + k];
    size[k] = 1;
    parent[k] = (unsigned short)k;
  }
  if (tid == 0) n_list = 0;
  __syncthreads();

  const double threshold = (double)a.threshold;
  int n_alive = n, n_merges = 0;
  while (n_alive > 1 && !(a.num_speakers > 0 && n_alive <= a.num_speakers)) {          // at most n - 1 turns
    // (a) the pair of largest similarity: the smallest row among the best, and that row's partner
    double best = cl_neg_inf();
    int i = kClNone;
    for (int k = tid; k < n; k += kClThreads)
      if (bv[k] > best) { best = bv[k]; i = k; }
    cl_block_best(best, i, part_v[0], part_a[0]);
    if (i == kClNone || (a.num_speakers <= 0 && best < threshold)) break;
    const int j = nn[i];
    const double si = (double)size[i], sj = (double)size[j], st = (double)((int)size[i] + (int)size[j]);
    // (b) row i and column i, row i's new partner, the partner maintenance of the rows in front of j
    double* __restrict__ ri = sim + (long long)i * n;
    const double* __restrict__ rj = sim + (long long)j * n;
    double rv = cl_neg_inf();
    int rk = kClNone;
    for (int k = tid; k < n; k += kClThreads) {
      if (size[k] == 0 || k == i || k == j) continue;
      const double v = __ddiv_rn(__dadd_rn(__dmul_rn(si, ri[k]), __dmul_rn(sj, rj[k])), st);
      ri[k] = v;
      sim[(long long)k * n + i] = v;
      if (k > i) {
        if (v > rv) { rv = v; rk = k; }
        if (k < j && nn[k] == j) list[atomicAdd(&n_list, 1)] = (unsigned short)k;
      } else {
        const int p = nn[k];
        if (p == j || p == i) list[atomicAdd(&n_list, 1)] = (unsigned short)k;
        else if (v > bv[k] || (v == bv[k] && i < p)) { nn[k] = (unsigned short)i; bv[k] = v; }
      }
    }
    cl_block_best(rv, rk, part_v[1], part_a[1]);
    // (c)
    if (tid == 0) {
      size[i] = (unsigned short)((int)size[i] + (int)size[j]);
      size[j] = 0;
      parent[j] = (unsigned short)i;
      nn[j] = kClNone16; bv[j] = cl_neg_inf();
      nn[i] = rk == kClNone ? kClNone16 : (unsigned short)rk; bv[i] = rv;
      if (merges) { merges[2 * n_merges] = i; merges[2 * n_merges + 1] = j; }
      if (heights) heights[n_merges] = best;
    }
    __syncthreads();
    // (d) one row per wave: the best live column beyond the row, the smallest on a tie
    const int n_rows = n_list;
    for (int q = wave; q < n_rows; q += kClWaves) {
      const int k = list[q];
      const double* __restrict__ rowk = sim + (long long)k * n;
      double v = cl_neg_inf();
      int p = kClNone;
      for (int c = k + 1 + lane; c < n; c += 64)
        if (size[c] != 0 && rowk[c] > v) { v = rowk[c]; p = c; }
      cl_wave_best(v, p);
      if (lane == 0) { nn[k] = p == kClNone ? kClNone16 : (unsigned short)p; bv[k] = v; }
    }
    __syncthreads();
    if (tid == 0) n_list = 0;
    --n_alive;
    ++n_merges;
  }
  __syncthreads();
  for (int m = n_merges + tid; m < n - 1; m += kClThreads) {     // the unused rows of the trace
    if (merges) { merges[2 * m] = -1; merges[2 * m + 1] = -1; }
    if (heights) heights[m] = 0.0;
  }

  // ---- the minor-cluster rule: a live cluster below min_cluster joins the major one it is most similar to, if there is one
  if (a.num_speakers <= 0) {
    int major = 0;
    for (int k = tid; k < n; k += kClThreads) major |= size[k] != 0 && (int)size[k] >= a.min_cluster;
    if (__syncthreads_or(major)) {
      for (int k = tid; k < n; k += kClThreads)
        if (size[k] != 0 && (int)size[k] < a.min_cluster) list[atomicAdd(&n_list, 1)] = (unsigned short)k;
      __syncthreads();
      const int n_rows = n_list;
      for (int q = wave; q < n_rows; q += kClWaves) {
        const int c = list[q];
        const double* __restrict__ rowc = sim + (long long)c * n;
        double v = cl_neg_inf();
        int t = kClNone;
        for (int k = lane; k < n; k += 64)
          if ((int)size[k] >= a.min_cluster && size[k] != 0 && rowc[k] > v) { v = rowc[k]; t = k; }
        cl_wave_best(v, t);
        if (lane == 0 && t != kClNone) parent[c] = (unsigned short)t;          // (sizes stay: they say who is major)
      }
    }
  }
  __syncthreads();

  // ---- every window's final cluster: pointer jumping, every round reads all grandparents before it writes any
  for (int r = 0; r < kClJumpRounds; ++r) {
    unsigned short up[kClPerThread];
#pragma unroll
    for (int e = 0; e < kClPerThread; ++e) {
      const int k = tid + e * kClThreads;
      up[e] = k < n ? parent[parent[k]] : 0;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kClPerThread; ++e) {
      const int k = tid + e * kClThreads;
      if (k < n) parent[k] = up[e];
    }
    __syncthreads();
  }
  // ---- labels in the order of each cluster's earliest window
  int* first = (int*)bv;
  int* rank = first + np;
  for (int k = tid; k < n; k += kClThreads) first[k] = kClNone;
  __syncthreads();
  for (int k = tid; k < n; k += kClThreads) atomicMin(&first[parent[k]], k);
  __syncthreads();
  int count = 0;                                                  // windows tid * 8 .. + 8: how many open a cluster
  unsigned flags = 0;
#pragma unroll
  for (int e = 0; e < kClPerThread; ++e) {
    const int k = tid * kClPerThread + e;
    if (k < n && first[parent[k]] == k) { flags |= 1u << e; ++count; }
  }
  int incl = count;
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(incl, off);
    if (lane >= off) incl += up;
  }
  if (lane == 63) wave_total[wave] = incl;
  __syncthreads();
  int before = incl - count, total = 0;
  for (int w = 0; w < kClWaves; ++w) {
    if (w < wave) before += wave_total[w];
    total += wave_total[w];
  }
#pragma unroll
  for (int e = 0; e < kClPerThread; ++e)
    if (flags & (1u << e)) rank[tid * kClPerThread + e] = before++;
  __syncthreads();
  for (int k = tid; k < n; k += kClThreads) a.labels[w0 + k] = rank[first[parent[k]]];
  if (tid == 0) a.n_speakers[s] = total;
}

namespace {
void cl_check(const SpkClusterLaunch& a) {
  PF_CHECK(a.S && a.n && a.woff && a.soff && a.moff && a.sim && a.nn0 && a.bv0 && a.labels && a.n_speakers && a.streams <= 65535 &&
               a.nmax <= PF_SPK_MAX_WINDOWS,
           PF_ERR_INVALID_ARG, "spk cluster: bad operand");
}
}  // namespace

void launch_spk_cluster_prep(hipStream_t s, const SpkClusterLaunch& a) {
  if (a.streams <= 0 || a.nmax <= 0) return;
  cl_check(a);
  hipLaunchKernelGGL(spk_cluster_prep_kernel, dim3((unsigned)cdiv(a.nmax, 64), (unsigned)a.streams), dim3(256), 0, s, a);
  PF_HIP(hipGetLastError());
}

void launch_spk_cluster_merge(hipStream_t s, const SpkClusterLaunch& a) {
  if (a.streams <= 0) return;
  cl_check(a);
  static DeviceOnce once;
  once.run([] { set_max_lds((const void*)spk_cluster_merge_kernel, 16 * PF_SPK_MAX_WINDOWS); });
  const size_t lds = (size_t)16 * (size_t)std::max((a.nmax + 3) & ~3, 4);
  hipLaunchKernelGGL(spk_cluster_merge_kernel, dim3((unsigned)a.streams), dim3(kClThreads), lds, s, a);
  PF_HIP(hipGetLastError());
}

}  // namespace pf
