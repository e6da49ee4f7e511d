// libh3d.so: the reductions under the reference's QC figures
// (analysis/plotting.py, plotting/*.py), which return arrays here instead of
// an axis:
//
//  * h3d_group_sums[_dev]   per-key column sums (the distance-dependence
//    curves of plotting/distance_dependence.py:34-43, the per-distance means
//    of plotting/dispersion.py:133-144, :182-183);
//  * h3d_histogram[_dev]    np.histogram with explicit edges
//    (plotting/histograms.py);
//  * h3d_ma_stats           condition means, M, A and the series label of
//    every pixel (analysis/plotting.py:307, plotting/ma.py:71-72, :131-155);
//  * h3d_density_grid       per-class np.histogram2d of a point cloud;
//  * h3d_rank_average       scipy.stats.rankdata(method='average') per column;
//  * h3d_corr_matrix        centred Pearson matrix of R columns;
//  * h3d_pixel_moments      per-pixel mean and ddof=1 variance over one
//    condition's replicates (analysis/plotting.py:128-129);
//  * h3d_balance_pixels     raw / (bias[row] * bias[col]) per replicate
//    (analysis/plotting.py:46-48).
//
// Every floating-point sum has one association, fixed by constants of this
// file alone (kSlices, kChunk, kSuper, kTile, the block size) and by the
// data's order: lane-strided running sums, an LDS tree per block, per-block
// partials, a final pass over the partials. No floating-point atomics; a
// rerun, another grid or another ctx gives the same bits. Counts are integer
// atomics (exact in any order).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "h3d.h"
#include "h3d_ctx.h"
#include "h3d_cub.h"
#include "h3d_devutil.h"
#include "h3d_errors.h"
#include "h3d_model.h"

#pragma clang fp contract(off)

using namespace h3dint;
using h3derr::fail;

namespace h3ddiag {

constexpr int kBlock = kLaunchBlock;
static_assert(kBlock == 256, "the reductions below are written for 256 lanes");
constexpr int kMaxKeys = 4096;   // K of h3d_group_sums
constexpr int kMaxCols = 64;     // C of h3d_group_sums
constexpr int kMaxEdges = 4097;  // bin edges per axis
constexpr int kMaxCorr = 32;     // columns of h3d_corr_matrix / h3d_rank_average
constexpr int kSlices = 16;      // partial sums per key (group sums)
constexpr int kChunk = 4096;     // rows per partial column sum (corr means)
constexpr int kTile = 128;       // rows per LDS tile of deviations
constexpr int kTileLd = kTile + 1;  // its LDS row stride (columns on distinct banks)
constexpr int kSuper = 8192;     // rows per partial product sum (kTile | kSuper)
constexpr int kMaxPairs = kMaxCorr * (kMaxCorr + 1) / 2;

struct Reps {
  int32_t r[h3d::kMaxReps];
};

// sum of the block's 256 values in a fixed tree (lds: 256 doubles); every
// lane returns it
__device__ inline double block_sum(double v, double* lds) {
  const int t = threadIdx.x;
  __syncthreads();
  lds[t] = v;
  __syncthreads();
  for (int h = kBlock / 2; h >= 1; h >>= 1) {
    if (t < h) lds[t] += lds[t + h];
    __syncthreads();
  }
  return lds[0];
}

// np.histogram's bin of v among E strictly increasing edges: [e_i, e_i+1),
// the last one closed; -1 for NaN and values outside [e_0, e_E-1]
__device__ inline int find_bin(const double* e, int E, double v) {
  if (!(v >= e[0]) || !(v <= e[E - 1])) return -1;
  int lo = 0, hi = E - 1;  // e[lo] <= v, and v < e[hi] unless hi == E - 1
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (e[mid] <= v) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ---- group sums ------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void k_gs_keys(const int32_t* __restrict__ keys, int64_t n,
                                                    int K, uint32_t* __restrict__ ku,
                                                    int32_t* __restrict__ idx) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlock) {
    const int32_t k = keys[i];
    ku[i] = (k < 0 || k >= K) ? (uint32_t)K : (uint32_t)k;  // K: dropped
    idx[i] = (int32_t)i;
  }
}

// start[k] = the first sorted position whose key is >= k, k = 0 .. K
__global__ __launch_bounds__(kBlock) void k_gs_bounds(const uint32_t* __restrict__ ks, int64_t n,
                                                      int K, int64_t* __restrict__ start) {
  for (int k = blockIdx.x * kBlock + threadIdx.x; k <= K; k += gridDim.x * kBlock) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (ks[mid] < (uint32_t)k) lo = mid + 1;
      else hi = mid;
    }
    start[k] = lo;
  }
}

// block (k, s): the members j of key k (in original order) with
// (j / M) % kSlices == s, M = 256 / Cq member lanes by Cq column lanes; lane
// (m, c) adds its members in order, the M lanes of a column fold in a tree
__global__ __launch_bounds__(kBlock) void k_gs_partial(const int32_t* __restrict__ idx_s,
                                                       const int64_t* __restrict__ start,
                                                       const double* __restrict__ values,
                                                       int64_t n, int C, int Cq,
                                                       double* __restrict__ partial) {
  __shared__ double lds[kBlock];
  const int k = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
  const int M = kBlock / Cq, m = t / Cq, c = t % Cq;
  const int64_t s0 = start[k], len = start[k + 1] - s0;
  double acc = 0.0;
  if (c < C)
    for (int64_t j = (int64_t)s * M + m; j < len; j += (int64_t)kSlices * M) {
      const int64_t row = idx_s[s0 + j];
      if (row >= 0 && row < n) acc += values[row * C + c];
    }
  lds[t] = acc;
  __syncthreads();
  for (int h = M / 2; h >= 1; h >>= 1) {
    if (m < h) lds[t] += lds[t + h * Cq];
    __syncthreads();
  }
  if (m == 0 && c < C) partial[((int64_t)k * kSlices + s) * C + c] = lds[t];
}

__global__ __launch_bounds__(kBlock) void k_gs_final(const double* __restrict__ partial,
                                                     const int64_t* __restrict__ start, int K,
                                                     int C, double* __restrict__ sums,
                                                     int64_t* __restrict__ counts) {
  const int64_t total = (int64_t)K * C;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * kBlock) {
    const int64_t k = e / C;
    const int c = (int)(e - k * C);
    double acc = partial[(k * kSlices) * C + c];
    for (int s = 1; s < kSlices; ++s) acc += partial[(k * kSlices + s) * C + c];
    sums[e] = acc;
    if (c == 0) counts[k] = start[k + 1] - start[k];
  }
}

int launch_group_sums(h3d_ctx* ctx, const int32_t* d_keys, const double* d_values, int64_t n,
                      int K, int C, double* d_sums, int64_t* d_counts) {
  hipStream_t s = ctx->stream;
  Scratch sc{ctx};
  uint32_t* ku = sc.get<uint32_t>("diag_ku", (size_t)n + 1);
  uint32_t* ks = sc.get<uint32_t>("diag_ks", (size_t)n + 1);
  int32_t* idx = sc.get<int32_t>("diag_idx", (size_t)n + 1);
  int32_t* idx_s = sc.get<int32_t>("diag_idx_s", (size_t)n + 1);
  int64_t* start = sc.get<int64_t>("diag_start", (size_t)K + 1);
  double* partial = sc.get<double>("diag_gs_partial", (size_t)K * kSlices * C);
  if (!sc.ok) return fail(H3D_ENOMEM, "group sums buffers");
  ProfScope ps(ctx, "diag_group_sums", n);
  if (n > 0) {
    hipLaunchKernelGGL(k_gs_keys, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, d_keys, n, K, ku,
                       idx);
    int end_bit = 1;
    while (end_bit < 32 && ((uint32_t)K >> end_bit)) ++end_bit;
    if (int rc = cub_call(ctx, "cub_tmp_diag", [&](void* tmp, size_t& bytes) {
          return sort_pairs(tmp, bytes, ku, ks, idx, idx_s, (int)n, 0, end_bit, s);
        }))
      return rc;
  }
  hipLaunchKernelGGL(k_gs_bounds, dim3(grid_for(ctx, K + 1)), dim3(kBlock), 0, s, ks, n, K,
                     start);
  int Cq = 1;
  while (Cq < C) Cq <<= 1;
  hipLaunchKernelGGL(k_gs_partial, dim3(K, kSlices), dim3(kBlock), 0, s, idx_s, start, d_values,
                     n, C, Cq, partial);
  hipLaunchKernelGGL(k_gs_final, dim3(grid_for(ctx, (int64_t)K * C)), dim3(kBlock), 0, s,
                     partial, start, K, C, d_sums, d_counts);
  HIP_TRY(hipGetLastError());
  return 0;
}

// the argument checks of h3d_group_sums and its _dev twin
int check_group_sums(const void* ctx, const void* keys, const void* values, int64_t n, int K,
                     int C, const void* sums, const void* counts) {
  if (int rc = check_count(ctx, n)) return rc;
  if (K < 1 || K > kMaxKeys) return fail(H3D_EARG, "K=%d outside [1, %d]", K, kMaxKeys);
  if (C < 1 || C > kMaxCols) return fail(H3D_EARG, "C=%d outside [1, %d]", C, kMaxCols);
  if (!sums || !counts) return fail(H3D_EARG, "null output");
  if (n > 0 && (!keys || !values)) return fail(H3D_EARG, "null keys / values");
  return 0;
}

// ---- histogram ---------------------------------------------------------------

// LDS: E edges, then one counter row of E - 1 bins per wave
__global__ __launch_bounds__(kBlock) void k_histogram(const double* __restrict__ values,
                                                      int64_t n, const double* __restrict__ edges,
                                                      int E, unsigned long long* __restrict__ out) {
  extern __shared__ double lds_hist[];
  double* e = lds_hist;
  unsigned int* cnt = (unsigned int*)(lds_hist + E);
  const int nb = E - 1, t = threadIdx.x, wave = t >> 6;
  constexpr int kWaves = kBlock / 64;
  for (int i = t; i < E; i += kBlock) e[i] = edges[i];
  for (int i = t; i < kWaves * nb; i += kBlock) cnt[i] = 0u;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * kBlock + t; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int b = find_bin(e, E, values[i]);
    if (b >= 0) atomicAdd(&cnt[wave * nb + b], 1u);
  }
  __syncthreads();
  for (int b = t; b < nb; b += kBlock) {
    unsigned long long tot = 0;
    for (int w = 0; w < kWaves; ++w) tot += cnt[w * nb + b];
    if (tot) atomicAdd(&out[b], tot);
  }
}

size_t hist_lds(int E) { return (size_t)E * 8 + (size_t)(kBlock / 64) * (E - 1) * 4; }

int check_edges(const double* edges, int E, const char* what) {
  if (!edges) return fail(H3D_EARG, "null %s", what);
  if (E < 2 || E > kMaxEdges)
    return fail(H3D_EARG, "%s: %d edges outside [2, %d]", what, E, kMaxEdges);
  for (int i = 0; i < E; ++i)
    if (!std::isfinite(edges[i])) return fail(H3D_EARG, "%s[%d] is not finite", what, i);
  for (int i = 1; i < E; ++i)
    if (!(edges[i] > edges[i - 1]))
      return fail(H3D_EARG, "%s must increase strictly (entry %d)", what, i);
  return 0;
}

// counts (E - 1) int64 on the device, zeroed here
int launch_histogram(h3d_ctx* ctx, const double* d_values, int64_t n, const double* edges, int E,
                     int64_t* d_counts) {
  hipStream_t s = ctx->stream;
  Scratch sc{ctx};
  double* d_edges = sc.get<double>("diag_edges", (size_t)kMaxEdges);
  if (!sc.ok) return fail(H3D_ENOMEM, "histogram edges");
  if (int rc = h2d_pinned(ctx, d_edges, edges, (size_t)E * 8, s)) return rc;
  HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)(E - 1) * 8, s));
  if (n == 0) return 0;
  if (int rc = allow_dynamic_lds(ctx, (const void*)k_histogram, (int)hist_lds(kMaxEdges)))
    return rc;
  ProfScope ps(ctx, "diag_histogram", n);
  hipLaunchKernelGGL(k_histogram, dim3(grid_for(ctx, n, 4)), dim3(kBlock), hist_lds(E), s,
                     d_values, n, d_edges, E, (unsigned long long*)d_counts);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- density grid -------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void k_density(const double* __restrict__ x,
                                                    const double* __restrict__ y,
                                                    const int8_t* __restrict__ label, int64_t n,
                                                    int L, const double* __restrict__ edges,
                                                    int Ex, int Ey,
                                                    unsigned long long* __restrict__ out) {
  extern __shared__ double lds_den[];
  double* ex = lds_den;
  double* ey = lds_den + Ex;
  const int t = threadIdx.x;
  for (int i = t; i < Ex + Ey; i += kBlock) lds_den[i] = edges[i];
  __syncthreads();
  const int64_t nbx = Ex - 1, nby = Ey - 1;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + t; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int l = label[i];
    if (l < 0 || l >= L) continue;
    const int bx = find_bin(ex, Ex, x[i]);
    if (bx < 0) continue;
    const int by = find_bin(ey, Ey, y[i]);
    if (by < 0) continue;
    atomicAdd(&out[((int64_t)l * nbx + bx) * nby + by], 1ull);
  }
}

// ---- MA statistics -------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void k_flag_to_int(const uint8_t* __restrict__ f, int64_t n,
                                                        int32_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlock)
    out[i] = f[i] ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void k_ma_stats(
    const double* __restrict__ scaled, int64_t n, int R, Reps reps0, int n0, Reps reps1, int n1,
    const uint8_t* __restrict__ loop, const int32_t* __restrict__ qpos,
    const double* __restrict__ q, int64_t nq, double fdr, double* __restrict__ mean,
    double* __restrict__ m_out, double* __restrict__ a_out, int8_t* __restrict__ label) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlock) {
    const double* row = scaled + i * R;
    double s0 = 0.0, s1 = 0.0;
    for (int k = 0; k < n0; ++k) s0 += row[reps0.r[k]];
    for (int k = 0; k < n1; ++k) s1 += row[reps1.r[k]];
    const double mean0 = s0 / (double)n0, mean1 = s1 / (double)n1;
    const double l0 = log2(mean0), l1 = log2(mean1);
    const double m = l0 - l1, a = 0.5 * (l0 + l1);
    mean[2 * i] = mean0;
    mean[2 * i + 1] = mean1;
    m_out[i] = m;
    a_out[i] = a;
    int8_t lab = 0;
    if (!loop || loop[i]) {
      const int64_t qi = loop ? (int64_t)qpos[i] : i;
      const double qv = (qi >= 0 && qi < nq) ? q[qi] : std::numeric_limits<double>::quiet_NaN();
      if (!(qv < fdr)) lab = 1;
      else if (m > 0.0) lab = 2;
      else if (m < 0.0) lab = 3;
      else lab = -1;
    }
    label[i] = lab;
  }
}

// ---- average ranks -------------------------------------------------------------

// order-preserving key of a double (-0.0 and +0.0 one value); a NaN sets bit 0
// of *flag
__global__ __launch_bounds__(kBlock) void k_rank_keys(const double* __restrict__ v, int64_t n,
                                                      uint64_t* __restrict__ keys,
                                                      int32_t* __restrict__ idx,
                                                      int* __restrict__ flag) {
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlock) {
    const double x = v[i];
    if (x != x) bad = 1;
    keys[i] = asc_key(x);
    idx[i] = (int32_t)i;
  }
  if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(flag, 1);
}

__global__ __launch_bounds__(kBlock) void k_rank_heads(const uint64_t* __restrict__ ks, int64_t n,
                                                       int32_t* __restrict__ head) {
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n;
       p += (int64_t)gridDim.x * kBlock)
    head[p] = (p == 0 || ks[p] != ks[p - 1]) ? 1 : 0;
}

// run_start (n + 1): the first position of run r, and n behind the last run
__global__ __launch_bounds__(kBlock) void k_rank_starts(const int32_t* __restrict__ head,
                                                        const int32_t* __restrict__ run_of,
                                                        int64_t n, int32_t* __restrict__ run_start) {
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n;
       p += (int64_t)gridDim.x * kBlock) {
    const int32_t r = run_of[p];  // 1-based, <= p + 1
    if (head[p]) run_start[r - 1] = (int32_t)p;
    if (p == n - 1) run_start[r] = (int32_t)n;
  }
}

__global__ __launch_bounds__(kBlock) void k_rank_write(const int32_t* __restrict__ idx_s,
                                                       const int32_t* __restrict__ run_of,
                                                       const int32_t* __restrict__ run_start,
                                                       int64_t n, const int* __restrict__ flag,
                                                       double* __restrict__ out) {
  const bool nan_col = (*flag & 1) != 0;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n;
       p += (int64_t)gridDim.x * kBlock) {
    const int32_t r = run_of[p] - 1;
    // positions s .. e - 1 share the ranks s + 1 .. e: their mean
    const int64_t s = run_start[r], e = run_start[r + 1];
    const int64_t dst = idx_s[p];
    if (dst >= 0 && dst < n)
      out[dst] = nan_col ? std::numeric_limits<double>::quiet_NaN() : 0.5 * (double)(s + e + 1);
  }
}

// ranks of R device columns of n; d_flags (R) int, bit 0: the column holds a NaN
int launch_rank_average(h3d_ctx* ctx, const double* d_values, int64_t n, int R, double* d_ranks,
                        int* d_flags) {
  hipStream_t s = ctx->stream;
  HIP_TRY(hipMemsetAsync(d_flags, 0, (size_t)R * sizeof(int), s));
  if (n == 0) return 0;
  Scratch sc{ctx};
  uint64_t* keys = sc.get<uint64_t>("diag_rk", (size_t)n);
  uint64_t* keys_s = sc.get<uint64_t>("diag_rk_s", (size_t)n);
  int32_t* idx = sc.get<int32_t>("diag_idx", (size_t)n + 1);
  int32_t* idx_s = sc.get<int32_t>("diag_idx_s", (size_t)n + 1);
  int32_t* head = sc.get<int32_t>("diag_head", (size_t)n);
  int32_t* run_of = sc.get<int32_t>("diag_run_of", (size_t)n);
  int32_t* run_start = sc.get<int32_t>("diag_run_start", (size_t)n + 1);
  if (!sc.ok) return fail(H3D_ENOMEM, "rank buffers");
  ProfScope ps(ctx, "diag_rank_average", n * R);
  const int g = grid_for(ctx, n);
  for (int c = 0; c < R; ++c) {
    const double* col = d_values + (int64_t)c * n;
    hipLaunchKernelGGL(k_rank_keys, dim3(g), dim3(kBlock), 0, s, col, n, keys, idx, d_flags + c);
    if (int rc = cub_call(ctx, "cub_tmp_diag", [&](void* tmp, size_t& bytes) {
          return sort_pairs(tmp, bytes, keys, keys_s, idx, idx_s, (int)n, 0, 64, s);
        }))
      return rc;
    hipLaunchKernelGGL(k_rank_heads, dim3(g), dim3(kBlock), 0, s, keys_s, n, head);
    if (int rc = cub_call(ctx, "cub_tmp_diag_s", [&](void* tmp, size_t& bytes) {
          return inclusive_sum(tmp, bytes, head, run_of, (int)n, s);
        }))
      return rc;
    hipLaunchKernelGGL(k_rank_starts, dim3(g), dim3(kBlock), 0, s, head, run_of, n, run_start);
    hipLaunchKernelGGL(k_rank_write, dim3(g), dim3(kBlock), 0, s, idx_s, run_of, run_start, n,
                       d_flags + c, d_ranks + (int64_t)c * n);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- correlation matrix ----------------------------------------------------------

// block (b, c): the sum of rows b * kChunk .. of column c (lane t adds rows
// t, t + 256, ... in order, then the tree); flags[c] bit 0: a NaN, bit 1: a
// value that differs from the column's first
__global__ __launch_bounds__(kBlock) void k_corr_colsum(const double* __restrict__ v, int64_t n,
                                                        int64_t n_chunks,
                                                        double* __restrict__ partial,
                                                        int* __restrict__ flags) {
  __shared__ double lds[kBlock];
  const int c = blockIdx.y, t = threadIdx.x;
  const double* col = v + (int64_t)c * n;
  const double first = col[0];
  for (int64_t b = blockIdx.x; b < n_chunks; b += gridDim.x) {
    const int64_t r0 = b * kChunk;
    const int64_t r1 = r0 + kChunk < n ? r0 + kChunk : n;
    double acc = 0.0;
    int fl = 0;
    for (int64_t i = r0 + t; i < r1; i += kBlock) {
      const double x = col[i];
      acc += x;
      if (x != x) fl |= 1;
      if (x != first) fl |= 2;
    }
    const double tot = block_sum(acc, lds);
    fl = __syncthreads_or(fl & 1) | (__syncthreads_or(fl & 2) ? 2 : 0);
    if (t == 0) {
      partial[(int64_t)c * n_chunks + b] = tot;
      if (fl) atomicOr(&flags[c], fl);
    }
  }
}

// block e: the sum of the m partials of entry e, then / div (div 0: the sum)
__global__ __launch_bounds__(kBlock) void k_corr_fold(const double* __restrict__ partial,
                                                      int64_t m, double div,
                                                      double* __restrict__ out) {
  __shared__ double lds[kBlock];
  const int64_t e = blockIdx.x;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < m; i += kBlock) acc += partial[e * m + i];
  const double tot = block_sum(acc, lds);
  if (threadIdx.x == 0) out[e] = div != 0.0 ? tot / div : tot;
}

// block sb: rows sb * kSuper .. in tiles of kTile; the tile's deviations
// x - mean go to LDS (rows behind n as 0), lane t owns the column pairs
// t, t + 256, t + 512 and adds each pair's products row by row
__global__ __launch_bounds__(kBlock) void k_corr_prod(const double* __restrict__ v, int64_t n,
                                                      int R, const double* __restrict__ mean,
                                                      int64_t n_super,
                                                      double* __restrict__ partial) {
  __shared__ double tile[kMaxCorr * kTileLd];
  __shared__ uint8_t pa[kMaxPairs], pb[kMaxPairs];
  const int t = threadIdx.x;
  const int n_pairs = R * (R + 1) / 2;
  if (t == 0) {
    int p = 0;
    for (int a = 0; a < R; ++a)
      for (int b = a; b < R; ++b) {
        pa[p] = (uint8_t)a;
        pb[p] = (uint8_t)b;
        ++p;
      }
  }
  __syncthreads();
  constexpr int kOwn = (kMaxPairs + kBlock - 1) / kBlock;
  for (int64_t sb = blockIdx.x; sb < n_super; sb += gridDim.x) {
    double acc[kOwn];
#pragma unroll
    for (int j = 0; j < kOwn; ++j) acc[j] = 0.0;
    const int64_t r0 = sb * kSuper;
    for (int64_t base = r0; base < r0 + kSuper && base < n; base += kTile) {
      __syncthreads();
      for (int e = t; e < R * kTile; e += kBlock) {
        const int c = e / kTile, i = e - c * kTile;
        const int64_t row = base + i;
        tile[c * kTileLd + i] = row < n ? v[(int64_t)c * n + row] - mean[c] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < kOwn; ++j) {
        const int p = t + j * kBlock;
        if (p < n_pairs) {
          const double* xa = tile + (int)pa[p] * kTileLd;
          const double* xb = tile + (int)pb[p] * kTileLd;
          double s = acc[j];
          for (int i = 0; i < kTile; ++i) s += xa[i] * xb[i];
          acc[j] = s;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
      const int p = t + j * kBlock;
      if (p < n_pairs) partial[(int64_t)p * n_super + sb] = acc[j];
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_corr_finish(const double* __restrict__ S, int R,
                                                        const int* __restrict__ flags,
                                                        double* __restrict__ out) {
  const int n_pairs = R * (R + 1) / 2;
  const int p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= n_pairs) return;
  int a = 0, rem = p;  // pair p of the (a, b >= a) enumeration
  while (rem >= R - a) {
    rem -= R - a;
    ++a;
  }
  const int b = a + rem;
  const int pa = a * R - a * (a - 1) / 2, pbb = b * R - b * (b - 1) / 2;  // (a, a), (b, b)
  double r = S[p] / sqrt(S[pa] * S[pbb]);
  if (r > 1.0) r = 1.0;
  if (r < -1.0) r = -1.0;
  const int fa = flags[a], fb = flags[b];
  // a NaN propagates; a constant column has no correlation (scipy: NaN)
  if ((fa & 1) || (fb & 1) || !(fa & 2) || !(fb & 2)) r = std::numeric_limits<double>::quiet_NaN();
  out[a * R + b] = r;
  out[b * R + a] = r;
}

// d_out (R, R) on the device from R device columns of n
int launch_corr(h3d_ctx* ctx, const double* d_values, int64_t n, int R, double* d_out) {
  hipStream_t s = ctx->stream;
  const int n_pairs = R * (R + 1) / 2;
  const int64_t n_chunks = (n + kChunk - 1) / kChunk, n_super = (n + kSuper - 1) / kSuper;
  Scratch sc{ctx};
  int* flags = sc.get<int>("diag_corr_flags", (size_t)kMaxCorr);
  double* mean = sc.get<double>("diag_corr_mean", (size_t)kMaxCorr);
  double* S = sc.get<double>("diag_corr_s", (size_t)kMaxPairs);
  double* p_col = sc.get<double>("diag_corr_pcol", (size_t)R * (n_chunks + 1));
  double* p_prod = sc.get<double>("diag_corr_pprod", (size_t)n_pairs * (n_super + 1));
  if (!sc.ok) return fail(H3D_ENOMEM, "correlation buffers");
  HIP_TRY(hipMemsetAsync(flags, 0, kMaxCorr * sizeof(int), s));
  ProfScope ps(ctx, "diag_corr_matrix", n * R);
  if (n > 0) {
    const int gx = (int)std::min<int64_t>(n_chunks, (int64_t)ctx->n_cu * 8);
    hipLaunchKernelGGL(k_corr_colsum, dim3(gx, R), dim3(kBlock), 0, s, d_values, n, n_chunks,
                       p_col, flags);
    hipLaunchKernelGGL(k_corr_fold, dim3(R), dim3(kBlock), 0, s, p_col, n_chunks, (double)n,
                       mean);
    const int gp = (int)std::min<int64_t>(n_super, (int64_t)ctx->n_cu * 4);
    hipLaunchKernelGGL(k_corr_prod, dim3(gp), dim3(kBlock), 0, s, d_values, n, R, mean, n_super,
                       p_prod);
    hipLaunchKernelGGL(k_corr_fold, dim3(n_pairs), dim3(kBlock), 0, s, p_prod, n_super, 0.0, S);
  } else {
    HIP_TRY(hipMemsetAsync(S, 0, kMaxPairs * sizeof(double), s));
  }
  hipLaunchKernelGGL(k_corr_finish, dim3((n_pairs + kBlock - 1) / kBlock), dim3(kBlock), 0, s, S,
                     R, flags, d_out);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- pixel moments, balanced pixels ------------------------------------------------

__global__ __launch_bounds__(kBlock) void k_pixel_moments(const double* __restrict__ scaled,
                                                          int64_t n, int R, Reps reps, int r,
                                                          double* __restrict__ mean,
                                                          double* __restrict__ var) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlock) {
    const double* row = scaled + i * R;
    double v[h3d::kMaxReps];
#pragma unroll
    for (int k = 0; k < h3d::kMaxReps; ++k) v[k] = k < r ? row[reps.r[k]] : 0.0;
    // numpy's two passes, each in its row-sum association (np_sum)
    const double mu = h3d::np_sum<h3d::kMaxReps>(v, r) / (double)r;
#pragma unroll
    for (int k = 0; k < h3d::kMaxReps; ++k) {
      const double d = v[k] - mu;
      v[k] = d * d;
    }
    mean[i] = mu;
    var[i] = h3d::np_sum<h3d::kMaxReps>(v, r) / (double)(r - 1);  // r = 1: 0 / 0
  }
}

// out (n, R) = raw / (bias[row] * bias[col]); a row or col outside the bias
// table gives NaN
__global__ __launch_bounds__(kBlock) void k_balance_pixels(
    const int32_t* __restrict__ row, const int32_t* __restrict__ col,
    const int64_t* __restrict__ raw, const double* __restrict__ bias, int64_t n, int R,
    int n_bins, double* __restrict__ out) {
  const int64_t total = n * R;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * kBlock) {
    const int64_t i = e / R;
    const int r = (int)(e - i * R);
    const int32_t a = row[i], b = col[i];
    double o = std::numeric_limits<double>::quiet_NaN();
    if (a >= 0 && a < n_bins && b >= 0 && b < n_bins)
      o = (double)raw[e] / (bias[(int64_t)a * R + r] * bias[(int64_t)b * R + r]);
    out[e] = o;
  }
}

// the argument checks of h3d_histogram and its _dev twin
int check_histogram(const void* ctx, const void* values, int64_t n, const double* edges, int E,
                    const void* counts) {
  if (int rc = check_count(ctx, n)) return rc;
  if (int rc = check_edges(edges, E, "edges")) return rc;
  if (!counts) return fail(H3D_EARG, "null output");
  if (n > 0 && !values) return fail(H3D_EARG, "null values");
  return 0;
}

}  // namespace h3ddiag

extern "C" {

int h3d_group_sums_dev(h3d_ctx* ctx, const int32_t* d_keys, const double* d_values, int64_t n,
                       int K, int C, double* d_sums, int64_t* d_counts) {
  using namespace h3ddiag;
  if (int rc = check_group_sums(ctx, d_keys, d_values, n, K, C, d_sums, d_counts)) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  if (int rc = launch_group_sums(ctx, d_keys, d_values, n, K, C, d_sums, d_counts)) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}

int h3d_group_sums(h3d_ctx* ctx, const int32_t* keys, const double* values, int64_t n, int K,
                   int C, double* sums, int64_t* counts) {
  using namespace h3ddiag;
  if (int rc = check_group_sums(ctx, keys, values, n, K, C, sums, counts)) return rc;
  HostCall hc(ctx);
  int32_t* d_keys = hc.out<int32_t>("diag_in_keys", (size_t)n + 1);
  double* d_values = hc.out<double>("diag_in_a", (size_t)n * C + 1);
  double* d_sums = hc.out<double>("diag_out_a", (size_t)K * C);
  int64_t* d_counts = hc.out<int64_t>("diag_out_i", (size_t)K);
  if (int rc = hc.ready("group sums buffers")) return rc;
  hc.up(d_keys, keys, (size_t)n);
  hc.up(d_values, values, (size_t)n * C);
  if (int rc = launch_group_sums(ctx, d_keys, d_values, n, K, C, d_sums, d_counts)) return rc;
  hc.back(sums, d_sums, (size_t)K * C);
  hc.back(counts, d_counts, (size_t)K);
  return hc.finish();
}

int h3d_histogram_dev(h3d_ctx* ctx, const double* d_values, int64_t n, const double* edges,
                      int E, int64_t* d_counts) {
  using namespace h3ddiag;
  if (int rc = check_histogram(ctx, d_values, n, edges, E, d_counts)) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  if (int rc = launch_histogram(ctx, d_values, n, edges, E, d_counts)) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}

int h3d_histogram(h3d_ctx* ctx, const double* values, int64_t n, const double* edges, int E,
                  int64_t* counts) {
  using namespace h3ddiag;
  if (int rc = check_histogram(ctx, values, n, edges, E, counts)) return rc;
  HostCall hc(ctx);
  double* d_values = hc.out<double>("diag_in_a", (size_t)n + 1);
  int64_t* d_counts = hc.out<int64_t>("diag_out_i", (size_t)kMaxEdges);
  if (int rc = hc.ready("histogram buffers")) return rc;
  hc.up(d_values, values, (size_t)n);
  if (int rc = launch_histogram(ctx, d_values, n, edges, E, d_counts)) return rc;
  hc.back(counts, d_counts, (size_t)(E - 1));
  return hc.finish();
}

int h3d_density_grid(h3d_ctx* ctx, const double* x, const double* y, const int8_t* label,
                     int64_t n, int L, const double* xedges, int Ex, const double* yedges,
                     int Ey, int64_t* counts) {
  using namespace h3ddiag;
  if (int rc = check_count(ctx, n)) return rc;
  if (L < 1 || L > 127) return fail(H3D_EARG, "L=%d outside [1, 127]", L);
  if (int rc = check_edges(xedges, Ex, "xedges")) return rc;
  if (int rc = check_edges(yedges, Ey, "yedges")) return rc;
  if (!counts) return fail(H3D_EARG, "null output");
  if (n > 0 && (!x || !y || !label)) return fail(H3D_EARG, "null x / y / label");
  const int64_t cells = (int64_t)L * (Ex - 1) * (Ey - 1);
  if (cells >= ((int64_t)1 << 28))
    return fail(H3D_EARG, "L * (Ex - 1) * (Ey - 1) = %lld is not below 2^28", (long long)cells);
  hipStream_t s = ctx->stream;
  HostCall hc(ctx);
  double* d_x = hc.out<double>("diag_in_a", (size_t)n + 1);
  double* d_y = hc.out<double>("diag_in_b", (size_t)n + 1);
  int8_t* d_label = hc.out<int8_t>("diag_in_l", (size_t)n + 1);
  double* d_edges = hc.out<double>("diag_edges2", (size_t)2 * kMaxEdges);
  int64_t* d_counts = hc.out<int64_t>("diag_out_grid", (size_t)cells);
  if (int rc = hc.ready("density grid buffers")) return rc;
  HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)cells * 8, s));
  if (n > 0) {
    hc.up(d_x, x, (size_t)n);
    hc.up(d_y, y, (size_t)n);
    hc.up(d_label, label, (size_t)n);
    if (int rc = h2d_pinned(ctx, d_edges, xedges, (size_t)Ex * 8, s)) return rc;
    if (int rc = h2d_pinned(ctx, d_edges + Ex, yedges, (size_t)Ey * 8, s)) return rc;
    if (int rc = allow_dynamic_lds(ctx, (const void*)k_density, 2 * kMaxEdges * 8)) return rc;
    ProfScope ps(ctx, "diag_density_grid", n);
    hipLaunchKernelGGL(k_density, dim3(grid_for(ctx, n, 4)), dim3(kBlock),
                       (size_t)(Ex + Ey) * 8, s, d_x, d_y, d_label, n, L, d_edges, Ex, Ey,
                       (unsigned long long*)d_counts);
    HIP_TRY(hipGetLastError());
  }
  hc.back(counts, d_counts, (size_t)cells);
  return hc.finish();
}

int h3d_ma_stats(h3d_ctx* ctx, const double* scaled, int64_t n, int R, int C,
                 const int32_t* cond_of_rep, int cond0, int cond1, const uint8_t* loop_idx,
                 const double* qvalues, int64_t n_q, double fdr, double* mean, double* m,
                 double* a, int8_t* label) {
  using namespace h3ddiag;
  if (int rc = check_count(ctx, n)) return rc;
  if (!cond_of_rep) return fail(H3D_EARG, "null cond_of_rep");
  std::vector<int> nrep;
  std::vector<int32_t> rep_idx;
  if (int rc = check_cond(cond_of_rep, R, C, &nrep, &rep_idx)) return rc;
  if (cond0 < 0 || cond0 >= C || cond1 < 0 || cond1 >= C)
    return fail(H3D_EARG, "conditions (%d, %d) outside [0, %d)", cond0, cond1, C);
  if (n_q < 0 || (!loop_idx && n_q != n))
    return fail(H3D_EARG, "%lld q-values for %lld loop pixels", (long long)n_q, (long long)n);
  if (n == 0) {
    if (n_q != 0) return fail(H3D_EARG, "%lld q-values for 0 loop pixels", (long long)n_q);
    return 0;
  }
  if (!scaled || !mean || !m || !a || !label) return fail(H3D_EARG, "null input / output");
  if (n_q > 0 && !qvalues) return fail(H3D_EARG, "null qvalues");
  Reps r0{}, r1{};
  for (int k = 0; k < nrep[cond0]; ++k) r0.r[k] = rep_idx[(size_t)cond0 * h3d::kMaxReps + k];
  for (int k = 0; k < nrep[cond1]; ++k) r1.r[k] = rep_idx[(size_t)cond1 * h3d::kMaxReps + k];
  hipStream_t s = ctx->stream;
  HostCall hc(ctx);
  double* d_scaled = hc.in("diag_in_a", scaled, (size_t)n * R);
  double* d_q = hc.out<double>("diag_in_b", (size_t)n_q + 1);
  hc.up(d_q, qvalues, (size_t)n_q);
  uint8_t* d_loop = (uint8_t*)hc.in("diag_in_l", (const int8_t*)loop_idx, (size_t)n);
  int32_t* d_flag = loop_idx ? hc.out<int32_t>("diag_head", (size_t)n) : nullptr;
  int32_t* d_qpos = loop_idx ? hc.out<int32_t>("diag_run_of", (size_t)n) : nullptr;
  double* d_out = hc.out<double>("diag_out_a", (size_t)n * 4);  // mean (n, 2) | m | a
  int8_t* d_label = hc.out<int8_t>("diag_out_l", (size_t)n);
  if (int rc = hc.ready("ma_stats buffers")) return rc;
  if (loop_idx) {
    ProfScope ps(ctx, "diag_ma_scan", n);
    hipLaunchKernelGGL(k_flag_to_int, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, d_loop, n,
                       d_flag);
    if (int rc = cub_call(ctx, "cub_tmp_diag_s", [&](void* tmp, size_t& bytes) {
          return exclusive_sum(tmp, bytes, d_flag, d_qpos, (int)n, s);
        }))
      return rc;
    // the loop pixels must be as many as the q-values, before q is indexed
    int32_t last[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&last[0], d_qpos + (n - 1), 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&last[1], d_flag + (n - 1), 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((int64_t)last[0] + last[1] != n_q)
      return fail(H3D_EARG, "%lld q-values for %lld loop pixels", (long long)n_q,
                  (long long)last[0] + last[1]);
  }
  {
    ProfScope ps(ctx, "diag_ma_stats", n);
    hipLaunchKernelGGL(k_ma_stats, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, d_scaled, n, R, r0,
                       nrep[cond0], r1, nrep[cond1], d_loop, d_qpos, d_q, n_q, fdr, d_out,
                       d_out + 2 * n, d_out + 3 * n, d_label);
  }
  HIP_TRY(hipGetLastError());
  hc.back(mean, d_out, (size_t)n * 2);
  hc.back(m, d_out + 2 * n, (size_t)n);
  hc.back(a, d_out + 3 * n, (size_t)n);
  hc.back(label, d_label, (size_t)n);
  return hc.finish();
}

int h3d_rank_average(h3d_ctx* ctx, const double* values, int64_t n, int R, double* ranks,
                     int32_t* nan_flags) {
  using namespace h3ddiag;
  if (int rc = check_count(ctx, n)) return rc;
  if (R < 1 || R > kMaxCorr) return fail(H3D_EARG, "R=%d outside [1, %d]", R, kMaxCorr);
  if (!nan_flags) return fail(H3D_EARG, "null flags");
  if (n > 0 && (!values || !ranks)) return fail(H3D_EARG, "null values / ranks");
  HostCall hc(ctx);
  double* d_values = hc.out<double>("diag_in_a", (size_t)n * R + 1);
  double* d_ranks = hc.out<double>("diag_out_a", (size_t)n * R + 1);
  int* d_flags = hc.out<int>("diag_rank_flags", (size_t)kMaxCorr);
  if (int rc = hc.ready("rank buffers")) return rc;
  hc.up(d_values, values, (size_t)n * R);
  if (int rc = launch_rank_average(ctx, d_values, n, R, d_ranks, d_flags)) return rc;
  hc.back(ranks, d_ranks, (size_t)n * R);
  hc.back(nan_flags, d_flags, (size_t)R);
  return hc.finish();
}

int h3d_corr_matrix(h3d_ctx* ctx, const double* values, int64_t n, int R, int ranked,
                    double* corr) {
  using namespace h3ddiag;
  if (int rc = check_count(ctx, n)) return rc;
  if (R < 1 || R > kMaxCorr) return fail(H3D_EARG, "R=%d outside [1, %d]", R, kMaxCorr);
  if (!corr) return fail(H3D_EARG, "null output");
  if (n > 0 && !values) return fail(H3D_EARG, "null values");
  HostCall hc(ctx);
  double* d_values = hc.out<double>("diag_in_a", (size_t)n * R + 1);
  double* d_ranks = ranked ? hc.out<double>("diag_out_a", (size_t)n * R + 1) : nullptr;
  int* d_flags = hc.out<int>("diag_rank_flags", (size_t)kMaxCorr);
  double* d_corr = hc.out<double>("diag_out_corr", (size_t)kMaxCorr * kMaxCorr);
  if (int rc = hc.ready("correlation buffers")) return rc;
  hc.up(d_values, values, (size_t)n * R);
  const double* src = d_values;
  if (ranked) {  // Spearman: Pearson of the average ranks
    if (int rc = launch_rank_average(ctx, d_values, n, R, d_ranks, d_flags)) return rc;
    src = d_ranks;
  }
  if (int rc = launch_corr(ctx, src, n, R, d_corr)) return rc;
  hc.back(corr, d_corr, (size_t)R * R);
  return hc.finish();
}

int h3d_pixel_moments(h3d_ctx* ctx, const double* scaled, int64_t n, int R, const int32_t* reps,
                      int n_reps, double* mean, double* var) {
  using namespace h3ddiag;
  if (int rc = check_count(ctx, n)) return rc;
  if (R < 1 || R > h3d::kMaxReps) return fail(H3D_EARG, "R=%d outside [1, %d]", R, h3d::kMaxReps);
  if (!reps || n_reps < 1 || n_reps > R)
    return fail(H3D_EARG, "%d replicates of R=%d", n_reps, R);
  Reps rr{};
  for (int k = 0; k < n_reps; ++k) {
    if (reps[k] < 0 || reps[k] >= R) return fail(H3D_EARG, "replicate %d outside [0, %d)", reps[k], R);
    rr.r[k] = reps[k];
  }
  if (n == 0) return 0;
  if (!scaled || !mean || !var) return fail(H3D_EARG, "null input / output");
  HostCall hc(ctx);
  double* d_scaled = hc.in("diag_in_a", scaled, (size_t)n * R);
  double* d_out = hc.out<double>("diag_out_a", (size_t)n * 2);  // mean | var
  if (int rc = hc.ready("pixel moments buffers")) return rc;
  {
    ProfScope ps(ctx, "diag_pixel_moments", n);
    hipLaunchKernelGGL(k_pixel_moments, dim3(grid_for(ctx, n)), dim3(kBlock), 0, ctx->stream,
                       d_scaled, n, R, rr, n_reps, d_out, d_out + n);
  }
  HIP_TRY(hipGetLastError());
  hc.back(mean, d_out, (size_t)n);
  hc.back(var, d_out + n, (size_t)n);
  return hc.finish();
}

int h3d_balance_pixels(h3d_ctx* ctx, const int32_t* row, const int32_t* col, const int64_t* raw,
                       const double* bias, int64_t n, int R, int n_bins, double* balanced) {
  using namespace h3ddiag;
  if (int rc = check_count(ctx, n)) return rc;
  if (R < 1 || R > h3d::kMaxReps) return fail(H3D_EARG, "R=%d outside [1, %d]", R, h3d::kMaxReps);
  if (n_bins < 0) return fail(H3D_EARG, "n_bins=%d", n_bins);
  if (n == 0) return 0;
  if (!row || !col || !raw || !balanced) return fail(H3D_EARG, "null input / output");
  if (n_bins > 0 && !bias) return fail(H3D_EARG, "null bias");
  HostCall hc(ctx);
  int32_t* d_row = hc.in("diag_idx", row, (size_t)n, 1);
  int32_t* d_col = hc.in("diag_idx_s", col, (size_t)n, 1);
  int64_t* d_raw = (int64_t*)hc.out<double>("diag_in_a", (size_t)n * R);
  hc.up(d_raw, raw, (size_t)n * R);
  double* d_bias = hc.out<double>("diag_in_b", (size_t)n_bins * R + 1);
  hc.up(d_bias, bias, (size_t)n_bins * R);
  double* d_out = hc.out<double>("diag_out_a", (size_t)n * R);
  if (int rc = hc.ready("balance buffers")) return rc;
  {
    ProfScope ps(ctx, "diag_balance_pixels", n * R);
    hipLaunchKernelGGL(k_balance_pixels, dim3(grid_for(ctx, n * R)), dim3(kBlock), 0, ctx->stream,
                       d_row, d_col, d_raw, d_bias, n, R, n_bins, d_out);
  }
  HIP_TRY(hipGetLastError());
  hc.back(balanced, d_out, (size_t)n * R);
  return hc.finish();
}

}  // extern "C"
