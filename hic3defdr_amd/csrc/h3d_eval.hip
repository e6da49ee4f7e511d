// libh3d.so: scoring an analysis against simulated truth on the GPU.
//
//   h3d_pixel_membership  analysis.py:117-125 / evaluation.py:38-41: is pixel
//                         (row, col) in a set of pixels -- the set's 64-bit
//                         keys radix-sorted once, one binary search per query;
//   h3d_roc_curve         evaluation.py:73-78: scikit-learn's
//                         _binary_clf_curve + roc_curve(drop_intermediate) and
//                         the FDR points, from ONE radix sort of the scores;
//   h3d_order_stats,      plotting/distance_bias.py:101-112: the order
//   h3d_bin_fractions     statistics np.percentile interpolates between, and
//                         per distance range the pixels and those below p*.
//
// Every output is an integer count or the correctly rounded quotient of two
// counts, so the results equal the host code's bit for bit, whatever the
// launch grid. No floating-point atomics: counts come from integer scans,
// ballots and integer atomics. n < 2^31 throughout.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <limits>

#include "h3d.h"
#include "h3d_ctx.h"
#include "h3d_cub.h"
#include "h3d_devutil.h"
#include "h3d_errors.h"

using namespace h3dint;
using h3derr::fail;

namespace h3deval {

constexpr int kBlock = kLaunchBlock;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxRanks = 64;   // K of h3d_order_stats
constexpr int kMaxRanges = 64;  // B of h3d_bin_fractions: one lane per range
constexpr int64_t kMaxN = ((int64_t)1 << 31) - 1;

// the block's sum of v, valid in thread 0
__device__ inline int block_sum(int v) {
  __shared__ int s_part[kWaves];
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kWaves; ++w) t += s_part[w];
  return t;
}

// ---- pixel membership ---------------------------------------------------------

// key = row << 32 | col; a set pixel with a coordinate outside [0, 2^31) gets
// the key ~0, which no query has (a query's key is below 2^63)
__global__ __launch_bounds__(kBlock) void k_mem_set_keys(const int64_t* __restrict__ prow,
                                                         const int64_t* __restrict__ pcol,
                                                         int64_t k, uint64_t* __restrict__ keys) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < k;
       i += (int64_t)gridDim.x * kBlock) {
    const uint64_t r = (uint64_t)prow[i], c = (uint64_t)pcol[i];
    keys[i] = (r <= (uint64_t)kMaxN && c <= (uint64_t)kMaxN) ? ((r << 32) | c) : ~0ull;
  }
}

// out[i] = 1 where the query's key is among the k sorted set keys; a query
// coordinate outside [0, 2^31) sets *flag
__global__ __launch_bounds__(kBlock) void k_mem_query(const int64_t* __restrict__ row,
                                                      const int64_t* __restrict__ col, int64_t n,
                                                      const uint64_t* __restrict__ set, int64_t k,
                                                      uint8_t* __restrict__ out,
                                                      int* __restrict__ flag) {
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlock) {
    const uint64_t r = (uint64_t)row[i], c = (uint64_t)col[i];
    uint8_t hit = 0;
    if (r > (uint64_t)kMaxN || c > (uint64_t)kMaxN) {
      bad = 1;
    } else {
      const uint64_t key = (r << 32) | c;
      int64_t lo = 0, hi = k;  // the first position whose key is >= key
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (set[mid] < key)
          lo = mid + 1;
        else
          hi = mid;
      }
      hit = (lo < k && set[lo] == key) ? 1 : 0;
    }
    out[i] = hit;
  }
  if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(flag, 1);
}

// device pointers in and out; *h_flag = 1 where a query was out of range.
// Synchronises the stream.
int launch_membership(h3d_ctx* ctx, const int64_t* d_row, const int64_t* d_col, int64_t n,
                      const int64_t* d_prow, const int64_t* d_pcol, int64_t k, uint8_t* d_out,
                      int* h_flag) {
  hipStream_t s = ctx->stream;
  Scratch sc{ctx};
  uint64_t* keys = sc.get<uint64_t>("eval_mk", (size_t)k);
  uint64_t* keys_s = sc.get<uint64_t>("eval_mk_s", (size_t)k);
  int* d_flag = sc.get<int>("eval_flag", 2);
  if (!sc.ok) return fail(H3D_ENOMEM, "membership buffers");
  ProfScope ps(ctx, "eval_membership", n);
  HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_mem_set_keys, dim3(grid_for(ctx, k)), dim3(kBlock), 0, s, d_prow, d_pcol,
                     k, keys);
  if (int rc = cub_call(ctx, "cub_tmp_eval", [&](void* tmp, size_t& bytes) {
        return sort_keys(tmp, bytes, keys, keys_s, (int)k, 0, 64, s);
      }))
    return rc;
  hipLaunchKernelGGL(k_mem_query, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, d_row, d_col, n,
                     keys_s, k, d_out, d_flag);
  HIP_TRY(hipGetLastError());
  return d2h_sync(ctx, h_flag, d_flag, sizeof(int), s);
}

// both membership entry points' checks: 0 = run it, 1 = n or k is 0, < 0 = an error
int check_membership(const void* ctx, const void* row, const void* col, int64_t n,
                     const void* prow, const void* pcol, int64_t k, const void* out) {
  if (int rc = check_count(ctx, n)) return rc;
  if (k < 0 || k > kMaxN) return fail(H3D_EARG, "k=%lld outside [0, 2^31)", (long long)k);
  if (n == 0) return 1;
  if (!row || !col || !out) return fail(H3D_EARG, "null query / output");
  if (k == 0) return 1;
  if (!prow || !pcol) return fail(H3D_EARG, "null set");
  return 0;
}

// ---- ROC / FDR curve ----------------------------------------------------------

// descending key of the score (the complement of asc_key), the score being
// 1 - v with `complement`; *nan_count += the NaN scores
__global__ __launch_bounds__(kBlock) void k_roc_keys(const double* __restrict__ v, int64_t n,
                                                     int complement,
                                                     uint64_t* __restrict__ keys,
                                                     int* __restrict__ nan_count) {
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlock) {
    double x = v[i];
    if (complement) x = 1.0 - x;
    if (x != x) bad += 1;
    keys[i] = ~asc_key(x);
  }
  const int t = block_sum(bad);
  if (threadIdx.x == 0 && t) atomicAdd(nan_count, t);
}

// packed[p] = (run end ? 1 : 0) << 32 | label: one inclusive sum gives, in the
// low word, the positives up to p (tps) and, in the high word, the run ends
// up to p (the compacted position + 1). Both stay below 2^31: no carry.
__global__ __launch_bounds__(kBlock) void k_roc_mark(const uint64_t* __restrict__ ks,
                                                     const uint8_t* __restrict__ lab, int64_t n,
                                                     int64_t* __restrict__ packed) {
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n;
       p += (int64_t)gridDim.x * kBlock) {
    const int64_t end = (p == n - 1 || ks[p] != ks[p + 1]) ? 1 : 0;
    packed[p] = (end << 32) | (lab[p] ? 1 : 0);
  }
}

// the run ends, compacted: run j ends at p with tps = cum[p] low word,
// fps = 1 + p - tps, key = the run's score key
__global__ __launch_bounds__(kBlock) void k_roc_runs(const uint64_t* __restrict__ ks,
                                                     const int64_t* __restrict__ cum, int64_t n,
                                                     int32_t* __restrict__ fps_r,
                                                     int32_t* __restrict__ tps_r,
                                                     uint64_t* __restrict__ key_r) {
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n;
       p += (int64_t)gridDim.x * kBlock) {
    if (p == n - 1 || ks[p] != ks[p + 1]) {
      const int64_t c = cum[p];
      const int64_t j = (c >> 32) - 1;  // in [0, p]
      const int64_t t = c & 0xffffffffll;
      tps_r[j] = (int32_t)t;
      fps_r[j] = (int32_t)(1 + p - t);
      key_r[j] = ks[p];
    }
  }
}

// keep[j] = 1 for the runs roc_curve keeps: all of them without `drop` or
// with at most two; else the first, the last and every interior one where
// the second difference of fps or of tps is non-zero. keep[j] = 0 for
// j >= the number of runs (the scan behind it covers all n)
__global__ __launch_bounds__(kBlock) void k_roc_keep(const int32_t* __restrict__ fps_r,
                                                     const int32_t* __restrict__ tps_r,
                                                     const int64_t* __restrict__ cum, int64_t n,
                                                     int drop, int32_t* __restrict__ keep) {
  const int64_t m = cum[n - 1] >> 32;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n;
       j += (int64_t)gridDim.x * kBlock) {
    int32_t k = 0;
    if (j < m) {
      k = 1;
      if (drop && m > 2 && j > 0 && j < m - 1) {
        const int64_t df = (int64_t)fps_r[j + 1] - 2 * (int64_t)fps_r[j] + fps_r[j - 1];
        const int64_t dt = (int64_t)tps_r[j + 1] - 2 * (int64_t)tps_r[j] + tps_r[j - 1];
        k = (df != 0 || dt != 0) ? 1 : 0;
      }
    }
    keep[j] = k;
  }
}

// the kept runs behind the origin: point i = pos[j] (pos the inclusive sum of
// keep, so i >= 1); point 0 = (0, 0, thresh[1] + 1), scikit-learn 0.24's
// opening; *m_out = the number of points
__global__ __launch_bounds__(kBlock) void k_roc_emit(
    const int32_t* __restrict__ fps_r, const int32_t* __restrict__ tps_r,
    const uint64_t* __restrict__ key_r, const int32_t* __restrict__ keep,
    const int32_t* __restrict__ pos, const int64_t* __restrict__ cum, int64_t n,
    int64_t* __restrict__ fps, int64_t* __restrict__ tps, double* __restrict__ thresh,
    int64_t* __restrict__ m_out) {
  const int64_t m = cum[n - 1] >> 32;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < m;
       j += (int64_t)gridDim.x * kBlock) {
    if (keep[j]) {
      const int64_t i = pos[j];  // in [1, j + 1], so below n + 1
      fps[i] = fps_r[j];
      tps[i] = tps_r[j];
      thresh[i] = asc_value(~key_r[j]);
    }
    if (j == 0) {
      fps[0] = 0;
      tps[0] = 0;
      thresh[0] = asc_value(~key_r[0]) + 1.0;
    }
    if (j == m - 1) *m_out = (int64_t)pos[j] + 1;
  }
}

// fpr = fps / fps[m - 1], tpr = tps / tps[m - 1] (0 / 0 = NaN), and fdr =
// fps / (fps + tps) at i = start, start + rate, ..., NaN elsewhere; start =
// the first i with tps[i] > 0 (tps ascends: a binary search), 0 without one
__global__ __launch_bounds__(kBlock) void k_roc_finish(
    const int64_t* __restrict__ fps, const int64_t* __restrict__ tps,
    const int64_t* __restrict__ m_p, int64_t n_fdr_points, double* __restrict__ fdr,
    double* __restrict__ fpr, double* __restrict__ tpr) {
  __shared__ int64_t s_start;
  const int64_t m = *m_p;
  if (threadIdx.x == 0) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (tps[mid] > 0)
        hi = mid;
      else
        lo = mid + 1;
    }
    s_start = lo < m ? lo : 0;
  }
  __syncthreads();
  const int64_t start = s_start;
  const int64_t rate = std::max<int64_t>(m / n_fdr_points, 1);
  const double f_last = (double)fps[m - 1], t_last = (double)tps[m - 1];
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * kBlock) {
    const int64_t f = fps[i], t = tps[i];
    fpr[i] = (double)f / f_last;
    tpr[i] = (double)t / t_last;
    fdr[i] = (i >= start && (i - start) % rate == 0)
                 ? (double)f / (double)(f + t)
                 : std::numeric_limits<double>::quiet_NaN();
  }
}

// everything on the device, outputs of capacity n + 1; d_m (int64) and
// d_nan (int) are filled on the stream. n >= 1.
int launch_roc(h3d_ctx* ctx, const uint8_t* d_labels, const double* d_scores, int64_t n,
               int64_t n_fdr_points, int drop, int complement, double* d_fdr, double* d_fpr,
               double* d_tpr, double* d_thresh, int64_t* d_fps, int64_t* d_tps, int64_t* d_m,
               int* d_nan) {
  hipStream_t s = ctx->stream;
  Scratch sc{ctx};
  uint64_t* keys = sc.get<uint64_t>("eval_rk", (size_t)n);  // then the packed marks
  uint64_t* keys_s = sc.get<uint64_t>("eval_rk_s", (size_t)n);
  uint8_t* lab_s = sc.get<uint8_t>("eval_lab_s", (size_t)n);
  int64_t* cum = sc.get<int64_t>("eval_cum", (size_t)n);
  int32_t* fps_r = sc.get<int32_t>("eval_fps_r", (size_t)n);
  int32_t* tps_r = sc.get<int32_t>("eval_tps_r", (size_t)n);
  uint64_t* key_r = sc.get<uint64_t>("eval_key_r", (size_t)n);
  int32_t* keep = sc.get<int32_t>("eval_keep", (size_t)n);
  int32_t* pos = sc.get<int32_t>("eval_pos", (size_t)n);
  if (!sc.ok) return fail(H3D_ENOMEM, "roc buffers");
  int64_t* packed = (int64_t*)keys;  // SortPairs leaves its input unread afterwards
  auto sort = [&](void* tmp, size_t& bytes) {
    return sort_pairs(tmp, bytes, keys, keys_s, d_labels, lab_s, (int)n, 0, 64, s);
  };
  auto scan_marks = [&](void* tmp, size_t& bytes) {
    return inclusive_sum(tmp, bytes, packed, cum, (int)n, s);
  };
  auto scan_keep = [&](void* tmp, size_t& bytes) {
    return inclusive_sum(tmp, bytes, keep, pos, (int)n, s);
  };
  // one temp for the three, reserved at the largest before the first runs
  size_t tb = 0, tb2 = 0, tb3 = 0;
  if (cub_bytes(sort, &tb) || cub_bytes(scan_marks, &tb2) || cub_bytes(scan_keep, &tb3))
    return H3D_EHIP;
  sc.get<char>("cub_tmp_eval", std::max(tb, std::max(tb2, tb3)));
  if (!sc.ok) return fail(H3D_ENOMEM, "roc buffers");
  ProfScope ps(ctx, "eval_roc", n);
  const int g = grid_for(ctx, n);
  HIP_TRY(hipMemsetAsync(d_nan, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_roc_keys, dim3(g), dim3(kBlock), 0, s, d_scores, n, complement, keys,
                     d_nan);
  if (int rc = cub_call(ctx, "cub_tmp_eval", sort)) return rc;
  hipLaunchKernelGGL(k_roc_mark, dim3(g), dim3(kBlock), 0, s, keys_s, lab_s, n, packed);
  if (int rc = cub_call(ctx, "cub_tmp_eval", scan_marks)) return rc;
  hipLaunchKernelGGL(k_roc_runs, dim3(g), dim3(kBlock), 0, s, keys_s, cum, n, fps_r, tps_r,
                     key_r);
  hipLaunchKernelGGL(k_roc_keep, dim3(g), dim3(kBlock), 0, s, fps_r, tps_r, cum, n, drop, keep);
  if (int rc = cub_call(ctx, "cub_tmp_eval", scan_keep)) return rc;
  hipLaunchKernelGGL(k_roc_emit, dim3(g), dim3(kBlock), 0, s, fps_r, tps_r, key_r, keep, pos,
                     cum, n, d_fps, d_tps, d_thresh, d_m);
  hipLaunchKernelGGL(k_roc_finish, dim3(g), dim3(kBlock), 0, s, d_fps, d_tps, d_m, n_fdr_points,
                     d_fdr, d_fpr, d_tpr);
  HIP_TRY(hipGetLastError());
  return 0;
}

// both roc entry points' checks (have_bufs: no input or output array is NULL)
int check_roc(const void* ctx, int64_t n, int64_t n_fdr_points, const void* m_out,
              const void* flags, bool have_bufs) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  if (n < 1 || n > kMaxN) return fail(H3D_EARG, "n=%lld outside [1, 2^31)", (long long)n);
  if (n_fdr_points < 1) return fail(H3D_EARG, "n_fdr_points=%lld", (long long)n_fdr_points);
  if (!m_out || !flags) return fail(H3D_EARG, "null m_out / flags");
  if (!have_bufs) return fail(H3D_EARG, "null argument");
  return 0;
}

// (m, NaN count) -> *m_out, *flags; synchronises the stream
int roc_status(h3d_ctx* ctx, const int64_t* d_m, const int* d_nan, int64_t n, int64_t* m_out,
               int* flags) {
  // d_m and d_nan are 8 bytes apart in one slot: one copy
  int64_t h[2] = {0, 0};
  if (int rc = d2h_sync(ctx, h, d_m, 16, ctx->stream)) return rc;
  int nan = 0;
  std::memcpy(&nan, &h[1], sizeof(int));
  *flags = nan ? H3D_FLAG_BADIN : 0;
  *m_out = h[0];
  if (h[0] < 2 || h[0] > n + 1) return fail(H3D_EHIP, "roc curve of %lld points", (long long)h[0]);
  return 0;
}

// ---- order statistics and per-range fractions ----------------------------------

// ascending keys, every NaN last (key ~0); *nan_count += the NaNs
__global__ __launch_bounds__(kBlock) void k_os_keys(const double* __restrict__ v, int64_t n,
                                                    uint64_t* __restrict__ keys,
                                                    int* __restrict__ nan_count) {
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlock) {
    const double x = v[i];
    const bool nan = x != x;
    if (nan) bad += 1;
    keys[i] = nan ? ~0ull : asc_key(x);
  }
  const int t = block_sum(bad);
  if (threadIdx.x == 0 && t) atomicAdd(nan_count, t);
}

struct Ranks {
  int64_t r[kMaxRanks];
};

// out[j] = the value at rank r[j] (each inside [0, n): checked on the host)
__global__ __launch_bounds__(64) void k_os_pick(const uint64_t* __restrict__ ks, Ranks ranks,
                                                int K, double* __restrict__ out) {
  const int j = threadIdx.x;
  if (j < K) out[j] = asc_value(ks[ranks.r[j]]);
}

struct Ranges {
  int64_t lo[kMaxRanges], hi[kMaxRanges];
};

// members[b] += the pixels with lo[b] <= dist <= hi[b], below[b] += those of
// them with p < p_star. A wave takes 64 pixels at a time; for each range one
// ballot counts its pixels and lane b keeps range b's running counts, so the
// loop has no memory traffic beyond the bounds (LDS, one address per wave).
// The waves' counts meet in LDS: one atomic per non-empty range and block.
__global__ __launch_bounds__(kBlock) void k_bin_fractions(
    const double* __restrict__ p, const int64_t* __restrict__ dist, int64_t n, Ranges rg, int B,
    double p_star, unsigned long long* __restrict__ members,
    unsigned long long* __restrict__ below) {
  __shared__ int64_t s_lo[kMaxRanges], s_hi[kMaxRanges];
  __shared__ uint32_t s_mem[kWaves][kMaxRanges], s_bel[kWaves][kMaxRanges];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if ((int)threadIdx.x < B) {
    s_lo[threadIdx.x] = rg.lo[threadIdx.x];
    s_hi[threadIdx.x] = rg.hi[threadIdx.x];
  }
  __syncthreads();
  uint32_t my_mem = 0, my_bel = 0;
  // the trip count is the wave's, not the lane's: every lane joins each ballot
  for (int64_t base = (int64_t)blockIdx.x * kBlock + wave * 64; base < n;
       base += (int64_t)gridDim.x * kBlock) {
    const int64_t i = base + lane;
    const bool live = i < n;
    const int64_t d = live ? dist[i] : 0;
    const bool lt = live && p[i] < p_star;
    for (int b = 0; b < B; ++b) {
      const bool in = live && d >= s_lo[b] && d <= s_hi[b];
      const unsigned long long m_in = __ballot(in), m_lt = __ballot(in && lt);
      if (lane == b) {
        my_mem += (uint32_t)__popcll(m_in);
        my_bel += (uint32_t)__popcll(m_lt);
      }
    }
  }
  s_mem[wave][lane] = my_mem;
  s_bel[wave][lane] = my_bel;
  __syncthreads();
  if ((int)threadIdx.x < B) {
    unsigned long long tm = 0, tb = 0;
    for (int w = 0; w < kWaves; ++w) {
      tm += s_mem[w][threadIdx.x];
      tb += s_bel[w][threadIdx.x];
    }
    if (tm) atomicAdd(members + threadIdx.x, tm);
    if (tb) atomicAdd(below + threadIdx.x, tb);
  }
}

}  // namespace h3deval

extern "C" {

int h3d_pixel_membership_dev(h3d_ctx* ctx, const int64_t* d_row, const int64_t* d_col, int64_t n,
                             const int64_t* d_prow, const int64_t* d_pcol, int64_t k,
                             uint8_t* d_out) {
  using namespace h3deval;
  const int rc = check_membership(ctx, d_row, d_col, n, d_prow, d_pcol, k, d_out);
  if (rc < 0 || n == 0) return rc < 0 ? rc : 0;
  HIP_TRY(hipSetDevice(ctx->device));
  if (k == 0) {
    HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)n, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
  }
  int flag = 0;
  if (int lrc = launch_membership(ctx, d_row, d_col, n, d_prow, d_pcol, k, d_out, &flag))
    return lrc;
  if (flag) return fail(H3D_EARG, "a query pixel has a coordinate outside [0, 2^31)");
  return 0;
}

int h3d_pixel_membership(h3d_ctx* ctx, const int64_t* row, const int64_t* col, int64_t n,
                         const int64_t* prow, const int64_t* pcol, int64_t k, uint8_t* out) {
  using namespace h3deval;
  const int rc = check_membership(ctx, row, col, n, prow, pcol, k, out);
  if (rc < 0 || n == 0) return rc < 0 ? rc : 0;
  if (k == 0) {
    std::memset(out, 0, (size_t)n);
    return 0;
  }
  HostCall hc(ctx);
  int64_t* d_row = hc.in("eval_in_row", row, (size_t)n);
  int64_t* d_col = hc.in("eval_in_col", col, (size_t)n);
  int64_t* d_prow = hc.in("eval_in_prow", prow, (size_t)k);
  int64_t* d_pcol = hc.in("eval_in_pcol", pcol, (size_t)k);
  uint8_t* d_out = hc.out<uint8_t>("eval_out_b", (size_t)n);
  if (int arc = hc.ready("membership buffers")) return arc;
  int flag = 0;
  if (int lrc = launch_membership(ctx, d_row, d_col, n, d_prow, d_pcol, k, d_out, &flag))
    return lrc;
  if (flag) return fail(H3D_EARG, "a query pixel has a coordinate outside [0, 2^31)");
  hc.back(out, d_out, (size_t)n);
  return hc.finish();
}

int h3d_roc_curve_dev(h3d_ctx* ctx, const uint8_t* d_labels, const double* d_scores, int64_t n,
                      int64_t n_fdr_points, int drop_intermediate, int complement,
                      double* d_fdr, double* d_fpr, double* d_tpr, double* d_thresh,
                      int64_t* d_fps, int64_t* d_tps, int64_t* m_out, int* flags) {
  using namespace h3deval;
  if (int rc = check_roc(ctx, n, n_fdr_points, m_out, flags,
                         d_labels && d_scores && d_fdr && d_fpr && d_tpr && d_thresh &&
                             d_fps && d_tps))
    return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  int64_t* d_st = (int64_t*)scratch(ctx, "eval_status", 16);
  if (!d_st) return fail(H3D_ENOMEM, "roc status");
  if (int rc = launch_roc(ctx, d_labels, d_scores, n, n_fdr_points, drop_intermediate,
                          complement, d_fdr, d_fpr, d_tpr, d_thresh, d_fps, d_tps, d_st,
                          (int*)(d_st + 1)))
    return rc;
  return roc_status(ctx, d_st, (int*)(d_st + 1), n, m_out, flags);
}

int h3d_roc_curve(h3d_ctx* ctx, const uint8_t* labels, const double* scores, int64_t n,
                  int64_t n_fdr_points, int drop_intermediate, int complement, double* fdr,
                  double* fpr, double* tpr, double* thresh, int64_t* fps, int64_t* tps,
                  int64_t* m_out, int* flags) {
  using namespace h3deval;
  if (int rc = check_roc(ctx, n, n_fdr_points, m_out, flags,
                         labels && scores && fdr && fpr && tpr && thresh && fps && tps))
    return rc;
  HostCall hc(ctx);
  uint8_t* d_labels = hc.in("eval_in_lab", labels, (size_t)n);
  double* d_scores = hc.in("eval_in_score", scores, (size_t)n);
  // fdr, fpr, tpr, thresh, fps, tps: six arrays of n + 1 words in one slot
  const size_t cap = (size_t)n + 1;
  double* d_out = hc.out<double>("eval_out_roc", 6 * cap);
  int64_t* d_st = hc.out<int64_t>("eval_status", 2);
  if (int rc = hc.ready("roc buffers")) return rc;
  int64_t* d_fps = (int64_t*)(d_out + 4 * cap);
  int64_t* d_tps = (int64_t*)(d_out + 5 * cap);
  if (int rc = launch_roc(ctx, d_labels, d_scores, n, n_fdr_points, drop_intermediate,
                          complement, d_out, d_out + cap, d_out + 2 * cap, d_out + 3 * cap,
                          d_fps, d_tps, d_st, (int*)(d_st + 1)))
    return rc;
  if (int rc = roc_status(ctx, d_st, (int*)(d_st + 1), n, m_out, flags)) return rc;
  const size_t m = (size_t)*m_out;
  hc.back(fdr, d_out, m);
  hc.back(fpr, d_out + cap, m);
  hc.back(tpr, d_out + 2 * cap, m);
  hc.back(thresh, d_out + 3 * cap, m);
  hc.back(fps, d_fps, m);
  hc.back(tps, d_tps, m);
  return hc.finish();
}

int h3d_order_stats(h3d_ctx* ctx, const double* values, int64_t n, const int64_t* ranks, int K,
                    double* out, int64_t* nan_count) {
  using namespace h3deval;
  if (int rc = check_count(ctx, n)) return rc;
  if (K < 0 || K > kMaxRanks) return fail(H3D_EARG, "K=%d outside [0, %d]", K, kMaxRanks);
  if (!nan_count || (K > 0 && (!ranks || !out))) return fail(H3D_EARG, "null argument");
  Ranks rk;
  std::memset(&rk, 0, sizeof(rk));
  for (int j = 0; j < K; ++j) {
    if (ranks[j] < 0 || ranks[j] >= n)
      return fail(H3D_EARG, "rank %lld outside [0, %lld)", (long long)ranks[j], (long long)n);
    rk.r[j] = ranks[j];
  }
  *nan_count = 0;
  if (n == 0) return 0;
  if (!values) return fail(H3D_EARG, "null values");
  hipStream_t s = ctx->stream;
  HostCall hc(ctx);
  double* d_v = hc.in("eval_in_score", values, (size_t)n);
  uint64_t* keys = hc.out<uint64_t>("eval_rk", (size_t)n);
  uint64_t* keys_s = hc.out<uint64_t>("eval_rk_s", (size_t)n);
  // the K picked values, then the NaN count, in one slot (one copy back)
  double* d_res = hc.out<double>("eval_os_res", kMaxRanks + 1);
  if (int rc = hc.ready("order statistics buffers")) return rc;
  int* d_nan = (int*)(d_res + kMaxRanks);
  {
    ProfScope ps(ctx, "eval_order_stats", n);
    HIP_TRY(hipMemsetAsync(d_nan, 0, 8, s));
    hipLaunchKernelGGL(k_os_keys, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, d_v, n, keys,
                       d_nan);
    if (int rc = cub_call(ctx, "cub_tmp_eval", [&](void* tmp, size_t& bytes) {
          return sort_keys(tmp, bytes, keys, keys_s, (int)n, 0, 64, s);
        }))
      return rc;
    if (K > 0) hipLaunchKernelGGL(k_os_pick, dim3(1), dim3(64), 0, s, keys_s, rk, K, d_res);
    HIP_TRY(hipGetLastError());
  }
  double h[kMaxRanks + 1];
  if (int rc = hc.finish(h, d_res, sizeof(h))) return rc;
  for (int j = 0; j < K; ++j) out[j] = h[j];
  int nan = 0;
  std::memcpy(&nan, &h[kMaxRanks], sizeof(int));
  *nan_count = nan;
  return 0;
}

int h3d_bin_fractions(h3d_ctx* ctx, const double* p, const int64_t* dist, int64_t n,
                      const int64_t* lo, const int64_t* hi, int B, double p_star,
                      int64_t* members, int64_t* below) {
  using namespace h3deval;
  if (int rc = check_count(ctx, n)) return rc;
  if (B < 1 || B > kMaxRanges) return fail(H3D_EARG, "B=%d outside [1, %d]", B, kMaxRanges);
  if (!lo || !hi || !members || !below) return fail(H3D_EARG, "null argument");
  for (int b = 0; b < B; ++b) members[b] = below[b] = 0;
  if (n == 0) return 0;
  if (!p || !dist) return fail(H3D_EARG, "null p / dist");
  Ranges rg;
  std::memset(&rg, 0, sizeof(rg));
  for (int b = 0; b < B; ++b) {
    rg.lo[b] = lo[b];
    rg.hi[b] = hi[b];
  }
  hipStream_t s = ctx->stream;
  HostCall hc(ctx);
  double* d_p = hc.in("eval_in_score", p, (size_t)n);
  int64_t* d_dist = hc.in("eval_in_row", dist, (size_t)n);
  unsigned long long* d_cnt = hc.out<unsigned long long>("eval_bf_cnt", 2 * kMaxRanges);
  if (int rc = hc.ready("bin fraction buffers")) return rc;
  {
    ProfScope ps(ctx, "eval_bin_fractions", n);
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 2 * kMaxRanges * 8, s));
    hipLaunchKernelGGL(k_bin_fractions, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, d_p, d_dist,
                       n, rg, B, p_star, d_cnt, d_cnt + kMaxRanges);
    HIP_TRY(hipGetLastError());
  }
  unsigned long long h[2 * kMaxRanges];
  if (int rc = hc.finish(h, d_cnt, sizeof(h))) return rc;
  for (int b = 0; b < B; ++b) {
    members[b] = (int64_t)h[b];
    below[b] = (int64_t)h[kMaxRanges + b];
  }
  return 0;
}

}  // extern "C"
