// libh3d.so: per-cluster statistics of a sparse table on the GPU
// (cluster_table.py:192-332 add_columns_to_cluster_table's arithmetic).
//
//   h3d_cluster_stats / _dev   mean, max and min of a table's K columns over
//                              the pixels of every cluster, and how many of a
//                              cluster's pixels the table holds.
//
// A keyed gather plus a segmented reduction: table keys (row << 32 | col) ->
// sorted with the table index as payload (or, under the `sorted` promise,
// checked in place) -> one lane per cluster pixel finds its table index by
// binary search -> the clusters are cut into tasks of at most kChunk pixels
// (per-cluster task counts, an inclusive sum, one lane per task finds its
// cluster) -> one wave per task folds its pixels into one partial per column
// -> one lane per (cluster, column) folds the cluster's partials in task
// order. The order of every floating-point operation is h3d_cstat.h's, so:
//   - no floating-point atomics: partials are stored, then summed;
//   - a cluster's results are a pure function of its pixel list, the table
//     and K: tasks, lanes and folds depend on the cluster's size alone, not
//     on the grid, the other clusters or the column blocking;
//   - no kernel waits for another workgroup: the phases are separate launches
//     and every loop has its bound next to it;
//   - bad input sets flag bits by compares ahead of any dependent read.
#include <hip/hip_runtime.h>

#include "h3d.h"
#include "h3d_cstat.h"
#include "h3d_ctx.h"
#include "h3d_cub.h"
#include "h3d_errors.h"

using namespace h3dint;
using h3derr::fail;

namespace h3dcstat {

static_assert(kFlagRepeat == H3D_CSTAT_REPEAT && kFlagOrder == H3D_CSTAT_ORDER &&
                  kFlagPixel == H3D_CSTAT_PIXEL && kFlagStarts == H3D_CSTAT_STARTS,
              "flag bits of h3d.h");
static_assert(kWantMean == H3D_CSTAT_MEAN && kWantMax == H3D_CSTAT_MAX &&
                  kWantMin == H3D_CSTAT_MIN,
              "want bits of h3d.h");

constexpr int kBlock = kLaunchBlock;
constexpr int kWaves = kBlock / kLanes;

#define H3D_GRID_STRIDE(i, n)                                          \
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < (n); \
       i += (int64_t)gridDim.x * kBlock)

// *flag |= the bits any thread of the block holds, once per block
// (__syncthreads_or gives a predicate, so each flag bit is voted on its own)
__device__ inline void raise(int bits, int* flag) {
  int any = 0;
  for (int b = kFlagRepeat; b <= kFlagStarts; b <<= 1)
    if (__syncthreads_or(bits & b)) any |= b;
  if (any && threadIdx.x == 0) atomicOr(flag, any);
}

// keys[i] of table pixel i; under the `sorted` promise also the order check
// against pixel i - 1 (k_run_heads' rule: strictly increasing)
__global__ __launch_bounds__(kBlock) void k_cstat_keys(const int64_t* __restrict__ row,
                                                       const int64_t* __restrict__ col, int64_t n,
                                                       int sorted, uint64_t* __restrict__ keys,
                                                       int* __restrict__ flag) {
  int bad = 0;
  H3D_GRID_STRIDE(i, n) {
    const uint64_t key = pixel_key(row[i], col[i]);
    keys[i] = key;
    if (sorted)
      bad |= sorted_flags(i > 0 ? pixel_key(row[i - 1], col[i - 1]) : 0, key, i > 0);
    else if (key == kBadKey)
      bad |= kFlagRepeat;
  }
  raise(bad, flag);
}

// after the sort: two equal neighbours are a repeated table pixel
__global__ __launch_bounds__(kBlock) void k_cstat_repeats(const uint64_t* __restrict__ keys,
                                                          int64_t n, int* __restrict__ flag) {
  int bad = 0;
  H3D_GRID_STRIDE(i, n) if (i > 0 && keys[i] == keys[i - 1]) bad |= kFlagRepeat;
  raise(bad, flag);
}

// ntask[k] of cluster k = pixels starts[k] .. starts[k + 1); a cluster
// without pixels (or starts[0] != 0) sets kFlagStarts and gets no task, so
// every pixel index a later kernel forms lies in [0, starts[nc]).
// st: [0] flags, [1] the task total (written after the sum), [2..3] starts[nc]
__global__ __launch_bounds__(kBlock) void k_cstat_counts(const int64_t* __restrict__ starts,
                                                         int32_t nc, int32_t* __restrict__ ntask,
                                                         int32_t* __restrict__ st) {
  int bad = 0;
  H3D_GRID_STRIDE(k, nc) {
    const int64_t a = starts[k], b = starts[k + 1];
    const bool ok = (k == 0 ? a == 0 : a > 0) && b > a && b - a <= kMaxN;
    if (!ok) bad |= kFlagStarts;
    ntask[k] = ok ? task_count(b - a) : 0;
    if (k == nc - 1) *(int64_t*)(st + 2) = b;
  }
  raise(bad, st);
}

// incl = the inclusive sum of ntask: cluster k's tasks are incl[k] - ntask[k]
// .. incl[k]. One lane per task finds its cluster: the first k with
// incl[k] > t. Terminates: hi - lo shrinks every step.
__global__ __launch_bounds__(kBlock) void k_cstat_tasks(const int32_t* __restrict__ incl,
                                                        int32_t nc, int32_t n_tasks,
                                                        int32_t* __restrict__ task_cl) {
  H3D_GRID_STRIDE(t, n_tasks) {
    int32_t lo = 0, hi = nc - 1;  // incl[nc - 1] = n_tasks > t
    while (lo < hi) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      if (incl[mid] <= (int32_t)t)
        lo = mid + 1;
      else
        hi = mid;
    }
    task_cl[t] = lo;
  }
}

// loc[p] = the table index of cluster pixel p, -1 for absent
__global__ __launch_bounds__(kBlock) void k_cstat_lookup(
    const int64_t* __restrict__ prow, const int64_t* __restrict__ pcol, int64_t n_pix,
    int64_t n_rows, int64_t n_cols, const uint64_t* __restrict__ keys,
    const int32_t* __restrict__ idx, int64_t n, int32_t* __restrict__ loc,
    int* __restrict__ flag) {
  int bad = 0;
  H3D_GRID_STRIDE(p, n_pix) {
    loc[p] = lookup(prow[p], pcol[p], n_rows, n_cols, keys, idx, n, &bad);
  }
  raise(bad ? kFlagPixel : 0, flag);
}

// A wave takes a task (grid-stride over tasks: the task loop's bound is
// wave-uniform, so every lane reaches the shuffles). Its lanes stride over
// the task's pixels; columns go in blocks of KB <= kColBlock held in
// registers. kVec: K is even and data 16-byte aligned, so a pixel's columns
// load as 16-byte pairs. part is (n_tasks, K) records of {sum, max, min};
// tfound[t] = the task's pixels that the table holds.
template <int KB, bool kVec>
__global__ __launch_bounds__(kBlock) void k_cstat_partial(
    const double* __restrict__ data, int K, const int32_t* __restrict__ loc,
    const int64_t* __restrict__ starts, const int32_t* __restrict__ incl,
    const int32_t* __restrict__ ntask, const int32_t* __restrict__ task_cl, int32_t n_tasks,
    Acc* __restrict__ part, int32_t* __restrict__ tfound) {
  static_assert(KB >= 1 && KB <= kColBlock && (!kVec || KB % 2 == 0), "column block");
  const int lane = threadIdx.x & (kLanes - 1);
  const int64_t n_waves = (int64_t)gridDim.x * kWaves;
  for (int64_t t = (int64_t)blockIdx.x * kWaves + (threadIdx.x / kLanes); t < n_tasks;
       t += n_waves) {
    const int32_t k = task_cl[t];
    const int64_t tk = t - (incl[k] - ntask[k]);
    const int64_t p0 = starts[k] + tk * kChunk;
    const int64_t rest = starts[k + 1] - p0;
    const int64_t p1 = p0 + (rest < kChunk ? rest : kChunk);
    for (int c0 = 0; c0 < K; c0 += KB) {
      Acc a[KB];
#pragma unroll
      for (int j = 0; j < KB; ++j) a[j] = acc_init();
      int32_t cnt = 0;
      for (int64_t p = p0 + lane; p < p1; p += kLanes) {
        const int32_t i = loc[p];
        double v[KB];
#pragma unroll
        for (int j = 0; j < KB; ++j) v[j] = 0.0;
        if (i >= 0) {  // an absent pixel never loads
          ++cnt;
          const double* src = data + (int64_t)i * K + c0;
          if constexpr (kVec) {
#pragma unroll
            for (int j = 0; j < KB; j += 2)
              if (c0 + j < K) {
                const double2 w = *reinterpret_cast<const double2*>(src + j);
                v[j] = w.x;
                v[j + 1] = w.y;
              }
          } else {
#pragma unroll
            for (int j = 0; j < KB; ++j)
              if (c0 + j < K) v[j] = src[j];
          }
        }
#pragma unroll
        for (int j = 0; j < KB; ++j) acc_add(a[j], v[j]);
      }
      for (int o = kLanes / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int j = 0; j < KB; ++j) {
          const Acc b{__shfl_down(a[j].sum, o, kLanes), __shfl_down(a[j].mx, o, kLanes),
                      __shfl_down(a[j].mn, o, kLanes)};
          a[j] = acc_fold(a[j], b);
        }
        cnt += __shfl_down(cnt, o, kLanes);
      }
      if (lane == 0) {
#pragma unroll
        for (int j = 0; j < KB; ++j)
          if (c0 + j < K) part[t * K + c0 + j] = a[j];
        if (c0 == 0) tfound[t] = cnt;
      }
    }
  }
}

// one lane per (cluster, column): the cluster's partials in task order
__global__ __launch_bounds__(kBlock) void k_cstat_final(
    const Acc* __restrict__ part, const int32_t* __restrict__ tfound, int K,
    const int64_t* __restrict__ starts, const int32_t* __restrict__ incl,
    const int32_t* __restrict__ ntask, int32_t nc, double* __restrict__ mean,
    double* __restrict__ vmax, double* __restrict__ vmin, int32_t* __restrict__ found) {
  H3D_GRID_STRIDE(e, (int64_t)nc * K) {
    const int32_t k = (int32_t)(e / K), c = (int32_t)(e - (int64_t)k * K);
    const int32_t nt = ntask[k];
    const int64_t t0 = incl[k] - nt;
    Acc a = acc_init();
    int32_t f = 0;
    for (int32_t t = 0; t < nt; ++t) {
      a = acc_fold(a, part[(t0 + t) * K + c]);
      f += tfound[t0 + t];
    }
    const double m = (double)(starts[k + 1] - starts[k]);
    if (mean) mean[e] = canon(a.sum / m);
    if (vmax) vmax[e] = canon(a.mx);
    if (vmin) vmin[e] = canon(a.mn);
    if (found && c == 0) found[k] = f;
  }
}

template <int KB, bool kVec>
void launch_partial(h3d_ctx* ctx, hipStream_t s, const double* data, int K, const int32_t* loc,
                    const int64_t* starts, const int32_t* incl,
                    const int32_t* ntask, const int32_t* task_cl, int32_t n_tasks, Acc* part,
                    int32_t* tfound) {
  hipLaunchKernelGGL((k_cstat_partial<KB, kVec>), dim3(grid_for(ctx, (int64_t)n_tasks * kLanes)),
                     dim3(kBlock), 0, s, data, K, loc, starts, incl, ntask, task_cl,
                     n_tasks, part, tfound);
}

// device pointers; synchronises the stream. *flags gets the H3D_CSTAT_* bits.
int stats_dev(h3d_ctx* ctx, const int64_t* d_row, const int64_t* d_col, const double* d_data,
              int64_t n, int K, int sorted, int64_t n_rows, int64_t n_cols, const int64_t* d_prow,
              const int64_t* d_pcol, const int64_t* d_starts, int64_t n_clusters, int want,
              double* d_mean, double* d_max, double* d_min, int32_t* d_found, int* flags) {
  hipStream_t s = ctx->stream;
  const int32_t nc = (int32_t)n_clusters;
  Scratch sc{ctx};
  uint64_t* keys = sc.get<uint64_t>("cstat_keys", (size_t)n);
  int32_t* ntask = sc.get<int32_t>("cstat_ntask", (size_t)nc);
  int32_t* incl = sc.get<int32_t>("cstat_incl", (size_t)nc);
  int32_t* d_st = sc.get<int32_t>("cstat_status", 4);
  if (!sc.ok) return fail(H3D_ENOMEM, "cluster statistics buffers");
  ProfScope ps(ctx, "cstat", n_clusters);
  HIP_TRY(hipMemsetAsync(d_st, 0, 16, s));
  const uint64_t* keys_s = keys;
  const int32_t* idx_s = nullptr;
  if (n) {
    hipLaunchKernelGGL(k_cstat_keys, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, d_row, d_col, n,
                       sorted, keys, (int*)d_st);
    if (!sorted) {
      uint64_t* ks = sc.get<uint64_t>("cstat_keys_s", (size_t)n);
      int32_t* iota = sc.get<int32_t>("cstat_iota", (size_t)n);
      int32_t* is = sc.get<int32_t>("cstat_idx_s", (size_t)n);
      if (!sc.ok) return fail(H3D_ENOMEM, "table sort buffers");
      launch_iota(ctx, s, iota, n);
      if (int rc = cub_call(ctx, "cub_tmp_cstat", [&](void* tmp, size_t& bytes) {
            return sort_pairs(tmp, bytes, (const uint64_t*)keys, ks, (const int32_t*)iota, is,
                              (int)n, 0, 64, s);
          }))
        return rc;
      hipLaunchKernelGGL(k_cstat_repeats, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, ks, n,
                         (int*)d_st);
      keys_s = ks;
      idx_s = is;
    }
  }
  hipLaunchKernelGGL(k_cstat_counts, dim3(grid_for(ctx, nc)), dim3(kBlock), 0, s, d_starts, nc,
                     ntask, d_st);
  if (int rc = cub_call(ctx, "cub_tmp_cstat", [&](void* tmp, size_t& bytes) {
        return inclusive_sum(tmp, bytes, ntask, incl, (int)nc, s);
      }))
    return rc;
  HIP_TRY(hipGetLastError());
  // the flags so far, the task total and the pixel total in one read
  HIP_TRY(hipMemcpyAsync(d_st + 1, incl + (nc - 1), 4, hipMemcpyDeviceToDevice, s));
  int32_t st[4] = {0, 0, 0, 0};
  if (int rc = d2h_sync(ctx, st, d_st, 16, s)) return rc;
  if (st[0]) {  // nothing past here runs on a broken table or broken starts
    *flags |= st[0];
    return 0;
  }
  const int32_t n_tasks = st[1];
  int64_t n_pix = 0;
  __builtin_memcpy(&n_pix, st + 2, 8);
  if (n_pix > kMaxN)
    return fail(H3D_EARG, "%lld cluster pixels, more than 2^31 - 2", (long long)n_pix);
  int32_t* loc = sc.get<int32_t>("cstat_loc", (size_t)n_pix);
  int32_t* task_cl = sc.get<int32_t>("cstat_task_cl", (size_t)n_tasks);
  Acc* part = sc.get<Acc>("cstat_part", (size_t)n_tasks * K);
  int32_t* tfound = sc.get<int32_t>("cstat_tfound", (size_t)n_tasks);
  if (!sc.ok) return fail(H3D_ENOMEM, "cluster task buffers");
  hipLaunchKernelGGL(k_cstat_tasks, dim3(grid_for(ctx, n_tasks)), dim3(kBlock), 0, s, incl, nc,
                     n_tasks, task_cl);
  hipLaunchKernelGGL(k_cstat_lookup, dim3(grid_for(ctx, n_pix)), dim3(kBlock), 0, s,
                     d_prow, d_pcol, n_pix, n_rows, n_cols, keys_s, idx_s, n, loc,
                     (int*)d_st);
  const bool vec = K % 2 == 0 && ((uintptr_t)d_data & 15) == 0;
#define H3D_CSTAT_PARTIAL(KB, VEC)                                                              \
  launch_partial<KB, VEC>(ctx, s, d_data, K, loc, d_starts, incl, ntask, task_cl, \
                          n_tasks, part, tfound)
  if (K == 1)
    H3D_CSTAT_PARTIAL(1, false);
  else if (K == 2)
    vec ? H3D_CSTAT_PARTIAL(2, true) : H3D_CSTAT_PARTIAL(2, false);
  else if (K <= 4)
    vec ? H3D_CSTAT_PARTIAL(4, true) : H3D_CSTAT_PARTIAL(4, false);
  else
    vec ? H3D_CSTAT_PARTIAL(8, true) : H3D_CSTAT_PARTIAL(8, false);
#undef H3D_CSTAT_PARTIAL
  hipLaunchKernelGGL(k_cstat_final, dim3(grid_for(ctx, (int64_t)nc * K)), dim3(kBlock), 0, s, part,
                     tfound, K, d_starts, incl, ntask, nc, (want & kWantMean) ? d_mean : nullptr,
                     (want & kWantMax) ? d_max : nullptr, (want & kWantMin) ? d_min : nullptr,
                     d_found);
  HIP_TRY(hipGetLastError());
  int fl = 0;
  if (int rc = d2h_sync(ctx, &fl, d_st, 4, s)) return rc;
  *flags |= fl;
  return 0;
}

int check_stats(const void* ctx, const void* row, const void* col, const void* data, int64_t n,
                int K, int64_t n_rows, int64_t n_cols, const void* prow, const void* pcol,
                const void* starts, int64_t n_clusters, int want, const void* mean,
                const void* vmax, const void* vmin, const void* flags) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  if (!flags) return fail(H3D_EARG, "null flags");
  if (n < 0 || n > kMaxN) return fail(H3D_EARG, "n=%lld outside [0, 2^31 - 2]", (long long)n);
  if (K < 1 || K > kMaxK) return fail(H3D_EARG, "K=%d outside [1, %d]", K, kMaxK);
  if (n_rows < 0 || n_rows > kMaxCoord + 1 || n_cols < 0 || n_cols > kMaxCoord + 1)
    return fail(H3D_EARG, "shape (%lld, %lld) outside [0, 2^31]", (long long)n_rows,
                (long long)n_cols);
  if (n_clusters < 0 || n_clusters > kMaxN)
    return fail(H3D_EARG, "n_clusters=%lld outside [0, 2^31 - 2]", (long long)n_clusters);
  if (want & ~(kWantMean | kWantMax | kWantMin)) return fail(H3D_EARG, "want=%d", want);
  if (n_clusters == 0) return 0;
  if (n && (!row || !col || !data)) return fail(H3D_EARG, "null table array");
  if (!prow || !pcol || !starts) return fail(H3D_EARG, "null cluster array");
  if (((want & kWantMean) && !mean) || ((want & kWantMax) && !vmax) ||
      ((want & kWantMin) && !vmin))
    return fail(H3D_EARG, "a wanted output is null");
  return 0;
}

}  // namespace h3dcstat

extern "C" {

int h3d_cluster_stats_dev(h3d_ctx* ctx, const int64_t* d_row, const int64_t* d_col,
                          const double* d_data, int64_t n, int K, int sorted, int64_t n_rows,
                          int64_t n_cols, const int64_t* d_prow, const int64_t* d_pcol,
                          const int64_t* d_starts, int64_t n_clusters, int want, double* d_mean,
                          double* d_max, double* d_min, int32_t* d_found, int* flags) {
  using namespace h3dcstat;
  if (int rc = check_stats(ctx, d_row, d_col, d_data, n, K, n_rows, n_cols, d_prow, d_pcol,
                           d_starts, n_clusters, want, d_mean, d_max, d_min, flags))
    return rc;
  *flags = 0;
  if (n_clusters == 0) return 0;
  HIP_TRY(hipSetDevice(ctx->device));
  return stats_dev(ctx, d_row, d_col, d_data, n, K, sorted, n_rows, n_cols, d_prow, d_pcol,
                   d_starts, n_clusters, want, d_mean, d_max, d_min, d_found, flags);
}

int h3d_cluster_stats(h3d_ctx* ctx, const int64_t* row, const int64_t* col, const double* data,
                      int64_t n, int K, int sorted, int64_t n_rows, int64_t n_cols,
                      const int64_t* prow, const int64_t* pcol, const int64_t* starts,
                      int64_t n_clusters, int want, double* mean, double* vmax, double* vmin,
                      int32_t* found, int* flags) {
  using namespace h3dcstat;
  if (int rc = check_stats(ctx, row, col, data, n, K, n_rows, n_cols, prow, pcol, starts,
                           n_clusters, want, mean, vmax, vmin, flags))
    return rc;
  *flags = 0;
  if (n_clusters == 0) return 0;
  const size_t nc = (size_t)n_clusters, out = nc * (size_t)K;
  // the pixels the clusters name: prow / pcol [0, starts[nc])
  const int64_t p_end = starts[nc];
  if (p_end < 0 || p_end > kMaxN)
    return fail(H3D_EARG, "starts[n_clusters]=%lld outside [0, 2^31 - 2]", (long long)p_end);
  HostCall hc(ctx);
  int64_t* d_row = hc.in("cstat_in_row", row, (size_t)n);
  int64_t* d_col = hc.in("cstat_in_col", col, (size_t)n);
  double* d_data = hc.in("cstat_in_data", data, (size_t)n * K);
  int64_t* d_prow = hc.in("cstat_in_prow", prow, (size_t)p_end);
  int64_t* d_pcol = hc.in("cstat_in_pcol", pcol, (size_t)p_end);
  int64_t* d_starts = hc.in("cstat_in_starts", starts, nc + 1);
  double* d_mean = (want & kWantMean) ? hc.out<double>("cstat_out_mean", out) : nullptr;
  double* d_max = (want & kWantMax) ? hc.out<double>("cstat_out_max", out) : nullptr;
  double* d_min = (want & kWantMin) ? hc.out<double>("cstat_out_min", out) : nullptr;
  int32_t* d_found = found ? hc.out<int32_t>("cstat_out_found", nc) : nullptr;
  if (int rc = hc.ready("cluster statistics buffers")) return rc;
  if (int rc = stats_dev(ctx, d_row, d_col, d_data, n, K, sorted, n_rows, n_cols, d_prow, d_pcol,
                         d_starts, n_clusters, want, d_mean, d_max, d_min, d_found, flags))
    return rc;
  if (*flags) return 0;  // the outputs are unspecified
  if (want & kWantMean) hc.back(mean, d_mean, out);
  if (want & kWantMax) hc.back(vmax, d_max, out);
  if (want & kWantMin) hc.back(vmin, d_min, out);
  hc.back(found, d_found, nc);
  return hc.finish();
}

}  // extern "C"
