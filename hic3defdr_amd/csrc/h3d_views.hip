// libh3d.so: dense views of sparse results -- many dense windows gathered
// from a CSR matrix or from the lexsorted pixel table of an outdir stage in
// one launch (h3d_window_gather[_dev]), and the per-cell aggregate of a stack
// of windows (h3d_stack_aggregate). They replace the reference's per-window
// host loops: util/matrices.py:132-160 select_matrix (a boolean mask over the
// whole table per window), analysis/core.py:255-291 get_matrix and
// util/apa.py:6-44 make_apa_stack (one scipy slice + toarray per cluster).
//
//  * k_rows_to_indptr: the table's (row, col) pairs are sorted by row, then
//    col, so the CSR row pointers are one lower-bound search per row;
//  * k_window_gather: one lane per output cell. The cell's column is looked up
//    by binary search inside its row's indptr range (at most dist_thresh_max
//    + 1 entries for an outdir table), once for all K data columns; the K
//    values are stored (consecutive lanes write consecutive addresses) or,
//    in mean mode, summed in list order and divided by K;
//  * k_stack_partial / k_stack_final: the aggregate in a fixed order -- the
//    windows in chunks of kAggChunk, each chunk summed window by window, the
//    chunk sums added chunk by chunk -- so a rerun gives the same bits
//    whatever the grid; no floating-point atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>

#include "h3d.h"
#include "h3d_ctx.h"
#include "h3d_errors.h"

#pragma clang fp contract(off)

using namespace h3dint;
using h3derr::fail;

namespace h3dviews {

constexpr int kBlock = kLaunchBlock;
constexpr int kMaxK = 64;         // data columns per call (kernel argument)
constexpr int kAggChunk = 128;    // windows per partial sum of the aggregate
constexpr int32_t kNanWindow = std::numeric_limits<int32_t>::min();

struct Cols {
  int32_t c[kMaxK];
};

// indptr[r] = the first table entry whose row is >= r, r = 0 .. n_rows
__global__ __launch_bounds__(kBlock) void k_rows_to_indptr(const int32_t* __restrict__ row,
                                                           int64_t nnz, int n_rows,
                                                           int64_t* __restrict__ indptr) {
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r <= n_rows;
       r += (int64_t)gridDim.x * kBlock) {
    int64_t lo = 0, hi = nnz;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (row[mid] < r) lo = mid + 1;
      else hi = mid;
    }
    indptr[r] = lo;
  }
}

// entry index of A[i, j], or -1 when it is not stored or lies outside the
// matrix (the bounds are tested before indptr is read)
__device__ inline int64_t find_entry(const int64_t* __restrict__ indptr,
                                     const int32_t* __restrict__ indices, int64_t nnz,
                                     int n_rows, int n_cols, int64_t i, int64_t j) {
  if (i < 0 || i >= n_rows || j < 0 || j >= n_cols) return -1;
  int64_t lo = indptr[i], hi = indptr[i + 1];
  lo = lo < 0 ? 0 : lo;  // (a caller's indptr never indexes outside indices)
  hi = hi > nnz ? nnz : hi;
  const int64_t end = hi;
  const int32_t want = (int32_t)j;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (indices[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  // at the row's end lo is another row's entry (or nnz)
  if (lo >= end) return -1;
  return indices[lo] == want ? lo : -1;
}

// out (K, W, h, w), or (W, h, w) with mean: cell (win, r, c) of the window at
// origins[win] = (row0, col0)
__global__ __launch_bounds__(kBlock) void k_window_gather(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const double* __restrict__ data, int64_t nnz, int ld, int n_rows, int n_cols, Cols cols,
    int K, const int32_t* __restrict__ origins, int64_t n_cells, int h, int w, int symmetrize,
    int mean, double fill, double* __restrict__ out) {
  const int64_t hw = (int64_t)h * w;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int64_t cell = (int64_t)blockIdx.x * kBlock + threadIdx.x; cell < n_cells;
       cell += (int64_t)gridDim.x * kBlock) {
    const int64_t win = cell / hw;
    const int rc = (int)(cell - win * hw);
    const int r = rc / w, c = rc - r * w;
    const int32_t row0 = origins[2 * win], col0 = origins[2 * win + 1];
    int64_t e = -1;
    const bool nan_window = row0 == kNanWindow;
    if (!nan_window) {
      const int64_t i = (int64_t)row0 + r, j = (int64_t)col0 + c;
      if (symmetrize) e = find_entry(indptr, indices, nnz, n_rows, n_cols, j, i);
      if (e < 0) e = find_entry(indptr, indices, nnz, n_rows, n_cols, i, j);
    }
    const double absent = nan_window ? nan : fill;
    if (mean) {
      double s = e >= 0 ? data[e * ld + cols.c[0]] : absent;
      for (int k = 1; k < K; ++k) s += e >= 0 ? data[e * ld + cols.c[k]] : absent;
      out[cell] = s / (double)K;
    } else {
      for (int k = 0; k < K; ++k)
        out[(int64_t)k * n_cells + cell] = e >= 0 ? data[e * ld + cols.c[k]] : absent;
    }
  }
}

// partial (n_chunks, cells): chunk q's non-NaN count and sum of every cell,
// over the windows q * kAggChunk .. in window order
__global__ __launch_bounds__(kBlock) void k_stack_partial(const double* __restrict__ stack,
                                                          int64_t W, int64_t cells,
                                                          int64_t n_chunks,
                                                          int64_t* __restrict__ pcount,
                                                          double* __restrict__ psum) {
  const int64_t total = n_chunks * cells;
  for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * kBlock) {
    const int64_t q = t / cells, cell = t - q * cells;
    const int64_t w0 = q * kAggChunk;
    const int64_t w1 = w0 + kAggChunk < W ? w0 + kAggChunk : W;
    int64_t n = 0;
    double s = 0.0;
    for (int64_t win = w0; win < w1; ++win) {
      const double v = stack[win * cells + cell];
      if (v == v) {
        s += v;
        n += 1;
      }
    }
    pcount[t] = n;
    psum[t] = s;
  }
}

__global__ __launch_bounds__(kBlock) void k_stack_final(const int64_t* __restrict__ pcount,
                                                        const double* __restrict__ psum,
                                                        int64_t cells, int64_t n_chunks,
                                                        int64_t* __restrict__ count,
                                                        double* __restrict__ sum) {
  for (int64_t cell = (int64_t)blockIdx.x * kBlock + threadIdx.x; cell < cells;
       cell += (int64_t)gridDim.x * kBlock) {
    int64_t n = 0;
    double s = 0.0;
    for (int64_t q = 0; q < n_chunks; ++q) {
      n += pcount[q * cells + cell];
      s += psum[q * cells + cell];
    }
    count[cell] = n;
    sum[cell] = s;
  }
}

// the argument checks shared by the two gather entry points (host or device
// buffers); *n_cells = the cells of one data column (W * h * w). 0 = run it,
// 1 = no windows, < 0 = an error
int check_gather(const void* ctx, const void* indptr, const void* row, const void* indices,
                 const void* data, int ld, int n_rows, int n_cols, const int32_t* cols, int K,
                 const void* origins, int64_t W, int h, int w, int64_t nnz, const void* out,
                 int64_t* n_cells) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  if (h < 1 || w < 1) return fail(H3D_EARG, "window shape %d x %d: h and w must be >= 1", h, w);
  if (K < 1) return fail(H3D_EARG, "K=%d: at least one data column", K);
  if (K > kMaxK) return fail(H3D_EARG, "K=%d: at most %d data columns per call", K, kMaxK);
  if (!cols) return fail(H3D_EARG, "null column list");
  if (ld < 1) return fail(H3D_EARG, "ld=%d", ld);
  for (int k = 0; k < K; ++k)
    if (cols[k] < 0 || cols[k] >= ld)
      return fail(H3D_EARG, "data column %d (list entry %d) not below ld=%d", cols[k], k, ld);
  if (W < 0 || nnz < 0 || n_rows < 0 || n_cols < 0)
    return fail(H3D_EARG, "negative size (W=%lld, nnz=%lld, shape %d x %d)", (long long)W,
                (long long)nnz, n_rows, n_cols);
  // K * W * h * w < 2^31, without overflow
  const int64_t cap = (int64_t)1 << 31;
  const int64_t per = (int64_t)h * w;  // < 2^62
  if (per >= cap || K * per >= cap || (W > 0 && W >= (cap + K * per - 1) / (K * per)))
    return fail(H3D_EARG, "K * W * h * w = %d * %lld * %d * %d is not below 2^31", K,
                (long long)W, h, w);
  *n_cells = W * per;
  if (W == 0) return 1;
  if (!origins || !out) return fail(H3D_EARG, "null origins / output");
  if (!indptr && !row && nnz > 0) return fail(H3D_EARG, "neither indptr nor row given");
  if (nnz > 0 && (!indices || !data)) return fail(H3D_EARG, "null indices / data");
  return 0;
}

// enqueues the gather on the ctx stream: device pointers throughout; with
// d_indptr NULL the row pointers are built from d_row into the ctx's scratch
int launch_gather(h3d_ctx* ctx, const int64_t* d_indptr, const int32_t* d_row,
                  const int32_t* d_indices, const double* d_data, int64_t nnz, int ld,
                  int n_rows, int n_cols, const int32_t* cols, int K, const int32_t* d_origins,
                  int64_t n_cells, int h, int w, int symmetrize, int mean, double fill,
                  double* d_out) {
  hipStream_t s = ctx->stream;
  if (!d_indptr) {
    Scratch sc{ctx};
    int64_t* ip = sc.get<int64_t>("views_indptr", (size_t)n_rows + 1);
    if (!sc.ok) return fail(H3D_ENOMEM, "row pointers");
    ProfScope ps(ctx, "views_indptr", n_rows);
    hipLaunchKernelGGL(k_rows_to_indptr, dim3(grid_for(ctx, (int64_t)n_rows + 1)), dim3(kBlock),
                       0, s, d_row, nnz, n_rows, ip);
    d_indptr = ip;
  }
  Cols cc{};
  for (int k = 0; k < K; ++k) cc.c[k] = cols[k];
  {
    ProfScope ps(ctx, "window_gather", n_cells);
    hipLaunchKernelGGL(k_window_gather, dim3(grid_for(ctx, n_cells)), dim3(kBlock), 0, s,
                       d_indptr, d_indices, d_data, nnz, ld, n_rows, n_cols, cc, K, d_origins,
                       n_cells, h, w, symmetrize ? 1 : 0, mean ? 1 : 0, fill, d_out);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace h3dviews

extern "C" {

int h3d_window_gather_dev(h3d_ctx* ctx, const int64_t* d_indptr, const int32_t* d_row,
                          const int32_t* d_indices, const double* d_data, int64_t nnz, int ld,
                          int n_rows, int n_cols, const int32_t* cols, int K,
                          const int32_t* d_origins, int64_t W, int h, int w, int symmetrize,
                          int mean, double fill, double* d_out) {
  using namespace h3dviews;
  int64_t n_cells = 0;
  if (int rc = check_gather(ctx, d_indptr, d_row, d_indices, d_data, ld, n_rows, n_cols, cols, K,
                            d_origins, W, h, w, nnz, d_out, &n_cells))
    return rc < 0 ? rc : 0;
  HIP_TRY(hipSetDevice(ctx->device));
  if (int rc = launch_gather(ctx, d_indptr, d_row, d_indices, d_data, nnz, ld, n_rows, n_cols,
                             cols, K, d_origins, n_cells, h, w, symmetrize, mean, fill, d_out))
    return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}

int h3d_window_gather(h3d_ctx* ctx, const int64_t* indptr, const int32_t* row,
                      const int32_t* indices, const double* data, int64_t nnz, int ld,
                      int n_rows, int n_cols, const int32_t* cols, int K,
                      const int32_t* origins, int64_t W, int h, int w, int symmetrize,
                      int mean, double fill, double* out) {
  using namespace h3dviews;
  int64_t n_cells = 0;
  if (int rc = check_gather(ctx, indptr, row, indices, data, ld, n_rows, n_cols, cols, K,
                            origins, W, h, w, nnz, out, &n_cells))
    return rc < 0 ? rc : 0;
  if (indptr) {  // a caller's row pointers must stay inside indices
    if (indptr[0] < 0 || indptr[n_rows] > nnz)
      return fail(H3D_EARG, "indptr spans [%lld, %lld], nnz = %lld", (long long)indptr[0],
                  (long long)indptr[n_rows], (long long)nnz);
    for (int r = 0; r < n_rows; ++r)
      if (indptr[r] > indptr[r + 1]) return fail(H3D_EARG, "indptr decreases at row %d", r);
  }
  const int64_t n_out = mean ? n_cells : (int64_t)K * n_cells;
  HostCall hc(ctx);
  int64_t* d_indptr = hc.in("views_indptr", indptr, (size_t)n_rows + 1);
  int32_t* d_row = indptr ? nullptr : hc.out<int32_t>("views_row", (size_t)nnz + 1);
  hc.up(d_row, row, (size_t)nnz);
  int32_t* d_indices = hc.out<int32_t>("views_indices", (size_t)nnz + 1);
  hc.up(d_indices, indices, (size_t)nnz);
  double* d_data = hc.out<double>("views_data", (size_t)nnz * ld + 1);
  hc.up(d_data, data, (size_t)nnz * ld);
  int32_t* d_origins = hc.in("views_origins", origins, (size_t)W * 2);
  double* d_out = hc.out<double>("views_out", (size_t)n_out);
  if (int rc = hc.ready("window gather buffers")) return rc;
  if (int rc = launch_gather(ctx, d_indptr, d_row, d_indices, d_data, nnz, ld, n_rows, n_cols,
                             cols, K, d_origins, n_cells, h, w, symmetrize, mean, fill, d_out))
    return rc;
  hc.back(out, d_out, (size_t)n_out);
  return hc.finish();
}

int h3d_stack_aggregate(h3d_ctx* ctx, const double* stack, int64_t W, int h, int w,
                        int64_t* count, double* sum) {
  using namespace h3dviews;
  if (!ctx) return fail(H3D_EARG, "null ctx");
  if (h < 1 || w < 1) return fail(H3D_EARG, "window shape %d x %d: h and w must be >= 1", h, w);
  if (W < 0) return fail(H3D_EARG, "W=%lld", (long long)W);
  if (!count || !sum) return fail(H3D_EARG, "null output");
  const int64_t cells = (int64_t)h * w;
  if (cells >= ((int64_t)1 << 31) || (W > 0 && W >= ((int64_t)1 << 40) / cells))
    return fail(H3D_EARG, "W * h * w = %lld * %d * %d is not below 2^40", (long long)W, h, w);
  if (W == 0) {
    for (int64_t i = 0; i < cells; ++i) {
      count[i] = 0;
      sum[i] = 0.0;
    }
    return 0;
  }
  if (!stack) return fail(H3D_EARG, "null stack");
  hipStream_t s = ctx->stream;
  const int64_t n_chunks = (W + kAggChunk - 1) / kAggChunk;
  HostCall hc(ctx);
  double* d_stack = hc.in("views_out", stack, (size_t)W * cells);
  int64_t* d_pcount = hc.out<int64_t>("views_pcount", (size_t)n_chunks * cells);
  double* d_psum = hc.out<double>("views_psum", (size_t)n_chunks * cells);
  int64_t* d_count = hc.out<int64_t>("views_count", (size_t)cells);
  double* d_sum = hc.out<double>("views_sum", (size_t)cells);
  if (int rc = hc.ready("stack aggregate buffers")) return rc;
  {
    ProfScope ps(ctx, "stack_aggregate", W * cells);
    hipLaunchKernelGGL(k_stack_partial, dim3(grid_for(ctx, n_chunks * cells)), dim3(kBlock), 0,
                       s, d_stack, W, cells, n_chunks, d_pcount, d_psum);
    hipLaunchKernelGGL(k_stack_final, dim3(grid_for(ctx, cells)), dim3(kBlock), 0, s, d_pcount,
                       d_psum, cells, n_chunks, d_count, d_sum);
  }
  HIP_TRY(hipGetLastError());
  hc.back(count, d_count, (size_t)cells);
  hc.back(sum, d_sum, (size_t)cells);
  return hc.finish();
}

}  // extern "C"
