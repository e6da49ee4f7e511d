// libh3d.so: the sparse-bin filter and Knight-Ruiz balancing of one
// upper-triangular CSR matrix on the device (h3d_filter_sparse_rows,
// h3d_kr_balance). They replace the scipy.sparse host code of the reference's
// util/filtering.py:8-33 filter_sparse_rows_count and util/balancing.py:5-208
// kr_balance, which the README's simulation workflow runs on every simulated
// replicate (README.md:602-614).
//
//  * filter: k_band_counts counts, per bin, the positive entries of its row
//    (downstream) and of its column (upstream) within k bins of the diagonal
//    (integer atomics: the counts are exact); k_wipe marks the bins below
//    min_nnz on both sides; an entry whose row or column is marked leaves.
//  * symmetrise: count -> scan -> fill. The kept entries of the upper
//    triangle keep their order (an exclusive scan of the keep flags); the
//    strictly lower triangle is the strictly upper one sorted stably by
//    column. Row i of the full matrix is its lower part (ascending column)
//    followed by its upper part (ascending column, the diagonal once):
//    scipy's order, and no floating-point atomics anywhere.
//  * the iteration (Newton outer loop, box-constrained CG inner loop) is the
//    arithmetic of balancing.py's KR class; rows without entries are masked:
//    no kernel reads or reduces them. One inner step is k_dir (p, x p),
//    k_apply (w, partial p.w), k_step (alpha, y + alpha p, r, z, partial
//    min / max / r.z) and k_fin_inner (the fixed-order final pass and the
//    clamp decision into the device state), whose record the host reads to
//    choose the next launch. Every reduction is lane -> wave -> LDS ->
//    per-block partial -> one fixed-order pass over the partials, which each
//    consumer block repeats for itself, so a rerun gives the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <utility>

#include "h3d.h"
#include "h3d_ctx.h"
#include "h3d_cub.h"
#include "h3d_errors.h"

#pragma clang fp contract(off)

using namespace h3dint;
using h3derr::fail;

namespace h3dbal {

constexpr int kBlock = kLaunchBlock;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxParts = 1024;      // blocks (= partials) of a reducing kernel
constexpr int kInnerGuard = 10000;   // inner steps of one call (H3D_ENOCONV)

// control scalars of one run; the host reads the record after k_fin_*
struct KrState {
  double res_sq;    // |1 - x (A x)|^2
  double rho;       // r.z of the current inner step
  double rho_prev;
  double alpha;
  int clamp;       // 0: inside the box, 1: low clamp, 2: high clamp
  int bad;          // a clamp found no candidate (the reference raises)
};

// meta words of the set-up stage
enum { kMetaWiped = 0, kMetaBadCol = 1, kMetaActive = 2, kMetaWords = 4 };

// ---- reductions ------------------------------------------------------------

struct OpSum {
  __device__ static double id() { return 0.0; }
  __device__ static double f(double a, double b) { return a + b; }
};
struct OpMin {
  __device__ static double id() { return std::numeric_limits<double>::infinity(); }
  __device__ static double f(double a, double b) { return b < a ? b : a; }
};
struct OpMax {
  __device__ static double id() { return -std::numeric_limits<double>::infinity(); }
  __device__ static double f(double a, double b) { return b > a ? b : a; }
};

// the block's value of v in every thread: lanes by halving strides, then the
// waves in order. sh: kWaves doubles, free for reuse after the call
template <typename Op>
__device__ inline double block_reduce(double v, double* sh) {
  for (int o = 32; o > 0; o >>= 1) v = Op::f(v, __shfl_down(v, o));
  __syncthreads();  // (sh may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = sh[0];
  for (int w = 1; w < kWaves; ++w) t = Op::f(t, sh[w]);
  return t;
}

// the final pass over a kernel's per-block partials, in a fixed order, the
// same in every block that calls it
template <typename Op>
__device__ inline double reduce_parts(const double* __restrict__ parts, int nparts, double* sh) {
  double v = Op::id();
  for (int i = threadIdx.x; i < nparts; i += kBlock) v = Op::f(v, parts[i]);
  return block_reduce<Op>(v, sh);
}

// ---- set-up: rows of the entries, filter, symmetrise -------------------------

// rowof[e] = the row whose indptr range holds entry e
__global__ __launch_bounds__(kBlock) void k_entry_rows(const int64_t* __restrict__ indptr, int n,
                                                       int64_t nnz,
                                                       int32_t* __restrict__ rowof) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz;
       e += (int64_t)gridDim.x * kBlock) {
    int lo = 0, hi = n;  // the last r in [0, n) with indptr[r] <= e
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (indptr[mid] <= e) lo = mid;
      else hi = mid;
    }
    rowof[e] = lo;
  }
}

__global__ __launch_bounds__(kBlock) void k_band_counts(const int32_t* __restrict__ rowof,
                                                        const int32_t* __restrict__ indices,
                                                        const double* __restrict__ data,
                                                        int64_t nnz, int n, int band,
                                                        int32_t* __restrict__ down,
                                                        int32_t* __restrict__ up) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz;
       e += (int64_t)gridDim.x * kBlock) {
    const int r = rowof[e], c = indices[e];
    if (c < 0 || c >= n) continue;
    const int off = c - r;
    if (off >= 1 && off <= band && data[e] > 0) {
      atomicAdd(&down[r], 1);
      atomicAdd(&up[c], 1);
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_wipe(const int32_t* __restrict__ down,
                                                 const int32_t* __restrict__ up, int n,
                                                 int min_nnz, int32_t* __restrict__ wipe,
                                                 int32_t* __restrict__ meta) {
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const int w = up[i] < min_nnz && down[i] < min_nnz;
    wipe[i] = w;
    if (w) atomicAdd(&meta[kMetaWiped], 1);
  }
}

// keep[e]: the entry stays. drop_zero != 0: an entry of value 0 is no entry
// (scipy's sums and products drop it). upper != 0 (the balancing set-up): a
// column outside [row, n) is flagged and dropped, and the strictly upper kept
// entries get their column as sort key (the others the sentinel n) and count
// into cnt_low[column].
__global__ __launch_bounds__(kBlock) void k_keep(const int32_t* __restrict__ rowof,
                                                 const int32_t* __restrict__ indices,
                                                 const double* __restrict__ data, int64_t nnz,
                                                 int n, const int32_t* __restrict__ wipe,
                                                 int drop_zero, int upper,
                                                 int32_t* __restrict__ keep,
                                                 int32_t* __restrict__ key,
                                                 int32_t* __restrict__ val,
                                                 int32_t* __restrict__ cnt_low,
                                                 int32_t* __restrict__ meta) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e <= nnz;
       e += (int64_t)gridDim.x * kBlock) {
    if (e == nnz) {  // the scan's last word: its exclusive sum is the total
      keep[e] = 0;
      continue;
    }
    const int r = rowof[e], c = indices[e];
    int k = 1;
    if (c < (upper ? r : 0) || c >= n) {
      atomicAdd(&meta[kMetaBadCol], 1);
      k = 0;
    } else {
      if (wipe && (wipe[r] || wipe[c])) k = 0;
      if (drop_zero && !(data[e] != 0)) k = 0;
    }
    keep[e] = k;
    if (upper) {
      const int low = k && c > r;
      key[e] = low ? c : n;
      val[e] = (int32_t)e;
      if (low) atomicAdd(&cnt_low[c], 1);
    }
  }
}

// the filter's output: the kept entries in their order, and their row pointers
__global__ __launch_bounds__(kBlock) void k_compact(const int64_t* __restrict__ indptr,
                                                    const int32_t* __restrict__ indices,
                                                    const double* __restrict__ data, int64_t nnz,
                                                    int n, const int32_t* __restrict__ keep,
                                                    const int32_t* __restrict__ pos,
                                                    int64_t* __restrict__ out_indptr,
                                                    int32_t* __restrict__ out_indices,
                                                    double* __restrict__ out_data) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz;
       e += (int64_t)gridDim.x * kBlock) {
    if (keep[e]) {
      out_indices[pos[e]] = indices[e];
      out_data[pos[e]] = data[e];
    }
    if (e <= n) out_indptr[e] = pos[indptr[e]];
  }
  // (nnz may be below n + 1)
  for (int64_t i = nnz + (int64_t)blockIdx.x * kBlock + threadIdx.x; i <= n;
       i += (int64_t)gridDim.x * kBlock)
    out_indptr[i] = pos[indptr[i]];
}

// row pointers of the full matrix: lower part (low_ptr) + kept upper part
__global__ __launch_bounds__(kBlock) void k_full_rowptr(const int64_t* __restrict__ indptr,
                                                        const int32_t* __restrict__ pos,
                                                        const int32_t* __restrict__ low_ptr,
                                                        int n, int32_t* __restrict__ rowptr,
                                                        int32_t* __restrict__ meta) {
  for (int i = blockIdx.x * kBlock + threadIdx.x; i <= n; i += gridDim.x * kBlock) {
    rowptr[i] = low_ptr[i] + pos[indptr[i]];
    if (i < n) {
      const int len = (low_ptr[i + 1] - low_ptr[i]) + (pos[indptr[i + 1]] - pos[indptr[i]]);
      if (len > 0) atomicAdd(&meta[kMetaActive], 1);
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_fill_upper(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ rowof,
    const int32_t* __restrict__ indices, const double* __restrict__ data, int64_t nnz,
    const int32_t* __restrict__ keep, const int32_t* __restrict__ pos,
    const int32_t* __restrict__ low_ptr, const int32_t* __restrict__ rowptr,
    int32_t* __restrict__ fcol, double* __restrict__ fval) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz;
       e += (int64_t)gridDim.x * kBlock) {
    if (!keep[e]) continue;
    const int r = rowof[e];
    const int dst = rowptr[r] + (low_ptr[r + 1] - low_ptr[r]) + (pos[e] - pos[indptr[r]]);
    fcol[dst] = indices[e];
    fval[dst] = data[e];
  }
}

// sorted entry t (t < the strictly upper kept entries) = A[row, c] becomes
// full[c, row]; the stable sort left a column's entries in ascending row
__global__ __launch_bounds__(kBlock) void k_fill_lower(
    const int32_t* __restrict__ skey, const int32_t* __restrict__ sval, int n_low,
    const int32_t* __restrict__ rowof, const double* __restrict__ data,
    const int32_t* __restrict__ low_ptr, const int32_t* __restrict__ rowptr,
    int32_t* __restrict__ fcol, double* __restrict__ fval) {
  for (int t = blockIdx.x * kBlock + threadIdx.x; t < n_low; t += gridDim.x * kBlock) {
    const int c = skey[t], e = sval[t];
    const int dst = rowptr[c] + (t - low_ptr[c]);
    fcol[dst] = rowof[e];
    fval[dst] = data[e];
  }
}

// ---- the iteration -----------------------------------------------------------

__device__ inline bool row_active(const int32_t* __restrict__ rowptr, int i) {
  return rowptr[i + 1] > rowptr[i];
}

__global__ __launch_bounds__(kBlock) void k_init_x(const int32_t* __restrict__ rowptr, int n,
                                                   const double* __restrict__ x0,
                                                   double* __restrict__ x,
                                                   double* __restrict__ y) {
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    x[i] = row_active(rowptr, i) ? (x0 ? x0[i] : 1.0) : 0.0;
    y[i] = 1.0;
  }
}

// sum over row i of val * in[col], L lanes per row; the group's lane 0 holds it
template <int L>
__device__ inline double row_dot(const int32_t* __restrict__ rowptr,
                                 const int32_t* __restrict__ fcol,
                                 const double* __restrict__ fval, const double* __restrict__ in,
                                 int i, bool valid, int lane) {
  double acc = 0.0;
  if (valid)
    for (int t = rowptr[i] + lane; t < rowptr[i + 1]; t += L) acc += fval[t] * in[fcol[t]];
  for (int o = L >> 1; o > 0; o >>= 1) acc += __shfl_down(acc, o, L);
  return acc;
}

// v = x (A x), r = 1 - v, z = r / v; partials of r.r and r.z
template <int L>
__global__ __launch_bounds__(kBlock) void k_rowsums(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ fcol,
    const double* __restrict__ fval, int n, const double* __restrict__ x,
    double* __restrict__ v, double* __restrict__ r, double* __restrict__ z,
    double* __restrict__ parts) {
  __shared__ double sh[kWaves];
  const int groups = gridDim.x * (kBlock / L);
  const int g = blockIdx.x * (kBlock / L) + threadIdx.x / L, lane = threadIdx.x % L;
  double rr = 0.0, rz = 0.0;
  for (int base = 0; base < n; base += groups) {
    const int i = base + g;
    const bool valid = i < n && row_active(rowptr, i);
    const double ax = row_dot<L>(rowptr, fcol, fval, x, i, valid, lane);
    if (valid && lane == 0) {
      const double vi = x[i] * ax, ri = 1 - vi, zi = ri / vi;
      v[i] = vi;
      r[i] = ri;
      z[i] = zi;
      rr += ri * ri;
      rz += ri * zi;
    }
  }
  rr = block_reduce<OpSum>(rr, sh);
  rz = block_reduce<OpSum>(rz, sh);
  if (threadIdx.x == 0) {
    parts[blockIdx.x] = rr;
    parts[kMaxParts + blockIdx.x] = rz;
  }
}

__global__ __launch_bounds__(kBlock) void k_fin_outer(const double* __restrict__ parts,
                                                      int nparts, KrState* __restrict__ st) {
  __shared__ double sh[kWaves];
  const double rr = reduce_parts<OpSum>(parts, nparts, sh);
  const double rz = reduce_parts<OpSum>(parts + kMaxParts, nparts, sh);
  if (threadIdx.x == 0) {
    st->res_sq = rr;
    st->rho = rz;
    st->clamp = 0;
  }
}

// p = z (first) or z + (rho / rho_prev) p; xp = x p
__global__ __launch_bounds__(kBlock) void k_dir(const int32_t* __restrict__ rowptr, int n,
                                                int first, const KrState* __restrict__ st,
                                                const double* __restrict__ z,
                                                const double* __restrict__ x,
                                                double* __restrict__ p,
                                                double* __restrict__ xp) {
  const double beta = first ? 0.0 : st->rho / st->rho_prev;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    if (!row_active(rowptr, i)) continue;
    const double pi = first ? z[i] : z[i] + beta * p[i];
    p[i] = pi;
    xp[i] = x[i] * pi;
  }
}

// w = x A(x p) + v p; partials of p.w
template <int L>
__global__ __launch_bounds__(kBlock) void k_apply(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ fcol,
    const double* __restrict__ fval, int n, const double* __restrict__ x,
    const double* __restrict__ v, const double* __restrict__ p, const double* __restrict__ xp,
    double* __restrict__ w, double* __restrict__ parts) {
  __shared__ double sh[kWaves];
  const int groups = gridDim.x * (kBlock / L);
  const int g = blockIdx.x * (kBlock / L) + threadIdx.x / L, lane = threadIdx.x % L;
  double pw = 0.0;
  for (int base = 0; base < n; base += groups) {
    const int i = base + g;
    const bool valid = i < n && row_active(rowptr, i);
    const double axp = row_dot<L>(rowptr, fcol, fval, xp, i, valid, lane);
    if (valid && lane == 0) {
      const double wi = x[i] * axp + v[i] * p[i];
      w[i] = wi;
      pw += p[i] * wi;
    }
  }
  pw = block_reduce<OpSum>(pw, sh);
  if (threadIdx.x == 0) parts[blockIdx.x] = pw;
}

// alpha = rho / p.w; y_try = y + alpha p; r -= alpha w; z = r / v; partials
// of min / max y_try and r.z (r and z are rebuilt by k_rowsums when the step
// is clamped, y_try is dropped)
__global__ __launch_bounds__(kBlock) void k_step(
    const int32_t* __restrict__ rowptr, int n, KrState* __restrict__ st,
    const double* __restrict__ parts_pw, int nparts_pw, const double* __restrict__ p,
    const double* __restrict__ w, const double* __restrict__ v, const double* __restrict__ y,
    double* __restrict__ ytry, double* __restrict__ r, double* __restrict__ z,
    double* __restrict__ parts) {
  __shared__ double sh[kWaves];
  const double pw = reduce_parts<OpSum>(parts_pw, nparts_pw, sh);
  const double alpha = st->rho / pw;
  double mn = OpMin::id(), mx = OpMax::id(), rz = 0.0;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    if (!row_active(rowptr, i)) continue;
    const double yt = y[i] + alpha * p[i];
    ytry[i] = yt;
    mn = OpMin::f(mn, yt);
    mx = OpMax::f(mx, yt);
    const double ri = r[i] - alpha * w[i], zi = ri / v[i];
    r[i] = ri;
    z[i] = zi;
    rz += ri * zi;
  }
  mn = block_reduce<OpMin>(mn, sh);
  mx = block_reduce<OpMax>(mx, sh);
  rz = block_reduce<OpSum>(rz, sh);
  if (threadIdx.x == 0) {
    parts[blockIdx.x] = mn;
    parts[kMaxParts + blockIdx.x] = mx;
    parts[2 * kMaxParts + blockIdx.x] = rz;
    if (blockIdx.x == 0) st->alpha = alpha;
  }
}

__global__ __launch_bounds__(kBlock) void k_fin_inner(const double* __restrict__ parts,
                                                      int nparts, double lo, double hi,
                                                      KrState* __restrict__ st) {
  __shared__ double sh[kWaves];
  const double mn = reduce_parts<OpMin>(parts, nparts, sh);
  const double mx = reduce_parts<OpMax>(parts + kMaxParts, nparts, sh);
  const double rz = reduce_parts<OpSum>(parts + 2 * kMaxParts, nparts, sh);
  if (threadIdx.x == 0) {
    if (mn <= lo) {
      st->clamp = 1;
    } else if (mx >= hi) {
      st->clamp = 2;
    } else {
      st->clamp = 0;
      st->rho_prev = st->rho;
      st->rho = rz;
    }
  }
}

// the clamp's multiple: min of (bound - y) / step over step < 0 (low) or
// y_try > bound (high), step = alpha p
__global__ __launch_bounds__(kBlock) void k_gamma(const int32_t* __restrict__ rowptr, int n,
                                                  const KrState* __restrict__ st, int high,
                                                  double bound, const double* __restrict__ p,
                                                  const double* __restrict__ y,
                                                  const double* __restrict__ ytry,
                                                  double* __restrict__ parts) {
  __shared__ double sh[kWaves];
  const double alpha = st->alpha;
  double mn = OpMin::id();
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    if (!row_active(rowptr, i)) continue;
    const double step = alpha * p[i];
    if (high ? ytry[i] > bound : step < 0) mn = OpMin::f(mn, (bound - y[i]) / step);
  }
  mn = block_reduce<OpMin>(mn, sh);
  if (threadIdx.x == 0) parts[blockIdx.x] = mn;
}

// y += gamma step
__global__ __launch_bounds__(kBlock) void k_clamp(const int32_t* __restrict__ rowptr, int n,
                                                  KrState* __restrict__ st,
                                                  const double* __restrict__ parts, int nparts,
                                                  const double* __restrict__ p,
                                                  double* __restrict__ y) {
  __shared__ double sh[kWaves];
  const double gamma = reduce_parts<OpMin>(parts, nparts, sh);
  const double alpha = st->alpha;
  const bool none = gamma == OpMin::id();
  if (blockIdx.x == 0 && threadIdx.x == 0) st->bad = none ? 1 : 0;
  if (none) return;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    if (!row_active(rowptr, i)) continue;
    const double step = alpha * p[i];
    y[i] = y[i] + gamma * step;
  }
}

// x *= y, y = 1
__global__ __launch_bounds__(kBlock) void k_xy(const int32_t* __restrict__ rowptr, int n,
                                               double* __restrict__ x, double* __restrict__ y) {
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    if (row_active(rowptr, i)) x[i] = x[i] * y[i];
    y[i] = 1.0;
  }
}

// ---- rescale and bias ---------------------------------------------------------

// partials of sum(full) and sum(diag(x) full diag(x))
template <int L>
__global__ __launch_bounds__(kBlock) void k_totals(const int32_t* __restrict__ rowptr,
                                                   const int32_t* __restrict__ fcol,
                                                   const double* __restrict__ fval, int n,
                                                   const double* __restrict__ x,
                                                   double* __restrict__ parts) {
  __shared__ double sh[kWaves];
  const int groups = gridDim.x * (kBlock / L);
  const int g = blockIdx.x * (kBlock / L) + threadIdx.x / L, lane = threadIdx.x % L;
  double t1 = 0.0, t2 = 0.0;
  for (int base = 0; base < n; base += groups) {
    const int i = base + g;
    if (i < n) {
      const double xi = x[i];
      for (int t = rowptr[i] + lane; t < rowptr[i + 1]; t += L) {
        t1 += fval[t];
        t2 += (xi * fval[t]) * x[fcol[t]];
      }
    }
  }
  t1 = block_reduce<OpSum>(t1, sh);
  t2 = block_reduce<OpSum>(t2, sh);
  if (threadIdx.x == 0) {
    parts[blockIdx.x] = t1;
    parts[kMaxParts + blockIdx.x] = t2;
  }
}

// scale = x sqrt(sum(full) / sum(scaled full)); bias = 1 / scale, 0 where
// the scale is 0
__global__ __launch_bounds__(kBlock) void k_bias(const double* __restrict__ parts, int nparts,
                                                 int n, const double* __restrict__ x,
                                                 double* __restrict__ scale,
                                                 double* __restrict__ bias) {
  __shared__ double sh[kWaves];
  const double t1 = reduce_parts<OpSum>(parts, nparts, sh);
  const double t2 = reduce_parts<OpSum>(parts + kMaxParts, nparts, sh);
  const double c = sqrt(t1 / t2);
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const double s = x[i] * c;
    scale[i] = s;
    bias[i] = s != 0 ? 1 / s : s;
  }
}

// the balanced upper triangle, entry for entry of the input, in place
__global__ __launch_bounds__(kBlock) void k_balanced(const int32_t* __restrict__ rowof,
                                                     const int32_t* __restrict__ indices,
                                                     const int32_t* __restrict__ keep,
                                                     int64_t nnz, const double* __restrict__ scale,
                                                     double* data) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz;
       e += (int64_t)gridDim.x * kBlock)
    data[e] = keep[e] ? (scale[rowof[e]] * data[e]) * scale[indices[e]] : 0.0;
}

// ---- host side -----------------------------------------------------------------

int parts_grid(int64_t threads) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((threads + kBlock - 1) / kBlock, kMaxParts));
}

// the argument checks shared by the two entry points (host arrays)
int check_csr(const void* ctx, const int64_t* indptr, const int32_t* indices, const double* data,
              int n, int64_t nnz) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  if (n < 0 || nnz < 0) return fail(H3D_EARG, "negative size (n=%d, nnz=%lld)", n, (long long)nnz);
  if (nnz >= ((int64_t)1 << 30))
    return fail(H3D_EARG, "nnz = %lld is not below 2^30", (long long)nnz);
  if (!indptr) return fail(H3D_EARG, "null indptr");
  if (nnz > 0 && (!indices || !data)) return fail(H3D_EARG, "null indices / data");
  if (indptr[0] != 0 || indptr[n] != nnz)
    return fail(H3D_EARG, "indptr spans [%lld, %lld], nnz = %lld", (long long)indptr[0],
                (long long)indptr[n], (long long)nnz);
  for (int r = 0; r < n; ++r)
    if (indptr[r] > indptr[r + 1]) return fail(H3D_EARG, "indptr decreases at row %d", r);
  return 0;
}

// the device copy of the matrix and what the set-up stage derives from it
struct Setup {
  HostCall& hc;
  int n;
  int64_t nnz;
  int64_t* d_indptr = nullptr;
  int32_t *d_indices = nullptr, *d_rowof = nullptr, *d_keep = nullptr, *d_pos = nullptr;
  int32_t *d_wipe = nullptr, *d_meta = nullptr;
  double* d_data = nullptr;
};

// uploads the CSR, finds the entries' rows and, with filter != 0, the wiped
// bins (d_wipe stays NULL otherwise). n > 0 and nnz > 0.
int upload_and_filter(Setup& u, const int64_t* indptr, const int32_t* indices,
                      const double* data, int filter, int min_nnz, int k) {
  HostCall& hc = u.hc;
  h3d_ctx* ctx = hc.ctx;
  hipStream_t s = ctx->stream;
  const int n = u.n;
  const int64_t nnz = u.nnz;
  u.d_indptr = hc.in("kr_indptr", indptr, (size_t)n + 1);
  u.d_indices = hc.in("kr_indices", indices, (size_t)nnz);
  u.d_data = hc.in("kr_data", data, (size_t)nnz);
  u.d_rowof = hc.out<int32_t>("kr_rowof", (size_t)nnz);
  u.d_keep = hc.out<int32_t>("kr_keep", (size_t)nnz + 1);
  u.d_pos = hc.out<int32_t>("kr_pos", (size_t)nnz + 1);
  u.d_meta = hc.out<int32_t>("kr_meta", kMetaWords);
  int32_t* d_cnt = hc.out<int32_t>("kr_band", 2 * (size_t)n);
  int32_t* d_wipe = hc.out<int32_t>("kr_wipe", (size_t)n);
  if (int rc = hc.ready("matrix buffers")) return rc;
  HIP_TRY(hipMemsetAsync(u.d_meta, 0, kMetaWords * 4, s));
  ProfScope ps(ctx, "kr_filter", nnz);
  hipLaunchKernelGGL(k_entry_rows, dim3(grid_for(ctx, nnz)), dim3(kBlock), 0, s, u.d_indptr, n,
                     nnz, u.d_rowof);
  if (filter) {
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 2 * (size_t)n * 4, s));
    hipLaunchKernelGGL(k_band_counts, dim3(grid_for(ctx, nnz)), dim3(kBlock), 0, s, u.d_rowof,
                       u.d_indices, u.d_data, nnz, n, std::min(n, k), d_cnt, d_cnt + n);
    hipLaunchKernelGGL(k_wipe, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, d_cnt, d_cnt + n, n,
                       min_nnz, d_wipe, u.d_meta);
    u.d_wipe = d_wipe;
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

int scan_i32(h3d_ctx* ctx, const int32_t* in, int32_t* out, int64_t count) {
  hipStream_t s = ctx->stream;
  return cub_call(ctx, "kr_cub", [&](void* tmp, size_t& tb) {
    return exclusive_sum(tmp, tb, in, out, (int)count, s);
  });
}

// one balancing run on the symmetrised matrix in the ctx's "kr_*" slots
struct Run {
  h3d_ctx* ctx;
  int n, L;
  const int32_t *rowptr, *fcol;
  const double* fval;
  double *x, *v, *r, *z, *p, *xp, *w, *y, *ytry, *parts_a, *parts_b;
  KrState* st;
  KrState* h_st;  // pinned
  int vec_grid, mv_grid;

  template <int LL>
  void rowsums_l() {
    hipLaunchKernelGGL(k_rowsums<LL>, dim3(mv_grid), dim3(kBlock), 0, ctx->stream, rowptr, fcol,
                       fval, n, x, v, r, z, parts_a);
  }
  template <int LL>
  void apply_l() {
    hipLaunchKernelGGL(k_apply<LL>, dim3(mv_grid), dim3(kBlock), 0, ctx->stream, rowptr, fcol,
                       fval, n, x, v, p, xp, w, parts_a);
  }
  template <int LL>
  void totals_l() {
    hipLaunchKernelGGL(k_totals<LL>, dim3(mv_grid), dim3(kBlock), 0, ctx->stream, rowptr, fcol,
                       fval, n, x, parts_a);
  }
  void rowsums() { L == 4 ? rowsums_l<4>() : L == 16 ? rowsums_l<16>() : rowsums_l<64>(); }
  void apply() { L == 4 ? apply_l<4>() : L == 16 ? apply_l<16>() : apply_l<64>(); }
  void totals() { L == 4 ? totals_l<4>() : L == 16 ? totals_l<16>() : totals_l<64>(); }

  // the device state into the pinned record, once the stream has drained
  int read_state() {
    HIP_TRY(hipMemcpyAsync(h_st, st, sizeof(KrState), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
  }
  // v, r, z and |r|^2 of the current x
  int scaled_rowsums(double* res_sq) {
    rowsums();
    hipLaunchKernelGGL(k_fin_outer, dim3(1), dim3(kBlock), 0, ctx->stream, parts_a, mv_grid, st);
    HIP_TRY(hipGetLastError());
    if (int rc = read_state()) return rc;
    *res_sq = h_st->res_sq;
    return 0;
  }
};

// the Newton / CG iteration of balancing.py's KR class; stats[0..3] = outer
// steps, inner steps, low clamps, high clamps
int iterate(Run& k, double tol, double lo, double hi, int max_iter, int64_t* stats,
            int32_t* hist_inner, double* hist_norm, int hist_cap) {
  hipStream_t s = k.ctx->stream;
  const double target = tol * tol, floor_eta = 0.5 * tol, g = 0.9, eta_cap = 0.1;
  double eta = eta_cap, res_sq = 0.0;
  if (int rc = k.scaled_rowsums(&res_sq)) return rc;
  double res_prev = res_sq;
  int64_t outer = 0, inner_total = 0, n_low = 0, n_high = 0;
  while (res_sq > target) {
    if (max_iter >= 0 && outer > max_iter) break;
    outer += 1;
    const double tol_in = std::max(eta * eta * res_sq, target);
    double rho = res_sq;
    int steps = 0;
    while (rho > tol_in) {
      steps += 1;
      inner_total += 1;
      if (inner_total > kInnerGuard)
        return fail(H3D_ENOCONV, "KR balancing: more than %d inner steps (outer step %lld)",
                    kInnerGuard, (long long)outer);
      hipLaunchKernelGGL(k_dir, dim3(k.vec_grid), dim3(kBlock), 0, s, k.rowptr, k.n,
                         steps == 1 ? 1 : 0, k.st, k.z, k.x, k.p, k.xp);
      k.apply();
      hipLaunchKernelGGL(k_step, dim3(k.vec_grid), dim3(kBlock), 0, s, k.rowptr, k.n, k.st,
                         k.parts_a, k.mv_grid, k.p, k.w, k.v, k.y, k.ytry, k.r, k.z, k.parts_b);
      hipLaunchKernelGGL(k_fin_inner, dim3(1), dim3(kBlock), 0, s, k.parts_b, k.vec_grid, lo, hi,
                         k.st);
      HIP_TRY(hipGetLastError());
      if (int rc = k.read_state()) return rc;
      const int clamp = k.h_st->clamp;
      if (clamp) {
        (clamp == 1 ? n_low : n_high) += 1;
        if (!(clamp == 1 && lo == 0)) {  // (a low clamp at lo == 0 keeps y)
          hipLaunchKernelGGL(k_gamma, dim3(k.vec_grid), dim3(kBlock), 0, s, k.rowptr, k.n, k.st,
                             clamp == 2 ? 1 : 0, clamp == 2 ? hi : lo, k.p, k.y, k.ytry,
                             k.parts_b);
          hipLaunchKernelGGL(k_clamp, dim3(k.vec_grid), dim3(kBlock), 0, s, k.rowptr, k.n, k.st,
                             k.parts_b, k.vec_grid, k.p, k.y);
          HIP_TRY(hipGetLastError());
          if (int rc = k.read_state()) return rc;
          if (k.h_st->bad)
            return fail(H3D_ENOCONV, "KR balancing: the %s clamp has no candidate step",
                        clamp == 1 ? "low" : "high");
        }
        break;
      }
      std::swap(k.y, k.ytry);
      rho = k.h_st->rho;
    }
    hipLaunchKernelGGL(k_xy, dim3(k.vec_grid), dim3(kBlock), 0, s, k.rowptr, k.n, k.x, k.y);
    if (int rc = k.scaled_rowsums(&res_sq)) return rc;
    const double ratio = res_sq / res_prev;
    res_prev = res_sq;
    const double norm = std::sqrt(res_sq);
    // forcing term of the inexact Newton step (Eisenstat-Walker)
    const double eta_last = eta;
    eta = g * ratio;
    if (g * (eta_last * eta_last) > 0.1) eta = std::max(eta, g * (eta_last * eta_last));
    eta = std::max(std::min(eta, eta_cap), floor_eta / norm);
    if (outer <= hist_cap) {
      if (hist_inner) hist_inner[outer - 1] = steps;
      if (hist_norm) hist_norm[outer - 1] = norm;
    }
  }
  stats[0] = outer;
  stats[1] = inner_total;
  stats[2] = n_low;
  stats[3] = n_high;
  return 0;
}

}  // namespace h3dbal

extern "C" {

int h3d_filter_sparse_rows(h3d_ctx* ctx, const int64_t* indptr, const int32_t* indices,
                           const double* data, int n, int64_t nnz, int min_nnz, int k,
                           int64_t* out_indptr, int32_t* out_indices, double* out_data,
                           int64_t* nnz_out, int64_t* n_wiped) {
  using namespace h3dbal;
  if (int rc = check_csr(ctx, indptr, indices, data, n, nnz)) return rc;
  if (!out_indptr || !nnz_out || (nnz > 0 && (!out_indices || !out_data)))
    return fail(H3D_EARG, "null output");
  if (min_nnz < 0 || k < 0) return fail(H3D_EARG, "min_nnz=%d, k=%d", min_nnz, k);
  const int filter = min_nnz > 0 && k > 0;
  if (n_wiped) *n_wiped = 0;
  if (nnz == 0 || n == 0) {  // nothing stored: nothing leaves
    for (int i = 0; i <= n; ++i) out_indptr[i] = 0;
    *nnz_out = 0;
    if (n_wiped && filter) *n_wiped = n;  // (every count is 0 < min_nnz)
    return 0;
  }
  hipStream_t s = ctx->stream;
  HostCall hc(ctx);
  Setup u{hc, n, nnz};
  if (int rc = upload_and_filter(u, indptr, indices, data, filter, min_nnz, k)) return rc;
  int64_t* d_oip = hc.out<int64_t>("kr_out_indptr", (size_t)n + 1);
  int32_t* d_oidx = hc.out<int32_t>("kr_out_indices", (size_t)nnz);
  double* d_odat = hc.out<double>("kr_out_data", (size_t)nnz);
  if (int rc = hc.ready("filter output")) return rc;
  hipLaunchKernelGGL(k_keep, dim3(grid_for(ctx, nnz + 1)), dim3(kBlock), 0, s, u.d_rowof,
                     u.d_indices, u.d_data, nnz, n, u.d_wipe, filter, 0, u.d_keep,
                     (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, u.d_meta);
  if (int rc = scan_i32(ctx, u.d_keep, u.d_pos, nnz + 1)) return rc;
  hipLaunchKernelGGL(k_compact, dim3(grid_for(ctx, std::max<int64_t>(nnz, (int64_t)n + 1))),
                     dim3(kBlock), 0, s, u.d_indptr, u.d_indices, u.d_data, nnz, n, u.d_keep,
                     u.d_pos, d_oip, d_oidx, d_odat);
  HIP_TRY(hipGetLastError());
  int32_t meta[kMetaWords];
  if (int rc = d2h_sync(ctx, meta, u.d_meta, sizeof(meta), s)) return rc;
  if (meta[kMetaBadCol])
    return fail(H3D_EINPUT, "%d column indices outside [0, %d)", meta[kMetaBadCol], n);
  // the kept count (the last row pointer) sizes the other two downloads
  hc.back(out_indptr, d_oip, (size_t)n + 1);
  if (int rc = hc.finish()) return rc;
  const int64_t kept = out_indptr[n];
  hc.back(out_indices, d_oidx, (size_t)kept);
  hc.back(out_data, d_odat, (size_t)kept);
  if (int rc = kept > 0 ? hc.finish() : 0) return rc;
  *nnz_out = kept;
  if (n_wiped) *n_wiped = meta[kMetaWiped];
  return 0;
}

int h3d_kr_balance(h3d_ctx* ctx, const int64_t* indptr, const int32_t* indices,
                   const double* data, int n, int64_t nnz, int min_nnz, int k, double tol,
                   double lo, double hi, int max_iter, const double* x0, double* bias_out,
                   double* balanced_out, int64_t* stats, int32_t* hist_inner, double* hist_norm,
                   int hist_cap) {
  using namespace h3dbal;
  if (int rc = check_csr(ctx, indptr, indices, data, n, nnz)) return rc;
  if (!bias_out && n > 0) return fail(H3D_EARG, "null bias output");
  if (!stats) return fail(H3D_EARG, "null stats");
  if (min_nnz < 0 || k < 0) return fail(H3D_EARG, "min_nnz=%d, k=%d", min_nnz, k);
  if (!(tol >= 0)) return fail(H3D_EARG, "tol=%g", tol);
  if (hist_cap < 0) return fail(H3D_EARG, "hist_cap=%d", hist_cap);
  const int filter = min_nnz > 0 && k > 0;
  for (int i = 0; i < 6; ++i) stats[i] = 0;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (n == 0) return 0;
  if (nnz == 0) {  // no rows in the iteration: 0 * sqrt(0 / 0)
    for (int i = 0; i < n; ++i) bias_out[i] = nan;
    stats[4] = filter ? n : 0;
    return 0;
  }
  hipStream_t s = ctx->stream;
  HostCall hc(ctx);
  Setup u{hc, n, nnz};
  if (int rc = upload_and_filter(u, indptr, indices, data, filter, min_nnz, k)) return rc;

  // symmetrise: keep flags and sort keys, scans, the stable sort, the fills
  Scratch& sc = hc.sc;
  int32_t* d_key = sc.get<int32_t>("kr_key", (size_t)nnz);
  int32_t* d_val = sc.get<int32_t>("kr_val", (size_t)nnz);
  int32_t* d_skey = sc.get<int32_t>("kr_skey", (size_t)nnz);
  int32_t* d_sval = sc.get<int32_t>("kr_sval", (size_t)nnz);
  int32_t* d_cntl = sc.get<int32_t>("kr_cnt_low", (size_t)n + 1);
  int32_t* d_lowptr = sc.get<int32_t>("kr_low_ptr", (size_t)n + 1);
  int32_t* d_rowptr = sc.get<int32_t>("kr_rowptr", (size_t)n + 1);
  int32_t* d_fcol = sc.get<int32_t>("kr_fcol", 2 * (size_t)nnz);
  double* d_fval = sc.get<double>("kr_fval", 2 * (size_t)nnz);
  double* d_vec = sc.get<double>("kr_vec", 11 * (size_t)n);
  double* d_parts = sc.get<double>("kr_parts", 6 * (size_t)kMaxParts);
  double* d_x0 = hc.in("kr_x0", x0, (size_t)n);
  KrState* d_st = sc.get<KrState>("kr_state", 1);
  if (int rc = hc.ready("balancing buffers")) return rc;
  KrState* h_st = (KrState*)pinned_rd(ctx, sizeof(KrState));
  if (!h_st) return fail(H3D_ENOMEM, "pinned record");
  int end_bit = 1;
  while (((int64_t)1 << end_bit) <= n) ++end_bit;  // the sentinel key n fits
  int32_t meta[kMetaWords], full_nnz = 0, n_low = 0;
  {
    ProfScope ps(ctx, "kr_symmetrise", nnz);
    HIP_TRY(hipMemsetAsync(d_cntl, 0, ((size_t)n + 1) * 4, s));
    HIP_TRY(hipMemsetAsync(d_st, 0, sizeof(KrState), s));
    hipLaunchKernelGGL(k_keep, dim3(grid_for(ctx, nnz + 1)), dim3(kBlock), 0, s, u.d_rowof,
                       u.d_indices, u.d_data, nnz, n, u.d_wipe, 1, 1, u.d_keep, d_key, d_val,
                       d_cntl, u.d_meta);
    if (int rc = scan_i32(ctx, u.d_keep, u.d_pos, nnz + 1)) return rc;
    if (int rc = scan_i32(ctx, d_cntl, d_lowptr, (int64_t)n + 1)) return rc;
    if (int rc = cub_call(ctx, "kr_cub", [&](void* tmp, size_t& tb) {
          return sort_pairs(tmp, tb, d_key, d_skey, d_val, d_sval, (int)nnz, 0, end_bit, s);
        }))
      return rc;
    hipLaunchKernelGGL(k_full_rowptr, dim3(grid_for(ctx, (int64_t)n + 1)), dim3(kBlock), 0, s,
                       u.d_indptr, u.d_pos, d_lowptr, n, d_rowptr, u.d_meta);
    HIP_TRY(hipGetLastError());
    if (int rc = d2h_sync(ctx, meta, u.d_meta, sizeof(meta), s)) return rc;
    if (int rc = d2h_sync(ctx, &full_nnz, d_rowptr + n, 4, s)) return rc;
    if (int rc = d2h_sync(ctx, &n_low, d_lowptr + n, 4, s)) return rc;
    if (meta[kMetaBadCol])
      return fail(H3D_EINPUT, "%d column indices outside [row, %d): the matrix must be upper "
                  "triangular", meta[kMetaBadCol], n);
    if (full_nnz > 0) {
      hipLaunchKernelGGL(k_fill_upper, dim3(grid_for(ctx, nnz)), dim3(kBlock), 0, s, u.d_indptr,
                         u.d_rowof, u.d_indices, u.d_data, nnz, u.d_keep, u.d_pos, d_lowptr,
                         d_rowptr, d_fcol, d_fval);
      if (n_low > 0)
        hipLaunchKernelGGL(k_fill_lower, dim3(grid_for(ctx, n_low)), dim3(kBlock), 0, s, d_skey,
                           d_sval, n_low, u.d_rowof, u.d_data, d_lowptr, d_rowptr, d_fcol, d_fval);
      HIP_TRY(hipGetLastError());
    }
  }
  const int n_active = meta[kMetaActive];
  stats[4] = meta[kMetaWiped];
  stats[5] = n_active;
  if (n_active == 0) {  // no rows left: 0 * sqrt(0 / 0), nothing launched
    for (int i = 0; i < n; ++i) bias_out[i] = nan;
    if (balanced_out)
      for (int64_t e = 0; e < nnz; ++e) balanced_out[e] = 0.0;
    return hc.finish();
  }

  Run run;
  run.ctx = ctx;
  run.n = n;
  // lanes per row from the mean row length (a band of a few hundred: 64)
  const double mean_len = (double)full_nnz / n_active;
  run.L = mean_len <= 6 ? 4 : mean_len <= 48 ? 16 : 64;
  run.rowptr = d_rowptr;
  run.fcol = d_fcol;
  run.fval = d_fval;
  double** vecs[] = {&run.x, &run.v, &run.r, &run.z, &run.p, &run.xp, &run.w, &run.y, &run.ytry};
  for (int i = 0; i < 9; ++i) *vecs[i] = d_vec + (size_t)i * n;
  double* d_scale = d_vec + 9 * (size_t)n;
  double* d_bias = d_vec + 10 * (size_t)n;
  run.parts_a = d_parts;
  run.parts_b = d_parts + 3 * (size_t)kMaxParts;
  run.st = d_st;
  run.h_st = h_st;
  run.vec_grid = parts_grid(n);
  run.mv_grid = parts_grid((int64_t)n * run.L);
  hipLaunchKernelGGL(k_init_x, dim3(run.vec_grid), dim3(kBlock), 0, s, d_rowptr, n, d_x0, run.x,
                     run.y);
  {
    ProfScope ps(ctx, "kr_iter", n_active);
    if (int rc = iterate(run, tol, lo, hi, max_iter, stats, hist_inner, hist_norm, hist_cap))
      return rc;
  }
  {
    ProfScope ps(ctx, "kr_rescale", n_active);
    run.totals();
    hipLaunchKernelGGL(k_bias, dim3(run.vec_grid), dim3(kBlock), 0, s, run.parts_a, run.mv_grid,
                       n, run.x, d_scale, d_bias);
    if (balanced_out)
      hipLaunchKernelGGL(k_balanced, dim3(grid_for(ctx, nnz)), dim3(kBlock), 0, s, u.d_rowof,
                         u.d_indices, u.d_keep, nnz, d_scale, u.d_data);
  }
  HIP_TRY(hipGetLastError());
  hc.back(bias_out, d_bias, (size_t)n);
  hc.back(balanced_out, u.d_data, (size_t)nnz);
  return hc.finish();
}

}  // extern "C"
