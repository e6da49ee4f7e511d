// libh3d.so: the prepare_data entry points (union of the replicate band
// matrices, size factors of every norm); shares the ctx / scratch / error
// helpers of h3d_api.hip through h3d_ctx.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "h3d.h"
#include "h3d_ctx.h"
#include "h3d_cub.h"
#include "h3d_errors.h"
#include "h3d_host.h"
#include "h3d_prepare.h"

using namespace h3d;
using namespace h3dint;
using h3derr::fail;

namespace {

constexpr int kBlock = kLaunchBlock;

// h3d_union_count reads as its stages; what they share travels in a
// UnionCall, their results in ctx->prep (for h3d_union_fill).
struct UnionCall {
  h3d_ctx* ctx;  // the request
  int R, n_bins;
  const int64_t* const* indptr;
  const int32_t* const* indices;
  const double* const* data;
  const int64_t* nnz;
  const double* bias;
  int dist_max;
  hipStream_t s = nullptr;
  int64_t sentinel = 0;  // n_bins^2: above every pixel's key
  int end_bit = 1;       // the keys' bits
  // one replicate's staging (reused by the next)
  int64_t* d_indptr = nullptr;
  int32_t *d_row = nullptr, *d_col = nullptr, *d_flag = nullptr, *d_pos = nullptr;
  double* d_val = nullptr;
  // the in-band entries of the replicates staged so far; the heads of their runs
  int64_t tot = 0;
  int64_t* d_keys = nullptr;
  int32_t *d_ent = nullptr, *d_head = nullptr;
};

// Stage: the argument checks, and the staging buffers with the bias in them.
// Only the in-band entries reach the per-entry key / sort / scan buffers, so
// their size and the 2^31 cap follow the band, not the whole-chromosome nnz.
int union_check_and_staging(UnionCall& u) {
  h3d_ctx* ctx = u.ctx;
  const int R = u.R, n_bins = u.n_bins;
  if (!ctx || !u.indptr || !u.indices || !u.data || !u.nnz || !u.bias)
    return fail(H3D_EARG, "null argument");
  if (R < 1 || R > kMaxReps || n_bins < 1 || u.dist_max < 0)
    return fail(H3D_EARG, "R=%d n_bins=%d dist_max=%d", R, n_bins, u.dist_max);
  HIP_TRY(hipSetDevice(ctx->device));
  u.s = ctx->stream;
  ctx->prep = PrepUnion();
  ctx->prep.R = R;
  ctx->prep.n_bins = n_bins;
  int64_t max_m = 0;
  for (int r = 0; r < R; ++r) {
    const int64_t m = u.nnz[r];
    if (m < 0 || (m > 0 && (!u.indices[r] || !u.data[r])) || !u.indptr[r])
      return fail(H3D_EARG, "replicate %d CSR", r);
    if (u.indptr[r][n_bins] != m) return fail(H3D_EARG, "replicate %d indptr[-1] != nnz", r);
    if (m >= ((int64_t)1 << 31)) return fail(H3D_EARG, "replicate %d: too many entries", r);
    max_m = std::max(max_m, m);
  }
  u.sentinel = (int64_t)n_bins * n_bins;
  while (u.end_bit < 63 && (((int64_t)1) << u.end_bit) <= u.sentinel) ++u.end_bit;
  const size_t mm = (size_t)std::max<int64_t>(max_m, 1);
  Scratch sc{ctx};
  ctx->prep.bias = sc.get<double>("u_bias", (size_t)n_bins * R);
  u.d_indptr = sc.get<int64_t>("u_indptr", (size_t)(n_bins + 1));
  u.d_row = sc.get<int32_t>("u_row_of", mm);
  u.d_col = sc.get<int32_t>("u_col", mm);
  u.d_val = sc.get<double>("u_val_in", mm);
  u.d_flag = sc.get<int32_t>("u_flag", mm);
  u.d_pos = sc.get<int32_t>("u_pos", mm);
  sc.get<int32_t>("u_cnt", 1);  // (no reader; the ctx goes on holding what it held)
  if (!sc.ok) return fail(H3D_ENOMEM, "union staging");
  return h2d_pinned(ctx, ctx->prep.bias, u.bias, (size_t)n_bins * R * 8, u.s);
}

// Stage: replicate r's m > 0 entries -- the in-band ones flagged, counted by
// a scan and appended (key, entry, replicate, value) to the earlier ones.
int union_stage_replicate(UnionCall& u, int r) {
  h3d_ctx* ctx = u.ctx;
  hipStream_t s = u.s;
  PrepUnion& P = ctx->prep;
  const int64_t m = u.nnz[r];
  HIP_TRY(hipMemcpyAsync(u.d_indptr, u.indptr[r], (size_t)(u.n_bins + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(u.d_col, u.indices[r], m * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(u.d_val, u.data[r], m * 8, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_csr_rows, dim3((u.n_bins + 255) / 256), dim3(256), 0, s, u.d_indptr,
                     u.n_bins, u.d_row);
  hipLaunchKernelGGL(k_union_flags, dim3(grid_for(ctx, m)), dim3(kBlock), 0, s, u.d_row,
                     u.d_col, u.d_val, m, u.n_bins, u.dist_max, u.d_flag);
  if (int rc = cub_call(ctx, "cub_tmp_s", [&](void* tmp, size_t& tb) {
        return exclusive_sum(tmp, tb, u.d_flag, u.d_pos, (int)m, s);
      }))
    return rc;
  int32_t last[2] = {0, 0};
  if (int rc = d2h_sync(ctx, &last[0], u.d_pos + m - 1, 4, s)) return rc;
  if (int rc = d2h_sync(ctx, &last[1], u.d_flag + m - 1, 4, s)) return rc;
  const int64_t kept = (int64_t)last[0] + last[1], tot = u.tot;
  if (tot + kept >= ((int64_t)1 << 31)) return fail(H3D_EARG, "too many in-band entries");
  // the kept-entry arrays grow (keeping what earlier replicates wrote)
  const size_t need = (size_t)std::max<int64_t>(tot + kept, 1);
  Scratch sc{ctx};
  u.d_keys = sc.keep<int64_t>("u_keys", need, tot);
  u.d_ent = sc.keep<int32_t>("u_ent", need, tot);
  P.ent_rep = sc.keep<int32_t>("u_ent_rep", need, tot);
  P.ent_val = sc.keep<double>("u_ent_val", need, tot);
  if (!sc.ok) return fail(H3D_ENOMEM, "union entries");
  hipLaunchKernelGGL(k_union_keys, dim3(grid_for(ctx, m)), dim3(kBlock), 0, s, u.d_row, u.d_col,
                     u.d_val, u.d_flag, u.d_pos, m, tot, r, u.n_bins, u.d_keys, u.d_ent,
                     P.ent_rep, P.ent_val);
  // the staging buffers are reused by the next replicate
  HIP_TRY(hipStreamSynchronize(s));
  u.tot += kept;
  return 0;
}

// Stage (tot > 0 entries): the entries sorted by pixel key, the heads of the
// runs of equal keys and the runs' count.
int union_sort_runs(UnionCall& u) {
  h3d_ctx* ctx = u.ctx;
  hipStream_t s = u.s;
  PrepUnion& P = ctx->prep;
  const int64_t tot = u.tot;
  Scratch sc{ctx};
  P.keys_sorted = sc.get<int64_t>("u_keys_s", tot);
  P.ent_sorted = sc.get<int32_t>("u_ent_s", tot);
  u.d_head = sc.get<int32_t>("u_head", tot);
  P.run_of = sc.get<int32_t>("u_run_incl", tot);
  if (!sc.ok) return fail(H3D_ENOMEM, "union scratch");
  if (int rc = cub_call(ctx, "cub_tmp_u", [&](void* tmp, size_t& tb) {
        return sort_pairs(tmp, tb, u.d_keys, P.keys_sorted, u.d_ent, P.ent_sorted, (int)tot, 0,
                          u.end_bit, s);
      }))
    return rc;
  hipLaunchKernelGGL(k_run_heads, dim3(grid_for(ctx, tot)), dim3(kBlock), 0, s, P.keys_sorted,
                     tot, u.sentinel, u.d_head);
  if (int rc = cub_call(ctx, "cub_tmp_s", [&](void* tmp, size_t& tb) {
        return inclusive_sum(tmp, tb, u.d_head, P.run_of, (int)tot, s);
      }))
    return rc;
  int32_t n_runs = 0;
  if (int rc = d2h_sync(ctx, &n_runs, P.run_of + tot - 1, 4, s)) return rc;
  P.n_runs = n_runs;
  return 0;
}

// Stage (tot > 0): the runs that are pixels of the union -- flagged in
// "u_keep", which h3d_union_fill takes by its slot -- and their count.
int union_keep_runs(UnionCall& u) {
  h3d_ctx* ctx = u.ctx;
  hipStream_t s = u.s;
  PrepUnion& P = ctx->prep;
  const int64_t n_runs = P.n_runs, tot = u.tot;
  Scratch sc{ctx};
  P.run_start = sc.get<int64_t>("u_run_start", std::max<int64_t>(n_runs, 1));
  int32_t* keep = sc.get<int32_t>("u_keep", std::max<int64_t>(n_runs, 1));
  P.px_of_run = sc.get<int32_t>("u_px_incl", std::max<int64_t>(n_runs, 1));
  if (!sc.ok) return fail(H3D_ENOMEM, "runs");
  if (n_runs == 0) return 0;
  hipLaunchKernelGGL(k_run_starts, dim3(grid_for(ctx, tot)), dim3(kBlock), 0, s, u.d_head,
                     P.run_of, tot, P.run_start);
  hipLaunchKernelGGL(k_run_keep, dim3(grid_for(ctx, n_runs)), dim3(kBlock), 0, s,
                     P.keys_sorted, P.ent_sorted, P.run_start, n_runs, tot, u.sentinel,
                     P.ent_rep, P.ent_val, u.R, u.n_bins, P.bias, keep);
  if (int rc = cub_call(ctx, "cub_tmp_s", [&](void* tmp, size_t& tb) {
        return inclusive_sum(tmp, tb, keep, P.px_of_run, (int)n_runs, s);
      }))
    return rc;
  int32_t n_px = 0;
  if (int rc = d2h_sync(ctx, &n_px, P.px_of_run + n_runs - 1, 4, s)) return rc;
  P.n_px = n_px;
  return 0;
}

}  // namespace

extern "C" {

int h3d_union_count(h3d_ctx* ctx, int R, int n_bins,
                    const int64_t* const* indptr, const int32_t* const* indices,
                    const double* const* data, const int64_t* nnz,
                    const double* bias, int dist_max, int64_t* n_px_out) {
  if (!n_px_out) return fail(H3D_EARG, "null argument");
  UnionCall u{ctx, R, n_bins, indptr, indices, data, nnz, bias, dist_max};
  if (int rc = union_check_and_staging(u)) return rc;
  for (int r = 0; r < R; ++r)
    if (nnz[r] > 0)
      if (int rc = union_stage_replicate(u, r)) return rc;
  ctx->prep.n_entries = u.tot;
  if (u.tot > 0) {
    if (int rc = union_sort_runs(u)) return rc;
    if (int rc = union_keep_runs(u)) return rc;
  }
  *n_px_out = ctx->prep.n_px;
  return 0;
}

int h3d_union_fill(h3d_ctx* ctx, int32_t* row, int32_t* col, int64_t* raw,
                   double* balanced, int64_t n_px) {
  return h3d_union_fill_dev(ctx, row, col, raw, balanced, n_px, nullptr, nullptr, nullptr,
                            nullptr);
}

int h3d_union_fill_dev(h3d_ctx* ctx, int32_t* row, int32_t* col, int64_t* raw,
                       double* balanced, int64_t n_px, int32_t* d_row_out,
                       int32_t* d_col_out, int32_t* d_raw_out, double* d_bal_out) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  PrepUnion& P = ctx->prep;
  if (n_px != P.n_px) return fail(H3D_EARG, "n_px %lld != counted %lld", (long long)n_px, (long long)P.n_px);
  if (n_px == 0) return 0;
  // raw may be NULL when the device copy d_raw_out is requested (the caller
  // fetches it in the background, analysis/d2h.py)
  if (!row || !col || (!raw && !d_raw_out) || (!balanced && !d_bal_out))
    return fail(H3D_EARG, "null output");
  HostCall hc(ctx);
  Scratch& sc = hc.sc;
  hipStream_t s = ctx->stream;
  const int R = P.R;
  int32_t* d_row = sc.get<int32_t>("u_out_row", n_px);
  int32_t* d_col = sc.get<int32_t>("u_out_col", n_px);
  int64_t* d_raw = sc.get<int64_t>("u_out_raw", n_px * R);
  double* d_bal = sc.get<double>("u_out_bal", n_px * R);
  // (h3d_union_count's flags, by their slot)
  int32_t* keep = sc.get<int32_t>("u_keep", std::max<int64_t>(P.n_runs, 1));
  int* d_ovf = sc.get<int>("ovf", 1);
  if (int rc = hc.ready("union out")) return rc;
  hipLaunchKernelGGL(k_union_fill, dim3(grid_for(ctx, P.n_runs)), dim3(kBlock), 0, s,
                     P.keys_sorted, P.ent_sorted, P.run_start, keep, P.px_of_run,
                     P.n_runs, P.n_entries, P.ent_rep, P.ent_val, R, P.n_bins, P.bias,
                     d_row, d_col, d_raw, d_bal);
  // the caller's device copies (the product's resident chromosome): the
  // counts as int32, the width every disp / lrt kernel reads
  if (d_row_out) HIP_TRY(hipMemcpyAsync(d_row_out, d_row, n_px * 4, hipMemcpyDeviceToDevice, s));
  if (d_col_out) HIP_TRY(hipMemcpyAsync(d_col_out, d_col, n_px * 4, hipMemcpyDeviceToDevice, s));
  if (d_bal_out)
    HIP_TRY(hipMemcpyAsync(d_bal_out, d_bal, n_px * R * 8, hipMemcpyDeviceToDevice, s));
  if (d_raw_out) {  // finish() reads the overflow word
    if (int rc = counts_to_i32(ctx, d_raw, d_raw_out, n_px * R, d_ovf)) return rc;
    hc.d_ovf = d_ovf;
    hc.ovf_msg = "raw counts must be in [0, 2^31) for the device copy";
  }
  hc.back(row, d_row, n_px);
  hc.back(col, d_col, n_px);
  hc.back(raw, d_raw, n_px * R);
  hc.back(balanced, d_bal, n_px * R);
  return hc.finish();
}

// d_disp_idx (n) 0/1 -> the chromosome's disp pixels (k_disp_pixels)
int h3d_disp_pixels_dev(h3d_ctx* ctx, const int32_t* d_row, const int32_t* d_col,
                        const int32_t* d_raw, const double* d_sf, int sf_per_rep,
                        const double* bias, int n_bins, const uint8_t* d_disp_idx,
                        int64_t n, int R, int64_t n_disp, int32_t* d_raw_out,
                        double* d_f_out, int32_t* d_dist_out) {
  if (!ctx || !bias) return fail(H3D_EARG, "null argument");
  if (R < 1 || R > kMaxReps || n_bins < 1 || n < 0 || n_disp < 0 || n_disp > n)
    return fail(H3D_EARG, "R=%d n_bins=%d n=%lld n_disp=%lld", R, n_bins, (long long)n,
                (long long)n_disp);
  if (n >= ((int64_t)1 << 31)) return fail(H3D_EARG, "n=%lld exceeds 2^31", (long long)n);
  if (n == 0) return 0;
  if (!d_row || !d_col || !d_raw || !d_sf || !d_disp_idx)
    return fail(H3D_EARG, "null device input");
  if (n_disp > 0 && (!d_raw_out || !d_f_out || !d_dist_out))
    return fail(H3D_EARG, "null device output");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  Scratch sc{ctx};
  int32_t* d_sel = sc.get<int32_t>("dp_sel", (size_t)std::max<int64_t>(n, 1));
  int32_t* d_cnt = sc.get<int32_t>("dp_cnt", 1);
  double* d_bias = sc.get<double>("dp_bias", (size_t)n_bins * R);
  if (!sc.ok) return fail(H3D_ENOMEM, "disp pixel scratch");
  if (int rc = h2d_pinned(ctx, d_bias, bias, (size_t)n_bins * R * 8, s)) return rc;
  if (int rc = cub_call(ctx, "cub_tmp_sel", [&](void* tmp, size_t& bytes) {
        return select_flagged_indices(tmp, bytes, d_disp_idx, d_sel, d_cnt, (int)n, s);
      }))
    return rc;
  int32_t cnt = 0;
  if (int rc = d2h_sync(ctx, &cnt, d_cnt, 4, s)) return rc;
  if (cnt != n_disp)
    return fail(H3D_EARG, "disp_idx selects %d pixels, caller expects %lld", cnt,
                (long long)n_disp);
  if (n_disp == 0) return 0;
  hipLaunchKernelGGL(k_disp_pixels, dim3(grid_for(ctx, n_disp)), dim3(kBlock), 0, s, d_sel,
                     n_disp, d_row, d_col, d_raw, d_sf, sf_per_rep, d_bias, R, d_raw_out,
                     d_f_out, d_dist_out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

int h3d_pixel_f_dev(h3d_ctx* ctx, const int32_t* d_row, const int32_t* d_dist,
                    const int32_t* d_chrom, const int32_t* d_sfi, int64_t n, int R,
                    const double* d_bias, const int64_t* d_boff, const double* d_sf,
                    const int64_t* d_soff, int nchrom, double* d_f_out) {
  if (!ctx) return fail(H3D_EARG, "null argument");
  if (R < 1 || R > kMaxReps || n < 0 || nchrom < 1)
    return fail(H3D_EARG, "R=%d n=%lld nchrom=%d", R, (long long)n, nchrom);
  if (n == 0) return 0;
  if (!d_row || !d_dist || !d_chrom || !d_sfi || !d_bias || !d_boff || !d_sf || !d_soff ||
      !d_f_out)
    return fail(H3D_EARG, "null device pointer");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  Scratch sc{ctx};
  int* d_bad = sc.get<int>("pf_bad", 1);
  if (!sc.ok) return fail(H3D_ENOMEM, "pixel f scratch");
  HIP_TRY(hipMemsetAsync(d_bad, 0, 4, s));
  hipLaunchKernelGGL(k_pixel_f, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, d_row, d_dist,
                     d_chrom, d_sfi, n, R, d_bias, d_boff, d_sf, d_soff, nchrom, d_f_out,
                     d_bad);
  HIP_TRY(hipGetLastError());
  int bad = 0;
  if (int rc = d2h_sync(ctx, &bad, d_bad, 4, s)) return rc;
  if (bad) return fail(H3D_EINPUT, "pixel keys outside the bias / size-factor tables");
  return 0;
}

int h3d_scale_disp_dev(h3d_ctx* ctx, const double* d_balanced, const double* d_sf,
                       int sf_per_rep, const int32_t* d_row, const int32_t* d_col, int64_t n,
                       int R, int C, const uint8_t* design, double mean_thresh,
                       int dist_thresh_min, double* scaled_out, uint8_t* flag_out,
                       uint8_t* d_flag_out, double* d_scaled_out) {
  if (!ctx || !design) return fail(H3D_EARG, "null argument");
  if (R < 1 || R > kMaxReps || C < 1 || C > kMaxConds || n < 0)
    return fail(H3D_EARG, "R=%d C=%d n=%lld", R, C, (long long)n);
  if (n == 0) return 0;
  if (!d_balanced || !d_sf || !d_row || !d_col) return fail(H3D_EARG, "null device input");
  if ((!scaled_out && !d_scaled_out) || !flag_out) return fail(H3D_EARG, "null output");
  ScaleDispArgs a{};
  for (int c = 0; c < C; ++c) {
    int cnt = 0;
    for (int k = 0; k < R; ++k)
      if (design[k * C + c]) {
        a.cond_mask[c] |= 1u << k;
        ++cnt;
      }
    // np.sum(design, axis=0): a condition without replicates divides by 0
    a.count[c] = (double)cnt;
  }
  a.C = C;
  a.mean_thresh = mean_thresh;
  a.dist_min = dist_thresh_min;
  HostCall hc(ctx);  // (device inputs: only the two results are staged)
  hipStream_t s = ctx->stream;
  double* d_scaled = d_scaled_out ? d_scaled_out : hc.out<double>("sd_scaled", (size_t)n * R);
  uint8_t* d_flag = d_flag_out ? d_flag_out : hc.out<uint8_t>("sd_flag", (size_t)n);
  if (int rc = hc.ready("scale / disp scratch")) return rc;
  hipLaunchKernelGGL(k_scale_disp, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, d_balanced,
                     d_sf, sf_per_rep, d_row, d_col, n, R, a, d_scaled, d_flag);
  HIP_TRY(hipGetLastError());
  hc.back(scaled_out, d_scaled, (size_t)n * R);
  // (the flags through the pinned landing zone: see h2d_pinned)
  return hc.finish(flag_out, d_flag, (size_t)n);
}

int h3d_table_gather_dev(h3d_ctx* ctx, const double* d_tables, int D, int C,
                         const int32_t* d_dist, int64_t n, double* d_out) {
  if (!ctx || !d_tables || D < 1 || C < 1 || C > kMaxConds || n < 0)
    return fail(H3D_EARG, "null argument / D / C / n");
  // a pending device smoother is settled first (a degenerate fit is redone
  // on the host into the same buffer)
  if (int rc = h3d_disp_tables_wait(ctx)) return rc;
  if (n == 0) return 0;
  if (!d_dist || !d_out) return fail(H3D_EARG, "null device buffer");
  HIP_TRY(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_table_gather, dim3(grid_for(ctx, n)), dim3(kBlock), 0, ctx->stream,
                     d_tables, D, C, d_dist, n, d_out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}

}  // extern "C"

namespace {

// The size factors of every norm (util/scaling.py). size_factors_impl reads
// as its stages; what they share travels in an SfCall.
struct SfCall {
  h3d_ctx* ctx;  // the request (balanced on the host or on the device)
  const double *balanced, *d_balanced;
  const int32_t* dist;
  int64_t n;
  int R, norm, n_bins;
  double *sf_out, *d_sf_out;
  hipStream_t s = nullptr;
  HostCall* hc = nullptr;  // stages balanced (from the host) and sf_out
  // per-distance factors (n, R), else one set (R,); by median of ratios, else
  // by simple scaling
  bool conditional = false, mor = false;
  const double* bal = nullptr;  // balanced on the device
  // the pixels in (stable) distance order: sorted position k is pixel
  // perm[k] at distance dist_s[k] in bin bin[k]; idx = 0 .. n - 1
  int32_t *d_dist = nullptr, *d_dist_s = nullptr, *d_idx = nullptr, *d_perm = nullptr,
          *d_bin = nullptr;
  int nb = 1;
  int64_t* d_bstart = nullptr;  // nb + 1 bin bounds (sorted positions)
  std::vector<int64_t> bstart;
  double *d_spb = nullptr, *d_dpb = nullptr;
  std::vector<double> spb;  // per-bin factors (nb, R)
  double* d_sf = nullptr;   // per-pixel factors (n, R)
};

// the (R,) factors of the global norms into the caller's device copy too
int sf_global_out(SfCall& c) {
  if (c.d_sf_out) {
    HIP_TRY(hipSetDevice(c.ctx->device));
    HIP_TRY(hipMemcpyAsync(c.d_sf_out, c.sf_out, c.R * 8, hipMemcpyHostToDevice,
                           c.ctx->stream));
    HIP_TRY(hipStreamSynchronize(c.ctx->stream));
  }
  return 0;
}

// Stage: the argument checks and the results that need no data pass
// (*done: the call is complete).
int sf_check_and_trivial(SfCall& c, bool* done) {
  const int R = c.R, norm = c.norm;
  c.conditional = norm == H3D_NORM_CONDITIONAL_MOR || norm == H3D_NORM_CONDITIONAL_SCALING;
  c.mor = norm == H3D_NORM_CONDITIONAL_MOR || norm == H3D_NORM_MEDIAN_OF_RATIOS;
  // sf_out may be NULL for the conditional norms when d_sf_out is given (the
  // caller fetches the (n, R) factors in the background)
  if (!c.ctx || (c.n > 0 && !c.balanced && !c.d_balanced) ||
      (!c.sf_out && !(c.conditional && c.d_sf_out)))
    return fail(H3D_EARG, "null argument");
  if (R < 1 || R > kMaxReps || c.n_bins < 0)
    return fail(H3D_EARG, "R=%d n_bins=%d", R, c.n_bins);
  if (norm < H3D_NORM_CONDITIONAL_MOR || norm > H3D_NORM_NO_SCALING)
    return fail(H3D_EARG, "norm %d", norm);
  *done = true;
  if (norm == H3D_NORM_NO_SCALING) {  // scaling.py:24: ones(R), no data pass
    for (int r = 0; r < R; ++r) c.sf_out[r] = 1.0;
    return sf_global_out(c);
  }
  if (c.conditional && c.n > 0 && !c.dist) return fail(H3D_EARG, "null dist");
  if (c.n == 0) {
    if (c.conditional) return 0;
    for (int r = 0; r < R; ++r) c.sf_out[r] = NAN;  // median / sums of nothing
    return sf_global_out(c);
  }
  if (c.n >= ((int64_t)1 << 31) / R) return fail(H3D_EARG, "n too large");
  *done = false;
  return 0;
}

// Stage: the distance order and the bins over it -- one bin holding every
// pixel in the original order (the global norms), n_bins equal-count bins, or
// one bin per distance -- and the bins' bounds, on the host too.
int sf_order_and_bins(SfCall& c) {
  h3d_ctx* ctx = c.ctx;
  const int64_t n = c.n;
  const int R = c.R;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = c.s = ctx->stream;
  Scratch& sc = c.hc->sc;
  double* d_bal = c.hc->in("sf_bal", c.balanced, n * R);
  c.d_dist = sc.get<int32_t>("sf_dist", n);
  c.d_dist_s = sc.get<int32_t>("sf_dist_s", n);
  c.d_idx = sc.get<int32_t>("sf_idx", n);
  c.d_perm = sc.get<int32_t>("sf_perm", n);
  c.d_bin = sc.get<int32_t>("sf_bin", n);
  c.d_sf = sc.get<double>("sf_out", n * R);
  if (int rc = c.hc->ready("size factor scratch")) return rc;
  c.bal = c.d_balanced ? c.d_balanced : d_bal;
  launch_iota(ctx, s, c.d_idx, n);
  if (!c.conditional) {
    HIP_TRY(hipMemcpyAsync(c.d_perm, c.d_idx, n * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemsetAsync(c.d_bin, 0, n * 4, s));
  } else {
    if (int rc = h2d_pinned(ctx, c.d_dist, c.dist, n * 4, s)) return rc;
    // stable sort by distance (the pinned equal_bin tie order)
    if (int rc = cub_call(ctx, "cub_tmp_sf", [&](void* tmp, size_t& bytes) {
          return sort_pairs(tmp, bytes, c.d_dist, c.d_dist_s, c.d_idx, c.d_perm, (int)n, 0, 31, s);
        }))
      return rc;
    if (c.n_bins > 0) {
      c.nb = c.n_bins;
      hipLaunchKernelGGL(k_equal_bin, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, n, c.n_bins,
                         c.d_bin);
    } else {
      int32_t* d_head = sc.get<int32_t>("sf_head", n);
      if (!sc.ok) return fail(H3D_ENOMEM, "heads");
      hipLaunchKernelGGL(k_dist_heads, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, c.d_dist_s,
                         n, d_head);
      if (int rc = cub_call(ctx, "cub_tmp_s", [&](void* tmp, size_t& bytes) {
            return inclusive_sum(tmp, bytes, d_head, c.d_bin, (int)n, s);
          }))
        return rc;
      hipLaunchKernelGGL(k_minus_one, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, c.d_bin, n);
      int32_t last = 0;
      if (int rc = d2h_sync(ctx, &last, c.d_bin + n - 1, 4, s)) return rc;
      c.nb = last + 1;
    }
  }
  const int nb = c.nb;
  c.d_bstart = sc.get<int64_t>("sf_bstart", (size_t)(nb + 1));
  c.d_spb = sc.get<double>("sf_spb", (size_t)nb * R);
  c.d_dpb = sc.get<double>("sf_dpb", (size_t)nb);
  if (!sc.ok) return fail(H3D_ENOMEM, "bins");
  hipLaunchKernelGGL(k_bin_bounds, dim3((nb + 1 + 255) / 256), dim3(256), 0, s, c.d_bin, n, nb,
                     c.d_bstart);
  c.bstart.resize(nb + 1);
  c.spb.resize((size_t)nb * R);
  return d2h_sync(ctx, c.bstart.data(), c.d_bstart, (nb + 1) * 8, s);
}

// Stage: per-bin factors by median_of_ratios (scaling.py:27-47): per
// replicate the median over the bin's all-positive rows of data / gmean(row);
// a segmented sort of the ratios per (replicate, bin), invalid rows keyed
// +inf past the valid ones
int sf_bin_factors_mor(SfCall& c) {
  h3d_ctx* ctx = c.ctx;
  hipStream_t s = c.s;
  const int64_t n = c.n;
  const int R = c.R, nb = c.nb;
  Scratch sc{ctx};
  int32_t* d_valid = sc.get<int32_t>("sf_valid", (size_t)nb);
  double* d_keys = sc.get<double>("sf_keys", n * R);
  double* d_keys_s = sc.get<double>("sf_keys_s", n * R);
  int64_t* d_segb = sc.get<int64_t>("sf_segb", (size_t)nb * R);
  int64_t* d_sege = sc.get<int64_t>("sf_sege", (size_t)nb * R);
  if (!sc.ok) return fail(H3D_ENOMEM, "median scratch");
  HIP_TRY(hipMemsetAsync(d_valid, 0, (size_t)nb * 4, s));
  hipLaunchKernelGGL(k_mor_keys, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, c.bal, c.d_perm, n,
                     R, c.d_bin, d_keys, d_valid);
  std::vector<int64_t> segb((size_t)nb * R), sege((size_t)nb * R);
  for (int r = 0; r < R; ++r)
    for (int b = 0; b < nb; ++b) {
      segb[(size_t)r * nb + b] = (int64_t)r * n + c.bstart[b];
      sege[(size_t)r * nb + b] = (int64_t)r * n + c.bstart[b + 1];
    }
  if (int rc = h2d_pinned(ctx, d_segb, segb.data(), segb.size() * 8, s)) return rc;
  if (int rc = h2d_pinned(ctx, d_sege, sege.data(), sege.size() * 8, s)) return rc;
  if (int rc = cub_call(ctx, "cub_tmp_seg", [&](void* tmp, size_t& bytes) {
        return segmented_sort_keys(tmp, bytes, d_keys, d_keys_s, (int)(n * R), nb * R, d_segb,
                                   d_sege, 0, 64, s);
      }))
    return rc;
  hipLaunchKernelGGL(k_mor_median, dim3((nb * R + 255) / 256), dim3(256), 0, s, d_keys_s,
                     c.d_bstart, d_valid, nb, n, R, c.d_spb);
  return d2h_sync(ctx, c.spb.data(), c.d_spb, (size_t)nb * R * 8, s);
}

// Stage: per-bin factors by simple_scaling (scaling.py:50-65): column sums
// over the bin's rows in their original order (members grouped by bin: a
// stable sort of the original-order bin labels), then s / gmean(s,
// pseudocount 1)
int sf_bin_factors_scaling(SfCall& c) {
  h3d_ctx* ctx = c.ctx;
  hipStream_t s = c.s;
  const int64_t n = c.n;
  const int R = c.R, nb = c.nb;
  int32_t* members = c.d_idx;
  if (c.conditional) {
    Scratch sc{ctx};
    int32_t* d_bin_orig = sc.get<int32_t>("sf_bin_orig", n);
    int32_t* d_bin_orig_s = sc.get<int32_t>("sf_bin_orig_s", n);
    int32_t* d_iota = sc.get<int32_t>("sf_iota2", n);
    members = sc.get<int32_t>("sf_members", n);
    if (!sc.ok) return fail(H3D_ENOMEM, "member scratch");
    hipLaunchKernelGGL(k_scatter_bin, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, c.d_perm,
                       c.d_bin, n, d_bin_orig);
    launch_iota(ctx, s, d_iota, n);
    int end_bit = 1;
    while (end_bit < 31 && (1 << end_bit) <= nb) ++end_bit;
    if (int rc = cub_call(ctx, "cub_tmp_sf", [&](void* tmp, size_t& bytes) {
          return sort_pairs(tmp, bytes, d_bin_orig, d_bin_orig_s, d_iota, members, (int)n, 0,
                            end_bit, s);
        }))
      return rc;
  }
  hipLaunchKernelGGL(k_bin_colsum, dim3((nb * R + 255) / 256), dim3(256), 0, s, c.bal, members,
                     c.d_bstart, nb, R, c.d_spb);
  std::vector<double> colsum((size_t)nb * R);
  if (int rc = d2h_sync(ctx, colsum.data(), c.d_spb, (size_t)nb * R * 8, s)) return rc;
  for (int b = 0; b < nb; ++b) {
    const double* cs = &colsum[(size_t)b * R];
    // gmean is exp(nanmean(log(s + 1))) - 1: numpy's nanmean sums the logs
    // with every NaN replaced by 0 and divides by the count of the others
    // (0 / 0 = NaN when there is none), so a replicate whose column sum is
    // NaN (a NaN-bias bin without a count: balanced 0 / NaN) gets a NaN
    // factor and leaves the other replicates' factors finite
    double lg[kMaxReps];
    int cnt = 0;
    for (int r = 0; r < R; ++r) {
      lg[r] = std::log(cs[r] + 1);
      if (std::isnan(lg[r]))
        lg[r] = 0.0;
      else
        ++cnt;
    }
    const double gm = std::exp(np_sum<kMaxReps>(lg, R) / cnt) - 1;
    for (int r = 0; r < R; ++r) c.spb[(size_t)b * R + r] = cs[r] / gm;
  }
  return 0;
}

// Stage (the conditional norms): per-pixel factors (scaling.py:88-105) --
// interpolated between the bins' mean distances, or each pixel its
// distance's own -- and the copies to the caller.
int sf_pixel_factors(SfCall& c) {
  h3d_ctx* ctx = c.ctx;
  hipStream_t s = c.s;
  const int64_t n = c.n;
  const int R = c.R, nb = c.nb;
  std::vector<double> xp, yp;  // (alive until the call's last synchronisation)
  if (c.n_bins > 0) {
    hipLaunchKernelGGL(k_bin_dist_sum, dim3(nb), dim3(256), 0, s, c.d_dist_s, c.d_bstart, nb,
                       c.d_dpb);
    std::vector<double> dpb(nb);
    HIP_TRY(hipMemcpyAsync(dpb.data(), c.d_dpb, nb * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // np.unique(bins): only non-empty bins take part in the interpolation
    for (int b = 0; b < nb; ++b)
      if (c.bstart[b + 1] > c.bstart[b]) {
        xp.push_back(dpb[b]);
        for (int r = 0; r < R; ++r) yp.push_back(c.spb[(size_t)b * R + r]);
      }
    const int m = (int)xp.size();
    if (m < 2) return fail(H3D_EARG, "fewer than two distance bins to interpolate");
    Scratch sc{ctx};
    double* d_xp = sc.get<double>("sf_xp", m);
    double* d_yp = sc.get<double>("sf_yp", (size_t)m * R);
    if (!sc.ok) return fail(H3D_ENOMEM, "interp");
    c.hc->up(d_xp, xp.data(), (size_t)m);
    c.hc->up(d_yp, yp.data(), (size_t)m * R);
    hipLaunchKernelGGL(k_sf_interp, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, c.d_dist, n, R,
                       d_xp, d_yp, m, c.d_sf);
  } else {
    c.hc->up(c.d_spb, c.spb.data(), (size_t)nb * R);
    hipLaunchKernelGGL(k_sf_exact, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, c.d_perm, c.d_bin,
                       n, R, c.d_spb, c.d_sf);
  }
  if (c.d_sf_out)
    HIP_TRY(hipMemcpyAsync(c.d_sf_out, c.d_sf, n * R * 8, hipMemcpyDeviceToDevice, s));
  c.hc->back(c.sf_out, c.d_sf, (size_t)n * R);
  return c.hc->finish();
}

int size_factors_impl(h3d_ctx* ctx, const double* balanced, const double* d_balanced,
                      const int32_t* dist, int64_t n, int R, int norm, int n_bins,
                      double* sf_out, double* d_sf_out) {
  SfCall c{ctx, balanced, d_balanced, dist, n, R, norm, n_bins, sf_out, d_sf_out};
  bool done = false;
  if (int rc = sf_check_and_trivial(c, &done)) return rc;
  if (done) return 0;
  HostCall hc(ctx);
  c.hc = &hc;
  if (int rc = sf_order_and_bins(c)) return rc;
  if (int rc = c.mor ? sf_bin_factors_mor(c) : sf_bin_factors_scaling(c)) return rc;
  if (c.conditional) return sf_pixel_factors(c);
  // a global norm: the one bin's factors are the result
  std::memcpy(sf_out, c.spb.data(), R * 8);
  return sf_global_out(c);
}

}  // namespace

extern "C" {

int h3d_size_factors(h3d_ctx* ctx, const double* balanced, const int32_t* dist,
                     int64_t n, int R, int norm, int n_bins, double* sf_out) {
  return size_factors_impl(ctx, balanced, nullptr, dist, n, R, norm, n_bins, sf_out,
                           nullptr);
}

int h3d_size_factors_dev(h3d_ctx* ctx, const double* d_balanced, const int32_t* dist,
                         int64_t n, int R, int norm, int n_bins, double* sf_out,
                         double* d_sf_out) {
  if (n > 0 && !d_balanced) return fail(H3D_EARG, "null device balanced");
  return size_factors_impl(ctx, nullptr, d_balanced, dist, n, R, norm, n_bins, sf_out,
                           d_sf_out);
}

int h3d_size_factors_cmor(h3d_ctx* ctx, const double* balanced,
                          const int32_t* dist, int64_t n, int R, int n_bins,
                          double* sf_out) {
  return h3d_size_factors(ctx, balanced, dist, n, R, H3D_NORM_CONDITIONAL_MOR, n_bins,
                          sf_out);
}

}  // extern "C"
