// k_lrt: the per-pixel LRT (lrt.py:7-50), one pixel per lane. Included by
// h3d_lrt.hip, which launches it, and by h3d_lrt_group.h (k_lrt8, the wide
// designs).
//
// Layout in HBM: the inputs stay in the reference's pixel
// order, replicate-minor (AoS): raw (n, R) int32, f (n, R) f64, dist (n)
// int32 -> one lane per pixel reads its R contiguous values (16 B / 32 B
// vector loads for R = 4).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "h3d_model.h"

namespace h3d {

constexpr int kLrtBlock = 256;  // lanes per workgroup of k_lrt / k_lrt8

// Per-pixel LRT (lrt.py:7-50) in the reference pixel order; disp from the
// (D, C) table (analysis.py:218: disp = disp_fn(dist), evaluated per d).
// TAB: the pipeline's call -- refit, the (D, C) table read by dist, no wide
// dispersions -- as compile-time facts, so the kernel carries none of the
// other modes' code (their registers and the SGPR spills around their
// uniform branches); the runtime flags are then ignored.
#ifndef H3D_LRT_WAVES
#define H3D_LRT_WAVES 1
#endif
template <int M, int CM, bool TAB = false>
__global__ __launch_bounds__(kLrtBlock, TAB ? H3D_LRT_WAVES : 1) void k_lrt(
    const int32_t* __restrict__ raw, const double* __restrict__ f,
    const int32_t* __restrict__ dist, const double* __restrict__ table,
    int64_t n, int R, int C, int D, const int32_t* __restrict__ cond_of_rep,
    int refit, double* __restrict__ p, double* __restrict__ llr,
    double* __restrict__ mu0, double* __restrict__ mu1,
    double* __restrict__ disp_out, int* __restrict__ flags, int wide) {
  int cond[M];
#pragma unroll
  for (int k = 0; k < M; ++k) cond[k] = (k < R) ? cond_of_rep[k] : -1;
  // the logpmf rows' log table in LDS (16 lookups per pixel at R = 4, each
  // on its term's dependency chain)
  __shared__ LogTab s_tab[kLogTabLen];
  for (int t = threadIdx.x; t < kLogTabLen; t += blockDim.x) s_tab[t] = kLogTab[t];
  __syncthreads();
  int fl_all = 0;
  if constexpr (TAB) {
    refit = 1;
    wide = 0;
  }
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    // dist == nullptr: `table` holds per-pixel dispersions, (n, C) -- or,
    // with `wide`, per replicate (n, R): lrt.py's disp argument as given
    const int d = (TAB || dist) ? dist[i] : 0;
    const double* trow = (TAB || dist) ? table + (int64_t)d * C
                                       : table + i * (wide ? R : C);
    const bool inb = (TAB || dist) ? (d >= 0 && d < D) : true;
    double dc[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) dc[c] = (c < C && inb && !wide) ? trow[c] : NAN;
    // counts stay int32 in registers (converted exactly where used): the
    // M = 24 / 32 instantiations must not spill
    int32_t x[M];
    double fv[M], a[M];
#pragma unroll
    for (int k = 0; k < M; ++k) {
      if (k < R) {
        x[k] = raw[i * R + k];
        fv[k] = f[i * R + k];
        double ak = 0.0;
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (c == cond[k]) ak = dc[c];
        a[k] = wide ? trow[k] : ak;
      } else {
        x[k] = 0;
        fv[k] = 1.0;
        a[k] = 1.0;
      }
    }
    double pv, lv, m0, m1[CM];
    fl_all |= lrt_pixel<M, CM>(x, fv, a, cond, R, C, refit != 0, &pv, &lv, &m0,
                               m1, s_tab);
    p[i] = pv;
    llr[i] = lv;
    mu0[i] = m0;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) {
        mu1[i * C + c] = m1[c];
        if (disp_out) disp_out[i * C + c] = dc[c];
      }
  }
  if (fl_all) atomicOr(flags, fl_all);
}

}  // namespace h3d
