// k_lrt8: the per-pixel LRT (lrt.py:7-50) for wide designs (R > 8, the
// R = 18 / C = 3 shape of BASELINE cfg4), one pixel per GROUP OF 8 LANES.
//
// k_lrt holds a pixel's R replicates in one lane's registers: past R = 8 that
// is > 256 VGPRs (x, f, a rows + the unrolled fits) and the compiler spills
// to scratch (measured at M = 32: 1 KiB scratch per lane, 1 wave/SIMD, 26.9 ms
// per cfg4 lrt). Here lane j of a group owns replicates j, j + 8, j + 16, ...
// (M / 8 slots), so the row reads are 8 contiguous values per group and the
// per-lane state is M / 8 slots.
//
// Sums over replicates go through a 3-level xor butterfly inside the group:
// every lane of the group ends with the same value (IEEE addition commutes),
// so the Newton iterations of the group stay in lockstep and the group exits
// its loops together.
#pragma once

#include "h3d_lrt_kernel.h"

namespace h3d {

constexpr int kGroup = 8;

__device__ inline double gsum8(double v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}
__device__ inline int gor8(int v) {
  v |= __shfl_xor(v, 1, 64);
  v |= __shfl_xor(v, 2, 64);
  v |= __shfl_xor(v, 4, 64);
  return v;
}

// fit_mu (h3d_model.h) over the group: the same bracketed Halley steps on
// g(theta) = mu S(mu) from sum(x) / sum(b), sums by butterfly (any fixed
// order; the root is unique and the solve runs to full precision). `slots` = this lane's bits of
// the fit's replicate mask (bit s: replicate lane + 8 s).
template <int J>
__device__ double fit_mu_g8(const int32_t* x, const double* b, const double* a,
                            unsigned slots, int* status) {
#pragma clang fp contract(fast)  // as fit_mu (h3d_model.h)
  double sx = 0.0, sb = 0.0;
  int bad = 0;
#pragma unroll
  for (int s = 0; s < J; ++s)
    if ((slots >> s) & 1u) {
      bad |= (!(a[s] > 0.0) || !(b[s] > 0.0) || is_inf(a[s]) || is_inf(b[s]) ||
              !(x[s] >= 0))
                 ? 1
                 : 0;
      sx += (double)x[s];
      sb += b[s];
    }
  bad = gor8(bad);
  sx = gsum8(sx);
  sb = gsum8(sb);
  if (bad) {
    *status |= kFlagBadInput;
    return NAN;
  }
  if (!(sx > 0.0)) {
    *status |= kFlagNoRoot;
    return NAN;
  }
  const double q0 = div_fast(sx, sb);
  double th = log_fast_checked(q0);
  double lo = -INFINITY, hi = INFINITY;
  for (int it = 0; it < 200; ++it) {
    const double mu = (it == 0) ? q0 : exp_fast(th);  // as fit_mu
    double g = 0.0, gp = 0.0, gpp = 0.0;
#pragma unroll
    for (int s = 0; s < J; ++s)
      if ((slots >> s) & 1u) {
        const double mb = mu * b[s];
        const double am = a[s] * mb;
        const double den = recip_fast(1.0 + am);
        g += ((double)x[s] - mb) * den;
        const double t = mb * (1.0 + a[s] * (double)x[s]) * den * den;
        gp -= t;
        gpp -= t * (1.0 - 2.0 * am * den);
      }
    g = gsum8(g);
    gp = gsum8(gp);
    gpp = gsum8(gpp);
    if (g > 0.0)
      lo = th;
    else if (g < 0.0)
      hi = th;
    else
      return mu;
    const double nt = g * recip_fast(gp);
    const double hf = 1.0 - 0.5 * nt * gpp * recip_fast(gp);
    const double dn = (hf >= 0.5 && hf <= 2.0) ? nt * recip_fast(hf) : nt;
    if (fabs(dn) <= 1e-5 * fmax(1.0, fabs(th)))  // as fit_mu
      return (fabs(dn) <= 1e-4)
                 ? mu + mu * (-dn * (1.0 + -dn * (0.5 + -dn * (1.0 / 6.0))))
                 : exp_fast(th - dn);
    double tn = th - dn;
    if (!(tn > lo && tn < hi)) {
      if (is_inf(lo))
        tn = hi - 2.0;
      else if (is_inf(hi))
        tn = lo + 2.0;
      else
        tn = 0.5 * (lo + hi);
    }
    const double step = fabs(tn - th);
    th = tn;
    if (step <= 1e-15 * fmax(1.0, fabs(th))) return exp_fast(th);
    if (!is_inf(lo) && !is_inf(hi) && (hi - lo) <= 4e-16 * fmax(1.0, fabs(th)))
      return exp_fast(th);
  }
  *status |= kFlagNoConv;
  return exp_fast(th);
}

// M = 16 / 24 / 32 (R <= M), CM >= C. Same arguments and outputs as k_lrt.
template <int M, int CM, bool TAB = false>
// TAB: the pipeline's call (refit, the (D, C) table by dist, no wide
// dispersions) as compile-time facts, as k_lrt.
// 2 waves per SIMD (<= 256 registers). (With the table log in its logpmf
// rows the M = 32 instantiation grew into AGPRs at 1 wave -- cfg4 lrt 22.7
// -> 31.0 ms, r03i --, while the rows still carried the cancelling prefix;
// without it the rows take the table log from LDS, as k_lrt.)
__global__ __launch_bounds__(kLrtBlock, 2) void k_lrt8(
    const int32_t* __restrict__ raw, const double* __restrict__ f,
    const int32_t* __restrict__ dist, const double* __restrict__ table,
    int64_t n, int R, int C, int D, const int32_t* __restrict__ cond_of_rep,
    int refit, double* __restrict__ p, double* __restrict__ llr,
    double* __restrict__ mu0, double* __restrict__ mu1,
    double* __restrict__ disp_out, int* __restrict__ flags, int wide) {
  constexpr int J = M / kGroup;
  const int lane = threadIdx.x & (kGroup - 1);
  const int base = (threadIdx.x & 63) & ~(kGroup - 1);  // group's first lane
  __shared__ LogTab s_tab[kLogTabLen];  // the rows' log table, as k_lrt
  for (int t = threadIdx.x; t < kLogTabLen; t += blockDim.x) s_tab[t] = kLogTab[t];
  __syncthreads();
  int cnd[J];
#pragma unroll
  for (int s = 0; s < J; ++s) {
    const int k = lane + kGroup * s;
    cnd[s] = (k < R) ? cond_of_rep[k] : -1;
  }
  int fl_all = 0;
  if constexpr (TAB) {
    refit = 1;
    wide = 0;
  }
  const int64_t groups = (int64_t)gridDim.x * (blockDim.x / kGroup);
  for (int64_t i = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kGroup; i < n;
       i += groups) {
    const int d = (TAB || dist) ? dist[i] : 0;
    const double* trow = (TAB || dist) ? table + (int64_t)d * C
                                       : table + i * (wide ? R : C);
    const bool inb = (TAB || dist) ? (d >= 0 && d < D) : true;
    double dc[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) dc[c] = (c < C && inb && !wide) ? trow[c] : NAN;
    int32_t x[J];
    double fv[J], a[J];
#pragma unroll
    for (int s = 0; s < J; ++s) {
      const int k = lane + kGroup * s;
      if (k < R) {
        x[s] = raw[i * R + k];
        fv[s] = f[i * R + k];
        double ak = 0.0;
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (c == cnd[s]) ak = dc[c];
        a[s] = wide ? trow[k] : ak;
      } else {
        x[s] = 0;
        fv[s] = 1.0;
        a[s] = 1.0;
      }
    }
    int st = 0;
    double m0 = 0.0, m1[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) m1[c] = 0.0;
    // fit 0 the null, fit t = c + 1 condition c (lrt_pixel's loop)
#pragma unroll 1
    for (int t = 0; t <= C; ++t) {
      unsigned slots = 0u;
#pragma unroll
      for (int s = 0; s < J; ++s)
        if (lane + kGroup * s < R && (t == 0 || cnd[s] == t - 1)) slots |= 1u << s;
      double mu;
      if (refit) {
        mu = fit_mu_g8<J>(x, fv, a, slots, &st);
      } else {
        // np.mean(raw / f) of the fit's replicates in replicate order: every
        // lane walks the compacted row (values fetched from their lanes)
        double q[J];
#pragma unroll
        for (int s = 0; s < J; ++s) q[s] = (double)x[s] / fv[s];
        unsigned rows = 0u;  // replicate mask of the fit (R <= 32)
#pragma unroll
        for (int s = 0; s < J; ++s)
          if ((slots >> s) & 1u) rows |= 1u << (lane + kGroup * s);
        rows = (unsigned)gor8((int)rows);
        const int cnt = __popc(rows);
        NpSumStream acc(cnt);
        int j = 0;
#pragma unroll
        for (int k = 0; k < M; ++k)
          if ((rows >> k) & 1u) {
            const double v = __shfl(q[k / kGroup], base + k % kGroup, 64);
            acc.add_dyn(j++, v);
          }
        mu = acc.sum() / cnt;
      }
      if (t == 0) m0 = mu;
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c == t - 1) m1[c] = mu;
    }
    // llr as lrt_pixel forms it: per replicate x log(mu0 / mu1) - (r + x)
    // log((r + m0) / (r + m1)) (the logpmf rows' difference term by term),
    // one log per replicate and one per condition
    // (the logs through log_quot, as lrt_pixel)
    double lq[CM];
    bool near[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      near[c] = c < C && m0 >= 0.5 * m1[c] && m0 <= 2.0 * m1[c];
      lq[c] = (c < C) ? log_quot(m0, m1[c], m0 - m1[c], near[c], s_tab) : 0.0;
    }
    double part = 0.0;
#pragma unroll
    for (int s = 0; s < J; ++s) {
      if (lane + kGroup * s >= R) continue;
      double m1k = 0.0, l = 0.0;
      bool nr = false;
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c == cnd[s]) {
          m1k = m1[c];
          l = lq[c];
          nr = near[c];
        }
      const double xk = (double)x[s];
      const double r = 1.0 / a[s];
      const double lr = log_quot(r + m0 * fv[s], r + m1k * fv[s], (m0 - m1k) * fv[s],
                                 nr, s_tab);
      part += xk * l - (r + xk) * lr;
    }
    const double lv = gsum8(part);
    fl_all |= st;
    if (lane == 0) {
      // chi2 sf, df = C - 1: the closed forms of df = 1 / 2 (chi2_sf) without
      // the general code's dispatch where the design has 2 / 3 conditions
      const double x2 = -2 * lv;
      p[i] = (x2 != x2) ? NAN
             : (x2 <= 0.0) ? 1.0
             : (C == 3)    ? exp(-x2 / 2.0)
             : (C == 2)    ? erfc(sqrt(x2 / 2.0))
                           : chi2_sf_cold((double)(C - 1), x2);
      llr[i] = lv;
      mu0[i] = m0;
    }
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C && c == lane) {
        mu1[i * C + c] = m1[c];
        if (disp_out) disp_out[i * C + c] = dc[c];
      }
  }
  fl_all = gor8(fl_all);
  if (fl_all && lane == 0) atomicOr(flags, fl_all);
}

}  // namespace h3d
