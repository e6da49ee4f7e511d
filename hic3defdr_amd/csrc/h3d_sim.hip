// libh3d.so: negative-binomial sampling for simulate(gpu=True) (h3d_nb_sample,
// h3d_simulate_dev; reference simulation.py:187-203). The arithmetic is
// h3d_sample.h's nb_draw on the counter-based stream of h3d_philox.h; these
// kernels only form a pixel's uniforms and mean, call it and store the count.
//
// One lane per pixel in the CALLER's pixel order (the union's (row, col)
// order: neighbouring lanes share a distance and have similar means, which
// keeps the lanes of a wave on one Poisson path most of the time; no sort).
// The fused kernel loops over the J replicates of its pixel and writes
// replicate-major (J, n) planes, so consecutive lanes store consecutive words.
#include <hip/hip_runtime.h>

#include "h3d.h"
#include "h3d_ctx.h"
#include "h3d_errors.h"
#include "h3d_model.h"
#include "h3d_philox.h"
#include "h3d_sample.h"

using namespace h3d;
using namespace h3dint;
using h3derr::fail;

namespace {

constexpr int kBlock = kLaunchBlock;

// OR of a wave's status words, then one atomic per wave (every lane of the
// wave reaches this: the grid-stride loops have reconverged)
__device__ inline void wave_flags(int fl, int* __restrict__ flags) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) fl |= __shfl_xor(fl, off, 64);
  if (fl && (threadIdx.x & 63) == 0) atomicOr(flags, fl);
}

// one replicate from the caller's bm and disp (h3d_nb_sample)
__global__ __launch_bounds__(kBlock) void k_nb_sample_one(
    const double* __restrict__ bm, const double* __restrict__ disp, int64_t n,
    uint64_t seed, uint32_t stream, uint32_t rep, int64_t pixel0,
    int32_t* __restrict__ counts, double* __restrict__ lambda, int* __restrict__ flags) {
  int fl = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    double u1, u2, lam;
    sim_uniforms(seed, stream, rep, (uint64_t)(pixel0 + i), &u1, &u2);
    counts[i] = nb_draw(bm[i], disp[i], u1, u2, &lam, &fl);
    if (lambda) lambda[i] = lam;
  }
  wave_flags(fl, flags);
}

// every replicate of a chromosome (h3d_simulate_dev)
__global__ __launch_bounds__(kBlock) void k_nb_sample(
    const int32_t* __restrict__ row, const int32_t* __restrict__ col,
    const double* __restrict__ meanA, const double* __restrict__ meanB,
    const double* __restrict__ bias, const double* __restrict__ sf, int sf_rows,
    const double* __restrict__ table, int D, int64_t n, int J, int n_bins, uint64_t seed,
    uint32_t stream, int64_t pixel0, int32_t* __restrict__ counts, int* __restrict__ flags) {
  int fl = 0;
  const int half = J / 2;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int r = row[i], c = col[i];
    const int64_t dist = (int64_t)c - r;
    const bool ok = r >= 0 && r < n_bins && c >= 0 && c < n_bins && dist >= 0 && dist < D;
    if (!ok) fl |= kFlagBadInput;
    const double disp = ok ? table[dist] : 1.0;
    const double mA = meanA[i], mB = meanB[i];
    const double* __restrict__ b_row = bias + (int64_t)(ok ? r : 0) * J;
    const double* __restrict__ b_col = bias + (int64_t)(ok ? c : 0) * J;
    const double* __restrict__ sfr = sf + (sf_rows == 1 || !ok ? 0 : dist * J);
    for (int j = 0; j < J; ++j) {
      int32_t k = -1;
      if (ok) {
        const double bm = sim_bm(j < half ? mA : mB, b_row[j], b_col[j], sfr[j]);
        double u1, u2, lam;
        sim_uniforms(seed, stream, (uint32_t)j, (uint64_t)(pixel0 + i), &u1, &u2);
        k = nb_draw(bm, disp, u1, u2, &lam, &fl);
      }
      counts[(int64_t)j * n + i] = k;
    }
  }
  wave_flags(fl, flags);
}

// the status word of a launch, read after the stream has drained
int read_flags(h3d_ctx* ctx, const int* d_fl, int* flags) {
  int fl = 0;
  if (int rc = d2h_sync(ctx, &fl, d_fl, 4, ctx->stream)) return rc;
  if (flags) *flags = fl;
  return 0;
}

// 0 = run it, 1 = nothing to do, < 0 = an error
int sample_args(h3d_ctx* ctx, int64_t n, int64_t pixel0, int* flags, bool have_bufs,
                bool host_bufs) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  if (flags) *flags = 0;
  if (n < 0) return fail(H3D_EARG, "n < 0");
  if (pixel0 < 0 || pixel0 > INT64_MAX - n) return fail(H3D_EARG, "pixel0 < 0 or pixel0 + n overflows");
  if (n == 0) return 1;
  if (!have_bufs) return fail(H3D_EARG, host_bufs ? "null buffer" : "null device buffer");
  return 0;
}

int* flag_word(h3d_ctx* ctx) {
  Scratch sc{ctx};
  int* d_fl = sc.get<int>("nb_flags", 1);
  if (d_fl && hipMemsetAsync(d_fl, 0, 4, ctx->stream) != hipSuccess) return nullptr;
  return d_fl;
}

// nb_sample over device buffers (arguments checked); drains the stream
int sample_run(h3d_ctx* ctx, const double* d_bm, const double* d_disp, int64_t n,
               uint64_t seed, uint32_t stream, uint32_t rep, int64_t pixel0,
               int32_t* d_counts, double* d_lambda, int* flags) {
  HIP_TRY(hipSetDevice(ctx->device));
  int* d_fl = flag_word(ctx);
  if (!d_fl) return fail(H3D_ENOMEM, "nb_sample flags");
  {
    ProfScope ps(ctx, "nb_sample_one", n);
    hipLaunchKernelGGL(k_nb_sample_one, dim3(grid_for(ctx, n, 16)), dim3(kBlock), 0,
                       ctx->stream, d_bm, d_disp, n, seed, stream, rep, pixel0, d_counts,
                       d_lambda, d_fl);
  }
  HIP_TRY(hipGetLastError());
  return read_flags(ctx, d_fl, flags);
}

}  // namespace

extern "C" {

int h3d_nb_sample_dev(h3d_ctx* ctx, const double* d_bm, const double* d_disp, int64_t n,
                      uint64_t seed, uint32_t stream, uint32_t rep, int64_t pixel0,
                      int32_t* d_counts, double* d_lambda, int* flags) {
  if (int rc = sample_args(ctx, n, pixel0, flags, d_bm && d_disp && d_counts, false))
    return rc < 0 ? rc : 0;
  return sample_run(ctx, d_bm, d_disp, n, seed, stream, rep, pixel0, d_counts, d_lambda,
                    flags);
}

int h3d_nb_sample(h3d_ctx* ctx, const double* bm, const double* disp, int64_t n,
                  uint64_t seed, uint32_t stream, uint32_t rep, int64_t pixel0,
                  int32_t* counts, double* lambda, int* flags) {
  if (int rc = sample_args(ctx, n, pixel0, flags, bm && disp && counts, true))
    return rc < 0 ? rc : 0;
  HostCall hc(ctx);
  double* d_bm = hc.in("sim_bm", bm, n);
  double* d_disp = hc.in("sim_disp", disp, n);
  int32_t* d_k = hc.out<int32_t>("sim_counts", n);
  double* d_lam = lambda ? hc.out<double>("sim_lambda", n) : nullptr;
  if (int rc = hc.ready("nb_sample buffers")) return rc;
  if (int rc = sample_run(ctx, d_bm, d_disp, n, seed, stream, rep, pixel0, d_k, d_lam, flags))
    return rc;
  hc.back(counts, d_k, n);
  hc.back(lambda, d_lam, n);
  return hc.finish();
}

int h3d_simulate_dev(h3d_ctx* ctx, const int32_t* d_row, const int32_t* d_col,
                     const double* d_meanA, const double* d_meanB, const double* d_bias,
                     const double* d_sf, int sf_rows, const double* d_table, int D, int64_t n,
                     int J, int n_bins, uint64_t seed, uint32_t stream, int64_t pixel0,
                     int32_t* d_counts, int* flags) {
  if (J < 1 || J > kMaxReps) return fail(H3D_EARG, "J=%d outside [1, %d]", J, kMaxReps);
  if (D < 1 || n_bins < 1) return fail(H3D_EARG, "D=%d, n_bins=%d: both >= 1", D, n_bins);
  if (sf_rows != 1 && sf_rows != D)
    return fail(H3D_EARG, "sf_rows=%d: 1 or D=%d", sf_rows, D);
  if (int rc = sample_args(ctx, n, pixel0, flags,
                           d_row && d_col && d_meanA && d_meanB && d_bias && d_sf &&
                               d_table && d_counts,
                           false))
    return rc < 0 ? rc : 0;
  HIP_TRY(hipSetDevice(ctx->device));
  int* d_fl = flag_word(ctx);
  if (!d_fl) return fail(H3D_ENOMEM, "simulate flags");
  {
    ProfScope ps(ctx, "nb_sample", n * J);
    hipLaunchKernelGGL(k_nb_sample, dim3(grid_for(ctx, n, 16)), dim3(kBlock), 0, ctx->stream,
                       d_row, d_col, d_meanA, d_meanB, d_bias, d_sf, sf_rows, d_table, D, n, J,
                       n_bins, seed, stream, pixel0, d_counts, d_fl);
  }
  HIP_TRY(hipGetLastError());
  return read_flags(ctx, d_fl, flags);
}

}  // extern "C"
