// libh3d.so: the scaled-NB operators (h3d_nb_*; reference util/scaled_nb.py:
// fit_mu_hat :71-183, equalize :186-214, q2qnbinom :217-275, logpmf :12-33) as
// kernels of their own. The arithmetic is h3d_model.h's -- fit_mu<M>,
// equalize_pixel<M>, q2q, logpmf, the functions k_disp_work and k_lrt fuse --
// unchanged; these kernels only load a pixel's row, call them and store what
// the fused kernels keep in registers.
//
// One lane per pixel in the CALLER's pixel order (no coherence sort as in
// estimate_disp), replicate-minor (n, R) rows as the LRT reads them, M in
// {2, 4, 8, 16, 32} slots chosen from R.
#include <hip/hip_runtime.h>

#include <cstring>

#include "h3d.h"
#include "h3d_ctx.h"
#include "h3d_errors.h"
#include "h3d_model.h"

using namespace h3d;
using namespace h3dint;
using h3derr::fail;

namespace {

constexpr int kBlock = kLaunchBlock;

// A lane's row of R values into M register slots (every index a compile-time
// constant). `vec` = values per load: the host passes 4 / 2 only when R is a
// multiple of it and the base pointer is aligned to the load, so that every
// row start is aligned too (16-byte loads for counts with R % 4 == 0 and for
// doubles with R % 2 == 0).
template <int M>
__device__ inline void load_row(const int32_t* __restrict__ p, int R, int vec,
                                int32_t* out) {
  if (M >= 4 && vec == 4) {
#pragma unroll
    for (int k = 0; k + 3 < M; k += 4) {
      int4 v = make_int4(0, 0, 0, 0);
      if (k < R) v = *reinterpret_cast<const int4*>(p + k);
      out[k] = v.x;
      out[k + 1] = v.y;
      out[k + 2] = v.z;
      out[k + 3] = v.w;
    }
  } else if (vec == 2) {
#pragma unroll
    for (int k = 0; k + 1 < M; k += 2) {
      int2 v = make_int2(0, 0);
      if (k < R) v = *reinterpret_cast<const int2*>(p + k);
      out[k] = v.x;
      out[k + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < M; ++k) out[k] = (k < R) ? p[k] : 0;
  }
}

template <int M>
__device__ inline void load_row(const double* __restrict__ p, int R, int vec,
                                double* out) {
  if (vec == 2) {
#pragma unroll
    for (int k = 0; k + 1 < M; k += 2) {
      double2 v = make_double2(1.0, 1.0);
      if (k < R) v = *reinterpret_cast<const double2*>(p + k);
      out[k] = v.x;
      out[k + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < M; ++k) out[k] = (k < R) ? p[k] : 1.0;
  }
}

// OR of a wave's status words, then one atomic per wave (every lane of the
// wave reaches this: the grid-stride loops above have reconverged)
__device__ inline void wave_flags(int fl, int* __restrict__ flags) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) fl |= __shfl_xor(fl, off, 64);
  if (fl && (threadIdx.x & 63) == 0) atomicOr(flags, fl);
}

// fit_mu_hat (scaled_nb.py:71-183): mu[i] = the MLE of pixel i. alpha is read
// at alpha[i * sa_px + k * sa_rep]: the reference's four broadcast forms
// (:110-127) -- scalar (0, 0), (R,) (0, 1), (n, 1) (1, 0), (n, R) (R, 1) --
// without a materialised (n, R) copy. A failed pixel's mean is NaN.
template <int M>
__global__ __launch_bounds__(kBlock) void k_nb_fit_mu(
    const int32_t* __restrict__ x, const double* __restrict__ b,
    const double* __restrict__ alpha, int64_t sa_px, int sa_rep, int64_t n, int R,
    int vx, int vd, double* __restrict__ mu, int* __restrict__ flags) {
  int fl = 0;
  const bool full = sa_rep == 1 && sa_px == R;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int32_t xs[M];
    double bs[M], as[M];
    load_row<M>(x + i * R, R, vx, xs);
    load_row<M>(b + i * R, R, vd, bs);
    if (full) {
      load_row<M>(alpha + i * R, R, vd, as);
    } else {
#pragma unroll
      for (int k = 0; k < M; ++k) as[k] = (k < R) ? alpha[i * sa_px + k * sa_rep] : 1.0;
    }
    mu[i] = fit_mu<M>(xs, bs, as, R, ~0u, &fl);
  }
  wave_flags(fl, flags);
}

// equalize (scaled_nb.py:186-214): pseudo (n, R) from counts x and factors f
// at a dispersion that is one scalar or one value per pixel (alpha_px). The
// row goes through equalize_pixel, so the clamp of mu_out carries from one
// replicate into the next as :209-213 does. mu_hat (optional): the pixel's
// fitted mean (a second fit_mu, only when asked for).
template <int M>
__global__ __launch_bounds__(kBlock) void k_nb_equalize(
    const int32_t* __restrict__ x, const double* __restrict__ f, double alpha,
    const double* __restrict__ alpha_px, int64_t n, int R, int vx, int vd,
    double* __restrict__ pseudo, double* __restrict__ mu_hat,
    int* __restrict__ flags) {
  __shared__ LogTab s_tab[kLogTabLen];
  for (int t = threadIdx.x; t < kLogTabLen; t += blockDim.x) s_tab[t] = kLogTab[t];
  __syncthreads();
  int fl = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int32_t xi[M];
    double xs[M], fs[M], ps[M];
    load_row<M>(x + i * R, R, vx, xi);
    load_row<M>(f + i * R, R, vd, fs);
#pragma unroll
    for (int k = 0; k < M; ++k) xs[k] = (double)xi[k];
    const double a = alpha_px ? alpha_px[i] : alpha;
    // (fit_mu's input check covers b and alpha; NaN out for such a pixel)
    fl |= equalize_pixel<M>(xs, fs, R, a, ps, s_tab);
    if (vd == 2) {
#pragma unroll
      for (int k = 0; k + 1 < M; k += 2)
        if (k < R)
          *reinterpret_cast<double2*>(pseudo + i * R + k) = make_double2(ps[k], ps[k + 1]);
    } else {
#pragma unroll
      for (int k = 0; k < M; ++k)
        if (k < R) pseudo[i * R + k] = ps[k];
    }
    if (mu_hat) {
      double as[M];
#pragma unroll
      for (int k = 0; k < M; ++k) as[k] = a;
      int st = 0;
      mu_hat[i] = fit_mu<M>(xs, fs, as, R, ~0u, &st, s_tab);
    }
  }
  wave_flags(fl, flags);
}

// q2qnbinom (scaled_nb.py:217-275), elementwise; the clamped means are
// written back, as the reference mutates its arguments (:240-242).
__global__ __launch_bounds__(kBlock) void k_nb_quantile_map(
    const double* __restrict__ x, double* __restrict__ mu_in,
    double* __restrict__ mu_out, double alpha, const double* __restrict__ alpha_el,
    int64_t n, double* __restrict__ out) {
  __shared__ LogTab s_tab[kLogTabLen];
  for (int t = threadIdx.x; t < kLogTabLen; t += blockDim.x) s_tab[t] = kLogTab[t];
  __syncthreads();
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    double mi = mu_in[i], mo = mu_out[i];
    out[i] = q2q(x[i], &mi, &mo, alpha_el ? alpha_el[i] : alpha, nullptr, s_tab);
    mu_in[i] = mi;
    mu_out[i] = mo;
  }
}

// logpmf (scaled_nb.py:12-33), elementwise
__global__ __launch_bounds__(kBlock) void k_nb_logpmf(
    const double* __restrict__ k, const double* __restrict__ m,
    const double* __restrict__ phi, int64_t n, double* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = logpmf(k[i], m[i], phi[i]);
}

int check_reps(int R) {
  if (R < 1 || R > kMaxReps)
    return fail(H3D_EINPUT, "R=%d outside [1, %d]", R, kMaxReps);
  return 0;
}

// values per load of a row of R elements of `size` bytes starting at p
int vec_of(const void* p, int R, int size) {
  const uintptr_t a = (uintptr_t)p;
  if (size == 4 && R % 4 == 0 && a % 16 == 0) return 4;
  if (size == 4 && R % 2 == 0 && a % 8 == 0) return 2;
  if (size == 8 && R % 2 == 0 && a % 16 == 0) return 2;
  return 1;
}

// the status word of a launch, read after the stream has drained
int read_flags(h3d_ctx* ctx, const int* d_fl, int* flags) {
  int fl = 0;
  if (int rc = d2h_sync(ctx, &fl, d_fl, 4, ctx->stream)) return rc;
  if (flags) *flags = fl;
  return 0;
}

#define H3D_NB_DISPATCH(KERNEL, R, ...)                                           \
  do {                                                                            \
    if ((R) <= 2) hipLaunchKernelGGL((KERNEL<2>), __VA_ARGS__);                   \
    else if ((R) <= 4) hipLaunchKernelGGL((KERNEL<4>), __VA_ARGS__);              \
    else if ((R) <= 8) hipLaunchKernelGGL((KERNEL<8>), __VA_ARGS__);              \
    else if ((R) <= 16) hipLaunchKernelGGL((KERNEL<16>), __VA_ARGS__);            \
    else hipLaunchKernelGGL((KERNEL<32>), __VA_ARGS__);                           \
  } while (0)

int alpha_count(int64_t sa_px, int64_t sa_rep, int64_t n, int R, int64_t* count) {
  if ((sa_rep != 0 && sa_rep != 1) || (sa_px != 0 && sa_px != (sa_rep ? R : 1)))
    return fail(H3D_EARG, "alpha strides (%lld, %lld): each is 0 or the natural one",
                (long long)sa_px, (long long)sa_rep);
  *count = (sa_px ? n : 1) * (sa_rep ? R : 1);
  return 0;
}

// the argument checks of fit_mu (host_bufs: host or device buffers, for the
// wording): 0 = run it, 1 = nothing to do, < 0 = an error
int fit_mu_args(h3d_ctx* ctx, int64_t sa_px, int64_t sa_rep, int64_t n, int R, int* flags,
                int64_t* na, bool have_bufs, bool host_bufs) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  if (flags) *flags = 0;
  if (int rc = check_reps(R)) return rc;
  if (int rc = alpha_count(sa_px, sa_rep, n, R, na)) return rc;
  if (n < 0) return fail(H3D_EARG, "n < 0");
  if (n == 0) return 1;
  if (!have_bufs) return fail(H3D_EARG, host_bufs ? "null buffer" : "null device buffer");
  return 0;
}

// fit_mu over device buffers (arguments checked); drains the stream
int fit_mu_run(h3d_ctx* ctx, const int32_t* d_x, const double* d_b,
               const double* d_alpha, int64_t sa_px, int64_t sa_rep, int64_t n, int R,
               double* d_mu, int* flags) {
  HIP_TRY(hipSetDevice(ctx->device));
  Scratch sc{ctx};
  int* d_fl = sc.get<int>("nb_flags", 1);
  if (!sc.ok) return fail(H3D_ENOMEM, "nb flags");
  HIP_TRY(hipMemsetAsync(d_fl, 0, 4, ctx->stream));
  const int vx = vec_of(d_x, R, 4);
  int vd = vec_of(d_b, R, 8);
  if (sa_rep == 1 && sa_px == R && vec_of(d_alpha, R, 8) != 2) vd = 1;
  {
    ProfScope ps(ctx, "nb_fit_mu", n);
    H3D_NB_DISPATCH(k_nb_fit_mu, R, dim3(grid_for(ctx, n, 16)), dim3(kBlock), 0,
                    ctx->stream, d_x, d_b, d_alpha, sa_px, (int)sa_rep, n, R, vx, vd,
                    d_mu, d_fl);
  }
  HIP_TRY(hipGetLastError());
  return read_flags(ctx, d_fl, flags);
}

// the same two for equalize
int equalize_args(h3d_ctx* ctx, int64_t n, int R, int* flags, bool have_bufs, bool host_bufs) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  if (flags) *flags = 0;
  if (int rc = check_reps(R)) return rc;
  if (n < 0) return fail(H3D_EARG, "n < 0");
  if (n == 0) return 1;
  if (!have_bufs) return fail(H3D_EARG, host_bufs ? "null buffer" : "null device buffer");
  return 0;
}

int equalize_run(h3d_ctx* ctx, const int32_t* d_x, const double* d_f, double alpha,
                 const double* d_alpha_px, int64_t n, int R, double* d_pseudo,
                 double* d_mu_hat, int* flags) {
  HIP_TRY(hipSetDevice(ctx->device));
  Scratch sc{ctx};
  int* d_fl = sc.get<int>("nb_flags", 1);
  if (!sc.ok) return fail(H3D_ENOMEM, "nb flags");
  HIP_TRY(hipMemsetAsync(d_fl, 0, 4, ctx->stream));
  const int vx = vec_of(d_x, R, 4);
  int vd = vec_of(d_f, R, 8);
  if (vec_of(d_pseudo, R, 8) != 2) vd = 1;
  {
    ProfScope ps(ctx, "nb_equalize", n);
    H3D_NB_DISPATCH(k_nb_equalize, R, dim3(grid_for(ctx, n, 16)), dim3(kBlock), 0,
                    ctx->stream, d_x, d_f, alpha, d_alpha_px, n, R, vx, vd, d_pseudo,
                    d_mu_hat, d_fl);
  }
  HIP_TRY(hipGetLastError());
  return read_flags(ctx, d_fl, flags);
}

}  // namespace

extern "C" {

int h3d_nb_fit_mu_dev(h3d_ctx* ctx, const int32_t* d_x, const double* d_b,
                      const double* d_alpha, int64_t alpha_px_stride,
                      int64_t alpha_rep_stride, int64_t n, int R, double* d_mu,
                      int* flags) {
  int64_t na = 0;
  if (int rc = fit_mu_args(ctx, alpha_px_stride, alpha_rep_stride, n, R, flags, &na,
                           d_x && d_b && d_alpha && d_mu, false))
    return rc < 0 ? rc : 0;
  return fit_mu_run(ctx, d_x, d_b, d_alpha, alpha_px_stride, alpha_rep_stride, n, R,
                    d_mu, flags);
}

int h3d_nb_fit_mu(h3d_ctx* ctx, const int64_t* x, const double* b, const double* alpha,
                  int64_t alpha_px_stride, int64_t alpha_rep_stride, int64_t n, int R,
                  double* mu, int* flags) {
  int64_t na = 0;
  if (int rc = fit_mu_args(ctx, alpha_px_stride, alpha_rep_stride, n, R, flags, &na,
                           x && b && alpha && mu, true))
    return rc < 0 ? rc : 0;
  HostCall hc(ctx);
  int32_t* d_x = hc.counts(x, n * R, "counts must be in [0, 2^31)");
  double* d_b = hc.in("in_f", b, n * R);
  double* d_a = hc.in("nb_alpha", alpha, na);
  double* d_mu = hc.out<double>("nb_out", n);
  if (int rc = hc.ready("nb_fit_mu buffers")) return rc;
  if (int rc = fit_mu_run(ctx, d_x, d_b, d_a, alpha_px_stride, alpha_rep_stride, n, R,
                          d_mu, flags))
    return rc;
  hc.back(mu, d_mu, n);
  return hc.finish();
}

int h3d_nb_equalize_dev(h3d_ctx* ctx, const int32_t* d_x, const double* d_f,
                        double alpha, const double* d_alpha_px, int64_t n, int R,
                        double* d_pseudo, double* d_mu_hat, int* flags) {
  if (int rc = equalize_args(ctx, n, R, flags, d_x && d_f && d_pseudo, false))
    return rc < 0 ? rc : 0;
  return equalize_run(ctx, d_x, d_f, alpha, d_alpha_px, n, R, d_pseudo, d_mu_hat, flags);
}

int h3d_nb_equalize(h3d_ctx* ctx, const int64_t* x, const double* f, double alpha,
                    const double* alpha_px, int64_t n, int R, double* pseudo,
                    double* mu_hat, int* flags) {
  if (int rc = equalize_args(ctx, n, R, flags, x && f && pseudo, true))
    return rc < 0 ? rc : 0;
  HostCall hc(ctx);
  int32_t* d_x = hc.counts(x, n * R, "counts must be in [0, 2^31)");
  double* d_f = hc.in("in_f", f, n * R);
  double* d_a = hc.in("nb_alpha", alpha_px, n);
  double* d_out = hc.out<double>("nb_out", n * R + n);  // pseudo | mu_hat
  if (int rc = hc.ready("nb_equalize buffers")) return rc;
  double* d_mu = mu_hat ? d_out + n * R : nullptr;
  if (int rc = equalize_run(ctx, d_x, d_f, alpha, d_a, n, R, d_out, d_mu, flags)) return rc;
  hc.back(pseudo, d_out, n * R);
  hc.back(mu_hat, d_mu, n);
  return hc.finish();
}

int h3d_nb_quantile_map(h3d_ctx* ctx, const double* x, double* mu_in, double* mu_out,
                        double alpha, const double* alpha_el, int64_t n, double* out) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  if (n < 0) return fail(H3D_EARG, "n < 0");
  if (n == 0) return 0;
  if (!x || !mu_in || !mu_out || !out) return fail(H3D_EARG, "null buffer");
  hipStream_t s = ctx->stream;
  HostCall hc(ctx);
  // x | mu_in | mu_out | out (| alpha)
  double* d = hc.out<double>("nb_out", n * (alpha_el ? 5 : 4));
  if (int rc = hc.ready("nb_quantile_map buffers")) return rc;
  double *d_x = d, *d_mi = d + n, *d_mo = d + 2 * n, *d_out = d + 3 * n;
  double* d_a = alpha_el ? d + 4 * n : nullptr;
  hc.up(d_x, x, n);
  hc.up(d_mi, mu_in, n);
  hc.up(d_mo, mu_out, n);
  hc.up(d_a, alpha_el, n);
  {
    ProfScope ps(ctx, "nb_quantile_map", n);
    hipLaunchKernelGGL(k_nb_quantile_map, dim3(grid_for(ctx, n, 16)), dim3(kBlock), 0, s,
                       d_x, d_mi, d_mo, alpha, d_a, n, d_out);
  }
  HIP_TRY(hipGetLastError());
  hc.back(mu_in, d_mi, n);
  hc.back(mu_out, d_mo, n);
  hc.back(out, d_out, n);
  return hc.finish();
}

int h3d_nb_logpmf(h3d_ctx* ctx, const double* k, const double* m, const double* phi,
                  int64_t n, double* out) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  if (n < 0) return fail(H3D_EARG, "n < 0");
  if (n == 0) return 0;
  if (!k || !m || !phi || !out) return fail(H3D_EARG, "null buffer");
  HostCall hc(ctx);
  double* d = hc.out<double>("nb_out", n * 4);  // k | m | phi | out
  if (int rc = hc.ready("nb_logpmf buffers")) return rc;
  hc.up(d, k, n);
  hc.up(d + n, m, n);
  hc.up(d + 2 * n, phi, n);
  {
    ProfScope ps(ctx, "nb_logpmf", n);
    hipLaunchKernelGGL(k_nb_logpmf, dim3(grid_for(ctx, n, 16)), dim3(kBlock), 0, ctx->stream,
                       d, d + n, d + 2 * n, n, d + 3 * n);
  }
  HIP_TRY(hipGetLastError());
  hc.back(out, d + 3 * n, n);
  return hc.finish();
}

}  // extern "C"
