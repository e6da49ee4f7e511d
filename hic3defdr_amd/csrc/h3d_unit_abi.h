// The unit-test ABI h3dt_*, defined once for both of its builds.
//
// h3d_hosttest.cpp (g++) and h3d_selftest.hip (hipcc, gfx950) include this
// header after they have defined, in an unnamed namespace, the backend every
// entry below is written against:
//
//   In<T>(host, count)         an input array; converts to const T*
//   Out<T>(host, count, fill)  an output array; converts to T*. A NULL host
//                              pointer is an output the caller does not want
//                              (it converts to NULL, and the body skips it);
//                              `fill` is what the caller reads after a failed
//                              call. fetch() makes the values written so far
//                              readable through `host` before the call ends.
//   for_each(n, body)          body(i) for every i in [0, n), each returning
//                              an int of status flags: their OR, or -2 where
//                              the device failed
//   H3DT_BODY                  marks a body (and the helpers bodies call) as
//                              device code; nothing on the host
//
// A body is a lambda that captures the buffers and scalars by value and
// handles one index: it reads its inputs, evaluates the h3d:: function under
// test into locals, then stores. Return codes: -1 for a bad argument (checked
// before any buffer exists, so the outputs stay untouched), -2 for a device
// failure, otherwise the OR of the flags.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "h3d_model.h"
#include "h3d_philox.h"
#include "h3d_sample.h"
#include "h3d_special.h"

namespace {

constexpr int M = h3d::kMaxReps;

// row i of an (n, r) array as doubles, the unused replicate slots set to `pad`
template <typename T>
H3DT_BODY void load_reps(const T* src, int64_t i, int r, double pad, double* dst) {
#pragma unroll
  for (int k = 0; k < M; ++k) dst[k] = k < r ? (double)src[i * r + k] : pad;
}

H3DT_BODY void store_reps(const double* src, int64_t i, int r, double* dst) {
#pragma unroll
  for (int k = 0; k < M; ++k)
    if (k < r) dst[i * r + k] = src[k];
}

// one data pass of qcml over a segment: equalize at the scalar `alpha` into
// `pseudo` (or, without `do_equalize`, read `pseudo` back), then the pixel's
// NLL term at `kc` where `term` is wanted
int equalize_nll(int64_t n, int r, const In<int32_t>& x, const In<double>& f, double alpha,
                 bool do_equalize, const Out<double>& pseudo, h3d::NllConst kc,
                 const Out<double>& term) {
  return for_each(n, [=] H3DT_BODY(int64_t i) {
    double ps[M];
    int st = 0;
    if (do_equalize) {
      double xs[M], fs[M];
      load_reps<int32_t>(x, i, r, 0.0, xs);
      load_reps<double>(f, i, r, 1.0, fs);
      st = h3d::equalize_pixel<M>(xs, fs, r, alpha, ps);
      store_reps(ps, i, r, pseudo);
    } else {
      load_reps<double>(pseudo, i, r, 0.0, ps);
    }
    if (term) term[i] = h3d::nll_pixel<M>(ps, r, kc);
    return st;
  });
}

}  // namespace

extern "C" {

#define H3DT_UNARY(name, fn)                                                    \
  void h3dt_##name(int64_t n, const double* x_, double* out_) {                 \
    In<double> x(x_, n);                                                        \
    Out<double> out(out_, n, NAN);                                              \
    for_each(n, [=] H3DT_BODY(int64_t i) { return out[i] = h3d::fn(x[i]), 0; }); \
  }
#define H3DT_BINARY(name, fn)                                                         \
  void h3dt_##name(int64_t n, const double* a_, const double* x_, double* out_) {     \
    In<double> a(a_, n), x(x_, n);                                                    \
    Out<double> out(out_, n, NAN);                                                    \
    for_each(n, [=] H3DT_BODY(int64_t i) { return out[i] = h3d::fn(a[i], x[i]), 0; }); \
  }

H3DT_UNARY(lgam, lgam)
H3DT_UNARY(lgam_nll, lgam_nll)
H3DT_UNARY(log_fast, log_fast)
H3DT_UNARY(log_fast_fp_index, log_fast_fp_index)
H3DT_UNARY(ndtr, ndtr)
H3DT_UNARY(ndtri, ndtri)
H3DT_UNARY(log1pmx, log1pmx)
H3DT_UNARY(lgam1p, lgam1p)
H3DT_BINARY(igam, igam)
H3DT_BINARY(igamc, igamc)
H3DT_BINARY(igami, igami)
H3DT_BINARY(igamci, igamci)
H3DT_BINARY(chi2_sf, chi2_sf)
H3DT_UNARY(exp_fast, exp_fast)
H3DT_UNARY(log_fast_checked, log_fast_checked)
H3DT_UNARY(recip_fast, recip_fast)
H3DT_BINARY(div_fast, div_fast)

// Philox4x32-10 of n (counter, key) pairs: ctr (n, 4), key (n, 2) -> out
// (n, 4) words, and the stream's two uniforms of each output (u (n, 2))
void h3dt_philox(int64_t n, const uint32_t* ctr_, const uint32_t* key_, uint32_t* out_,
                 double* u_) {
  In<uint32_t> ctr(ctr_, 4 * n), key(key_, 2 * n);
  Out<uint32_t> out(out_, 4 * n, ~0u);
  Out<double> u(u_, 2 * n, NAN);
  for_each(n, [=] H3DT_BODY(int64_t i) {
    const h3d::Philox4 c = {ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3]};
    const h3d::Philox4 o = h3d::philox4x32_10(c, key[2 * i], key[2 * i + 1]);
    out[4 * i] = o.w0, out[4 * i + 1] = o.w1, out[4 * i + 2] = o.w2, out[4 * i + 3] = o.w3;
    u[2 * i] = h3d::philox_uniform(o.w0, o.w1);
    u[2 * i + 1] = h3d::philox_uniform(o.w2, o.w3);
    return 0;
  });
}

// the stream's uniform of the words (lo[i], hi[i])
void h3dt_philox_uniform(int64_t n, const uint32_t* lo_, const uint32_t* hi_, double* u_) {
  In<uint32_t> lo(lo_, n), hi(hi_, n);
  Out<double> u(u_, n, NAN);
  for_each(n, [=] H3DT_BODY(int64_t i) { return u[i] = h3d::philox_uniform(lo[i], hi[i]), 0; });
}

// nb_draw elementwise: the gamma stage's lambda, the count k (-1: bad input)
// and, optionally, the Poisson path taken (h3d_sample.h kPois*)
int h3dt_nb_draw(int64_t n, const double* bm_, const double* disp_, const double* u1_,
                 const double* u2_, double* lambda_, int32_t* k_, int32_t* path_) {
  In<double> bm(bm_, n), disp(disp_, n), u1(u1_, n), u2(u2_, n);
  Out<double> lambda(lambda_, n, NAN);
  Out<int32_t> k(k_, n, -2), path(path_, n, -2);
  return for_each(n, [=] H3DT_BODY(int64_t i) {
    double lam;
    int fl = 0, pth;
    const int32_t count = h3d::nb_draw(bm[i], disp[i], u1[i], u2[i], &lam, &fl, &pth);
    lambda[i] = lam;
    k[i] = count;
    if (path) path[i] = pth;
    return fl;
  });
}

// the biased means and dispersions h3d_simulate_dev draws from (its
// arguments): bm and disp as (J, n) planes; -1, with nothing staged, for a
// row / col outside [0, n_bins) or a col - row outside [0, D)
int h3dt_sim_bm(int64_t n, int J, int n_bins, int D, const int32_t* row_,
                const int32_t* col_, const double* meanA_, const double* meanB_,
                const double* bias_, const double* sf_, int sf_rows, const double* table_,
                double* bm_, double* disp_) {
  for (int64_t i = 0; i < n; ++i)
    if (row_[i] < 0 || row_[i] >= n_bins || col_[i] < row_[i] || col_[i] >= n_bins ||
        col_[i] - row_[i] >= D)
      return -1;
  In<int32_t> row(row_, n), col(col_, n);
  In<double> meanA(meanA_, n), meanB(meanB_, n), bias(bias_, (int64_t)n_bins * J),
      sf(sf_, (int64_t)(sf_rows == 1 ? 1 : D) * J), table(table_, D);
  Out<double> bm(bm_, n * J, NAN), disp(disp_, n * J, NAN);
  return for_each(n, [=] H3DT_BODY(int64_t i) {
    const int64_t dist = (int64_t)col[i] - row[i];
    for (int j = 0; j < J; ++j) {
      const double s = sf[(sf_rows == 1 ? 0 : dist * J) + j];
      bm[j * n + i] = h3d::sim_bm(j < J / 2 ? meanA[i] : meanB[i],
                                  bias[(int64_t)row[i] * J + j],
                                  bias[(int64_t)col[i] * J + j], s);
      disp[j * n + i] = table[dist];
    }
    return 0;
  });
}

// poisson_quantile elementwise (lambda >= 0 finite, u in (0, 1)); k as a double
void h3dt_poisson_quantile(int64_t n, const double* lambda_, const double* u_, double* k_,
                           int32_t* path_) {
  In<double> lambda(lambda_, n), u(u_, n);
  Out<double> k(k_, n, NAN);
  Out<int32_t> path(path_, n, -2);
  for_each(n, [=] H3DT_BODY(int64_t i) {
    int pth;
    k[i] = h3d::poisson_quantile(lambda[i], u[i], &pth);
    if (path) path[i] = pth;
    return 0;
  });
}

// igam_pq as q2q_core / igam_inv call it: lga = lgam_q2q(a), tail -1 / 0 / 1
void h3dt_igam_pq(int64_t n, const double* a_, const double* x_, int tail, double* P_,
                  double* Q_, double* fac_) {
  In<double> a(a_, n), x(x_, n);
  Out<double> P(P_, n, NAN), Q(Q_, n, NAN), fac(fac_, n, NAN);
  for_each(n, [=] H3DT_BODY(int64_t i) {
    double p, q, fc;
    h3d::igam_pq(a[i], x[i], h3d::lgam_q2q(a[i]), &p, &q, &fc, tail);
    P[i] = p, Q[i] = q, fac[i] = fc;
    return 0;
  });
}

// igam_inv with lga = lgam_q2q(a); guess[i] <= 0: no guess
void h3dt_igam_inv(int64_t n, const double* a_, const double* t_, int upper,
                   const double* guess_, double* out_) {
  In<double> a(a_, n), t(t_, n), guess(guess_, n);
  Out<double> out(out_, n, NAN);
  for_each(n, [=] H3DT_BODY(int64_t i) {
    out[i] = h3d::igam_inv(a[i], t[i], upper != 0, h3d::lgam_q2q(a[i]),
                           guess[i] > 0.0 ? guess[i] : -1.0);
    return 0;
  });
}

// igam_taylor_ok, and igam_step_taylor where it holds (NaN elsewhere)
void h3dt_igam_step_taylor(int64_t n, const double* a_, const double* xe_, const double* h_,
                           int32_t* ok_, double* dint_, double* ratio_) {
  In<double> a(a_, n), xe(xe_, n), h(h_, n);
  Out<int32_t> ok(ok_, n, -2);
  Out<double> dint(dint_, n, NAN), ratio(ratio_, n, NAN);
  for_each(n, [=] H3DT_BODY(int64_t i) {
    const bool w = h3d::igam_taylor_ok(a[i], xe[i], h[i]);
    double d = NAN, rt = NAN;
    if (w) h3d::igam_step_taylor(a[i], xe[i], h[i], &d, &rt);
    ok[i] = w ? 1 : 0;
    dint[i] = d, ratio[i] = rt;
    return 0;
  });
}

// log_fast's table bucket of frexp(x)'s mantissa: from its bits (the form in
// use) and by the FP64 expression it replaced
void h3dt_log_index(int64_t n, const double* x_, int32_t* bits_, int32_t* fp_) {
  In<double> x(x_, n);
  Out<int32_t> bits(bits_, n, -2), fp(fp_, n, -2);
  for_each(n, [=] H3DT_BODY(int64_t i) {
    int e;
    const double m = frexp(x[i], &e);
    bits[i] = h3d::log_fast_index(m);
    fp[i] = h3d::log_fast_index_fp(m);
    return 0;
  });
}

// q2qnbinom elementwise (single replicate, no clamp carry)
void h3dt_q2q(int64_t n, const double* x_, const double* mu_in_, const double* mu_out_,
              const double* alpha_, double* out_) {
  In<double> x(x_, n), mu_in(mu_in_, n), mu_out(mu_out_, n), alpha(alpha_, n);
  Out<double> out(out_, n, NAN);
  for_each(n, [=] H3DT_BODY(int64_t i) {
    double mi = mu_in[i], mo = mu_out[i];
    out[i] = h3d::q2q(x[i], &mi, &mo, alpha[i]);
    return 0;
  });
}

// fit_mu_hat per pixel: x (n, r) int32, b (n, r), alpha (n, r) -> mu (n)
int h3dt_fit_mu(int64_t n, int r, const int32_t* x_, const double* b_, const double* alpha_,
                double* mu_) {
  if (r < 1 || r > M) return -1;
  In<int32_t> x(x_, n * r);
  In<double> b(b_, n * r), alpha(alpha_, n * r);
  Out<double> mu(mu_, n, NAN);
  return for_each(n, [=] H3DT_BODY(int64_t i) {
    double xs[M], bs[M], as[M];
    load_reps<int32_t>(x, i, r, 0.0, xs);
    load_reps<double>(b, i, r, 1.0, bs);
    load_reps<double>(alpha, i, r, 1.0, as);
    int st = 0;
    mu[i] = h3d::fit_mu<M>(xs, bs, as, r, ~0u, &st);
    return st;
  });
}

// equalize with one alpha per pixel: data (n, r) int32, f (n, r), alpha (n)
int h3dt_equalize_alpha(int64_t n, int r, const int32_t* x_, const double* f_,
                        const double* alpha_, double* out_) {
  if (r < 1 || r > M) return -1;
  In<int32_t> x(x_, n * r);
  In<double> f(f_, n * r), alpha(alpha_, n);
  Out<double> out(out_, n * r, NAN);
  return for_each(n, [=] H3DT_BODY(int64_t i) {
    double xs[M], fs[M], ps[M];
    load_reps<int32_t>(x, i, r, 0.0, xs);
    load_reps<double>(f, i, r, 1.0, fs);
    const int st = h3d::equalize_pixel<M>(xs, fs, r, alpha[i], ps);
    store_reps(ps, i, r, out);
    return st;
  });
}

// equalize one segment: data (n, r) int32, f (n, r), scalar alpha
int h3dt_equalize(int64_t n, int r, const int32_t* x_, const double* f_, double alpha,
                  double* out_) {
  if (r < 1 || r > M) return -1;
  In<int32_t> x(x_, n * r);
  In<double> f(f_, n * r);
  Out<double> out(out_, n * r, NAN), no_term(nullptr, 0, NAN);
  return equalize_nll(n, r, x, f, alpha, true, out, h3d::NllConst{}, no_term);
}

// per-pixel NLL terms at delta by the general / mid (r >= 10) / large
// (r >= 20) forms of the Brent kernels (mode 0 / 1 / 2), and their r >= 5 /
// n r >= 5 forms (mode 3 / 4)
int h3dt_nll_terms(int64_t n, int r, const double* pseudo_, double delta, int mode,
                   double* out_) {
  if (r < 1 || r > M || mode < 0 || mode > 4) return -1;
  const h3d::NllConst kc = h3d::nll_const(delta, r);
  In<double> pseudo(pseudo_, n * r);
  Out<double> out(out_, n, NAN);
  return for_each(n, [=] H3DT_BODY(int64_t i) {
    double ps[M];
    load_reps<double>(pseudo, i, r, 0.0, ps);
    out[i] = mode == 4   ? h3d::nll_pixel_nr5<M>(ps, r, kc)
             : mode == 3 ? h3d::nll_pixel_r5<M>(ps, r, kc)
             : mode == 2 ? h3d::nll_pixel_large<M>(ps, r, kc)
             : mode == 1 ? h3d::nll_pixel_mid<M>(ps, r, kc)
                         : h3d::nll_pixel<M>(ps, r, kc);
    return 0;
  });
}

// per-pixel LRT with per-replicate dispersions (lrt.py:7-50)
int h3dt_lrt(int64_t n, int R, int C, const int32_t* raw_, const double* f_,
             const double* disp_wide_, const int32_t* cond_of_rep_, int refit, double* p_,
             double* llr_, double* mu0_, double* mu1_) {
  if (R < 1 || R > M || C < 1 || C > h3d::kMaxConds) return -1;
  In<int32_t> raw(raw_, n * R), cond_of_rep(cond_of_rep_, R);
  In<double> f(f_, n * R), disp_wide(disp_wide_, n * R);
  Out<double> p(p_, n, NAN), llr(llr_, n, NAN), mu0(mu0_, n, NAN), mu1(mu1_, n * C, NAN);
  return for_each(n, [=] H3DT_BODY(int64_t i) {
    int cond[M];
#pragma unroll
    for (int k = 0; k < M; ++k) cond[k] = k < R ? cond_of_rep[k] : -1;
    double xs[M], fs[M], as[M];
    load_reps<int32_t>(raw, i, R, 0.0, xs);
    load_reps<double>(f, i, R, 1.0, fs);
    load_reps<double>(disp_wide, i, R, 1.0, as);
    double pv, lv, m0, m1[h3d::kMaxConds];
    const int st = h3d::lrt_pixel<M, h3d::kMaxConds>(xs, fs, as, cond, R, C, refit != 0,
                                                     &pv, &lv, &m0, m1);
    p[i] = pv, llr[i] = lv, mu0[i] = m0;
    for (int c = 0; c < C; ++c) mu1[i * C + c] = m1[c];
    return st;
  });
}

// full qcml on one segment: the data passes (equalize, NLL terms) go through
// for_each; the bounded-Brent / qcml state machine (h3d_model.h seg_step)
// and the sum of the pixel terms, in index order, stay on the host
double h3dt_qcml(int64_t n, int r, const int32_t* x_, const double* f_, int* status) {
  if (r < 1 || r > M) {
    *status = -1;
    return NAN;
  }
  std::vector<double> pseudo_h(n * r), term_h(n);
  In<int32_t> x(x_, n * r);
  In<double> f(f_, n * r);
  Out<double> pseudo(pseudo_h.data(), n * r, NAN), term(term_h.data(), n, NAN);
  h3d::SegState st;
  h3d::seg_init(&st, n, r);
  int guard = 0;
  while (st.phase != h3d::kDone && guard++ < 100000) {
    const int fl = equalize_nll(n, r, x, f, st.disp, st.phase == h3d::kEqualize, pseudo,
                                st.k, term);
    if (fl < 0 || !term.fetch()) {
      *status = -2;
      return NAN;
    }
    st.flags |= fl;
    double total = 0.0;
    for (int64_t i = 0; i < n; ++i) total += term_h[i];
    h3d::seg_step(&st, total, r);
  }
  *status = st.flags;
  return st.result;
}

}  // extern "C"
