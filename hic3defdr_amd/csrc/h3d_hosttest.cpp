// Host build of the device numerics, for CPU unit tests ONLY.
//
// The same headers the gfx950 kernels include (h3d_special.h, h3d_model.h,
// h3d_philox.h, h3d_sample.h, h3d_ccl.h)
// compiled with g++ and exported over a flat C ABI so tests/ can check them
// against scipy / the oracle without a GPU. The product never loads this
// library (hic3defdr_amd loads libh3d.so and fails loudly without it).
#include <cstdint>
#include <vector>

#include "h3d_ccl.h"
#include "h3d_model.h"
#include "h3d_philox.h"
#include "h3d_sample.h"
#include "h3d_special.h"

namespace {
constexpr int M = h3d::kMaxReps;
}

extern "C" {

#define H3DT_UNARY(name, fn)                                   \
  void h3dt_##name(int64_t n, const double* x, double* out) { \
    for (int64_t i = 0; i < n; ++i) out[i] = h3d::fn(x[i]);   \
  }
#define H3DT_BINARY(name, fn)                                     \
  void h3dt_##name(int64_t n, const double* a, const double* x,  \
                   double* out) {                                 \
    for (int64_t i = 0; i < n; ++i) out[i] = h3d::fn(a[i], x[i]); \
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
// exp_fast's gfx950 straight line evaluated here (host build only)
H3DT_UNARY(exp_fast_straight, exp_fast_straight)

// Philox4x32-10 of n (counter, key) pairs: ctr (n, 4), key (n, 2) -> out
// (n, 4) words, and the stream's two uniforms of each output (u (n, 2))
void h3dt_philox(int64_t n, const uint32_t* ctr, const uint32_t* key, uint32_t* out,
                 double* u) {
  for (int64_t i = 0; i < n; ++i) {
    const h3d::Philox4 c = {ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3]};
    const h3d::Philox4 o = h3d::philox4x32_10(c, key[2 * i], key[2 * i + 1]);
    out[4 * i] = o.w0, out[4 * i + 1] = o.w1, out[4 * i + 2] = o.w2, out[4 * i + 3] = o.w3;
    u[2 * i] = h3d::philox_uniform(o.w0, o.w1);
    u[2 * i + 1] = h3d::philox_uniform(o.w2, o.w3);
  }
}

// the stream's uniform of the words (lo[i], hi[i])
void h3dt_philox_uniform(int64_t n, const uint32_t* lo, const uint32_t* hi, double* u) {
  for (int64_t i = 0; i < n; ++i) u[i] = h3d::philox_uniform(lo[i], hi[i]);
}

// nb_draw elementwise: the gamma stage's lambda, the count k (-1: bad input)
// and, optionally, the Poisson path taken (h3d_sample.h kPois*); returns the
// OR of the flags
int h3dt_nb_draw(int64_t n, const double* bm, const double* disp, const double* u1,
                 const double* u2, double* lambda, int32_t* k, int32_t* path) {
  int fl = 0;
  for (int64_t i = 0; i < n; ++i) {
    int pth;
    k[i] = h3d::nb_draw(bm[i], disp[i], u1[i], u2[i], &lambda[i], &fl, &pth);
    if (path) path[i] = pth;
  }
  return fl;
}

// the biased means and dispersions h3d_simulate_dev draws from (its
// arguments): bm and disp as (J, n) planes; -1 for a row / col outside
// [0, n_bins) or a col - row outside [0, D)
int h3dt_sim_bm(int64_t n, int J, int n_bins, int D, const int32_t* row,
                const int32_t* col, const double* meanA, const double* meanB,
                const double* bias, const double* sf, int sf_rows, const double* table,
                double* bm, double* disp) {
  for (int64_t i = 0; i < n; ++i)
    if (row[i] < 0 || row[i] >= n_bins || col[i] < row[i] || col[i] >= n_bins ||
        col[i] - row[i] >= D)
      return -1;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t dist = (int64_t)col[i] - row[i];
    for (int j = 0; j < J; ++j) {
      const double s = sf[(sf_rows == 1 ? 0 : dist * J) + j];
      bm[j * n + i] = h3d::sim_bm(j < J / 2 ? meanA[i] : meanB[i],
                                  bias[(int64_t)row[i] * J + j],
                                  bias[(int64_t)col[i] * J + j], s);
      disp[j * n + i] = table[dist];
    }
  }
  return 0;
}

// poisson_quantile elementwise (lambda >= 0 finite, u in (0, 1)); k as a double
void h3dt_poisson_quantile(int64_t n, const double* lambda, const double* u, double* k,
                           int32_t* path) {
  for (int64_t i = 0; i < n; ++i) {
    int pth;
    k[i] = h3d::poisson_quantile(lambda[i], u[i], &pth);
    if (path) path[i] = pth;
  }
}

// igam_pq as q2q_core / igam_inv call it: lga = lgam_q2q(a), tail -1 / 0 / 1
void h3dt_igam_pq(int64_t n, const double* a, const double* x, int tail,
                  double* P, double* Q, double* fac) {
  for (int64_t i = 0; i < n; ++i)
    h3d::igam_pq(a[i], x[i], h3d::lgam_q2q(a[i]), &P[i], &Q[i], &fac[i], tail);
}

// igam_inv with lga = lgam_q2q(a); guess[i] <= 0: no guess
void h3dt_igam_inv(int64_t n, const double* a, const double* t, int upper,
                   const double* guess, double* out) {
  for (int64_t i = 0; i < n; ++i)
    out[i] = h3d::igam_inv(a[i], t[i], upper != 0, h3d::lgam_q2q(a[i]),
                           guess[i] > 0.0 ? guess[i] : -1.0);
}

// igam_taylor_ok, and igam_step_taylor where it holds (NaN elsewhere)
void h3dt_igam_step_taylor(int64_t n, const double* a, const double* xe,
                           const double* h, int32_t* ok, double* dint,
                           double* ratio) {
  for (int64_t i = 0; i < n; ++i) {
    ok[i] = h3d::igam_taylor_ok(a[i], xe[i], h[i]) ? 1 : 0;
    dint[i] = ratio[i] = NAN;
    if (ok[i]) h3d::igam_step_taylor(a[i], xe[i], h[i], &dint[i], &ratio[i]);
  }
}

// equalize with one alpha per pixel: data (n, r) int32, f (n, r), alpha (n)
int h3dt_equalize_alpha(int64_t n, int r, const int32_t* x, const double* f,
                        const double* alpha, double* out) {
  if (r < 1 || r > M) return -1;
  int bad = 0;
  for (int64_t i = 0; i < n; ++i) {
    double xs[M], fs[M], ps[M];
    for (int k = 0; k < r; ++k) {
      xs[k] = x[i * r + k];
      fs[k] = f[i * r + k];
    }
    bad |= h3d::equalize_pixel<M>(xs, fs, r, alpha[i], ps);
    for (int k = 0; k < r; ++k) out[i * r + k] = ps[k];
  }
  return bad;
}

// log_fast's table bucket of frexp(x)'s mantissa: from its bits (the form in
// use) and by the FP64 expression it replaced
void h3dt_log_index(int64_t n, const double* x, int32_t* bits, int32_t* fp) {
  for (int64_t i = 0; i < n; ++i) {
    int e;
    const double m = frexp(x[i], &e);
    bits[i] = h3d::log_fast_index(m);
    fp[i] = h3d::log_fast_index_fp(m);
  }
}

// fit_mu_hat per pixel: x (n, r) int32, b (n, r), alpha (n, r) -> mu (n)
int h3dt_fit_mu(int64_t n, int r, const int32_t* x, const double* b,
                const double* alpha, double* mu) {
  int bad = 0;
  for (int64_t i = 0; i < n; ++i) {
    double xs[M], bs[M], as[M];
    for (int k = 0; k < r; ++k) {
      xs[k] = x[i * r + k];
      bs[k] = b[i * r + k];
      as[k] = alpha[i * r + k];
    }
    int st = 0;
    mu[i] = h3d::fit_mu<M>(xs, bs, as, r, ~0u, &st);
    bad |= st;
  }
  return bad;
}

// q2qnbinom elementwise (single replicate, no clamp carry)
void h3dt_q2q(int64_t n, const double* x, const double* mu_in,
              const double* mu_out, const double* alpha, double* out) {
  for (int64_t i = 0; i < n; ++i) {
    double mi = mu_in[i], mo = mu_out[i];
    out[i] = h3d::q2q(x[i], &mi, &mo, alpha[i]);
  }
}

// equalize one segment: data (n, r) int32, f (n, r), scalar alpha
int h3dt_equalize(int64_t n, int r, const int32_t* x, const double* f,
                  double alpha, double* out) {
  int bad = 0;
  for (int64_t i = 0; i < n; ++i) {
    double xs[M], fs[M], ps[M];
    for (int k = 0; k < r; ++k) {
      xs[k] = x[i * r + k];
      fs[k] = f[i * r + k];
    }
    bad |= h3d::equalize_pixel<M>(xs, fs, r, alpha, ps);
    for (int k = 0; k < r; ++k) out[i * r + k] = ps[k];
  }
  return bad;
}

// per-pixel NLL terms at delta by the general / mid (r >= 10) / large
// (r >= 20) forms of the Brent kernels (mode 0 / 1 / 2), and their r >= 5 /
// n r >= 5 forms (mode 3 / 4)
int h3dt_nll_terms(int64_t n, int r, const double* pseudo, double delta, int mode,
                   double* out) {
  if (r < 1 || r > M || mode < 0 || mode > 4) return -1;
  const h3d::NllConst kc = h3d::nll_const(delta, r);
  for (int64_t i = 0; i < n; ++i) {
    double ps[M];
    for (int k = 0; k < M; ++k) ps[k] = k < r ? pseudo[i * r + k] : 0.0;
    out[i] = mode == 4   ? h3d::nll_pixel_nr5<M>(ps, r, kc)
             : mode == 3 ? h3d::nll_pixel_r5<M>(ps, r, kc)
             : mode == 2 ? h3d::nll_pixel_large<M>(ps, r, kc)
             : mode == 1 ? h3d::nll_pixel_mid<M>(ps, r, kc)
                         : h3d::nll_pixel<M>(ps, r, kc);
  }
  return 0;
}

// per-pixel LRT with per-replicate dispersions (lrt.py:7-50)
int h3dt_lrt(int64_t n, int R, int C, const int32_t* raw, const double* f,
             const double* disp_wide, const int32_t* cond_of_rep, int refit,
             double* p, double* llr, double* mu0, double* mu1) {
  int bad = 0;
  int cond[M];
  for (int k = 0; k < R; ++k) cond[k] = cond_of_rep[k];
  for (int64_t i = 0; i < n; ++i) {
    double xs[M], fs[M], as[M];
    for (int k = 0; k < R; ++k) {
      xs[k] = raw[i * R + k];
      fs[k] = f[i * R + k];
      as[k] = disp_wide[i * R + k];
    }
    double m1[h3d::kMaxConds];
    bad |= h3d::lrt_pixel<M, h3d::kMaxConds>(xs, fs, as, cond, R, C,
                                             refit != 0, &p[i], &llr[i],
                                             &mu0[i], m1);
    for (int c = 0; c < C; ++c) mu1[i * C + c] = m1[c];
  }
  return bad;
}

// full qcml on one segment, driven by the same state machine as the kernels
double h3dt_qcml(int64_t n, int r, const int32_t* x, const double* f,
                 int* status) {
  std::vector<double> pseudo(n * r);
  h3d::SegState st;
  h3d::seg_init(&st, n, r);
  int guard = 0;
  while (st.phase != h3d::kDone && guard++ < 100000) {
    double total = 0.0;
    if (st.phase == h3d::kEqualize) {
      for (int64_t i = 0; i < n; ++i) {
        double xs[M], fs[M];
        for (int k = 0; k < r; ++k) {
          xs[k] = x[i * r + k];
          fs[k] = f[i * r + k];
        }
        st.flags |= h3d::equalize_pixel<M>(xs, fs, r, st.disp, &pseudo[i * r]);
      }
    }
    for (int64_t i = 0; i < n; ++i)
      total += h3d::nll_pixel<M>(&pseudo[i * r], r, st.k);
    h3d::seg_step(&st, total, r);
  }
  *status = st.flags;
  return st.result;
}

// Host emulation of the multi-rank estimate_disp driver (h3d_disp_per_dist_dev
// with an all-reduce hook): this rank's pixels, stable-ordered by distance;
// per data pass every active segment's local NLL total, summed across ranks
// by `reduce`, then the shared qcml/Brent state machines advance. Used by the
// gloo world_size-2 tests to check the sharded algorithm on CPU.
typedef int (*h3dt_reduce_fn)(double* buf, int64_t count, void* user);

int h3dt_disp_rounds(int64_t n, int R, int C, const int32_t* raw,
                     const double* f, const int32_t* dist,
                     const int32_t* cond_of_rep, int D, h3dt_reduce_fn reduce,
                     void* user, double* out, int32_t* flags_out) {
  const int S = D * C;
  std::vector<int> nrep(C, 0), rep_idx(C * M, 0);
  for (int r = 0; r < R; ++r) rep_idx[cond_of_rep[r] * M + nrep[cond_of_rep[r]]++] = r;
  std::vector<std::vector<int64_t>> px(D);
  for (int64_t i = 0; i < n; ++i) px[dist[i]].push_back(i);
  std::vector<double> cnt(S, 0.0), tot(S, 0.0);
  for (int d = 0; d < D; ++d)
    for (int c = 0; c < C; ++c) cnt[d * C + c] = (double)px[d].size();
  if (reduce && reduce(cnt.data(), S, user)) return -2;
  std::vector<h3d::SegState> st(S);
  for (int s = 0; s < S; ++s) h3d::seg_init(&st[s], (long long)cnt[s], nrep[s % C]);
  std::vector<double> pd((size_t)n * R, 0.0);
  for (int guard = 0; guard < 200000; ++guard) {
    bool any = false;
    for (int s = 0; s < S; ++s) any |= st[s].phase != h3d::kDone;
    if (!any) break;
    for (int s = 0; s < S; ++s) {
      tot[s] = 0.0;
      if (st[s].phase == h3d::kDone) continue;
      const int d = s / C, c = s % C, nr = nrep[c];
      for (int64_t i : px[d]) {
        double x[M], fv[M], dd[M];
        for (int k = 0; k < nr; ++k) {
          const int r = rep_idx[c * M + k];
          x[k] = raw[i * R + r];
          fv[k] = f[i * R + r];
          dd[k] = pd[i * R + r];
        }
        if (st[s].phase == h3d::kEqualize) {
          st[s].flags |= h3d::equalize_pixel<M>(x, fv, nr, st[s].disp, dd);
          for (int k = 0; k < nr; ++k) pd[i * R + rep_idx[c * M + k]] = dd[k];
        }
        tot[s] += h3d::nll_pixel<M>(dd, nr, st[s].k);
      }
    }
    if (reduce && reduce(tot.data(), S, user)) return -2;
    for (int s = 0; s < S; ++s)
      if (st[s].phase != h3d::kDone) h3d::seg_step(&st[s], tot[s], nrep[s % C]);
  }
  for (int s = 0; s < S; ++s) {
    out[s] = st[s].result;
    if (flags_out) flags_out[s] = st[s].flags;
  }
  return 0;
}

// h3d_label_components (h3d_clusters.hip) with a serial union-find in place
// of the CAS: the same input check, run-head / run-tail predicates and link
// enumeration (h3d_ccl.h), run ids from a serial count, labels by first
// pixel. Returns 16 (H3D_FLAG_BADIN; label all -1, *n_clusters 0) where the
// input breaks the (row, col) rule, -1 for a bad argument, 0 otherwise.
int h3dt_ccl_labels(const int64_t* row, const int64_t* col, const uint8_t* cls, int64_t n,
                    int connectivity, int32_t* label, int64_t* n_clusters) {
  using namespace h3dccl;
  if (n < 0 || n > (((int64_t)1 << 31) - 2) || !n_clusters) return -1;
  if (connectivity != 1 && connectivity != 2) return -1;
  *n_clusters = 0;
  if (n == 0) return 0;
  if (!row || !col || !cls || !label) return -1;
  bool bad = false;
  for (int64_t i = 0; i < n; ++i) {
    bad = bad || bad_pixel(row, col, i);
    label[i] = -1;
  }
  if (bad) return 16;
  std::vector<int32_t> incl((size_t)n), first;
  std::vector<uint64_t> key0, key1;
  std::vector<uint8_t> rcls;
  int32_t count = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (run_head(row, col, cls, i)) {
      ++count;
      first.push_back((int32_t)i);
      key0.push_back(pixel_key(row[i], col[i]));
      key1.push_back(0);
      rcls.push_back(cls[i]);
    }
    incl[i] = count;
    if (run_tail(row, col, cls, i, n)) key1[count - 1] = pixel_key(row[i], col[i]);
  }
  if (count == 0) return 0;
  std::vector<int32_t> parent((size_t)count);
  for (int32_t r = 0; r < count; ++r) parent[r] = r;
  auto find = [&](int32_t x) {
    while (parent[x] != x) x = parent[x] = parent[parent[x]];
    return x;
  };
  const Runs runs{first.data(), key0.data(), key1.data(), rcls.data(), count};
  for (int32_t r = 0; r < count; ++r)
    for_each_link(runs, r, connectivity, [&](int32_t a, int32_t b) {
      a = find(a), b = find(b);
      if (a != b) parent[a > b ? a : b] = a > b ? b : a;  // the smaller id stays the root
    });
  std::vector<int32_t> rank((size_t)count);
  int32_t n_roots = 0;
  for (int32_t r = 0; r < count; ++r) rank[r] = find(r) == r ? n_roots++ : -1;
  for (int64_t i = 0; i < n; ++i)
    if (cls[i] != kAbsent) label[i] = rank[find(incl[i] - 1)];
  *n_clusters = n_roots;
  return 0;
}

// q_class / argmax_class of h3d_ccl.h over n pixels (value (n, C) row-major)
void h3dt_q_class(int64_t n, const double* q, double fdr, uint8_t* cls) {
  for (int64_t i = 0; i < n; ++i) cls[i] = h3dccl::q_class(q[i], fdr);
}
void h3dt_argmax_class(int64_t n, int C, const double* value, const uint8_t* member,
                       uint8_t* cls) {
  for (int64_t i = 0; i < n; ++i)
    cls[i] = member[i] ? h3dccl::argmax_class(value + i * C, C) : h3dccl::kAbsent;
}

}  // extern "C"
