// Negative-binomial draws by inversion, host + device (simulate(gpu=True),
// DESIGN.md §1 F9; reference simulation.py:187-203 draws the same
// distribution from numpy's stream).
//
// numpy's negative_binomial(n, p) is poisson(gamma(n, (1 - p) / p)); with the
// reference's n = 1 / disp and p = bm / var (var = bm + bm^2 disp) that is a
// Poisson whose mean is Gamma(shape 1 / disp, scale bm disp). nb_draw takes
// the two stages by inversion from two uniforms:
//   lambda = bm disp igami(1 / disp, u1)         (igamci(., 1 - u1) above 1/2)
//   k      = min {k : P(X <= k | lambda) >= u2}  (the Poisson quantile)
// through the incomplete-gamma functions of h3d_special.h, so each count can
// be checked against scipy.special one draw at a time.
#pragma once

#include "h3d_model.h"
#include "h3d_special.h"

namespace h3d {

// which way a Poisson quantile was decided (measurement and tests only)
constexpr int kPoisSum = 0;         // pmf sum from exp(-lambda), lambda < 12
constexpr int kPoisSumVerify = 1;   // ... settled by fresh tails
constexpr int kPoisWalk = 2;        // Cornish-Fisher start, short pmf walk
constexpr int kPoisWalkVerify = 3;  // ... settled by fresh tails
constexpr int kPoisBisect = 4;      // bisection on the tail

constexpr double kPoisSmallLambda = 12.0;
constexpr int kPoisWalkMax = 64;   // recurrence steps before bisection
constexpr int kPoisWalkTrust = 4;  // steps the recurrence decides alone
constexpr double kCountLimit = 2147483648.0;  // counts and lambda below 2^31

// The tail of X ~ Poisson(lam) that holds the uniform, at k >= 0: P(X > k) =
// P(k + 1, lam) (upper) or P(X <= k) = Q(k + 1, lam), evaluated directly (the
// accurate side of igam_pq); *pmf (optional) = P(X = k).
H3D_HD double poisson_tail(double k, double lam, bool upper, double* pmf = nullptr) {
  const double a = k + 1.0;
  double P, Q, fac;
  igam_pq(a, lam, lgam(a), &P, &Q, &fac, upper ? 0 : 1);
  if (pmf) *pmf = fac / lam;  // lam^(k+1) e^-lam / k! / lam
  return upper ? P : Q;
}

// whether k is at or beyond the quantile, from its tail T: P(X <= k) >= u,
// as P(X > k) <= 1 - u on the upper side
H3D_HD bool poisson_reached(double T, double t, bool upper) {
  return upper ? T <= t : T >= t;
}

// The quantile from a candidate k by fresh tail evaluations only: a bracket
// (lo has not reached the quantile, hi has; lo = -1 never has) closed by
// galloping away from the candidate in doubling steps, never past the
// bracket's midpoint, so a candidate that is right costs two evaluations (k
// and k - 1), one that is off by a few a handful, and any other a bisection.
// One evaluation per trip and at most 160 trips: no input can spin.
H3D_HD double poisson_settle(double k, double lam, double t, bool upper, int* path) {
  double lo = -1.0, hi = -1.0, probe = k, step = 1.0;
  for (int it = 0; it < 160; ++it) {
    if (it == 6) *path = kPoisBisect;
    if (poisson_reached(poisson_tail(probe, lam, upper), t, upper))
      hi = probe;
    else
      lo = probe;
    if (hi >= 0.0 && hi - lo <= 1.0) return hi;
    probe = (hi < 0.0) ? lo + step : fmax(hi - step, floor(0.5 * (lo + hi)));
    step *= 2.0;
  }
  return (hi >= 0.0) ? hi : lo + 1.0;
}

// The smallest integer k with P(X <= k | lam) >= u, for lam >= 0 finite and u
// in (0, 1), decided in the tail that holds u (the sf against 1 - u above
// 1/2; 1 - u is exact for the stream's uniforms).
//   lam < 12: the pmf summed upward from exp(-lam). All terms positive, so
//   the cdf is good to ~k ulp relative and decides the lower side alone. On
//   the upper side 1 - cdf carries the sum's absolute rounding (< 2e-14: at
//   most ~80 terms below 1); a decision closer than that to either
//   neighbour's tail is settled by fresh evaluations.
//   Otherwise: start at the Cornish-Fisher point lam + z sqrt(lam) +
//   (z^2 - 1) / 6, z = ndtri(u), one igam_pq there, then walk by the pmf
//   recurrence pmf lam / (k + 1). A walk longer than kPoisWalkTrust steps is
//   settled by fresh evaluations at k and k - 1, one that exhausts
//   kPoisWalkMax by the bisection those fall back to.
// (one call site each for the start's and the settling evaluation: inlined,
// igam_pq is most of the kernel's code)
H3D_HD double poisson_quantile(double lam, double u, int* path) {
  const bool upper = u > 0.5;
  const double t = upper ? 1.0 - u : u;
  *path = kPoisSum;
  if (!(lam > 0.0)) return 0.0;
  double k = 0.0;
  bool settle;
  if (lam < kPoisSmallLambda) {
    double p = exp(-lam), c = p;
    double s_prev = 1.0, s = 1.0 - c;
    while ((upper ? s > t : c < t) && k < 256.0) {
      k += 1.0;
      p *= lam / k;
      c += p;
      s_prev = s;
      s = 1.0 - c;
    }
    const double slack = 2e-14;
    settle = upper && !(t - s > slack && s_prev - t > slack);
  } else {
    *path = kPoisWalk;
    const double z = upper ? -ndtri_lower(t) : ndtri_lower(t);
    k = floor(fmax(lam + z * sqrt(lam) + (z * z - 1.0) / 6.0, 0.0));
    double pmf;
    double T = poisson_tail(k, lam, upper, &pmf);
    int steps = 0;
    if (poisson_reached(T, t, upper)) {
      // down while k - 1 has reached it too: T(k - 1) = T(k) -/+ pmf(k)
      while (k > 0.0 && steps < kPoisWalkMax) {
        const double Tm = upper ? T + pmf : T - pmf;
        if (!poisson_reached(Tm, t, upper)) break;
        T = Tm;
        pmf *= k / lam;
        k -= 1.0;
        ++steps;
      }
    } else {
      while (steps < kPoisWalkMax) {
        k += 1.0;
        pmf *= lam / k;
        T = upper ? T - pmf : T + pmf;
        ++steps;
        if (poisson_reached(T, t, upper)) break;
      }
    }
    settle = steps > kPoisWalkTrust;
  }
  if (settle) {
    *path += 1;  // kPoisSumVerify / kPoisWalkVerify
    k = poisson_settle(k, lam, t, upper, path);
  }
  return k;
}

// A replicate's biased mean at a pixel in the reference's association
// (simulation.py:190-194: f = bias[row, j] * bias[col, j] * sf; bm = m * f)
H3D_HD double sim_bm(double m, double bias_row, double bias_col, double sf) {
  const double f = bias_row * bias_col * sf;
  return m * f;
}

// One negative-binomial count of mean bm and dispersion disp from the
// uniforms u1 (gamma stage) and u2 (Poisson stage), both in (0, 1). *lambda:
// the gamma stage's value. bm or disp not positive finite, or lambda (or the
// count) not below 2^31: kFlagBadInput into *flags, count -1.
H3D_HD int32_t nb_draw(double bm, double disp, double u1, double u2, double* lambda,
                       int* flags, int* path = nullptr) {
  int pth = -1;
  int32_t count = -1;
  double lam = NAN;
  const double r = 1.0 / disp;
  if (bm > 0.0 && bm < INFINITY && disp > 0.0 && disp < INFINITY && r < INFINITY) {
    // igami(r, u1), or igamci(r, 1 - u1) above 1/2, as their one body
    const bool up1 = u1 > 0.5;
    const double g = igam_inv(r, up1 ? 1.0 - u1 : u1, up1, lgam(r));
    lam = bm * disp * g;
    if (lam >= 0.0 && lam < kCountLimit) {
      const double k = poisson_quantile(lam, u2, &pth);
      if (k < kCountLimit) count = (int32_t)k;
    }
  }
  if (count < 0) *flags |= kFlagBadInput;
  *lambda = lam;
  if (path) *path = pth;
  return count;
}

}  // namespace h3d
