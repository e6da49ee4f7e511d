"""Exact references for tests/test_special_paths.py, written to
tests/golden/unit_special_mp.npz (inputs and references as float64).

Needs mpmath (1.3.0) and the host test library; the tests read only the npz
(test_fixture_subsample_recomputed recomputes a subsample where mpmath is
installed). Run from the repository root:

    python tests/golden/make_golden_special_mp.py [--jobs N]

The regularised incomplete gamma function is evaluated here, not by
mp.gammainc (which raises NoConvergence at shapes ~3e3..5e4):

    P(a, x) = x^a e^-x / Gamma(a + 1) * sum_n x^n / ((a + 1) ... (a + n))

with the sum in 1300-bit fixed point (stopped once n > x - a and the term is
below 2^-1230 of the sum) and the prefactor at mp.dps = 380, so Q = 1 - P
holds ~70 digits down to Q ~ 1e-300. exp is stored as (hi, lo): the
correctly rounded double and the remainder in ulps of hi. Arguments that
are not doubles (the shapes mu / (1 + alpha mu) of the q2q chain, Newton iterates) are rounded to
160 bits first, 1e-48 relative. The inverse is Newton (with the Halley
correction) on the tail from the host build's answer.
"""
import argparse
import ctypes
import multiprocessing
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'unit_special_mp.npz')

mp.mp.dps = 380
mpf = mp.mpf
BITS = 1300          # fixed-point fraction bits of the series sum
STOP = 1230          # stop once term < sum 2^-STOP (1e-370)
ARG_BITS = 160       # non-double arguments are rounded to this

D = ctypes.POINTER(ctypes.c_double)
_host = None


def host():
    global _host
    if _host is None:
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        from hic3defdr_amd import build as h3dbuild
        _host = ctypes.CDLL(h3dbuild.build_hosttest())
    return _host


def rnd(v):
    """v as an mpf of at most ARG_BITS bits (a double passes unchanged)."""
    if not isinstance(v, mp.mpf):
        v = float(v)
    with mp.workprec(ARG_BITS):
        return +mpf(v)


def to_double(v):
    """v correctly rounded to a double (float(mpf) rounds a subnormal result
    twice)."""
    if v != 0 and abs(v) < mpf(2) ** -1022:
        return float(np.ldexp(float(int(mp.nint(mp.ldexp(v, 1074)))), -1074))
    return float(v)


def series_sum(a, x):
    """sum_n x^n / ((a+1) ... (a+n)), a and x mpf of <= ARG_BITS bits."""
    am, ae = a.man_exp
    xm, xe = x.man_exp
    e = min(ae, xe, 0)
    A, X, one = am << (ae - e), xm << (xe - e), 1 << -e
    term = s = 1 << BITS
    n, lim, den = 0, float(x - a), A
    while True:
        n += 1
        den += one
        term = term * X // den
        s += term
        if n > lim and term < (s >> STOP):
            break
    return mp.ldexp(mpf(s), -BITS)


def igam_all(a, x):
    """(P, Q, fac = x^a e^-x / Gamma(a)) at rnd(a), rnd(x)."""
    a, x = rnd(a), rnd(x)
    pre = mp.exp(a * mp.log(x) - x - mp.loggamma(a + 1))
    P = pre * series_sum(a, x)
    return P, 1 - P, pre * a


def host_inv(a, t, upper):
    a_ = np.array([float(a)])
    t_ = np.array([float(t)])
    g = np.array([-1.0])
    out = np.empty(1)
    host().h3dt_igam_inv(ctypes.c_int64(1), a_.ctypes.data_as(D),
                         t_.ctypes.data_as(D), int(bool(upper)),
                         g.ctypes.data_as(D), out.ctypes.data_as(D))
    return out[0]


def igam_inverse(a, t, upper, x0=None):
    """Root x of Q(a, x) = t (upper) or P(a, x) = t, t an mpf in (0, 1)."""
    a, t = rnd(a), mpf(t)
    if x0 is None:
        tf = float(t)
        if tf > 0.9:
            x0 = host_inv(a, max(float(1 - t), 1e-300), not upper)
        else:
            x0 = host_inv(a, max(tf, 1e-300), upper)
    x = rnd(x0)
    for _ in range(40):
        P, Q, fac = igam_all(a, x)
        F = (Q - t) if upper else (P - t)
        dens = fac / x
        nwt = (-F if upper else F) / dens
        fpp = (a - 1) / x - 1
        step = nwt / (1 - nwt * fpp / 2)
        xn = x - step
        if not xn > 0:
            xn = x / 2
            step = x
        # what a Halley step leaves: ~ step^3 (fpp^2 + |fpp'|) / x relative
        curv = fpp * fpp + abs(a - 1) / (x * x) + 1
        if abs(step) ** 3 * curv < mpf(10) ** -40 * xn:
            return xn
        x = rnd(xn)
    raise RuntimeError('igam_inverse did not converge: %r' % ((a, t, upper),))


def q2q_core_ref(x, mi, mo, alpha):
    """q2qnbinom (scaled_nb.py:217-275) on clamped means, exact; None where
    the point has no finite exact reference (the normal tail underflows, or
    the input tail is outside [1e-300, 1 - 1e-17]) and where the normal and
    gamma halves cancel to less than 1e-3 of their size: any double
    evaluation of the reference's formula (q_norm + q_gamma) / 2 is then off
    by 1.1e-16 x that ratio relative (x = 1 at mu_in = 9119, mu_out = 8332,
    alpha = 0.031: q_norm = 8332 - 8332.46, ratio 4e4, host 2.9e-12), which no
    fixed relative bar measures."""
    x, mi, mo, alpha = [v if isinstance(v, mp.mpf) else mpf(float(v))
                        for v in (x, mi, mo, alpha)]
    r_in, r_out = 1 + alpha * mi, 1 + alpha * mo
    v_in, v_out = mi * r_in, mo * r_out
    a_in, a_out = mi / r_in, mo / r_out
    right = x >= mi
    if (x - mi) ** 2 / (2 * v_in) > 700:   # ndtr underflows past 709.78
        return None
    qn = mo + mp.sqrt(v_out / v_in) * (x - mi)
    xs = x / r_in
    if xs <= 0:
        qg = mpf(0)          # x = 0 < mu_in: cdf 0, ppf(0) = 0
    else:
        P, Q, _ = igam_all(a_in, xs)
        tg = Q if right else P
        if not (mpf(10) ** -300 <= tg <= 1 - mpf(10) ** -17):
            return None
        qg = igam_inverse(a_out, tg, right) * r_out
    pc = (qn + qg) / 2
    if max(abs(qn), abs(qg), abs(mo)) > 1000 * abs(pc):
        return None
    return pc if pc >= 0 else mpf(0)


def q2q_ref(x, mu_in, mu_out, alpha):
    if not (mu_in >= 0.25 and mu_out >= 0.25):
        mu_in = mu_out = 0.25
    return q2q_core_ref(x, mu_in, mu_out, alpha)


def fit_mu_ref(xs, fs, alpha, mu0):
    """Root of the score (scaled_nb.py:143-147) by Newton from mu0."""
    xs, fs, al = ([mpf(int(v)) for v in xs], [mpf(float(v)) for v in fs],
                  mpf(float(alpha)))
    m = mpf(mu0)
    for _ in range(60):
        S = sum((x - m * f) / (1 + al * m * f) for x, f in zip(xs, fs))
        dS = sum(-f * (1 + al * x) / (1 + al * m * f) ** 2
                 for x, f in zip(xs, fs))
        step = S / dS
        m -= step
        if abs(step) < mpf(10) ** -300 * m:
            return m
    raise RuntimeError('fit_mu_ref did not converge')


def host_fit_mu(xs, fs, alpha):
    n = len(xs)
    x = np.ascontiguousarray(xs, dtype=np.int32).reshape(1, n)
    f = np.ascontiguousarray(fs, dtype=np.float64).reshape(1, n)
    al = np.full((1, n), float(alpha))
    mu = np.empty(1)
    host().h3dt_fit_mu(ctypes.c_int64(1), n,
                       x.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                       f.ctypes.data_as(D), al.ctypes.data_as(D),
                       mu.ctypes.data_as(D))
    return mu[0]


def equalize_ref(xs, fs, alpha):
    """equalize (scaled_nb.py:186-214) for one pixel, the mu_out clamp
    carried from replicate to replicate (:209-213); None where a replicate
    has no finite exact reference."""
    mu = fit_mu_ref(xs, fs, alpha, host_fit_mu(xs, fs, alpha))
    f_mean = mp.exp(sum(mp.log(mpf(float(f))) for f in fs) / len(fs))
    mu_out = mu * f_mean
    out = []
    for x, f in zip(xs, fs):
        mu_in = mu * mpf(float(f))
        if not (mu_in >= 0.25 and mu_out >= 0.25):
            mu_in = mu_out = mpf(0.25)
        v = q2q_core_ref(int(x), mu_in, mu_out, alpha)
        if v is None:
            return None
        out.append(float(v))
    return out


def taylor_ref(a, xe, h):
    """(ratio, dint): P'(xe + h) / P'(xe) and (P(xe + h) - P(xe)) / P'(xe) =
    integral_0^h exp(g(s)) ds, g(s) = (a - 1) ln(1 + s / xe) - s."""
    a, xe, h = mpf(float(a)), mpf(float(xe)), mpf(float(h))

    def eg(s):
        return mp.exp((a - 1) * mp.log1p(s / xe) - s)
    with mp.workdps(40):
        return float(eg(h)), float(mp.quad(eg, [0, h / 2, h]))


def taylor_dint_by_definition(a, xe, h):
    P1, _, _ = igam_all(a, mpf(float(xe)) + mpf(float(h)))
    P0, _, fac = igam_all(a, xe)
    return float((P1 - P0) / (fac / rnd(xe)))


def exp_ref(x):
    """(hi, lo): e^x correctly rounded and (e^x - hi) in ulps of hi (in
    ulps, not as a second double: below 2^-1022 the remainder of a
    subnormal hi is not a double)."""
    if np.isnan(x):
        return np.nan, 0.0
    if np.isinf(x):
        return (np.inf if x > 0 else 0.0), 0.0
    v = mp.exp(mpf(float(x)))
    if v > mpf(2) ** 1024 * (1 - mpf(2) ** -54):
        return np.inf, 0.0
    hi = to_double(v)
    return hi, float((v - mpf(hi)) / mpf(float(np.spacing(hi))))


def ev(task):
    kind = task[0]
    if kind == 'pq':
        return tuple(to_double(v) for v in igam_all(task[1], task[2]))
    if kind == 'inv':
        return to_double(igam_inverse(task[1], task[2], task[3]))
    if kind == 'q2q':
        v = q2q_ref(*task[1:])
        return None if v is None else float(v)
    if kind == 'eq':
        return equalize_ref(task[1], task[2], task[3])
    if kind == 'ty':
        return taylor_ref(*task[1:])
    if kind == 'exp':
        return exp_ref(task[1])
    raise ValueError(kind)


# ---- the inputs ----------------------------------------------------------

EXP_RANGES = ((-1.0, 1.0), (-40.0, 40.0), (-700.0, 700.0), (700.0, 709.78),
              (-708.39, -700.0), (-745.13, -708.4))
EXP_EDGES = np.array([
    0.0, -0.0, 709.782712893384, np.nextafter(709.782712893384, np.inf),
    -745.13321910194111, np.nextafter(-745.13321910194111, -np.inf),
    np.inf, -np.inf, np.nan, 1e300, -1e300, 5e-324, -5e-324])


def f32(v):
    """rounded to float32 precision (the npz compresses the zero bits)."""
    return np.asarray(v, dtype=np.float32).astype(np.float64)


def f32m(v):
    """the significand rounded to 24 bits, the exponent kept (f32 would
    overflow below 1e-38): the npz compresses the zero bits."""
    m, e = np.frexp(np.asarray(v, dtype=np.float64))
    return np.ldexp(m.astype(np.float32).astype(np.float64), e)


def ulp_sides(v):
    return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]


def pq_edges():
    """(a, x) one ulp either side of (and on) every dispatch edge of
    igam_pq / igam_fac_l."""
    pts = []
    for x0 in (0.5, 1.0, 1.1):
        for a in (0.05, 0.3, 0.7, 1.0, 1.05, 2.5, 9.0):
            pts += [(a, x) for x in ulp_sides(x0)]
    for a in (0.2, 0.9, 1.5, 3.0, 7.5, 8.0, 20.0, 49.0, 50.0, 300.0, 5000.0,
              40000.0):
        pts += [(a, x) for x in ulp_sides(a)]
    for a in (0.1, 1.0, 3.0, 8.0, 30.0, 100.0, 1000.0, 3000.0):
        pts += [(a, x) for x in ulp_sides(1.5 * a + 5.0)]
    # tail 1 below the mean: the series from x < a - sqrt(a) / 2 on (a >= 8)
    for a in (8.0, 9.5, 30.0, 1000.0, 4e4):
        pts += [(a, x) for x in ulp_sides(a - 0.5 * np.sqrt(a))]
    for a in (0.3, 1.5, 2.7, 5.0, 7.9):
        pts += [(a, x) for x in ulp_sides(a + 3.0 * np.sqrt(a))]
        if a - 3.0 * np.sqrt(a) > 1.0:
            pts += [(a, x) for x in ulp_sides(a - 3.0 * np.sqrt(a))]
    for a in ulp_sides(8.0):
        pts += [(a, 8.0 + 2.7 * np.sqrt(8.0)), (a, 8.0), (a, 3.0)]
    for a in ulp_sides(50.0):
        pts += [(a, 35.0), (a, 50.0), (a, 65.0)]
    for a in (50.0, 60.0, 200.0, 5000.0):
        pts += [(a, x) for x in ulp_sides(0.6 * a)]
        pts += [(a, x) for x in ulp_sides(1.4 * a)]
    for x in (0.1, 0.3, 0.5):
        pts += [(a, x) for a in ulp_sides(-0.4 / np.log(x))]
    # the prefactor underflows: on the continued-fraction side (P = 1, Q =
    # 0) and on the series side (P = 0, Q = 1)
    pts += [(2000.0, 5000.0), (1e4, 2e4), (0.5, 800.0), (30.0, 1100.0),
            (300.0, 1.0), (2000.0, 900.0), (4e4, 3.5e4)]
    return np.array(pts)


def taylor_points(rng, n):
    """inside the window of igam_taylor_ok: n random points, then points just
    inside each of its three limits with both signs of h; and the same limit
    points just outside."""
    a = f32m(10 ** rng.uniform(-3, 4.7, n))
    xe = f32m(a * np.exp(rng.normal(0, 0.5, n)))
    umax = np.minimum(np.minimum(0.05, 0.4 / np.abs(a - 1 - xe)),
                      np.sqrt(0.25 / np.abs(a - 1)))
    h = f32m(xe * umax * rng.uniform(0.02, 0.98, n) * rng.choice([-1.0, 1.0], n))
    ins, outs = [], []
    # |u| = 0.05 binds: |a - 1 - xe| <= 8, |a - 1| <= 100
    lim_u = [(0.5, 0.3), (1.0, 2.0), (3.0, 2.5), (20.0, 15.0), (90.0, 95.0)]
    # |((a - 1) / xe - 1) h| = 0.4 binds
    lim_g = [(0.01, 30.0), (2.0, 40.0), (300.0, 200.0), (3000.0, 3300.0),
             (4e4, 3.9e4)]
    # |a - 1| u^2 = 0.25 binds: xe ~ a - 1 large
    lim_c = [(400.0, 399.5), (2500.0, 2498.0), (3e4, 3.0005e4)]
    for grp, fn in ((lim_u, lambda a_, x_: 0.05),
                    (lim_g, lambda a_, x_: 0.4 / abs(a_ - 1 - x_)),
                    (lim_c, lambda a_, x_: np.sqrt(0.25 / abs(a_ - 1)))):
        for a_, x_ in grp:
            u = fn(a_, x_)
            all_ = min(0.05, 0.4 / abs(a_ - 1 - x_), np.sqrt(0.25 / abs(a_ - 1))
                       if a_ != 1 else np.inf)
            assert abs(u - all_) <= 1e-12 * u, (a_, x_, u, all_)
            for sgn in (-1.0, 1.0):
                ins.append((a_, x_, sgn * u * x_ * (1 - 1e-6)))
                outs.append((a_, x_, sgn * u * x_ * (1 + 1e-6)))
    ins, outs = np.array(ins), np.array(outs)
    return (np.concatenate([a, ins[:, 0]]), np.concatenate([xe, ins[:, 1]]),
            np.concatenate([h, ins[:, 2]]), outs)


def q2q_candidates(rng, regime, n):
    if regime == 0:      # typical
        alpha = 10 ** rng.uniform(-4, np.log10(3.0), n)
        mu = 10 ** rng.uniform(np.log10(0.5), np.log10(2e4), n)
    elif regime == 1:    # deep tails
        alpha = 10 ** rng.uniform(-4, 0, n)
        mu = 10 ** rng.uniform(0.5, 4, n)
    elif regime == 2:    # small shapes and clamps
        alpha = 10 ** rng.uniform(-2, 2, n)
        mu = 10 ** rng.uniform(-1.5, 0.7, n)
    else:                # large shapes
        alpha = 10 ** rng.uniform(-4, -3, n)
        mu = 10 ** rng.uniform(np.log10(3e3), np.log10(3e4), n)
    mu_in = f32(mu * np.exp(rng.normal(0, 0.5, n)))
    mu_out = f32(mu * np.exp(rng.normal(0, 0.5, n)))
    alpha = f32(alpha)
    mi = np.maximum(mu_in, 0.25)
    sd = np.sqrt(mi * (1 + alpha * mi))
    if regime == 1:
        x = mi + rng.choice([-1.0, 1.0], n) * rng.uniform(4, 9, n) * sd
    elif regime == 2:
        x = rng.integers(1, 12, n).astype(float)
    else:
        x = rng.negative_binomial(1 / alpha, 1 / (1 + alpha * mi)).astype(float)
    x = np.round(x)
    x[~(x >= 1)] = 1.0
    return x, mu_in, mu_out, alpha


def eq_candidates(rng, r, n):
    alpha = f32(10 ** rng.uniform(-4, 0.5, n))
    mu = 10 ** rng.uniform(-0.5, np.log10(3e4), n)
    f = np.exp(rng.normal(0, 0.5, (n, r)))
    far = rng.random(n) < 0.15     # some size factors far apart
    f[far, 0] *= 1e-2
    f[far, r - 1] *= 1e2
    f = f32(f)
    mean = np.minimum(mu[:, None] * f, 3e4)
    x = rng.negative_binomial(1 / alpha[:, None], 1 / (1 + alpha[:, None] * mean))
    x = np.minimum(x, 30000)
    x[rng.random((n, r)) < 0.08] = 0   # some replicates zero
    x[x.sum(1) == 0, 0] = 1
    return x.astype(np.int32), f, alpha


def build_tasks(seed=20):
    rng = np.random.default_rng(seed)
    t = {}
    # exp: 150 per range and the edges
    ex = f32m(np.concatenate([rng.uniform(lo, hi, 80) for lo, hi in EXP_RANGES]))
    t['exp'] = [('exp', v) for v in np.concatenate([ex, EXP_EDGES])]
    # igam_pq: random, then the dispatch edges, then the kMaxIter probe
    a = f32m(10 ** rng.uniform(-3, 4.7, 400))
    x = f32m(a * np.exp(rng.normal(0, 0.5, 400)))
    a2 = f32m(10 ** rng.uniform(-3, 4.7, 250))
    x2 = a2 + rng.uniform(-8, 12, 250) * np.sqrt(a2)
    x2 = f32m(np.where(x2 > 0, x2, a2 * rng.uniform(0.01, 1, 250)))
    edges = pq_edges()
    probe_a = np.array([1000.0, 2000.0, 4000.0, 8000.0])
    pa = np.concatenate([a, a2, edges[:, 0], probe_a])
    px = np.concatenate([x, x2, edges[:, 1], 1.5 * probe_a + 4.9])
    t['pq'] = [('pq', u, v) for u, v in zip(pa, px)]
    t['pq_counts'] = (650, len(edges), 4)
    # igam_inv
    tasks = []
    for upper in (0, 1):
        a = f32m(10 ** rng.uniform(-3, 4.7, 250))
        # (lower tail: the root ~ (t Gamma(a + 1))^(1/a) stays above 1e-290)
        lo = np.where(upper == 1, -300.0, np.maximum(-300.0, -290.0 * a))
        tt = f32m(10 ** rng.uniform(lo, 0))
        tt = np.minimum(tt, 1 - 1e-16)
        tasks += [('inv', u, v, upper) for u, v in zip(a, tt)]
        for u in (0.3, 2.5, 40.0, 700.0, 2e4):
            tasks += [('inv', u, v, upper)
                      for v in ulp_sides(0.9) + [1 - 1e-16]]
    t['inv'] = tasks
    # where q2q_core's gated Wilson-Hilferty guess can be 5 % off: shapes 1 ..
    # 200, tails down to 1e-30 (test_igam_inv_with_and_without_a_guess)
    tasks = []
    for upper in (0, 1):
        a = f32m(10 ** rng.uniform(0, 2.3, 150))
        tt = np.minimum(f32m(10 ** rng.uniform(-30, 0, 150)), 1 - 1e-16)
        tasks += [('inv', u, v, upper) for u, v in zip(a, tt)]
    t['inv5'] = tasks
    # roots / slopes in the subnormal range (igam_inv's nrm == false steps)
    t['invsub'] = [('inv', 0.5, v, 0) for v in
                   (1e-140, 1e-150, np.nextafter(1e-150, 0),
                    np.nextafter(1e-150, 1), 1e-152, 1e-155)]
    t['invsub'] += [('inv', 1.0, 1e-305, 0), ('inv', 0.25, 1e-76, 0),
                    ('inv', 2.0, 1e-300, 0)]
    ta, txe, th, touts = taylor_points(rng, 300)
    t['ty'] = [('ty', u, v, w) for u, v, w in zip(ta, txe, th)]
    t['tyout'] = touts
    for reg, n in ((0, 800), (1, 400), (2, 400), (3, 400)):
        c = q2q_candidates(rng, reg, int(n * 1.5))
        t['q2q%d' % reg] = [('q2q', *v) for v in zip(*c)]
        t['q2q%d_n' % reg] = n
    for r in (2, 3, 8):
        xs, f, al = eq_candidates(rng, r, 400)
        t['eq%d' % r] = [('eq', xs[i], f[i], al[i]) for i in range(len(al))]
    return t


def self_check():
    """the series against mp.gammainc where that converges, and the two
    definitions of the Taylor increment against each other."""
    rng = np.random.default_rng(1)
    for a, x in zip(10 ** rng.uniform(-3, 2, 12), 10 ** rng.uniform(-2, 2, 12)):
        P, Q, _ = igam_all(a, x)
        with mp.workdps(80):
            a_, x_ = mpf(float(a)), mpf(float(x))
            assert abs(mp.gammainc(a_, 0, x_, regularized=True) / P - 1) < 1e-40
            assert abs(mp.gammainc(a_, x_, mp.inf, regularized=True) / Q - 1) < 1e-40
    for a, xe, h in ((2.5, 3.0, 0.1), (300.0, 200.0, -0.7), (0.01, 30.0, 0.3)):
        _, d = taylor_ref(a, xe, h)
        assert abs(taylor_dint_by_definition(a, xe, h) / d - 1) < 1e-15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--jobs', type=int, default=os.cpu_count() or 1)
    args = ap.parse_args()
    host()
    self_check()
    t = build_tasks()
    with multiprocessing.Pool(args.jobs) as pool:
        def run(key):
            res = pool.map(ev, t[key], chunksize=4)
            print(key, len(res), file=sys.stderr)
            return res
        out = {}
        r = np.array(run('exp'))
        ex = np.array([v[1] for v in t['exp']])
        ne = len(EXP_EDGES)
        out.update(exp_x=ex[:-ne], exp_hi=r[:-ne, 0], exp_lo=r[:-ne, 1],
                   exp_edge_x=ex[-ne:], exp_edge_ref=r[-ne:, 0])
        r = np.array(run('pq'))
        out.update(pq_a=np.array([v[1] for v in t['pq']]),
                   pq_x=np.array([v[2] for v in t['pq']]), pq_P=r[:, 0],
                   pq_Q=r[:, 1], pq_fac=r[:, 2],
                   pq_counts=np.array(t['pq_counts']))
        for key in ('inv', 'inv5', 'invsub'):
            out.update({key + '_a': np.array([v[1] for v in t[key]]),
                        key + '_t': np.array([v[2] for v in t[key]]),
                        key + '_upper': np.array([v[3] for v in t[key]],
                                                 dtype=np.int8),
                        key + '_root': np.array(run(key))})
        r = np.array(run('ty'))
        out.update(ty_a=np.array([v[1] for v in t['ty']]),
                   ty_xe=np.array([v[2] for v in t['ty']]),
                   ty_h=np.array([v[3] for v in t['ty']]), ty_ratio=r[:, 0],
                   ty_dint=r[:, 1], tyout=t['tyout'])
        cols, regs = [], []
        for reg in range(4):
            key = 'q2q%d' % reg
            res = run(key)
            keep = [(*task[1:], v) for task, v in zip(t[key], res)
                    if v is not None][:t[key + '_n']]
            assert len(keep) == t[key + '_n'], (key, len(keep))
            cols += keep
            regs += [reg] * len(keep)
        cols = np.array(cols)
        out.update(q2q_x=cols[:, 0], q2q_mu_in=cols[:, 1],
                   q2q_mu_out=cols[:, 2], q2q_alpha=cols[:, 3],
                   q2q_ref=cols[:, 4], q2q_regime=np.array(regs, dtype=np.int8))
        for rr in (2, 3, 8):
            key = 'eq%d' % rr
            res = run(key)
            keep = [(task, v) for task, v in zip(t[key], res)
                    if v is not None][:300]
            assert len(keep) == 300, (key, len(keep))
            out.update({key + '_x': np.array([k[0][1] for k in keep],
                                             dtype=np.int32),
                        key + '_f': np.array([k[0][2] for k in keep]),
                        key + '_alpha': np.array([k[0][3] for k in keep]),
                        key + '_ref': np.array([k[1] for k in keep])})
    np.savez_compressed(OUT, **out)
    print('wrote %s: %d bytes' % (OUT, os.path.getsize(OUT)), file=sys.stderr)


if __name__ == '__main__':
    main()
