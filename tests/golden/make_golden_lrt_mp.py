"""Exact references for the per-pixel LRT (lrt.py:7-50), written to
tests/golden/unit_lrt_mp.npz; read by tests/lrt_mp_cases.py (the GPU kernels
in test_gpu_lrt_edges.py, the host / self-test builds in
test_lrt_mp_host.py).

Needs mpmath (1.3.0); the tests read only the npz
(test_fixture_subsample_recomputed recomputes 60 pixels where mpmath is
installed). Run from the repository root:

    python tests/golden/make_golden_lrt_mp.py [--jobs N]

Per pixel, at mp.dps = 70:

- the root in theta = log mu of the score sum_k (x_k - mu b_k) / (1 + a_k mu
  b_k) (scaled_nb.py:143-147 times mu), for the null fit and each
  condition's fit: bracketed by unit steps from log(sum x / sum b), then
  mp.findroot (illinois) and Newton steps until one is below 1e-55;
- llr = sum(null logpmf row) - sum(alt logpmf row), the rows by
  scaled_nb.py:12-33 with mp.loggamma;
- p = Q((C - 1) / 2, -llr), p = 1 where -2 llr <= 0 (Q by the upward
  recurrence Q(a + 1, x) = Q(a, x) + x^a e^-x / Gamma(a + 1) from erfc(sqrt
  x) or e^-x: positive terms only);
- the same llr and p at the refit_mu=False means mean(x / f);
- S, the llr conditioning scale (lrt_mp_cases.llr_bound), rounded up to
  float32.

The inputs are stored (numpy's distribution streams are not a contract),
f and the dispersions rounded to float32 precision so that the file
compresses. A pixel whose score has no finite root is redrawn; the count is
stored and at most 2 % of a cell may be redrawn.

The generator asserts, on every pixel and in both modes, that a plain numpy
float64 evaluation of the simplified llr (csrc/h3d_model.h, lrt_pixel) at the
mp means rounded to double meets the llr bound (8 + R) 2.2e-16 S, and that
scipy.stats.chi2.sf agrees with mp at every fixture x2 within igam_err's
tolerance (the tests use scipy as the tail function) -- except where scipy
returns 0 for a subnormal p (its igamc gives up once the prefactor's exponent
is below -709.78; counted in *_sf_flushed), which is why the ends of the
interval the llr bound leaves p, Q(-llr_mp +- B), are stored from mp too.
It stores the errors of oracle.lrt against mp per (family, design) for the
record, and stops if that record is not finite.
"""
import argparse
import multiprocessing
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'unit_lrt_mp.npz')
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from lrt_mp_cases import (DESIGNS, FAMILIES, NPIX, SUBNORMAL,  # noqa: E402
                          llr_bound, llr_simple, scale_S)

mp.mp.dps = 70
mpf = mp.mpf


def f32m(v):
    """the significand rounded to 24 bits, the exponent kept."""
    m, e = np.frexp(np.asarray(v, dtype=np.float64))
    return np.ldexp(m.astype(np.float32).astype(np.float64), e)


def up32(v):
    """v rounded up to a float32 (as a double)."""
    w = np.float32(v)
    if float(w) < v:
        w = np.nextafter(w, np.float32(np.inf))
    return float(w)


def to_double(v):
    """v correctly rounded to a double (float(mpf) rounds a subnormal result
    twice)."""
    if v != 0 and abs(v) < mpf(2) ** -1022:
        return float(np.ldexp(float(int(mp.nint(mp.ldexp(v, 1074)))), -1074))
    return float(v)


# ---- the exact LRT -------------------------------------------------------

def score_root(xs, bs, al):
    """theta with sum (x - mu b) / (1 + a mu b) = 0, mu = e^theta; None where
    no sign change is found within e^+-1500 of sum x / sum b."""
    def g(th):
        mu = mp.exp(th)
        return mp.fsum((x - mu * b) / (1 + a * mu * b)
                       for x, b, a in zip(xs, bs, al))

    def dg(th):
        mu = mp.exp(th)
        return -mp.fsum(mu * b * (1 + a * x) / (1 + a * mu * b) ** 2
                        for x, b, a in zip(xs, bs, al))
    sx = mp.fsum(xs)
    if not sx > 0:
        return None
    lo = hi = mp.log(sx / mp.fsum(bs))
    for _ in range(1500):
        if g(lo) > 0:
            break
        lo -= 1
    else:
        return None
    for _ in range(1500):
        if g(hi) < 0:
            break
        hi += 1
    else:
        return None
    th = mp.findroot(g, (lo, hi), solver='illinois', tol=mpf(10) ** -40,
                     verify=False)
    for _ in range(8):
        step = g(th) / dg(th)
        th -= step
        if abs(step) < mpf(10) ** -55:
            return th
    raise RuntimeError('score_root did not converge')


def q_half_integer(df, x):
    """Q(df / 2, x), x > 0."""
    if df % 2:
        q, a = mp.erfc(mp.sqrt(x)), mpf(1) / 2
    else:
        q, a = mp.exp(-x), mpf(1)
    while 2 * a < df:
        q += mp.exp(a * mp.log(x) - x - mp.loggamma(a + 1))
        a += 1
    return q


def lrt_exact(raw, f, disp, cond, C):
    """One pixel: None where a score has no finite root."""
    R = len(raw)
    xs = [mpf(int(v)) for v in raw]
    fs = [mpf(float(v)) for v in f]
    al = [mpf(float(disp[c])) for c in cond]
    rs = [1 / a for a in al]
    ths = []
    for t in range(C + 1):
        idx = [k for k in range(R) if t == 0 or cond[k] == t - 1]
        th = score_root([xs[k] for k in idx], [fs[k] for k in idx],
                        [al[k] for k in idx])
        if th is None:
            return None
        ths.append(th)
    mus = [mp.exp(th) for th in ths]
    nr = []
    for t in range(C + 1):
        idx = [k for k in range(R) if t == 0 or cond[k] == t - 1]
        nr.append(mp.fsum(xs[k] / fs[k] for k in idx) / len(idx))
    # the terms of a logpmf row that do not depend on the mean
    const = [mp.loggamma(r + x) - mp.loggamma(x + 1) - mp.loggamma(r)
             + r * mp.log(r) for x, r in zip(xs, rs)]

    def row_sum(means):
        tot = mpf(0)
        for k in range(R):
            m = means[k] * fs[k]
            tot += (const[k] - rs[k] * mp.log(rs[k] + m) + xs[k] * mp.log(m)
                    - xs[k] * mp.log(rs[k] + m))
        return tot

    out = {}
    for tag, m in (('', mus), ('_nr', nr)):
        m0, m1 = m[0], m[1:]
        llr = row_sum([m0] * R) - row_sum([m1[c] for c in cond])
        p = q_half_integer(C - 1, -llr) if -2 * llr > 0 else mpf(1)
        S = mpf(0)
        for k in range(R):
            S += xs[k] * abs(mp.log(m0 / m1[cond[k]]))
            S += (rs[k] + xs[k]) * (abs(mp.log(
                (rs[k] + m0 * fs[k]) / (rs[k] + m1[cond[k]] * fs[k]))) + 1)
        # the ends of the interval the llr bound B leaves p
        Sf = up32(float(S))
        B = mpf(float(llr_bound(R, Sf)))
        out['p_lo' + tag] = to_double(q_half_integer(C - 1, -llr + B)) \
            if -llr + B > 0 else 1.0
        out['p_hi' + tag] = to_double(q_half_integer(C - 1, -llr - B)) \
            if -llr - B > 0 else 1.0
        out['mu0' + tag] = float(m0)
        out['mu1' + tag] = [float(v) for v in m1]
        out['llr' + tag] = float(llr)
        out['p' + tag] = to_double(p)
        out['lnp' + tag] = float(mp.log(p))
        out['S' + tag] = Sf
    return out


def ev(task):
    return lrt_exact(*task)


# ---- the inputs ----------------------------------------------------------

def loguni(rng, lo, hi, size):
    return 10 ** rng.uniform(np.log10(lo), np.log10(hi), size)


def draw(family, rng, n, cond, C):
    """raw (n, R) int64, f (n, R), disp (n, C): NB draws (gamma-Poisson) at
    the family's mean and dispersion."""
    R = len(cond)
    fold = np.ones((n, C))
    if family == 'benign':   # test_lrt_wide_designs_vs_oracle's ranges
        f = np.exp(rng.normal(0, 0.3, (n, R)))
        mu = rng.gamma(2.0, 20.0, n)
        a = rng.uniform(0.01, 0.3, (n, C))
    elif family == 'sparse':
        f = loguni(rng, 0.1, 10, (n, R))
        mu = loguni(rng, 1e-2, 1, n)
        a = loguni(rng, 1e-3, 3, (n, C))
    elif family == 'large':
        f = loguni(rng, 0.3, 3, (n, R))
        mu = loguni(rng, 1e5, 3e7, n)
        a = loguni(rng, 1e-4, 1e-1, (n, C))
    elif family == 'lowdisp':
        f = np.exp(rng.normal(0, 0.3, (n, R)))
        mu = loguni(rng, 1, 1e4, n)
        a = loguni(rng, 1e-7, 1e-4, (n, C))
    elif family == 'highdisp':
        f = np.exp(rng.normal(0, 0.3, (n, R)))
        mu = loguni(rng, 1, 1e3, n)
        a = loguni(rng, 1, 10, (n, C))
    elif family == 'widef':
        f = loguni(rng, 1e-3, 1e3, (n, R))
        f[:, 0], f[:, R - 1] = 1e-3, 1e3    # the whole range in every pixel
        mu = loguni(rng, 1, 1e3, n)
        a = rng.uniform(0.01, 0.3, (n, C))
    elif family == 'differential':
        f = np.exp(rng.normal(0, 0.3, (n, R)))
        mu = loguni(rng, 100, 1e5, n)
        a = rng.uniform(0.01, 0.3, (n, C))
        fold = loguni(rng, 1e-3, 1e3, (n, C))
    else:
        raise ValueError(family)
    f, a = f32m(f), f32m(a)
    mean = mu[:, None] * fold[:, cond] * f
    if family == 'large':
        mean = np.minimum(mean, 1e8)
    aw = a[:, cond]
    raw = rng.poisson(rng.gamma(1 / aw, aw * mean)).astype(np.int64)
    raw = np.minimum(raw, 2 ** 31 - 1)
    for c in range(C):   # no all-zero condition (the MLE has no root)
        first = np.flatnonzero(cond == c)[0]
        raw[raw[:, cond == c].sum(axis=1) == 0, first] = 1
    return raw, f, a


def make_cond(rng, R, C):
    """C conditions over R shuffled replicates, of unequal sizes unless
    C = R."""
    while True:
        cond = np.sort(np.r_[np.arange(C), rng.integers(0, C, R - C)])
        if C == R or len(set(np.bincount(cond))) > 1:
            break
    rng.shuffle(cond)
    return cond.astype(np.int32)


def q_check():
    """q_half_integer against mp.gammainc."""
    for df in range(1, 8):
        for x in (1e-7, 0.3, 2.0, 40.0, 700.0):
            want = mp.gammainc(mpf(df) / 2, mpf(x), mp.inf, regularized=True)
            assert abs(q_half_integer(df, mpf(x)) / want - 1) < mpf(10) ** -50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--jobs', type=int, default=os.cpu_count() or 1)
    args = ap.parse_args()
    import scipy.stats as stats
    import oracle
    from test_special_host import igam_err
    q_check()
    rng = np.random.default_rng(20)
    out = {}
    with multiprocessing.Pool(args.jobs) as pool:
        for R, C in DESIGNS:
            key = 'R%dC%d' % (R, C)
            cond = make_cond(rng, R, C)
            design = np.eye(C, dtype=bool)[cond]
            cols = {}
            redraws = np.zeros(len(FAMILIES), dtype=np.int32)
            orc = np.full((len(FAMILIES), 4), np.nan)
            flushed = np.zeros(len(FAMILIES), dtype=np.int32)
            for fi, fam in enumerate(FAMILIES):
                raw, f, a = draw(fam, rng, NPIX, cond, C)
                res = pool.map(ev, [(raw[i], f[i], a[i], cond, C)
                                    for i in range(NPIX)], chunksize=1)
                for i in range(NPIX):
                    while res[i] is None:
                        redraws[fi] += 1
                        r1, f1, a1 = draw(fam, rng, 1, cond, C)
                        raw[i], f[i], a[i] = r1[0], f1[0], a1[0]
                        res[i] = lrt_exact(raw[i], f[i], a[i], cond, C)
                assert redraws[fi] <= 0.02 * NPIX, (key, fam, redraws[fi])
                cell = dict(raw=raw, f=f, disp=a)
                for name in res[0]:
                    cell[name] = np.array([r[name] for r in res])
                aw = a[:, cond]
                for tag in ('', '_nr'):
                    # an independent float64 evaluation meets the llr bound
                    got = llr_simple(raw, f, aw, cond, cell['mu0' + tag],
                                     cell['mu1' + tag])
                    S = scale_S(raw, f, aw, cond, cell['mu0' + tag],
                                cell['mu1' + tag])
                    assert np.all(S <= cell['S' + tag] * (1 + 1e-6))
                    B = llr_bound(R, cell['S' + tag])
                    frac = np.abs(got - cell['llr' + tag]) / B
                    assert frac.max() <= 1, (key, fam, tag, frac.max())
                    # scipy's tail function at the fixture's x2
                    x2 = -2 * cell['llr' + tag]
                    pos = x2 > 0
                    sf = stats.chi2.sf(x2[pos], C - 1)
                    pm = cell['p' + tag][pos]
                    # (scipy's igamc returns 0 once its prefactor's exponent
                    # is below -709.78: no stand-in for a subnormal p)
                    pos2 = ~((sf == 0) & (pm < SUBNORMAL))
                    flushed[fi] += int((~pos2).sum())
                    assert igam_err(sf[pos2], pm[pos2],
                                    np.full(pos2.sum(), (C - 1) / 2),
                                    x2[pos][pos2] / 2) < 1, (key, fam, tag)
                # the float64 restatement against mp, for the record
                with np.errstate(all='ignore'):
                    op, ollr, om0, om1 = oracle.lrt(raw, f, aw, design)
                ok = (cell['p'] >= 1e-300) & (-2 * cell['llr'] >= 1e-6)
                assert ok.any()
                orc[fi] = (
                    np.max(np.abs(op[ok] / cell['p'][ok] - 1)),
                    np.max(np.abs(ollr - cell['llr'])
                           / llr_bound(R, cell['S'])),
                    np.max(np.abs(om0 / cell['mu0'] - 1)),
                    np.max(np.abs(om1 / cell['mu1'] - 1)))
                assert np.all(np.isfinite(orc[fi])), (key, fam, orc[fi])
                for name, v in cell.items():
                    cols.setdefault(name, []).append(v)
                print(key, fam, 'redraws', redraws[fi], 'oracle', orc[fi],
                      file=sys.stderr)
            out[key + '_cond'] = cond
            out[key + '_redraws'] = redraws
            out[key + '_oracle_err'] = orc
            out[key + '_sf_flushed'] = flushed
            for name, v in cols.items():
                v = np.stack(v)
                if name.startswith(('S', 'lnp')):
                    v = v.astype(np.float32)
                out[key + '_' + name] = v
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print('wrote %s: %d bytes' % (OUT, size), file=sys.stderr)
    assert size < 1000000


if __name__ == '__main__':
    main()
