"""Exact references for the CML dispersion search (dispersion.py:46-80),
written to tests/golden/unit_cml_mp.npz; read by tests/cml_mp_cases.py (the
per-pixel NLL term through the host / self-test builds in
test_cml_mp_host.py, the Brent kernels and drivers in
test_gpu_cml_exact.py).

Needs mpmath (1.3.0); the tests read only the npz. Run from the repository
root:

    python tests/golden/make_golden_cml_mp.py [--jobs N]

Every draw comes from a generator seeded by its own case, and the archive is
written with fixed member dates: the same bytes on every run, whatever
``--jobs`` is. mp.dps = 50 throughout.

**Term cases** (cml_mp_cases.TERM_N x TERM_FAMILIES x 32 pixels x
term_deltas()). Per pixel and delta, with r = 1 / delta - 1 in double as
nll_const rounds it and everything after that exact: the term sum_j lgamma(d_j
+ r) + lgamma(n r) - lgamma(z + n r) - n lgamma(r), rounded to double, and the
scale S (cml_mp_cases' docstring), rounded down to float32.

**Segment cases** (cml_mp_cases.seg_cases()). f(delta) = -(sum of the
pixel terms), delta real. Stored per case: the data, and ``_ref`` = (delta_star,
E, lo, hi, oracle, f1_err):

- delta_star, the minimiser of f on [1e-4, 100/101]: an end where f' does
  not change sign inside, otherwise the root of f' (digamma sums) by
  bisection to 1e-11;
- E = sum_i 32 eps S_i + eps n_pixels sum_i |term_i| at delta_star;
- lo, hi: the ends of {delta : f(delta) <= f(delta_star) + 2 E} by bisection
  to 1e-12 (the inner point of the last bracket), or the interval's end;
- oracle: delta of oracle.cml on the same data (for the record);
- f1_err: for the integer-count families of the f = 1 runs, the largest
  |equalize(x, 1, disp) - x| / max(x, 1e-3) of oracle.equalize at the exact
  optimum and 1e-4 to either side of it, which is where the qcml iteration
  that ends the loop equalizes (NaN elsewhere). Relative to x for every
  count >= 1; a zero count may come back as rounding noise (~1e-14), which
  the 1e-3 floor holds to 1e-12 absolute, test_q2q_vs_goldens' atol.
  (Earlier iterations only choose where the last one starts. ``over`` is
  not among these families: cml_mp_cases.QCML_FAMILIES says why.)

Asserted for every case kept (conditions, not measurements):

- hi - lo <= tol2(delta_star);
- f is unimodal on a 200-point geometric grid over the interval;
- lo - tol2 <= oracle <= hi + tol2;
- f1_err <= 1e-9;
- ``under`` has f'(1e-4) >= 0 and ``ceiling`` f'(100/101) <= 0 (minimisers
  on the bounds); ``poisson`` is redrawn until oracle.cml lands in [4e-4,
  9e-4] (an interior minimiser next to the lower bound).

``large`` starts at means around 1e6 and is lowered by factors of ~3 until
every replicate count meets the flat-region condition: at 1e6 the log-gammas
are ~1e7 and 32 eps of them, over 65 pixels, is a flat region wider than
tol2. The mean used is stored (``seg_large_mean``) and printed. A (family, n)
whose condition cannot be met is not written and is listed in
``seg_dropped``; the generator stops if more than one family is touched.
"""
import argparse
import io
import multiprocessing
import os
import sys
import zipfile

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'unit_cml_mp.npz')
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cml_mp_cases as cc  # noqa: E402

mp.mp.dps = 50
mpf = mp.mpf
EPS = mpf(cc.EPS)
A, B = mpf(cc.BRENT_A), mpf(cc.BRENT_B)
LARGE_MEANS = (1e6, 3e5, 1e5, 3e4, 1e4, 3e3, 1e3, 300.)


def down32(v):
    """v rounded down to a float32"""
    w = np.float32(v)
    if float(w) > v:
        w = np.nextafter(w, np.float32(-np.inf))
    return w


def rng_for(*key):
    return np.random.default_rng([20, 46] + [int(k) for k in key])


def lg1(v):
    return max(mpf(1), abs(v))


# ---- term cases ------------------------------------------------------------

def term_data(fi, n):
    fam = cc.TERM_FAMILIES[fi]
    rng = rng_for(1, fi, n)
    shape = (cc.NPIX, n)
    if fam == 'zeros':
        d = np.zeros(shape)
    elif fam == 'tiny':       # equalize returns such values for a zero count
        d = 10 ** rng.uniform(-17, -6, shape)
    elif fam == 'sparse':
        d = rng.choice([0., 1., 2., 3.], size=shape, p=[.8, .1, .06, .04])
    elif fam == 'frac':
        d = rng.gamma(0.7, 3.0, shape)
    elif fam == 'benign':
        d = rng.gamma(2.0, 60.0, shape)
    elif fam == 'large':
        d = 10 ** rng.uniform(5, 7, shape)
    elif fam == 'mixed':      # 0 to 1e6 inside one pixel
        d = np.where(rng.random(shape) < 0.25, 0., 10 ** rng.uniform(-6, 6, shape))
        if n >= 2:
            d[:, 0], d[:, n - 1] = 0., 1e6
    else:
        raise ValueError(fam)
    return np.ascontiguousarray(d, dtype=np.float64)


def term_exact(row, r, n):
    """(term, S) of one pixel at the double r"""
    r = mpf(float(r))
    nr = n * r
    ds = [mpf(float(v)) for v in row]
    z = mp.fsum(ds)
    lgd = [mp.loggamma(d + r) for d in ds]
    lnr, lz, lr = mp.loggamma(nr), mp.loggamma(z + nr), mp.loggamma(r)
    term = mp.fsum(lgd) + lnr - lz - n * lr
    if z == 0 or n == 1:
        # the four groups cancel identically (mp leaves ~1e-49 of rounding)
        assert abs(term) < mpf(10) ** -40
        term = mpf(0)
    S = mp.fsum(lg1(v) for v in lgd) + lg1(lz) + lg1(lnr) + n * lg1(lr)
    return term, S


def term_job(n):
    deltas = cc.term_deltas()
    nf = len(cc.TERM_FAMILIES)
    data = np.stack([term_data(fi, n) for fi in range(nf)])
    want = np.empty((nf, len(deltas), cc.NPIX))
    S = np.empty((nf, len(deltas), cc.NPIX), dtype=np.float32)
    for fi in range(nf):
        for di, delta in enumerate(deltas):
            r = cc.r_of(delta)
            for i in range(cc.NPIX):
                t, s = term_exact(data[fi, i], r, n)
                want[fi, di, i] = float(t)
                S[fi, di, i] = down32(float(s))
    # all-zero pseudodata and n = 1: exactly 0
    assert np.all(want[0] == 0)
    if n == 1:
        assert np.all(want == 0)
    return n, data, want, S


# ---- segment cases ---------------------------------------------------------

def nb(rng, mean, disp):
    size = 1. / disp
    return rng.negative_binomial(size, size / (size + mean))


def seg_draw(fam, n, length, large_mean, attempt=0):
    fi = cc.SEG_FAMILIES.index(fam)
    rng = rng_for(2, fi, n, length, attempt)
    if fam == 'frac':
        return np.ascontiguousarray(rng.gamma(0.7, 3.0, (length, n)))

    def draw():
        mu = rng.uniform(20., 200., (length, 1)) * np.ones((1, n))
        if fam == 'benign':
            return nb(rng, mu, 0.02)
        if fam == 'over':
            return nb(rng, mu, 2.)
        if fam == 'huge':
            return nb(rng, mu, 30.)
        if fam == 'poisson':
            return rng.poisson(mu)
        if fam == 'under':
            return np.round(mu) + rng.integers(0, 2, (length, n))
        if fam == 'ceiling':
            d = np.where(rng.random((length, n)) < 0.03, 10000, 0)
            d[0, 0], d[length // 2, n - 1] = 10000, 10000
            d[0, 1:], d[length // 2, :n - 1] = 0, 0
            return d
        if fam == 'sparse':
            return nb(rng, 0.3 * np.ones((length, n)), 2.)
        if fam == 'large':
            return nb(rng, mu * (large_mean / 110.), 0.02)
        raise ValueError(fam)

    d = draw()
    if fam in cc.QCML_FAMILIES:
        # no all-zero pixel, as the pipeline's own filter leaves none: the
        # mean fit of the equalize pass has no root there (kFlagNoRoot), and
        # such a pixel's term is exactly 0 at every delta
        while True:
            bad = d.sum(axis=1) == 0
            if not bad.any():
                break
            d[bad] = draw()[bad]
    d = np.ascontiguousarray(d, dtype=np.int64)
    assert d.min() >= 0 and d.max() < 2 ** 31
    return d


class Objective:
    """f and the sign-carrying part of f' over one segment, the equal
    arguments of its log-gammas evaluated once"""

    def __init__(self, data):
        self.L, self.n = data.shape
        self.rows = [[mpf(float(v)) for v in row] for row in data]
        self.z = [mp.fsum(row) for row in self.rows]
        self.du, self.zu = {}, {}
        for row in self.rows:
            for v in row:
                self.du[v] = self.du.get(v, 0) + 1
        for v in self.z:
            self.zu[v] = self.zu.get(v, 0) + 1

    def total(self, delta, fn):
        r = 1 / delta - 1
        n, L = self.n, self.L
        nr = n * r
        return (mp.fsum(c * fn(v + r) for v, c in self.du.items())
                + L * fn(nr)
                - mp.fsum(c * fn(v + nr) for v, c in self.zu.items())
                - L * n * fn(r))

    def f(self, delta):
        return -self.total(delta, mp.loggamma)

    def slope(self, delta):
        """the sign of f'(delta): d(sum of terms) / dr, since dr / ddelta =
        -1 / delta^2. (The four groups' r-derivatives: psi(d + r), n psi(n
        r), n psi(z + n r), n psi(r).)"""
        r = 1 / delta - 1
        n, L = self.n, self.L
        nr = n * r
        psi = mp.digamma
        return (mp.fsum(c * psi(v + r) for v, c in self.du.items())
                + L * n * psi(nr)
                - n * mp.fsum(c * psi(v + nr) for v, c in self.zu.items())
                - L * n * psi(r))

    def noise(self, delta):
        """E at delta"""
        r = 1 / delta - 1
        n = self.n
        nr = n * r
        lgd = {v: mp.loggamma(v + r) for v in self.du}
        lgz = {v: mp.loggamma(v + nr) for v in self.zu}
        lnr, lr = mp.loggamma(nr), mp.loggamma(r)
        sS, sT = mpf(0), mpf(0)
        for row, z in zip(self.rows, self.z):
            sS += (mp.fsum(lg1(lgd[v]) for v in row) + lg1(lgz[z]) + lg1(lnr)
                   + n * lg1(lr))
            sT += abs(mp.fsum(lgd[v] for v in row) + lnr - lgz[z] - n * lr)
        return cc.TERM_UNITS * EPS * sS + EPS * self.L * sT


def bisect(fn, inside, outside, width):
    """fn(inside) true, fn(outside) false: the last inside point once the
    bracket is below width"""
    while abs(outside - inside) > width:
        mid = (inside + outside) / 2
        if fn(mid):
            inside = mid
        else:
            outside = mid
    return inside


def level_end(obj, ds, level, end):
    """the end of {f <= level} on the side of ``end``"""
    if obj.f(end) <= level:
        return end
    sgn = 1 if end > ds else -1
    step = mpf(10) ** -8
    inside = ds
    while True:
        x = ds + sgn * step
        if sgn * (x - end) >= 0:
            outside = end
            break
        if obj.f(x) > level:
            outside = x
            break
        inside = x
        step *= 4
    return bisect(lambda x: obj.f(x) <= level, inside, outside,
                  mpf(10) ** -12)


def solve(data, grid=True):
    """dict of the stored values and the conditions' figures"""
    obj = Objective(data)
    sa, sb = obj.slope(A), obj.slope(B)
    if sa >= 0:
        ds = A
    elif sb <= 0:
        ds = B
    else:
        # slope < 0 at `inside`: the last point with f still falling
        ds = bisect(lambda x: obj.slope(x) < 0, A, B, mpf(10) ** -11)
    E = obj.noise(ds)
    level = obj.f(ds) + 2 * E
    lo, hi = level_end(obj, ds, level, A), level_end(obj, ds, level, B)
    out = dict(delta_star=float(ds), E=float(E), lo=float(lo), hi=float(hi),
               slope_a=float(sa), slope_b=float(sb),
               flat_ok=bool(hi - lo <= cc.tol2(float(ds))))
    if grid:
        xs = [A * (B / A) ** (mpf(k) / 199) for k in range(200)]
        fs = [obj.f(x) for x in xs]
        rising = False
        uni = True
        for f0, f1 in zip(fs, fs[1:]):
            if f1 > f0:
                rising = True
            elif f1 < f0 and rising:
                uni = False
        out['unimodal'] = uni
    return out


def oracle_delta(data):
    import oracle
    with np.errstate(all='ignore'):
        disp = oracle.cml(data.astype(np.float64))
    return disp / (1. + disp)


def f1_error(data, delta_star):
    import oracle
    x = data.astype(np.float64)
    worst = 0.
    at = delta_star / (1. - delta_star)
    for disp in (at, at + 1e-4, max(at - 1e-4, 0.5 * at)):
        with np.errstate(all='ignore'):
            eq = oracle.equalize(data, np.ones_like(x), disp)
        worst = max(worst, float(np.max(np.abs(eq - x) / np.maximum(x, 1e-3))))
    return worst


def seg_job(task):
    fam, n, length, large_mean, full = task
    attempt = 0
    data = seg_draw(fam, n, length, large_mean)
    if fam == 'poisson':
        while not 4e-4 <= oracle_delta(data) <= 9e-4:
            attempt += 1
            assert attempt < 2000, (fam, n)
            data = seg_draw(fam, n, length, large_mean, attempt)
    res = solve(data, grid=full)
    res.update(family=fam, n=n, length=length, data=data, redraws=attempt)
    if not full:
        return res
    res['oracle'] = oracle_delta(data)
    t = cc.tol2(res['oracle'])
    res['oracle_ok'] = bool(res['lo'] - t <= res['oracle'] <= res['hi'] + t)
    res['f1_err'] = (f1_error(data, res['delta_star'])
                     if fam in cc.QCML_FAMILIES else np.nan)
    return res


# ---- the archive -----------------------------------------------------------

def write_npz(path, arrays):
    """np.savez_compressed with fixed member dates (numpy stamps the time of
    the run)"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for name, arr in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr),
                                      allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--jobs', type=int, default=os.cpu_count() or 1)
    args = ap.parse_args()
    out = {'term_deltas': cc.term_deltas()}
    for r0, k in ((5., 2), (10., 5), (20., 8)):
        below, at, above = (cc.r_of(d) for d in out['term_deltas'][k:k + 3])
        assert below < r0 <= at < above, (r0, below, at, above)
    with multiprocessing.Pool(args.jobs) as pool:
        # the largest `large` mean at which every replicate count's flat
        # region fits tol2
        large_mean = None
        for mean in LARGE_MEANS:
            res = pool.map(seg_job, [('large', n, cc.SEG_LEN, mean, False)
                                     for n in cc.SEG_N], chunksize=1)
            width = max(r['hi'] - r['lo'] for r in res)
            print('large at mean %g: widest flat region %.3g (tol2 %.3g)'
                  % (mean, width, cc.tol2(res[0]['delta_star'])),
                  file=sys.stderr)
            if all(r['flat_ok'] for r in res):
                large_mean = mean
                break
        assert large_mean is not None
        out['seg_large_mean'] = np.float64(large_mean)

        tasks = [(fam, n, ln, large_mean, True) for fam, n, ln in cc.seg_cases()]
        # (the long and wide cases first: they take longest)
        order = sorted(range(len(tasks)),
                       key=lambda i: -tasks[i][1] * tasks[i][2])
        seg_async = pool.map_async(seg_job, [tasks[i] for i in order],
                                   chunksize=1)
        for n, data, want, S in pool.map(term_job, cc.TERM_N, chunksize=1):
            out['term_n%d_data' % n] = data
            out['term_n%d_want' % n] = want
            out['term_n%d_S' % n] = S
            print('terms n=%d' % n, file=sys.stderr)
        got = seg_async.get()
    results = [None] * len(tasks)
    for i, r in zip(order, got):
        results[i] = r
    dropped = []
    for r in results:
        key = cc.seg_key(r['family'], r['n'], r['length'])
        t2 = cc.tol2(r['delta_star'])
        print('%-24s delta_star=%.10g E=%.3g width=%.3g (tol2 %.3g) '
              'oracle-delta_star=%.3g f1_err=%.3g redraws=%d slopes %.3g %.3g'
              % (key, r['delta_star'], r['E'], r['hi'] - r['lo'], t2,
                 r['oracle'] - r['delta_star'], r['f1_err'], r['redraws'],
                 r['slope_a'], r['slope_b']), file=sys.stderr)
        if not r['flat_ok']:
            print('  DROPPED: flat region wider than tol2', file=sys.stderr)
            dropped.append(key)
            continue
        assert r['unimodal'], key
        assert r['oracle_ok'], key
        if r['family'] in cc.QCML_FAMILIES:
            assert r['f1_err'] <= 1e-9, (key, r['f1_err'])
        if r['family'] == 'under':
            assert r['slope_a'] >= 0 and r['delta_star'] == cc.BRENT_A, key
        if r['family'] == 'ceiling':
            assert r['slope_b'] <= 0 and r['delta_star'] == cc.BRENT_B, key
        data = r['data']
        if data.dtype != np.float64:
            data = data.astype(np.int32)
        out[key + '_data'] = data
        out[key + '_ref'] = np.array([r['delta_star'], r['E'], r['lo'],
                                      r['hi'], r['oracle'], r['f1_err']])
    fams = sorted({k.split('_')[1] for k in dropped})
    assert len(fams) <= 1, dropped
    out['seg_dropped'] = np.array(dropped, dtype='U32')
    write_npz(OUT, out)
    size = os.path.getsize(OUT)
    print('wrote %s: %d bytes' % (OUT, size), file=sys.stderr)
    assert size < 1000000


if __name__ == '__main__':
    main()
