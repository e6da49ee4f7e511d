"""Two builds of one unit-test library (libh3d_hosttest.so, or
libh3d_selftest.so on a machine with a device), entry by entry.

    python tools/unit_abi_ab.py PARENT_SO HEAD_SO

Every entry the two builds of the test ABI share (tests/unit_abi.py SHARED)
is called in both libraries on the same seeded inputs -- the unit tests'
ranges, a few thousand elements each, every replicate count of {1, 2, 4, 9,
32}, every mode / tail / upper / refit, C of 2 and 3, and n = 0 -- and the
return codes and the bytes of every output (NaNs by bit pattern) must be
equal. Arguments an entry rejects are left out: their handling is the tests'
(tests/test_unit_abi.py). Prints one line per entry, with the largest
difference in ulps where doubles differ; exit status 1 if any differs.
"""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                os.pardir, 'tests'))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                os.pardir))
from unit_abi import SHARED  # noqa: E402

N = 3000
REPS = (1, 2, 4, 9, 32)
i64, dbl = ctypes.c_int64, ctypes.c_double


def out(shape, dtype=np.float64):
    """an output array, preset so that an element left alone compares equal"""
    n = int(np.prod(shape))
    return np.full(n * np.dtype(dtype).itemsize, 0x5A, np.uint8).view(dtype).reshape(shape)


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def logu(rng, lo, hi, n):
    return 10. ** rng.uniform(np.log10(lo), np.log10(hi), n)


def stream_u(rng, n):
    """uniforms of the stream's form, (m + 1/2) 2^-52"""
    return (rng.integers(0, 2 ** 52, n).astype(np.float64) + 0.5) * 2. ** -52


def pixels(rng, n, r):
    """counts (n, r) int32 around per-pixel means, and factors near 1"""
    mu = logu(rng, 0.05, 3e3, n)[:, None]
    x = rng.poisson(mu * rng.gamma(20., 1 / 20., (n, r))).astype(np.int32)
    f = np.exp(rng.normal(0, 0.3, (n, r)))
    return np.ascontiguousarray(x), np.ascontiguousarray(f)


UNARY = {
    'lgam': lambda g, n: np.r_[logu(g, 1e-6, 1e6, n), -g.uniform(0, 20, 50)],
    'lgam_nll': lambda g, n: logu(g, 1e-4, 1e8, n),
    'log_fast': lambda g, n: logu(g, 1e-300, 1e300, n),
    'log_fast_fp_index': lambda g, n: logu(g, 1e-300, 1e300, n),
    'ndtr': lambda g, n: g.uniform(-40, 40, n),
    'ndtri': lambda g, n: np.r_[g.uniform(0, 1, n), logu(g, 1e-300, 1e-3, 200)],
    'log1pmx': lambda g, n: np.r_[g.uniform(-0.99, 10, n), g.normal(0, 1e-3, 200)],
    'lgam1p': lambda g, n: np.r_[g.uniform(-0.9, 50, n), g.normal(0, 1e-3, 200)],
    'exp_fast': lambda g, n: np.r_[g.uniform(-746, 746, n), g.uniform(-2, 2, n),
                                   [np.inf, -np.inf, np.nan, 0., -0.]],
    'log_fast_checked': lambda g, n: np.r_[logu(g, 1e-300, 1e300, n),
                                           [0., -0., np.inf, np.nan, -1., 5e-324]],
    'recip_fast': lambda g, n: logu(g, 1e-200, 1e200, n) * g.choice([-1., 1.], n),
}
BINARY = {
    'igam': lambda g, n: (logu(g, 1e-3, 2e3, n), logu(g, 1e-3, 4e3, n)),
    'igamc': lambda g, n: (logu(g, 1e-3, 2e3, n), logu(g, 1e-3, 4e3, n)),
    'igami': lambda g, n: (logu(g, 1e-2, 2e3, n), g.uniform(0, 1, n)),
    'igamci': lambda g, n: (logu(g, 1e-2, 2e3, n), g.uniform(0, 1, n)),
    'chi2_sf': lambda g, n: (g.integers(1, 6, n).astype(float), logu(g, 1e-3, 1e3, n)),
    'div_fast': lambda g, n: (logu(g, 1e-100, 1e100, n) * g.choice([-1., 1.], n),
                              logu(g, 1e-100, 1e100, n)),
}


def cases(rng):
    """(entry, label, call): call(lib) -> (return code, [output arrays])"""
    def elementwise(name, arrays, outs, *mid):
        # h3dt_<name>(n, arrays..., mid..., outs...) over arrays[0].size elements
        def call(lib):
            o = [out(s, t) for s, t in outs]
            rc = getattr(lib, 'h3dt_' + name)(
                i64(arrays[0].shape[0]), *[ptr(a) for a in arrays], *mid,
                *[ptr(a) for a in o])
            return rc, o
        return call

    for name, gen in UNARY.items():
        for n in (N, 0):
            x = np.ascontiguousarray(gen(rng, N)[:None if n else 0])
            yield name, 'n=%d' % x.size, elementwise(name, [x], [(x.shape, float)])
    for name, gen in BINARY.items():
        for n in (N, 0):
            a, x = (np.ascontiguousarray(v[:None if n else 0]) for v in gen(rng, N))
            yield name, 'n=%d' % a.size, elementwise(name, [a, x], [(a.shape, float)])

    for n in (N, 257, 0):
        ctr = rng.integers(0, 2 ** 32, (n, 4), dtype=np.uint64).astype(np.uint32)
        key = rng.integers(0, 2 ** 32, (n, 2), dtype=np.uint64).astype(np.uint32)
        yield 'philox', 'n=%d' % n, elementwise(
            'philox', [ctr, key], [((n, 4), np.uint32), ((n, 2), float)])
        yield 'philox_uniform', 'n=%d' % n, elementwise(
            'philox_uniform', [ctr[:, 0].copy(), ctr[:, 1].copy()], [((n,), float)])

    for n in (N, 0):
        bm, disp = logu(rng, 1e-3, 2e4, n), logu(rng, 1e-4, 5, n)
        u1, u2 = stream_u(rng, n), stream_u(rng, n)
        if n:
            disp[-1], bm[-2] = np.nan, -1.
        for with_path in (1, 0):
            def call(lib, a=(bm, disp, u1, u2), n=n, with_path=with_path):
                lam, k, path = out((n,)), out((n,), np.int32), out((n,), np.int32)
                rc = lib.h3dt_nb_draw(i64(n), *[ptr(v) for v in a], ptr(lam), ptr(k),
                                      ptr(path) if with_path else None)
                return rc, [lam, k, path]
            yield 'nb_draw', 'n=%d path=%d' % (n, with_path), call
        lam = np.r_[logu(rng, 1e-3, 2e4, n), np.zeros(min(n, 3))]
        yield 'poisson_quantile', 'n=%d' % lam.size, elementwise(
            'poisson_quantile', [lam, stream_u(rng, lam.size)],
            [(lam.shape, float), (lam.shape, np.int32)])

    for J, sf_rows, n in ((2, 1, N), (4, 0, N), (6, 0, 0)):
        n_bins, D = 400, 60
        row = rng.integers(0, n_bins - D, n).astype(np.int32)
        col = (row + rng.integers(0, D, n)).astype(np.int32)
        mA, mB = logu(rng, 1e-2, 1e3, n), logu(rng, 1e-2, 1e3, n)
        bias = np.exp(rng.normal(0, 0.3, (n_bins, J)))
        sf = np.exp(rng.normal(0, 0.2, (1 if sf_rows == 1 else D, J)))
        table = logu(rng, 1e-3, 0.5, D)

        def call(lib, a=(row, col, mA, mB, bias, sf), sf_rows=sf_rows,
                 table=table, J=J, n=n):
            bm, dp = out((J, n)), out((J, n))
            rc = lib.h3dt_sim_bm(i64(n), J, n_bins, D, *[ptr(v) for v in a],
                                 sf_rows, ptr(table), ptr(bm), ptr(dp))
            return rc, [bm, dp]
        yield 'sim_bm', 'n=%d J=%d sf_rows=%d' % (n, J, sf_rows), call

    for tail in (-1, 0, 1):
        for n in ((N, 0) if tail == 0 else (N,)):
            a, x = logu(rng, 1e-3, 2e3, n), logu(rng, 1e-3, 4e3, n)
            yield 'igam_pq', 'n=%d tail=%d' % (n, tail), elementwise(
                'igam_pq', [a, x], [((n,), float)] * 3, ctypes.c_int(tail))
    for upper in (0, 1):
        for n in ((N, 0) if upper == 0 else (N,)):
            a, t = logu(rng, 1e-1, 2e3, n), logu(rng, 1e-30, 0.5, n)
            guess = np.where(rng.uniform(size=n) < 0.5, 0., a * rng.uniform(0.5, 1.5, n))

            def call(lib, a=a, t=t, guess=guess, upper=upper, n=n):
                o = out((n,))
                lib.h3dt_igam_inv(i64(n), ptr(a), ptr(t), upper, ptr(guess), ptr(o))
                return None, [o]
            yield 'igam_inv', 'n=%d upper=%d' % (n, upper), call
    for n in (N, 0):
        a = logu(rng, 1e-3, 5e4, n)
        xe = a * np.exp(rng.normal(0, 0.5, n))
        h = xe * rng.uniform(-0.08, 0.08, n)   # either side of the 0.05 window
        yield 'igam_step_taylor', 'n=%d' % n, elementwise(
            'igam_step_taylor', [a, xe, h],
            [((n,), np.int32), ((n,), float), ((n,), float)])
        bits = rng.integers(1, 2 ** 52, n) | (rng.integers(0, 2047, n) << 52)
        yield 'log_index', 'n=%d' % n, elementwise(
            'log_index', [np.ascontiguousarray(bits).view(np.float64)],
            [((n,), np.int32)] * 2)
        mu_in, mu_out = logu(rng, 0.05, 3e3, n), logu(rng, 0.05, 3e3, n)
        x = rng.poisson(mu_in).astype(np.float64)
        yield 'q2q', 'n=%d' % n, elementwise(
            'q2q', [x, mu_in, mu_out, logu(rng, 1e-4, 2, n)], [((n,), float)])

    for r in REPS:
        for n in ((N, 0) if r == 2 else (N,)):
            x, f = pixels(rng, n, r)
            alpha_px = logu(rng, 1e-4, 2, n)
            alpha_rep = np.ascontiguousarray(logu(rng, 1e-4, 2, (n, r)))
            lab = 'n=%d r=%d' % (n, r)

            def fit_mu(lib, x=x, f=f, al=alpha_rep, n=n, r=r):
                mu = out((n,))
                return lib.h3dt_fit_mu(i64(n), r, ptr(x), ptr(f), ptr(al), ptr(mu)), [mu]

            def eq_alpha(lib, x=x, f=f, al=alpha_px, n=n, r=r):
                o = out((n, r))
                return lib.h3dt_equalize_alpha(i64(n), r, ptr(x), ptr(f), ptr(al),
                                               ptr(o)), [o]

            def eq(lib, x=x, f=f, n=n, r=r):
                o = out((n, r))
                return lib.h3dt_equalize(i64(n), r, ptr(x), ptr(f), dbl(0.03), ptr(o)), [o]

            def qcml(lib, x=x, f=f, n=n, r=r):
                st = ctypes.c_int(-99)
                d = lib.h3dt_qcml(i64(n), r, ptr(x), ptr(f), ctypes.byref(st))
                return st.value, [np.array([d])]
            yield 'fit_mu', lab, fit_mu
            yield 'equalize_alpha', lab, eq_alpha
            yield 'equalize', lab, eq
            yield 'qcml', lab, qcml
            pseudo = np.ascontiguousarray(
                logu(rng, 1e-2, 1e4, (n, r)) * (rng.uniform(size=(n, r)) > 0.1))
            for mode in range(5):
                for delta in (0.3, 0.06, 0.02, 1e-4):
                    def nll(lib, ps=pseudo, n=n, r=r, mode=mode, delta=delta):
                        o = out((n,))
                        return lib.h3dt_nll_terms(i64(n), r, ptr(ps), dbl(delta), mode,
                                                  ptr(o)), [o]
                    yield 'nll_terms', '%s mode=%d delta=%g' % (lab, mode, delta), nll

    for R in REPS[1:]:
        for C in (2, 3):
            if C > R:
                continue
            for refit in (0, 1):
                for n in ((N, 0) if (R, C, refit) == (4, 2, 0) else (N,)):
                    x, f = pixels(rng, n, R)
                    disp = np.ascontiguousarray(logu(rng, 1e-3, 1, (n, R)))
                    cond = (np.arange(R) % C).astype(np.int32)
                    cond.sort()

                    def lrt(lib, x=x, f=f, disp=disp, cond=cond, n=n, R=R, C=C,
                            refit=refit):
                        o = [out((n,)), out((n,)), out((n,)), out((n, C))]
                        rc = lib.h3dt_lrt(i64(n), R, C, ptr(x), ptr(f), ptr(disp),
                                          ptr(cond), refit, *[ptr(a) for a in o])
                        return rc, o
                    yield 'lrt', 'n=%d R=%d C=%d refit=%d' % (n, R, C, refit), lrt


VOID = {'h3dt_' + n for n in list(UNARY) + list(BINARY) + [
    'philox', 'philox_uniform', 'poisson_quantile', 'igam_pq', 'igam_inv',
    'igam_step_taylor', 'log_index', 'q2q']}


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in SHARED:
        getattr(lib, name).restype = None if name in VOID else ctypes.c_int
    lib.h3dt_qcml.restype = ctypes.c_double
    return lib


def ulps(a, b):
    """largest distance of two double arrays in units in the last place"""
    def key(v):
        k = v.view(np.int64).astype(object)
        return np.where(k < 0, -(k & (2 ** 63 - 1)), k)
    d = np.abs(key(a.ravel()) - key(b.ravel()))
    return int(d.max()) if d.size else 0


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    try:  # one HIP runtime per process: torch's first (tests/unit_abi.py)
        import torch  # noqa: F401
    except ImportError:
        pass
    parent, head = load(argv[1]), load(argv[2])
    worst, seen = {}, set()
    for name, label, call in cases(np.random.default_rng(20260)):
        seen.add('h3dt_' + name)
        (rc_a, out_a), (rc_b, out_b) = call(parent), call(head)
        diff = [] if rc_a == rc_b else ['return code %r / %r' % (rc_a, rc_b)]
        for k, (a, b) in enumerate(zip(out_a, out_b)):
            if a.tobytes() != b.tobytes():
                n_bad = int(np.sum(a.view(np.uint8) != b.view(np.uint8)))
                diff.append('output %d: %d bytes differ%s' % (
                    k, n_bad, ', %d ulp at most' % ulps(a, b)
                    if a.dtype == np.float64 else ''))
        if diff:
            print('DIFFERS %s %s: %s' % (name, label, '; '.join(diff)))
        worst.setdefault(name, []).extend(diff)
    missing = sorted(set(SHARED) - seen)
    for name in sorted(worst):
        print('%-18s %s' % (name, 'DIFFERS' if worst[name] else 'equal'))
    if missing:
        print('no case for:', ' '.join(missing))
    bad = sorted(n for n in worst if worst[n])
    print('%d entries, %d differ%s' % (len(worst), len(bad),
                                       ': ' + ' '.join(bad) if bad else ''))
    return 1 if bad or missing else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
