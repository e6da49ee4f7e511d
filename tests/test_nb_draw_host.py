"""nb_draw (csrc/h3d_sample.h), the inversion sampler behind
simulate(gpu=True), against scipy one draw at a time and in distribution,
through the host build and the gfx950 build of the same source (h3dt_nb_draw,
as tests/test_special_host.py does for the special functions).

The uniforms have the stream's own form (csrc/h3d_philox.h): (m + 1/2) 2^-52
for a 52-bit integer m, so they lie in [2^-53, 1 - 2^-53] and 1 - u is exact.
(53 bits plus the half would need 54 significant bits: the largest such
value, 1 - 2^-54, is not a double and rounds to 1.) The tail cases also feed
2^-54, which the sampler accepts although the stream never produces it.

Bounds: (a) the project's igami / igamci bar, 1e-11 relative of scipy; (b)
the definition of the quantile with the igam_err slack of
test_special_host.py; (c) at most 1e-4 of a cell's draws may differ from
scipy.stats.poisson.ppf, and those still meet (b); (d) a chi-square below
chi2.isf(1e-6, df) and a mean within 5 standard errors."""
import ctypes

import numpy as np
import pytest
import scipy.special as sc
import scipy.stats as st

from conftest import rel_err

from unit_abi import load_gfx950, load_host

D = ctypes.POINTER(ctypes.c_double)
I = ctypes.POINTER(ctypes.c_int32)

CELLS = [(1e-3, 0.1), (0.25, 1.0), (1.0, 0.01), (7.0, 0.05), (30.0, 5.0),
         (300.0, 1e-4), (2e4, 0.02), (2e4, 1e-4)]
N_DRAWS = 200000
U_MIN, U_MAX = 2.0 ** -53, 1 - 2.0 ** -53
H3D_FLAG_BADIN = 16


@pytest.fixture(scope='module',
                params=['host', pytest.param('gfx950', marks=pytest.mark.gpu)])
def lib(request):
    return load_host() if request.param == 'host' else load_gfx950()


def nb_draw(lib, bm, disp, u1, u2):
    """(lambda, k, flags) of h3dt_nb_draw over broadcast inputs."""
    bm, disp, u1, u2 = (np.ascontiguousarray(a, dtype=np.float64) for a in
                        np.broadcast_arrays(bm, disp, u1, u2))
    lam = np.empty(bm.shape)
    k = np.empty(bm.shape, dtype=np.int32)
    lib.h3dt_nb_draw.restype = ctypes.c_int
    fl = lib.h3dt_nb_draw(
        ctypes.c_int64(bm.size), bm.ctypes.data_as(D), disp.ctypes.data_as(D),
        u1.ctypes.data_as(D), u2.ctypes.data_as(D), lam.ctypes.data_as(D),
        k.ctypes.data_as(I), None)
    return lam, k, fl


def stream_uniforms(rng, n):
    return (rng.integers(0, 2 ** 52, n).astype(np.float64) + 0.5) * 2.0 ** -52


def gamma_ref(bm, disp, u1):
    r = 1 / disp
    with np.errstate(all='ignore'):
        g = np.where(u1 <= 0.5, sc.gammaincinv(r, np.minimum(u1, 0.5)),
                     sc.gammainccinv(r, np.minimum(1 - u1, 0.5)))
    return bm * disp * g


def quantile_violations(lam, k, u2):
    """Draws whose k is not the Poisson(lam) quantile of u2 by definition,
    pdtr(k - 1) < u2 <= pdtr(k), compared in the tail that holds u2 with the
    relative slack of igam_err."""
    lam, u2 = np.asarray(lam, dtype=float), np.asarray(u2, dtype=float)
    kf = np.asarray(k, dtype=float)
    with np.errstate(all='ignore'):
        kl = np.where(kf > 0, kf * np.log(lam), 0.0)
        slack = 1e-12 + 2 * 2.2e-16 * (np.abs(kl) + lam + sc.gammaln(kf + 1))
        km = np.maximum(kf - 1, 0)
        up = u2 > 0.5
        t = 1 - u2
        ok_at = np.where(up, sc.pdtrc(kf, lam) <= t * (1 + slack),
                         sc.pdtr(kf, lam) >= u2 * (1 - slack))
        ok_below = np.where(up, sc.pdtrc(km, lam) > t * (1 - slack),
                            sc.pdtr(km, lam) < u2 * (1 + slack))
    return np.flatnonzero(~(ok_at & ((kf == 0) | ok_below)))


_cache = {}


def cell_draws(lib, cell):
    key = (id(lib), cell)
    if key not in _cache:
        bm, disp = cell
        rng = np.random.default_rng([CELLS.index(cell), 20211021])
        u1 = stream_uniforms(rng, N_DRAWS)
        u2 = stream_uniforms(rng, N_DRAWS)
        _cache.clear()   # one cell's arrays at a time
        _cache[key] = (u1, u2) + nb_draw(lib, bm, disp, u1, u2)
    return _cache[key]


@pytest.mark.parametrize('cell', CELLS, ids=lambda c: '%g-%g' % c)
def test_draws_vs_scipy(lib, cell):
    bm, disp = cell
    u1, u2, lam, k, fl = cell_draws(lib, cell)
    assert fl == 0 and np.all(k >= 0) and np.all(np.isfinite(lam))
    # (a) the gamma stage
    err = rel_err(lam, gamma_ref(bm, disp, u1))
    print('gamma stage rel err %.3g' % err)
    assert err < 1e-11
    # (b) the Poisson stage by definition, on the library's own lambda
    bad = quantile_violations(lam, k, u2)
    print('quantile violations', bad.size)
    assert bad.size == 0, (lam[bad[:5]], k[bad[:5]], u2[bad[:5]])
    # (c) scipy's quantile
    with np.errstate(all='ignore'):
        ref = st.poisson.ppf(u2, lam)
    ref = np.where(lam == 0, 0, ref)
    differ = int(np.sum(k != ref))
    print('differ from poisson.ppf', differ)
    assert differ <= 1e-4 * N_DRAWS
    # (d) the distribution: chi-square over <= 60 quantile bins of the
    # reference's negative binomial, each with an expected count >= 5
    r = 1 / disp
    nb = st.nbinom(r, 1 / (1 + bm * disp))
    edges = np.unique(nb.ppf(np.linspace(0, 1, 61)[1:-1]))
    cdf = np.concatenate([[0.0], nb.cdf(edges), [1.0]])
    expect = np.diff(cdf) * N_DRAWS
    obs = np.bincount(np.searchsorted(edges, k, side='left'),
                      minlength=len(expect)).astype(float)
    while len(expect) > 1 and expect.min() < 5:   # merge into a neighbour
        i = int(np.argmin(expect))
        j = i - 1 if i > 0 else 1
        expect[j] += expect[i]
        obs[j] += obs[i]
        expect, obs = np.delete(expect, i), np.delete(obs, i)
    if len(expect) > 1:
        chi = float(np.sum((obs - expect) ** 2 / expect))
        bound = st.chi2.isf(1e-6, len(expect) - 1)
        print('chi2 %.3g bound %.3g bins %d' % (chi, bound, len(expect)))
        assert chi < bound
    se = np.sqrt((bm + bm ** 2 * disp) / N_DRAWS)
    print('mean off by %.3g se' % (abs(k.mean() - bm) / se))
    assert abs(k.mean() - bm) < 5 * se


def test_tails(lib):
    """(e) the extreme uniforms of the stream (and 2^-54) at every cell, in
    either stage: finite lambda, the quantile's definition, no flag."""
    ends = np.array([2.0 ** -54, U_MIN, U_MAX])
    mid = stream_uniforms(np.random.default_rng(5), 16)
    for bm, disp in CELLS:
        u1 = np.concatenate([np.repeat(ends, 3), np.repeat(ends, mid.size),
                             np.tile(mid, 3)])
        u2 = np.concatenate([np.tile(ends, 3), np.tile(mid, 3),
                             np.repeat(ends, mid.size)])
        lam, k, fl = nb_draw(lib, bm, disp, u1, u2)
        assert fl == 0 and np.all(k >= 0), (bm, disp)
        assert np.all(np.isfinite(lam)) and np.all(lam >= 0)
        assert rel_err(lam, gamma_ref(bm, disp, u1)) < 1e-11
        bad = quantile_violations(lam, k, u2)
        assert bad.size == 0, (bm, disp, lam[bad], k[bad], u2[bad])


def test_bad_inputs(lib):
    """(f) bm or disp in {0, -1, inf, nan}: the flag, count -1, and the
    neighbouring draws what they are alone."""
    rng = np.random.default_rng(9)
    n = 64
    bm = np.full(n, 7.0)
    disp = np.full(n, 0.05)
    u1, u2 = stream_uniforms(rng, n), stream_uniforms(rng, n)
    lam0, k0, fl0 = nb_draw(lib, bm, disp, u1, u2)
    assert fl0 == 0
    for which in (bm, disp):
        for j, v in enumerate((0.0, -1.0, np.inf, np.nan)):
            a = which.copy()
            a[5 + 9 * j] = v
            lam, k, fl = nb_draw(lib, *((a, disp) if which is bm else (bm, a)),
                                 u1, u2)
            assert fl & H3D_FLAG_BADIN
            assert k[5 + 9 * j] == -1
            keep = np.arange(n) != 5 + 9 * j
            np.testing.assert_array_equal(k[keep], k0[keep])
            np.testing.assert_array_equal(lam[keep], lam0[keep])
    # lambda at or beyond 2^31 is refused too
    lam, k, fl = nb_draw(lib, 1e12, 0.05, 0.5, 0.5)
    assert fl & H3D_FLAG_BADIN and k[()] == -1


def test_poisson_quantile_entry(lib):
    """h3dt_poisson_quantile alone: both sides of the lam = 12 switch, against
    the definition; lam = 0 gives 0."""
    rng = np.random.default_rng(11)
    lam = np.concatenate([10 ** rng.uniform(-6, np.log10(12), 3000),
                          np.nextafter(12, [0, 20]),
                          10 ** rng.uniform(np.log10(12), 5, 3000), [0.0]])
    u = stream_uniforms(rng, lam.size)
    k = np.empty(lam.size)
    path = np.empty(lam.size, dtype=np.int32)
    lib.h3dt_poisson_quantile(ctypes.c_int64(lam.size), lam.ctypes.data_as(D),
                              u.ctypes.data_as(D), k.ctypes.data_as(D),
                              path.ctypes.data_as(I))
    assert k[-1] == 0
    assert np.all(path[lam < 12] <= 1) and np.all(path[lam >= 12] >= 2)
    bad = quantile_violations(lam[:-1], k[:-1], u[:-1])
    assert bad.size == 0, (lam[bad[:5]], k[bad[:5]], u[bad[:5]])
