"""The production LRT kernels (k_lrt, k_lrt8 with fit_mu_g8; TAB and non-TAB)
on a real MI355X against the exact (50+ digit mpmath) LRT of
tests/golden/unit_lrt_mp.npz: every (M, CM) instantiation lrt_run dispatches,
on seven input families of 32 pixels per design, in four modes. The bounds
are those of lrt_mp_cases.py (derived, or the project's own).

Designs and the branch of lrt_run (csrc/h3d_lrt.hip: m = 4 / 8 / 16 / 24 / 32
from R, cm = 2 / 4 / 8 from C) each reaches:

    R   C   branch
    3   2   k_lrt<4,2>
    4   3   k_lrt<4,4>
    4   4   k_lrt<4,4>; single-replicate conditions, df 3
    5   2   k_lrt<8,2>
    8   2   k_lrt<8,2>
    7   3   k_lrt<8,4>
    8   4   k_lrt<8,4>
    6   5   k_lrt8<16,8>, the group kernel at R < 8 (m <= 16, cm = 8)
    8   8   k_lrt8<16,8>; df 7
    9   2   k_lrt8<16,2>
    16  4   k_lrt8<16,4>
    17  3   k_lrt8<24,4>; a one-lane tail slot
    24  4   k_lrt8<24,4>
    25  2   k_lrt8<32,8> at C = 2
    32  8   k_lrt8<32,8>

Modes: the (D, C) table by dist with refit (the TAB kernels); per-pixel (n,
C) dispersions with dist=None; lrt_wide's (n, R) dispersions; refit_mu=False.
The per-pixel and wide modes must equal the table mode bit for bit.

Input families (make_golden_lrt_mp.py): benign (the ranges of
test_lrt_wide_designs_vs_oracle), sparse (mu 1e-2 .. 1, f 0.1 .. 10, a 1e-3
.. 3), large (counts to 1e8), lowdisp (a 1e-7 .. 1e-4), highdisp (a 1 ..
10), widef (f 1e-3 .. 1e3 in one pixel), differential (folds 1e-3 .. 1e3: p
underflows).

Measured on an MI355X (this file; lrt_pixel is test_lrt_mp_host.py's gfx950
leg), the largest figure of any design of the class, refit / refit_mu=False.
mu, llr and p_sf are in units of their bounds (mu: 1e-12 / 1e-14; llr: (8 + R)
eps S; p_sf: igam_err's tolerance against scipy at the kernel's own llr),
p_rel is the relative error against p_mp (bar 1e-6):

    k_lrt (R <= 8, C <= 4)
    family        mu            llr          p_sf         p_rel
    benign        0.0049/0.026  0.029/0.035  0.029/0.029  5.0e-14/2.9e-14
    sparse        0.0008/0.026  0.059/0.054  0.027/0.030  3.1e-13/2.0e-13
    large         0.25/0.026    0.018/0.016  0.029/0.030  9.3e-9/4.4e-9
    lowdisp       0.050/0.027   0.043/0.024  0.028/0.029  1.6e-9/7.4e-10
    highdisp      0.012/0.037   0.054/0.049  0.025/0.028  1.0e-11/1.9e-12
    widef         0.0092/0.024  0.044/0.051  0.029/0.025  9.1e-11/1.1e-10
    differential  0.056/0.034   0.057/0.071  0.079/0.056  2.9e-8/1.8e-8

    k_lrt8 (R > 8 or C > 4)
    benign        0.0069/0.035  0.021/0.019  0.030/0.031  6.2e-14/3.8e-14
    sparse        0.0026/0.024  0.043/0.042  0.025/0.024  2.3e-13/2.8e-13
    large         0.35/0.034    0.0062/0.0074 0.029/0.030 7.6e-9/6.6e-9
    lowdisp       0.045/0.028   0.017/0.017  0.030/0.030  1.7e-10/7.6e-10
    highdisp      0.022/0.030   0.033/0.023  0.030/0.031  2.7e-12/2.2e-12
    widef         0.011/0.028   0.019/0.028  0.024/0.026  1.5e-10/6.2e-11
    differential  0.17/0.031    0.040/0.047  0.078/0.059  7.1e-8/9.8e-8

    lrt_pixel, gfx950 self-test kernel (every design, CM = 8)
    benign        0.0069/0.035  0.029/0.035  0.030/0.031  6.2e-14/3.8e-14
    sparse        0.0029/0.026  0.059/0.054  0.027/0.030  3.1e-13/2.8e-13
    large         0.35/0.034    0.018/0.016  0.029/0.030  9.3e-9/6.6e-9
    lowdisp       0.050/0.028   0.043/0.024  0.030/0.030  1.6e-9/7.6e-10
    highdisp      0.022/0.037   0.054/0.049  0.030/0.031  1.0e-11/2.2e-12
    widef         0.011/0.028   0.044/0.051  0.029/0.026  9.8e-11/1.1e-10
    differential  0.17/0.034    0.057/0.071  0.079/0.059  7.1e-8/9.8e-8

fit_mu_g8 meets the 1e-12 of fit_mu everywhere (0.35 of it at worst, as
fit_mu on the same pixels): the twins have not diverged. p lies inside the mp
interval on every pixel, as written at normal ends and to one unit of the
subnormal grid at subnormal ones (the host build needs that unit nowhere). 58 (refit) and
62 (not) differential pixels of the fixture have p_mp < 5e-324, where the
kernels return 0, and 3 and 2 a subnormal p_mp, which they return. At R = 32
/ C = 8 that leaves 6 (4) of the differential cell's 32 pixels with a
non-zero p through k_lrt8<32,8>; the other families carry that kernel's p
checks. No pixel of the fixture had to be redrawn.

The kernel fix these tests needed: the llr took log(mu0 / mu1) and log((r +
mu0 f) / (r + mu1 f)) of the rounded quotients, ~1e-16 absolute per log
whatever its size, times counts of 1e8: llr off by 8.5e-8 (0.026 of its
bound) and, at x2 = 2e-3 with one degree of freedom, p off by 1.05e-6
relative at R = 25 / C = 2 in `large` (9.3e-7 at R = 3 / C = 2) -- past the
1e-6 bar in k_lrt8 and lrt_pixel alike. log_quot (csrc/h3d_model.h) now goes
through the difference mu0 - mu1 where the means are within a factor of 2;
the figures above are with it (large: p 1.05e-6 -> 9.3e-9).

And a second one: chi2_sf's general branch (designs of four or more
conditions) returned exactly 0 for a subnormal tail -- igamc keeps cephes'
rule of giving up once the prefactor's exponent is below -709.78 -- where
the closed forms of two and three conditions return the subnormal: p = 0
for p_mp = 3.4993e-314 (R = 32 / C = 8, differential pixel 218), 5e-324
(pixel 194) and 6.697e-320 (R = 8 / C = 8, pixel 193), outside the interval
the llr bound leaves. chi2_sf now continues through igamc_tiny
(csrc/h3d_special.h) there; in the host build the three pixels come out as
the correctly rounded p_mp, and gfx950 passes the same interval check.

The float64 restatement oracle.lrt against the same fixture (stored in the
npz as *_oracle_err; the largest of any design): its p is off by up to 1.1e-5
relative in `large` (R = 3, C = 2), 6.6e-7 in lowdisp, 6.1e-7 in
differential, 1.5e-8 in widef and <= 2.1e-10 elsewhere; its llr is at up to
1.6 times the bound (8 + R) eps S in widef (1.3 large, 1.1 lowdisp, <= 0.78
elsewhere); its means hold to 7.8e-12. It cannot certify the 1e-6 p bar at
those edges.
"""
import numpy as np
import pytest

import lrt_mp_cases as cases

pytestmark = pytest.mark.gpu

H3D_ENOCONV = -3
H3D_EINPUT = -5


@pytest.fixture(scope='module')
def ctx():
    from hic3defdr_amd import _native
    return _native.context(0)


def _kind(R, C):
    return 'k_lrt' if (R <= 8 and C <= 4) else 'k_lrt8'


@pytest.mark.parametrize('R,C', cases.DESIGNS)
def test_lrt_kernels_vs_mp(ctx, R, C):
    d = cases.design(R, C)
    kind = _kind(R, C)
    # the (D, C) table by dist, refit: the TAB kernel
    p, llr, m0, m1, disp = ctx.lrt(d.raw, d.f, d.dist, d.table, d.cond)
    np.testing.assert_array_equal(disp, d.disp)
    cases.check(d, (p, llr, m0, m1), True, kind + ' table')
    # per-pixel (n, C) dispersions and lrt.py's (n, R): the same bits
    pp, pllr, pm0, pm1, pdisp = ctx.lrt(d.raw, d.f, None, d.disp, d.cond)
    wp, wllr, wm0, wm1 = ctx.lrt_wide(d.raw, d.f, d.disp_wide, d.cond, C)
    for got in ((pp, pllr, pm0, pm1), (wp, wllr, wm0, wm1)):
        for a, b in zip(got, (p, llr, m0, m1)):
            np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(pdisp, d.disp)
    # refit_mu=False, by the table and by the (n, R) dispersions
    q, qllr, qm0, qm1, _ = ctx.lrt(d.raw, d.f, d.dist, d.table, d.cond,
                                   refit_mu=False)
    cases.check(d, (q, qllr, qm0, qm1), False, kind + ' table')
    wq = ctx.lrt_wide(d.raw, d.f, d.disp_wide, d.cond, C, refit_mu=False)
    for a, b in zip(wq, (q, qllr, qm0, qm1)):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('R,C', [(7, 3), (17, 3)])
def test_lrt_pixels_are_independent(ctx, R, C):
    """The benign cell tiled to n = 4099: one call equals, bit for bit, the
    concatenation of calls on chunks of 37 pixels (the grid stride, the tail,
    groups straddling waves)."""
    d = cases.design(R, C)
    n, step = 4099, 37
    idx = np.arange(n) % cases.NPIX      # the benign cell is the first
    raw, f = d.raw[idx], d.f[idx]
    dist = d.dist[idx]
    for refit in (True, False):
        whole = ctx.lrt(raw, f, dist, d.table, d.cond, refit_mu=refit)
        parts = [ctx.lrt(raw[i:i + step], f[i:i + step], dist[i:i + step],
                         d.table, d.cond, refit_mu=refit)
                 for i in range(0, n, step)]
        for k in range(5):
            np.testing.assert_array_equal(
                whole[k], np.concatenate([pt[k] for pt in parts]))
        # and every tile of the cell repeats the cell
        for k in range(4):
            np.testing.assert_array_equal(whole[k], whole[k][:cases.NPIX][idx])


def _raises(code, fn, *a, **kw):
    from hic3defdr_amd import _native
    with pytest.raises(_native.H3DError) as e:
        fn(*a, **kw)
    assert e.value.code == code, e.value


@pytest.mark.parametrize('R,C', [(4, 2), (12, 3)])
def test_lrt_failure_paths(ctx, R, C):
    """kFlagNoRoot -> H3D_ENOCONV (an all-zero condition), kFlagBadInput ->
    H3D_EINPUT (a dist outside [0, D), a NaN or 0 dispersion, f = 0), for
    k_lrt (R = 4) and k_lrt8 (R = 12), TAB and non-TAB; and the flag word is
    reset: the well-formed call gives its answer again after every raise."""
    rng = np.random.default_rng(R)
    n, D = 70, 9
    cond = (np.arange(R) % C).astype(np.int32)
    f = np.exp(rng.normal(0, 0.3, (n, R)))
    raw = rng.poisson(30.0 * f).astype(np.int64) + 1
    dist = rng.integers(0, D, n).astype(np.int32)
    tab = rng.uniform(0.01, 0.3, (D, C))
    good = ctx.lrt(raw, f, dist, tab, cond)
    assert np.all(np.isfinite(good[0]))

    def still_good():
        for a, b in zip(ctx.lrt(raw, f, dist, tab, cond), good):
            np.testing.assert_array_equal(a, b)

    px = 41
    zero = raw.copy()
    zero[px, cond == 1] = 0
    for kw in (dict(), dict(per_pixel=True), dict(wide=True)):
        def call(raw_=raw, f_=f, dist_=dist, tab_=tab, kw=kw):
            if kw.get('wide'):
                return ctx.lrt_wide(raw_, f_, tab_[dist_][:, cond], cond, C)
            if kw.get('per_pixel'):
                return ctx.lrt(raw_, f_, None, tab_[dist_], cond)
            return ctx.lrt(raw_, f_, dist_, tab_, cond)
        _raises(H3D_ENOCONV, call, raw_=zero)
        still_good()
        for bad in (np.nan, 0.0):
            t2 = tab.copy()
            t2[dist[px], 1] = bad
            _raises(H3D_EINPUT, call, tab_=t2)
            still_good()
        f2 = f.copy()
        f2[px, R - 1] = 0.0
        _raises(H3D_EINPUT, call, f_=f2)
        still_good()
    for bad, where in ((-1, px), (D, n - 1)):
        d2 = dist.copy()
        d2[where] = bad
        _raises(H3D_EINPUT, ctx.lrt, raw, f, d2, tab, cond)
        still_good()
