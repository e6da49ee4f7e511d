"""The exact LRT fixture tests/golden/unit_lrt_mp.npz (written by
tests/golden/make_golden_lrt_mp.py) and the bounds every implementation of
the per-pixel LRT is held to against it: shared by test_gpu_lrt_edges.py (the
production kernels) and test_lrt_mp_host.py (lrt_pixel through the host and
self-test builds).

The bounds are derived or are the project's own; none is taken from what
the code gives:

- refit means: 1e-12 relative of the mp roots, the bound
  test_fit_mu_is_converged_to_full_precision holds fit_mu to (RTOL_MU = 1e-8
  is the project's hard cap);
- refit_mu=False means: 1e-14;
- llr: |llr - llr_mp| <= B = (8 + R) 2.2e-16 S, with S = sum_k x_k |ln(mu0 /
  mu1)| + (r_k + x_k) (|ln((r_k + mu0 f_k) / (r_k + mu1 f_k))| + 1), r = 1 /
  a: one rounding per product and quotient, one ulp of each log, R additions;
- p against scipy: within igam_err's tolerance of chi2.sf(-2 llr, C - 1) at
  the implementation's own llr (each tail switch on its own). scipy returns
  0 for a subnormal tail (cephes igamc gives up once the prefactor's exponent
  is below -709.78), so a pixel where scipy gives 0 and p is subnormal is
  left to the interval check, whose ends are exact;
- p against the llr interval: Q(-llr_mp + B) <= p <= Q(max(-llr_mp - B, 0)),
  Q = Q((C - 1) / 2, .), the ends stored from mp (correctly rounded), as
  written wherever an end is a normal double. An end below 2.2e-308 is itself
  rounded to the subnormal grid, whose spacing 2^-1074 is absolute, so there p
  may lie one such unit beyond it: what one rounding of an exact value costs;
- the project's p bar: within 1e-6 relative of p_mp where p_mp >= 1e-300 and
  x2_mp >= 1e-6;
- underflow: where p_mp < 5e-324, p is 0 or inside the interval.
"""
import numpy as np

from conftest import golden

# (R, C): the dispatch branch of lrt_run each reaches is in the docstring of
# test_gpu_lrt_edges.py
DESIGNS = ((3, 2), (4, 3), (4, 4), (5, 2), (8, 2), (7, 3), (8, 4), (6, 5),
           (8, 8), (9, 2), (16, 4), (17, 3), (24, 4), (25, 2), (32, 8))
FAMILIES = ('benign', 'sparse', 'large', 'lowdisp', 'highdisp', 'widef',
            'differential')
NPIX = 32
EPS = 2.2e-16
TOL_MU = 1e-12
TOL_MU_NR = 1e-14
RTOL_P = 1e-6
LN_MIN_SUBNORMAL = -744.4400719213812   # ln(5e-324)
SUBNORMAL = 2.2250738585072014e-308     # below it a double is subnormal


def llr_bound(R, S):
    return (8 + R) * EPS * np.asarray(S, dtype=np.float64)


def _wide(m1, cond):
    return np.asarray(m1)[:, cond]


def llr_simple(raw, f, aw, cond, m0, m1):
    """The simplified llr (lrt_pixel, csrc/h3d_model.h) in plain float64."""
    x = raw.astype(np.float64)
    r = 1.0 / aw
    m0 = np.asarray(m0)[:, None]
    m1 = _wide(m1, cond)
    return (x * np.log(m0 / m1)
            - (r + x) * np.log((r + m0 * f) / (r + m1 * f))).sum(axis=1)


def scale_S(raw, f, aw, cond, m0, m1):
    x = raw.astype(np.float64)
    r = 1.0 / aw
    m0 = np.asarray(m0)[:, None]
    m1 = _wide(m1, cond)
    return (x * np.abs(np.log(m0 / m1)) + (r + x) * (
        np.abs(np.log((r + m0 * f) / (r + m1 * f))) + 1)).sum(axis=1)


class Design:
    """One design's cells, the families concatenated: n = 7 x 32 pixels."""

    def __init__(self, g, R, C):
        key = 'R%dC%d_' % (R, C)
        self.R, self.C = R, C
        self.cond = g[key + 'cond']
        self.redraws = g[key + 'redraws']
        self.oracle_err = g[key + 'oracle_err']

        def flat(name):
            v = g[key + name]
            return np.ascontiguousarray(v.reshape((-1,) + v.shape[2:]))
        self.raw, self.f, self.disp = flat('raw'), flat('f'), flat('disp')
        self.n = len(self.raw)
        self.disp_wide = np.ascontiguousarray(self.disp[:, self.cond])
        self.ref = {}
        for refit, tag in ((True, ''), (False, '_nr')):
            self.ref[refit] = {k: flat(k + tag).astype(np.float64)
                               for k in ('mu0', 'mu1', 'llr', 'p', 'lnp', 'S',
                                         'p_lo', 'p_hi')}
        # the (D, C) table and dist that give every pixel its own dispersions
        rng = np.random.default_rng(R * 100 + C)
        self.dist = rng.permutation(self.n).astype(np.int32)
        self.table = np.empty_like(self.disp)
        self.table[self.dist] = self.disp

    def family_slices(self):
        return [(fam, slice(i * NPIX, (i + 1) * NPIX))
                for i, fam in enumerate(FAMILIES)]


_cache = {}


def design(R, C):
    if 'g' not in _cache:
        _cache['g'] = golden('unit_lrt_mp.npz')
    if (R, C) not in _cache:
        _cache[(R, C)] = Design(_cache['g'], R, C)
    return _cache[(R, C)]


def _rel(got, ref):
    with np.errstate(all='ignore'):
        e = np.abs(got - ref) / np.abs(ref)
    e[got == ref] = 0
    return e


def figures(d, got, refit):
    """Per family: every checked quantity in units of its bound (<= 1
    passes), and the raw errors they come from. ``got`` = (p, llr, mu0,
    mu1) over the design's n pixels."""
    import scipy.stats as stats
    from test_special_host import igam_err
    p, llr, m0, m1 = got
    ref = d.ref[refit]
    df = d.C - 1
    out = {}
    for fam, s in d.family_slices():
        r = {k: v[s] for k, v in ref.items()}
        ps, ls = p[s], llr[s]
        fig = {}
        mu_err = max(_rel(m0[s], r['mu0']).max(), _rel(m1[s], r['mu1']).max())
        fig['mu'] = float(mu_err)
        fig['mu_units'] = fig['mu'] / (TOL_MU if refit else TOL_MU_NR)
        B = llr_bound(d.R, r['S'])
        fig['llr_units'] = float(np.max(np.abs(ls - r['llr']) / B))
        fig['llr_abs'] = float(np.max(np.abs(ls - r['llr'])))
        # p against scipy at the implementation's own llr
        x2k = -2 * ls
        pos = x2k > 0
        fig['p_one'] = bool(np.all(ps[~pos] == 1.0))
        sf = stats.chi2.sf(x2k, df)
        # (scipy returns 0 for a subnormal tail, see the module docstring)
        pos &= ~((sf == 0) & (ps < SUBNORMAL))
        a = np.full(int(pos.sum()), df / 2.0)
        fig['p_sf_units'] = igam_err(ps[pos], sf[pos], a,
                                     x2k[pos] / 2) if pos.any() else 0.0
        # p inside the interval the llr bound allows (ends from mp): as
        # written at a normal end, one unit of the subnormal grid beyond a
        # subnormal one
        x2 = -2 * r['llr']
        lo, hi = r['p_lo'], r['p_hi']
        unit = 2.0 ** -1074
        out_lo = (lo - np.where(lo < SUBNORMAL, unit, 0.0)) - ps
        out_hi = ps - (hi + np.where(hi < SUBNORMAL, unit, 0.0))
        worst = np.maximum(out_lo, out_hi)
        fig['p_interval_ok'] = bool(np.all(worst <= 0))
        with np.errstate(all='ignore'):
            fig['p_interval_out'] = float(np.max(np.where(
                worst > 0, worst / np.maximum(hi, unit), 0.0)))
        # the project's p bar
        ok = (r['p'] >= 1e-300) & (x2 >= 1e-6)
        fig['p_rel'] = float(_rel(ps[ok], r['p'][ok]).max()) if ok.any() else 0.0
        fig['p_rel_units'] = fig['p_rel'] / RTOL_P
        # underflow
        under = r['lnp'] < LN_MIN_SUBNORMAL
        fig['n_underflow'] = int(under.sum())
        fig['underflow_ok'] = bool(np.all((ps[under] == 0) | (ps[under] <= hi[under])))
        out[fam] = fig
    return out


UNIT_KEYS = ('mu_units', 'llr_units', 'p_sf_units', 'p_rel_units')


def check(d, got, refit, what):
    """Print every figure, then assert every bound."""
    figs = figures(d, got, refit)
    for fam, fig in figs.items():
        print('%s R=%d C=%d refit=%d %-12s %s' % (
            what, d.R, d.C, refit, fam,
            ' '.join('%s=%.3g' % (k, v) for k, v in fig.items())))
    bad = []
    for fam, fig in figs.items():
        for k in UNIT_KEYS:
            if not fig[k] <= 1:
                bad.append((fam, k, fig[k]))
        for k in ('p_one', 'p_interval_ok', 'underflow_ok'):
            if not fig[k]:
                bad.append((fam, k, fig[k]))
    assert not bad, (what, d.R, d.C, refit, bad)
    return figs
