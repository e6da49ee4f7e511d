"""Alternative models (reference analysis/alternatives.py, SURVEY.md §8(f)
#4) vs the reference's own outputs (tests/golden/alt_small2.npz, written by
tests/golden/make_golden.py running the reference): the oracle restatement on
the CPU, the product classes (Poisson / MME / one-segment qcml kernels) on the
GPU.

Parity bar: p / q within 1e-6 relative (north star), closed-form Poisson means
and MME dispersions to ~1e-13, loop_idx bit-exact, identical calls."""
import os
import shutil
import tempfile
import warnings

import numpy as np
import pandas as pd
import pytest

import oracle
from conftest import e2e_inputs, golden, rel_err

CLASSES = ['Poisson3DeFDR', 'Unsmoothed3DeFDR', 'Global3DeFDR']


def _inputs(g, kw, chrom):
    bias = oracle.load_bias([p.replace('<chrom>', chrom)
                             for p in kw['bias_patterns']])
    di = g['disp_idx__%s' % chrom]
    row, col = g['row__%s' % chrom][di], g['col__%s' % chrom][di]
    f = bias[row] * bias[col] * g['size_factors__%s' % chrom][di]
    return g['raw__%s' % chrom][di], f, g['scaled__%s' % chrom][di]


def test_oracle_poisson_lrt_vs_reference():
    g, kw = e2e_inputs('small2')
    alt = golden('alt_small2.npz')
    for c in kw['chroms']:
        raw, f, _ = _inputs(g, kw, c)
        p, llr, m0, m1 = oracle.poisson_lrt(raw, f, kw['design'])
        assert rel_err(p, alt['Poisson3DeFDR__pvalues__%s' % c]) < 1e-12
        assert rel_err(llr, alt['Poisson3DeFDR__llr__%s' % c]) < 1e-12
        assert rel_err(m0, alt['Poisson3DeFDR__mu_hat_null__%s' % c]) < 1e-15
        assert rel_err(m1, alt['Poisson3DeFDR__mu_hat_alt__%s' % c]) < 1e-15


def test_oracle_mme_per_pixel_vs_reference():
    g, kw = e2e_inputs('small2')
    alt = golden('alt_small2.npz')
    design = kw['design']
    for c in kw['chroms']:
        _, _, scaled = _inputs(g, kw, c)
        disp = np.stack([np.maximum(oracle.mme_per_pixel(scaled[:, design[:, k]]),
                                    1e-7) for k in range(design.shape[1])], 1)
        assert rel_err(disp, alt['Unsmoothed3DeFDR__disp__%s' % c]) < 1e-15


@pytest.mark.gpu
@pytest.mark.parametrize('cls', CLASSES)
def test_alternative_run_to_qvalues_matches_reference(cls):
    from hic3defdr_amd.analysis import alternatives
    g, kw = e2e_inputs('small2')
    alt = golden('alt_small2.npz')
    outdir = tempfile.mkdtemp(prefix='h3d_alt_')
    try:
        design = pd.DataFrame(kw['design'], index=kw['reps'],
                              columns=kw['conds'])
        h = getattr(alternatives, cls)(
            raw_npz_patterns=kw['raw_npz_patterns'],
            bias_patterns=kw['bias_patterns'], chroms=kw['chroms'],
            design=design, outdir=outdir,
            dist_thresh_max=kw['dist_thresh_max'],
            loop_patterns=kw['loop_patterns'])
        h.run_to_qvalues(verbose=False)
        # Global: Brent on one pooled segment (qcml tolerance). Unsmoothed:
        # (var - mean) / mean^2 of the product's own scaled values, whose
        # ~1e-13 size-factor differences the var - mean cancellation
        # amplifies (measured 2.3e-12). Poisson: zeros.
        tol_disp = {'Global3DeFDR': 1e-6, 'Unsmoothed3DeFDR': 1e-9,
                    'Poisson3DeFDR': 1e-13}[cls]
        for c in kw['chroms']:
            def ld(st):
                return np.load(os.path.join(outdir, '%s_%s.npy' % (st, c)))
            ref = lambda st: alt['%s__%s__%s' % (cls, st, c)]  # noqa: E731
            np.testing.assert_array_equal(ld('loop_idx'), ref('loop_idx'))
            assert rel_err(ld('disp'), ref('disp')) < tol_disp
            if cls == 'Unsmoothed3DeFDR':
                # pixels floored at disp = 1e-7 (r = 1e7): logpmf's
                # lgamma(r + k) - lgamma(r) cancels ~1e8-sized terms, so llr
                # carries ~1e-8 absolute rounding in ANY implementation, and
                # p = chi2(1).sf(-2 llr) has an infinite slope at llr -> 0.
                # There: llr to 1e-6 absolute; elsewhere the 1e-6 p bar.
                ok = ref('disp').min(axis=1) > 1e-6
                assert np.max(np.abs(ld('llr') - ref('llr'))) < 1e-6
                assert rel_err(ld('pvalues')[ok], ref('pvalues')[ok]) < 1e-6
            else:
                assert rel_err(ld('pvalues'), ref('pvalues')) < 1e-6
                assert rel_err(ld('qvalues'), ref('qvalues')) < 1e-6
            assert rel_err(ld('mu_hat_null'), ref('mu_hat_null')) < 1e-8
            assert rel_err(ld('mu_hat_alt'), ref('mu_hat_alt')) < 1e-8
            for fdr in (0.01, 0.05, 0.1):
                np.testing.assert_array_equal(ld('qvalues') < fdr,
                                              ref('qvalues') < fdr)
        key = '%s__disp_per_dist' % cls
        if key in alt.files:
            dpd = np.load(os.path.join(outdir, 'disp_per_dist.npy'))
            assert rel_err(dpd, alt[key]) < tol_disp
    finally:
        shutil.rmtree(outdir, ignore_errors=True)


@pytest.mark.gpu
def test_poisson_lrt_refit_false_raises_like_reference():
    from hic3defdr_amd.analysis.alternatives import poisson_lrt
    with pytest.raises(ValueError):
        poisson_lrt(np.ones((3, 4), dtype=np.int64), np.ones((3, 4)),
                    np.array([[1, 0], [1, 0], [0, 1], [0, 1]], dtype=bool),
                    refit_mu=False)


# ---- every k_lrt_poisson / k_mme_per_pixel instantiation ------------------

EPS = 2.2e-16


def _alt_inputs(R, C):
    """n = 300 pixels: mu 1e-1 .. 1e3, f 0.1 .. 10, 20 % of the counts
    zeroed (all-zero conditions and pixels included); the last condition has
    a single replicate (MME: NaN), so (18, 2) has one of 17 (the pairwise
    branch of np_sum_mask, >= 8 per condition) -- and a two-condition design
    has one condition with an MME value, the other all NaN."""
    rng = np.random.default_rng(100 * R + C)
    n = 300
    cond = np.r_[np.arange(C), rng.integers(0, C - 1, R - C)]
    rng.shuffle(cond)
    mu = 10 ** rng.uniform(-1, 3, (n, 1))
    f = 10 ** rng.uniform(-1, 1, (n, R))
    raw = rng.poisson(mu * f).astype(np.int64)
    raw[rng.random((n, R)) < 0.2] = 0
    design = np.eye(C, dtype=bool)[cond]
    assert np.any(raw[:, design[:, 0]].sum(axis=1) == 0)
    assert np.bincount(cond)[C - 1] == 1
    return raw, f, cond.astype(np.int32), design


@pytest.fixture(scope='module')
def alt_ctx():
    from hic3defdr_amd import _native
    return _native.context(0)


@pytest.mark.gpu
@pytest.mark.parametrize('R,C', [(4, 2), (4, 3), (7, 2), (8, 4), (12, 5),
                                 (18, 2), (32, 8)])
def test_poisson_lrt_instantiations_vs_oracle(alt_ctx, R, C):
    """k_lrt_poisson<4,2>, <4,4>, <8,4> (R = 7 and 8), <16,8>, <32,8> (R = 18
    and 32) against oracle.poisson_lrt. Means: 64 eps relative (positive-term
    sums; a product may fuse into the sum). llr: (8 + R) eps sum_k (|x ln m| +
    lgamma(x + 1) + m) over both rows. p: scipy's chi2.sf at the kernel's own
    llr within igam_err's tolerance."""
    import scipy.special as sc
    import scipy.stats as stats
    from test_special_host import igam_err
    raw, f, cond, design = _alt_inputs(R, C)
    if (R, C) == (18, 2):
        assert np.bincount(cond).max() >= 8
    p, llr, m0, m1 = alt_ctx.lrt_poisson(raw, f, cond, C)
    with np.errstate(all='ignore'):
        rp, rllr, rm0, rm1 = oracle.poisson_lrt(raw, f, design)
    np.testing.assert_array_equal(np.isnan(m1), np.isnan(rm1))
    assert not np.isnan(m0).any() and not np.isnan(llr).any()
    e0, e1 = rel_err(m0, rm0), rel_err(m1, rm1)
    x = raw.astype(float)
    scale = np.zeros(len(raw))
    for m in (rm0[:, None] * f, np.dot(rm1, design.T) * f):
        with np.errstate(all='ignore'):
            xl = np.where(x > 0, np.abs(x * np.log(m)), 0.0)
        scale += (xl + sc.gammaln(x + 1) + m).sum(axis=1)
    bound = (8 + R) * EPS * scale
    tiny = bound == 0        # an all-zero pixel: llr = 0 exactly
    assert np.all(llr[tiny] == rllr[tiny])
    units = float(np.max(np.abs(llr - rllr)[~tiny] / bound[~tiny]))
    x2 = -2 * llr
    pos = x2 > 0
    sf = stats.chi2.sf(x2, C - 1)
    pos &= ~((sf == 0) & (p < 2.2250738585072014e-308))  # scipy flushes
    perr = igam_err(p[pos], sf[pos], np.full(int(pos.sum()), (C - 1) / 2.0),
                    x2[pos] / 2)
    print('poisson R=%d C=%d mu0=%.3g mu1=%.3g (of 64 eps = %.3g) '
          'llr=%.3g of its bound, p=%.3g of igam_err tol'
          % (R, C, e0, e1, 64 * EPS, units, perr))
    assert e0 <= 64 * EPS and e1 <= 64 * EPS
    assert units <= 1
    assert np.all(p[x2 <= 0] == 1.0)
    assert perr < 1


@pytest.mark.gpu
@pytest.mark.parametrize('R,C', [(4, 2), (7, 2), (18, 2)])
def test_mme_per_pixel_instantiations_vs_oracle(alt_ctx, R, C):
    """k_mme_per_pixel<4>, <8>, <32> against oracle.mme_per_pixel: the NaN
    layout (a single-replicate condition, an all-zero condition) matches, and
    |delta| <= 64 eps (var + m) / m^2."""
    raw, f, cond, design = _alt_inputs(R, C)
    got = alt_ctx.mme_per_pixel(raw.astype(np.float64), f, cond, C)
    worst = 0.0
    for c in range(C):
        data = raw[:, design[:, c]] / f[:, design[:, c]]
        with np.errstate(all='ignore'), warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)   # ddof = n = 1
            ref = oracle.mme_per_pixel(data)
            m = data.mean(axis=1)
            bound = 64 * EPS * (data.var(axis=1, ddof=1) + m) / m ** 2
        np.testing.assert_array_equal(np.isnan(got[:, c]), np.isnan(ref))
        ok = ~np.isnan(ref)
        if design[:, c].sum() == 1:
            assert not ok.any()
        else:
            assert ok.sum() > 100
            worst = max(worst, float(np.max(
                np.abs(got[ok, c] - ref[ok]) / bound[ok])))
    print('mme R=%d C=%d: %.3g of its bound' % (R, C, worst))
    assert worst <= 1
