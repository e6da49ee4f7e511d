"""The diagnostics kernels (csrc/h3d_diag.hip) behind util/diagnostics.py and
the DiagnosticHiC3DeFDR methods, against the numpy / scipy expressions the
reference's plotting modules evaluate (tests/diag_cases.py). Sums are held
to derived bounds, counts, ranks and labels to equality, reruns to the same
bits."""
import shutil
import tempfile

import numpy as np
import pandas as pd
import pytest
import scipy.stats as st

from conftest import e2e_inputs

import diag_cases as dc
from diag_cases import U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def diag():
    from hic3defdr_amd.util import diagnostics
    return diagnostics


@pytest.fixture(scope='module')
def ctx():
    from hic3defdr_amd import _native
    return _native.context(0)


def rel_close(got, want, tol, what):
    """|got - want| <= tol * |want| where want is finite; the same
    non-finite values elsewhere."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, what
    fin = np.isfinite(want)
    np.testing.assert_array_equal(got[~fin], want[~fin], what)
    err = np.abs(got - want)[fin]
    bound = tol * np.abs(want)[fin]
    print('%s: worst |err| / bound = %.3f' % (
        what, float(np.max(err / np.maximum(bound, 1e-300)))
        if err.size else 0.))
    assert np.all(err <= bound), what


# -- dd_curves ----------------------------------------------------------------

@pytest.fixture(scope='module')
def dd_tables():
    return {R: dc.dd_table(400, R, seed=R) for R in (1, 4, 9, 32)}


@pytest.mark.parametrize('R', [1, 4, 9, 32])
def test_dd_curves(diag, dd_tables, R):
    from hic3defdr_amd import _native
    t = dd_tables[R]
    before = dc.balanced_ref(t['raw'], t['bias'], t['row'], t['col'])
    assert np.isinf(before).any() and np.isnan(before).any()
    bs, bm, am, members = dc.dd_curves_ref(t['row'], t['col'], before,
                                           t['scaled'])
    assert members[2] == 0 and members[0] > 0 and len(bs) >= 30
    got_bs, got_b, got_a = diag.dd_curves(t['row'], t['col'], before,
                                          t['scaled'])
    np.testing.assert_array_equal(got_bs, bs)
    assert not np.isfinite(bm).all()
    dc.assert_sum_bound(got_b, bm, members, 'before R=%d' % R)
    dc.assert_sum_bound(got_a, am, members, 'after R=%d' % R)
    assert (got_a[2] == 0).all() and (got_b[2] == 0).all()
    # a rerun and a second context: the same bits
    again = diag.dd_curves(t['row'], t['col'], before, t['scaled'])
    dc.same_bits(again[1], got_b)
    dc.same_bits(again[2], got_a)
    other = _native.Context(0)
    try:
        keys = np.where(diag.dd_bins(t['col'] - t['row']) > 0,
                        diag.dd_bins(t['col'] - t['row']), -1)
        vals = np.concatenate([before, t['scaled']], axis=1)
        s1, c1 = other.group_sums(keys, vals, 102)
        s2, c2 = _native.context(0).group_sums(keys, vals, 102)
        dc.same_bits(s1, s2)
        np.testing.assert_array_equal(c1, c2)
        np.testing.assert_array_equal(c1[1:len(bs) + 1], members)
    finally:
        other.close()


def test_dd_curves_beyond_distance_1000(diag):
    t = dc.dd_table(1200, 4, seed=77, far=True)
    before = dc.balanced_ref(t['raw'], t['bias'], t['row'], t['col'])
    bs, bm, am, members = dc.dd_curves_ref(t['row'], t['col'], before,
                                           t['scaled'])
    assert bs[-1] == 101 and members[100] >= 3 and members[99] >= 1
    got_bs, got_b, got_a = diag.dd_curves(t['row'], t['col'], before,
                                          t['scaled'])
    np.testing.assert_array_equal(got_bs, bs)
    dc.assert_sum_bound(got_b, bm, members, 'before, far')
    dc.assert_sum_bound(got_a, am, members, 'after, far')


@pytest.mark.parametrize('n', dc.TAILS)
def test_dd_curves_launch_tails(diag, dd_tables, n):
    t = dd_tables[4]
    row, col = t['row'][:n], t['col'][:n]
    after = t['scaled'][:n]
    before = dc.balanced_ref(t['raw'], t['bias'], t['row'], t['col'])[:n]
    got = diag.dd_curves(row, col, before, after)
    if n == 0:
        assert got[0].shape == (0,) and got[1].shape == got[2].shape == (0, 4)
        return
    bs, bm, am, members = dc.dd_curves_ref(row, col, before, after)
    np.testing.assert_array_equal(got[0], bs)
    dc.assert_sum_bound(got[1], bm, members, 'before n=%d' % n)
    dc.assert_sum_bound(got[2], am, members, 'after n=%d' % n)


def test_group_sums_dev_matches_host(ctx):
    import torch
    t = dc.dd_table(400, 4, seed=4)
    keys = (t['col'] - t['row']).astype(np.int32)
    keys[::7] = -1
    vals = t['scaled']
    s, c = ctx.group_sums(keys, vals, 400)
    ds, dcnt = ctx.group_sums_dev(torch.from_numpy(keys).cuda(),
                                  torch.from_numpy(vals).cuda(), 400)
    dc.same_bits(ds.cpu().numpy(), s)
    np.testing.assert_array_equal(dcnt.cpu().numpy(), c)
    np.testing.assert_array_equal(
        c, np.bincount(keys[keys >= 0], minlength=400))


# -- value_histogram -----------------------------------------------------------

@pytest.mark.parametrize('edges', [np.linspace(0, 1, 21),
                                   np.array([0.05, 0.95]),
                                   np.linspace(-0.25, 1.25, 4097)],
                         ids=['E21', 'E2', 'E4097'])
def test_value_histogram_edges_and_drops(diag, ctx, edges):
    import torch
    v = dc.edge_values()
    counts, e = diag.value_histogram(v, edges)
    assert counts.dtype == np.int64
    np.testing.assert_array_equal(e, edges)
    np.testing.assert_array_equal(counts, np.histogram(v, bins=edges)[0])
    dev = ctx.histogram_dev(torch.from_numpy(v).cuda(), edges)
    np.testing.assert_array_equal(dev.cpu().numpy(), counts)


def test_value_histogram_default_edges_and_tails(diag):
    v = dc.edge_values()
    for n in dc.TAILS:
        counts, e = diag.value_histogram(v[:n])
        np.testing.assert_array_equal(e, np.linspace(0, 1, 21))
        np.testing.assert_array_equal(counts, np.histogram(v[:n], bins=e)[0])


def test_value_histogram_three_million(diag):
    rng = np.random.default_rng(9)
    v = rng.uniform(-0.1, 1.1, 3_000_000)
    v[::1000] = np.nan
    with np.errstate(invalid='ignore'):
        dropped = int((~((v >= 0) & (v <= 1))).sum())
    counts, e = diag.value_histogram(v)
    assert counts.sum() == len(v) - dropped
    np.testing.assert_array_equal(counts, np.histogram(v, bins=e)[0])


# -- ma_stats -------------------------------------------------------------------

@pytest.fixture(scope='module')
def ma_cases():
    out = {}
    for name in dc.DESIGNS:
        c = dc.ma_case(name)
        c['ref'] = dc.ma_ref(c['scaled'], c['design'], c['cond_idx'],
                             c['qvalues'], c['fdr'], c['loop_idx'])
        out[name] = c
    return out


def check_ma(got, ref, what):
    mean, m, a, label = ref
    rel_close(got['mean'], mean, 4 * U, what + ' mean')
    with np.errstate(all='ignore'):
        l0, l1 = np.abs(np.log2(mean[:, 0])), np.abs(np.log2(mean[:, 1]))
    scale = np.maximum(1.0, np.maximum(l0, l1))
    for k, want in (('m', m), ('a', a)):
        fin = np.isfinite(want)
        np.testing.assert_array_equal(got[k][~fin], want[~fin], what + k)
        assert np.all(np.abs(got[k] - want)[fin] <= (8 * U * scale)[fin]), \
            what + ' ' + k
    assert got['label'].dtype == np.int8
    cmp_ = np.abs(m) > 1e-12
    np.testing.assert_array_equal(got['label'][cmp_], label[cmp_], what)
    return cmp_


@pytest.mark.parametrize('name', sorted(dc.DESIGNS))
def test_ma_stats(diag, ma_cases, name):
    c = ma_cases[name]
    design = pd.DataFrame(c['design'], columns=c['names'])
    got = diag.ma_stats(c['scaled'], design, c['conds'], c['qvalues'],
                        c['fdr'], loop_idx=c['loop_idx'])
    cmp_ = check_ma(got, c['ref'], name)
    # at most 1 % of the significant pixels stay out of the label comparison
    sig = (c['ref'][3] >= 2) | (c['ref'][3] == -1)
    assert (sig & ~cmp_).sum() <= 0.01 * sig.sum()
    # the planted ties and the 0 / 0 pixel: in no series, on both sides
    np.testing.assert_array_equal(got['label'][:6], [-1, -1, -1, -1, 3, 2])
    np.testing.assert_array_equal(c['ref'][3][:6], [-1, -1, -1, -1, 3, 2])
    assert np.isnan(got['m'][3]) and got['m'][4] == -np.inf and \
        got['m'][5] == np.inf
    assert np.isnan(c['qvalues']).any()
    # loop_idx=None: every pixel a loop pixel
    loops = c['loop_idx']
    sub = diag.ma_stats(c['scaled'][loops], design, c['conds'], c['qvalues'],
                        c['fdr'])
    ref = dc.ma_ref(c['scaled'][loops], c['design'], c['cond_idx'],
                    c['qvalues'], c['fdr'])
    check_ma(sub, ref, name + ' loops only')
    assert (sub['label'] != 0).all()
    dc.same_bits(sub['m'], got['m'][loops])
    np.testing.assert_array_equal(sub['label'], got['label'][loops])
    # an integer design with condition indices
    again = diag.ma_stats(c['scaled'], c['design'], c['cond_idx'],
                          c['qvalues'], c['fdr'], loop_idx=loops)
    for k in ('mean', 'm', 'a', 'label'):
        dc.same_bits(again[k], got[k])


@pytest.mark.parametrize('n', dc.TAILS)
def test_ma_stats_launch_tails(diag, ma_cases, n):
    c = ma_cases['3+1+2']
    design = pd.DataFrame(c['design'], columns=c['names'])
    full = diag.ma_stats(c['scaled'], design, c['conds'], c['qvalues'],
                         c['fdr'], loop_idx=c['loop_idx'])
    loops = c['loop_idx'][:n]
    got = diag.ma_stats(c['scaled'][:n], design, c['conds'],
                        c['qvalues'][:int(loops.sum())], c['fdr'],
                        loop_idx=loops)
    for k in ('mean', 'm', 'a', 'label'):
        assert len(got[k]) == n
        dc.same_bits(got[k], full[k][:n])


# -- density_grid ---------------------------------------------------------------

@pytest.fixture(scope='module')
def cloud():
    rng = np.random.default_rng(31)
    n = 4097
    x, y = rng.normal(3, 2, n), rng.normal(0, 1.5, n)
    label = rng.integers(-1, 5, n).astype(np.int8)     # -1 and 4: dropped
    xe, ye = np.linspace(-2, 8, 73), np.linspace(-4, 4, 73)
    x[:73], y[73:146] = xe, ye                          # on every edge
    x[200:204] = [np.inf, -np.inf, np.nan, 8.0]
    y[204:208] = [np.inf, -np.inf, np.nan, 4.0]
    return x, y, label, xe, ye


@pytest.mark.parametrize('shape', ['1x1', '72x72', '72x5'])
def test_density_grid(diag, cloud, shape):
    x, y, label, xe, ye = cloud
    if shape == '1x1':
        xe, ye = xe[[0, -1]], ye[[0, -1]]
    elif shape == '72x5':
        ye = ye[::12][:6]
    got = diag.density_grid(x, y, label, 4, xe, ye)
    assert got.dtype == np.int64 and \
        got.shape == (4, len(xe) - 1, len(ye) - 1)
    fin = np.isfinite(x) & np.isfinite(y)
    for l in range(4):
        s = fin & (label == l)
        np.testing.assert_array_equal(
            got[l], np.histogram2d(x[s], y[s], bins=[xe, ye])[0])
    np.testing.assert_array_equal(got, dc.density_ref(x, y, label, 4, xe, ye))
    for n in dc.TAILS:
        np.testing.assert_array_equal(
            diag.density_grid(x[:n], y[:n], label[:n], 4, xe, ye),
            dc.density_ref(x[:n], y[:n], label[:n], 4, xe, ye))


# -- ranks and correlations -------------------------------------------------------

@pytest.fixture(scope='module')
def corr_data():
    return {(R, kind): dc.corr_columns(R, kind)
            for R in (2, 4, 9, 32) for kind in ('counts', 'scaled')}


@pytest.mark.parametrize('kind', ['counts', 'scaled'])
@pytest.mark.parametrize('R', [2, 4, 9, 32])
def test_ranks_equal_scipy_rankdata(diag, ctx, corr_data, R, kind):
    data = corr_data[R, kind]
    ranks, flags = ctx.rank_average(data)
    for c in range(R):
        if np.isnan(data[c]).any():
            assert flags[c] == 1 and np.isnan(ranks[c]).all()
        else:
            assert flags[c] == 0
            np.testing.assert_array_equal(ranks[c], st.rankdata(data[c]))
    # -0.0 and 0.0 are one value
    assert len(set(ranks[0, [0, 1, 2, 3, 5]])) == 1
    dc.same_bits(diag.rank_average(data), ranks)


@pytest.mark.parametrize('n', dc.TAILS)
def test_ranks_launch_tails(diag, n):
    """A column whose tail sorts last: the prefix's ranks are the prefix
    call's, bit for bit."""
    rng = np.random.default_rng(2)
    col = np.concatenate([rng.poisson(3.0, 4097).astype(float)[:n],
                          100.0 + np.arange(64)])
    full = diag.rank_average(col[None, :])[0]
    assert full[n:].tolist() == list(range(n + 1, n + 65))
    got = diag.rank_average(col[None, :n])
    assert got.shape == (1, n)
    dc.same_bits(got[0], full[:n])
    if n:
        np.testing.assert_array_equal(got[0], st.rankdata(col[:n]))


@pytest.mark.parametrize('correlation', ['spearman', 'pearson'])
@pytest.mark.parametrize('kind', ['counts', 'scaled'])
@pytest.mark.parametrize('R', [2, 4, 9, 32])
def test_correlation_matrix(diag, corr_data, R, kind, correlation):
    data = corr_data[R, kind]
    n = data.shape[1]
    got = diag.correlation_matrix(data, correlation=correlation)
    want = dc.scipy_corr(data, correlation)
    assert got.shape == (R, R)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got - want)[ok]
    print('R=%d %s %s: worst |dr| = %.3e (bound %.3e)'
          % (R, kind, correlation, err.max(), 4 * n * U))
    assert err.max() <= 4 * n * U
    dc.same_bits(got, got.T.copy())
    if R >= 4:
        assert np.isnan(got[R - 2]).all() and np.isnan(got[R - 1]).all()
        assert abs(got[0, R - 3] - 1.0) <= 4 * n * U     # identical columns
    dc.same_bits(diag.correlation_matrix(data, correlation=correlation), got)


@pytest.mark.parametrize('n', dc.TAILS)
def test_correlation_launch_tails(diag, corr_data, n):
    data = corr_data[9, 'scaled'][:3, :n]
    for correlation in ('spearman', 'pearson'):
        got = diag.correlation_matrix(data, correlation=correlation)
        if n < 2:
            assert np.isnan(got).all()
            continue
        want = dc.scipy_corr(data, correlation)
        assert np.abs(got - want).max() <= 4 * n * U


# -- mvr_data ---------------------------------------------------------------------

def carried_members(ref):
    """Per distance, the member count of the distance whose mean the
    monotone pass of plotting/dispersion.py:135-144 put there."""
    k, src = np.ones(len(ref['dist_mean']), dtype=np.int64), -1
    for d, v in enumerate(ref['raw_means']):
        if np.isfinite(v) and (src < 0 or v < ref['raw_means'][src]):
            src = d
        if src >= 0:
            k[d] = ref['members'][src]
    return k


@pytest.mark.parametrize('r', [1, 2, 3, 9])
def test_mvr_data(diag, r):
    c = dc.mvr_case(r)
    ref = dc.mvr_ref(c['scaled'], c['dist'], c['disp_fit'],
                     c['disp_per_dist'])
    raw = ref['raw_means']
    assert ref['members'][5] == 0 and np.isnan(raw[5])
    assert raw[9] > raw[8] and raw[12] > raw[11]      # the pass has work
    got = diag.mvr_data(c['scaled'], c['dist'], c['disp_fit'],
                        c['disp_per_dist'])
    rel_close(got['pixel_mean'], ref['pixel_mean'], 8 * U, 'pixel_mean')
    if r == 1:
        assert np.isnan(got['pixel_var']).all() and \
            np.isnan(ref['pixel_var']).all()
    else:
        rel_close(got['pixel_var'], ref['pixel_var'], 8 * U, 'pixel_var')
    np.testing.assert_array_equal(got['dist_range'], ref['dist_range'])
    k = np.maximum(ref['members'], 1)
    dc.assert_sum_bound(got['dist_disp_fit'], ref['dist_disp_fit'], k,
                        'dist_disp_fit')
    # the monotone pass carries the mean of an earlier distance: that
    # distance's member count bounds the carried value
    k_src = carried_members(ref)
    got_mean = got['dist_mean']
    dc.assert_sum_bound(got_mean, ref['dist_mean'], k_src, 'dist_mean')
    assert got_mean[9] == got_mean[8] and np.all(np.diff(got_mean) <= 0)
    np.testing.assert_array_equal(got['dist_per_bin'], ref['dist_per_bin'])
    np.testing.assert_array_equal(got['disp_per_bin'], ref['disp_per_bin'])
    at = np.minimum(ref['dist_per_bin'], len(k_src) - 1)
    dc.assert_sum_bound(got['mean_per_bin'], ref['mean_per_bin'], k_src[at],
                        'mean_per_bin')
    # the distance= branch (analysis/plotting.py:132-140)
    one = diag.mvr_data(c['scaled'], c['dist'], c['disp_fit'],
                        c['disp_per_dist'], distance=7)
    at = c['dist'] == 7
    dc.same_bits(one['pixel_mean'], got['pixel_mean'][at])
    dc.same_bits(one['pixel_var'], got['pixel_var'][at])
    np.testing.assert_array_equal(
        one['pixel_disp_fit'], np.ones(at.sum()) * c['disp_per_dist'][7])
    assert one['dist_mean'] is None and one['dist_per_bin'] is None


@pytest.mark.parametrize('n', dc.TAILS)
def test_pixel_moments_launch_tails(ctx, diag, n):
    c = dc.mvr_case(9)
    wide = np.concatenate([c['scaled'], c['scaled'][:, :3] * 0.5], axis=1)
    reps = np.array([0, 2, 3, 4, 5, 7, 8, 10, 11], dtype=np.int32)
    if n == 0:
        out = diag.mvr_data(c['scaled'][:0], c['dist'][:0], c['disp_fit'][:0])
        assert out['pixel_mean'].shape == (0,) and out['dist_mean'] is None
        return
    full_m, full_v = ctx.pixel_moments(wide, reps)
    m, v = ctx.pixel_moments(wide[:n], reps)
    dc.same_bits(m, full_m[:n])
    dc.same_bits(v, full_v[:n])
    rel_close(m, np.mean(wide[:n][:, reps], axis=1), 8 * U, 'mean')
    rel_close(v, np.var(wide[:n][:, reps], ddof=1, axis=1), 8 * U, 'var')


# -- through the class ---------------------------------------------------------------

@pytest.fixture(scope='module')
def small2_run():
    from hic3defdr_amd import HiC3DeFDR
    g, kw = e2e_inputs('small2')
    outdir = tempfile.mkdtemp(prefix='h3d_diag_')
    design = pd.DataFrame(kw['design'], index=kw['reps'], columns=kw['conds'])
    h = HiC3DeFDR(raw_npz_patterns=kw['raw_npz_patterns'],
                  bias_patterns=kw['bias_patterns'], chroms=kw['chroms'],
                  design=design, outdir=outdir,
                  dist_thresh_max=kw['dist_thresh_max'],
                  loop_patterns=kw['loop_patterns'], res=10000)
    h.run_to_qvalues(verbose=False)
    yield h, kw, g
    h.flush()
    shutil.rmtree(outdir, ignore_errors=True)


def test_class_dd_curves(small2_run):
    h, kw, g = small2_run
    chrom = kw['chroms'][0]
    row, col = h.load_data('row', chrom), h.load_data('col', chrom)
    before = dc.balanced_ref(h.load_data('raw', chrom), h.load_bias(chrom),
                             row, col)
    bs, bm, am, members = dc.dd_curves_ref(row, col, before,
                                           h.load_data('scaled', chrom))
    got_bs, got_b, got_a, names = h.dd_curves(chrom)
    assert names == kw['reps']
    np.testing.assert_array_equal(got_bs, bs)
    # (the device forms balanced with numpy's own two operations)
    dc.assert_sum_bound(got_b, bm, members, 'class before')
    dc.assert_sum_bound(got_a, am, members, 'class after')


def test_class_distributions(small2_run):
    h, kw, g = small2_run
    e = np.linspace(0, 1, 21)
    loop_idx, _ = h.load_data('loop_idx', 'all')
    p_all, _ = h.load_data('pvalues', 'all')
    q_all, _ = h.load_data('qvalues', 'all')
    for idx, values in (('disp', p_all), ('loop', p_all[loop_idx])):
        counts, edges = h.pvalue_distribution(idx=idx)
        np.testing.assert_array_equal(edges, e)
        np.testing.assert_array_equal(counts,
                                      np.histogram(values, bins=e)[0])
    counts, edges = h.qvalue_distribution()
    np.testing.assert_array_equal(counts, np.histogram(q_all, bins=e)[0])
    assert counts.sum() == np.isfinite(q_all).sum() > 0
    with pytest.raises(ValueError, match='idx must be loop or disp'):
        h.pvalue_distribution(idx='x')


@pytest.mark.parametrize('include_non_loops', [True, False])
def test_class_ma_data(small2_run, include_non_loops):
    h, kw, g = small2_run
    disp_idx, _ = h.load_data('disp_idx', 'all')
    loop_idx, _ = h.load_data('loop_idx', 'all')
    scaled, _ = h.load_data('scaled', 'all', idx=disp_idx)
    q, _ = h.load_data('qvalues', 'all')
    design = np.asarray(h.design, dtype=bool)
    if include_non_loops:
        ref = dc.ma_ref(scaled, design, [0, 1], q, 0.05, loop_idx)
    else:
        ref = dc.ma_ref(scaled[loop_idx], design, [0, 1], q, 0.05)
    xe, ye = np.linspace(-2, 12, 73), np.linspace(-4, 4, 73)
    got = h.ma_data(include_non_loops=include_non_loops, grid=(xe, ye))
    assert got['conds'] == kw['conds'][:2]
    check_ma(got, ref, 'class')
    assert (0 in got['label']) == include_non_loops
    np.testing.assert_array_equal(
        got['density'], dc.density_ref(got['a'], got['m'], got['label'], 4,
                                       xe, ye))
    assert got['density'].sum() > 0


@pytest.mark.parametrize('correlation', ['spearman', 'pearson'])
@pytest.mark.parametrize('idx', ['loop', 'disp'])
def test_class_correlation_matrix(small2_run, idx, correlation):
    h, kw, g = small2_run
    disp_idx, _ = h.load_data('disp_idx', 'all')
    sel = disp_idx if idx == 'disp' else \
        (disp_idx, h.load_data('loop_idx', 'all')[0])
    data = h.load_data('scaled', 'all', idx=sel)[0].T
    got, names = h.correlation_matrix(idx=idx, correlation=correlation)
    assert names == kw['reps']
    want = dc.scipy_corr(np.ascontiguousarray(data), correlation)
    assert np.abs(got - want).max() <= 4 * data.shape[1] * U
    raw, _ = h.correlation_matrix(stage='raw', idx=idx,
                                  correlation=correlation)
    data = h.load_data('raw', 'all', idx=sel)[0].T.astype(float)
    want = dc.scipy_corr(np.ascontiguousarray(data), correlation)
    assert np.abs(raw - want).max() <= 4 * data.shape[1] * U


def test_class_dispersion_fit_and_ddr(small2_run):
    h, kw, g = small2_run
    disp_idx, _ = h.load_data('disp_idx', 'all')
    row, _ = h.load_data('row', 'all', idx=disp_idx)
    col, _ = h.load_data('col', 'all', idx=disp_idx)
    dist = col - row
    for ci, cond in enumerate(kw['conds']):
        scaled = h.load_data('scaled', 'all', idx=disp_idx)[0][
            :, np.asarray(h.design[cond], dtype=bool)]
        disp = h.load_data('disp', 'all')[0][:, ci]
        dpd = h.load_data('disp_per_dist')[:, ci]
        ref = dc.mvr_ref(np.ascontiguousarray(scaled), dist, disp, dpd)
        got = h.dispersion_fit_data(cond)
        rel_close(got['pixel_mean'], ref['pixel_mean'], 8 * U, 'class mean')
        rel_close(got['pixel_var'], ref['pixel_var'], 8 * U, 'class var')
        np.testing.assert_array_equal(got['pixel_dist'], dist)
        k = np.maximum(ref['members'], 1)
        dc.assert_sum_bound(got['dist_disp_fit'], ref['dist_disp_fit'], k,
                            'class dist_disp_fit')
        dc.assert_sum_bound(got['dist_mean'], ref['dist_mean'],
                            carried_members(ref), 'class dist_mean')
        np.testing.assert_array_equal(got['dist_per_bin'],
                                      ref['dist_per_bin'])
        d = int(ref['dist_per_bin'][len(ref['dist_per_bin']) // 2])
        one = h.dispersion_fit_data(cond, distance=d)
        assert one['pixel_dist'] is None and one['dist_per_bin'] is None
        dc.same_bits(one['pixel_mean'], got['pixel_mean'][dist == d])
        assert (one['pixel_disp_fit'] == dpd[d]).all()
        # ddr_data, and the reference's own disp_per_dist (the e2e bar)
        ddr = h.ddr_data(cond)
        gold = g['disp_per_dist'][:, ci]
        np.testing.assert_array_equal(ddr['dist_per_bin'],
                                      np.flatnonzero(np.isfinite(gold)))
        np.testing.assert_allclose(ddr['disp_per_bin'],
                                   gold[np.isfinite(gold)], rtol=1e-6,
                                   atol=1e-12)
        np.testing.assert_array_equal(
            ddr['xs'], np.arange(ddr['dist_per_bin'].min(),
                                 ddr['dist_per_bin'].max() + 1))
        np.testing.assert_array_equal(ddr['ys'],
                                      h.load_disp_fn(cond)(ddr['xs']))
