"""Dense views on the GPU (h3d_window_gather / h3d_stack_aggregate) behind
select_matrix, make_apa_stack, HiC3DeFDR.get_matrix / apa_stack / apa_mean,
against the reference's own outputs (views.npz, made by
tests/golden/make_golden_views.py)."""
import shutil
import tempfile

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sparse

from conftest import e2e_inputs, golden, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def views():
    return golden('views.npz')


@pytest.fixture(scope='module')
def ctx():
    from hic3defdr_amd import _native
    return _native.context(0)


def golden_clusters(g):
    pts, starts = g['apa_points'], g['apa_starts']
    return [[tuple(int(v) for v in p) for p in pts[a:b]]
            for a, b in zip(starts[:-1], starts[1:])]


def assert_same_bits(a, b):
    """Equal values, NaN in the same places, zeros of the same sign."""
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(np.signbit(a) & ~np.isnan(a),
                                  np.signbit(b) & ~np.isnan(b))


# -- select_matrix ----------------------------------------------------------

def test_select_matrix_matches_reference_bit_for_bit(views):
    from hic3defdr_amd.util.matrices import select_matrix
    row, col, data = views['sel_row'], views['sel_col'], views['sel_data']
    shapes = set()
    for i, (r0, r1, c0, c1, sym) in enumerate(views['sel_windows']):
        got = select_matrix(slice(int(r0), int(r1)), slice(int(c0), int(c1)),
                            row, col, data, symmetrize=bool(sym))
        want = views['sel_out_%d' % i]
        assert got.dtype == np.float64 and got.shape == want.shape
        assert_same_bits(got, want)
        shapes.add(got.shape)
    assert {(5, 7), (65, 3), (1, 1)} <= shapes
    # the planted NaN, inf and -0.0 came through (window 0, 1 and 3)
    k_nan, k_inf, k_nz = views['sel_planted']
    w = views['sel_windows']
    for k, i in ((k_nan, 0), (k_inf, 1), (k_nz, 3)):
        assert w[i, 0] <= row[k] < w[i, 1] and w[i, 2] <= col[k] < w[i, 3]


def test_select_matrix_integer_and_boolean_data(views):
    from hic3defdr_amd.util.matrices import select_matrix
    row, col = views['sel_row'], views['sel_col']
    counts = (np.arange(len(row)) % 7).astype(np.int64)
    rs, cs = slice(40, 52), slice(38, 55)
    want = select_matrix(rs, cs, row, col, counts.astype(np.float64))
    assert_same_bits(select_matrix(rs, cs, row, col, counts), want)
    flags = counts > 2
    got = select_matrix(rs, cs, row, col, flags)
    np.testing.assert_array_equal(got, np.where(np.isnan(want), np.nan,
                                                want > 2))
    empty = select_matrix(slice(5, 5), cs, row, col, counts)
    assert empty.shape == (0, 17)


# -- make_apa_stack ---------------------------------------------------------

def apa_matrix(g):
    n = int(g['apa_size'])
    return sparse.coo_matrix((g['apa_data'], (g['apa_row'], g['apa_col'])),
                             shape=(n, n))


@pytest.mark.parametrize('width,min_dist,key', [
    (5, None, 'apa_stack_w5'), (11, None, 'apa_stack_w11'),
    (5, 3, 'apa_stack_w5_min3')])
def test_make_apa_stack_matches_reference_bit_for_bit(views, width, min_dist,
                                                      key):
    from hic3defdr_amd.util.apa import make_apa_stack
    m = apa_matrix(views)
    nnz_before = m.nnz
    got = make_apa_stack(m, golden_clusters(views), width, min_dist=min_dist)
    want = views[key]
    assert got.shape == want.shape == (len(views['apa_starts']) - 1, width,
                                       width)
    np.testing.assert_array_equal(got, want)
    assert m.nnz == nnz_before      # the caller's matrix is left alone
    # a CSR input with unsorted, repeated entries is canonicalised on a copy
    got2 = make_apa_stack(m.tocsr(), golden_clusters(views), width,
                          min_dist=min_dist)
    np.testing.assert_array_equal(got2, want)


@pytest.mark.parametrize('width', [5, 11])
def test_make_apa_stack_empty_inputs(views, width):
    from hic3defdr_amd.util.apa import make_apa_stack
    n = int(views['apa_size'])
    got = make_apa_stack(apa_matrix(views), [], width)
    assert got.shape == views['apa_none_w%d' % width].shape == (0, width,
                                                                width)
    got = make_apa_stack(sparse.coo_matrix((n, n)), golden_clusters(views),
                         width)
    np.testing.assert_array_equal(got, views['apa_nnz0_w%d' % width])


# -- the ABI's refusals and edge cases --------------------------------------

def test_window_gather_refuses_bad_arguments(ctx):
    from hic3defdr_amd import _native
    ind = np.array([0, 1, 2], dtype=np.int32)
    ptr = np.array([0, 1, 2, 3], dtype=np.int64)
    data = np.arange(6, dtype=np.float64).reshape(3, 2)
    org = np.zeros((1, 2), dtype=np.int32)

    def call(h=2, w=2, cols=(0,), origins=org, indptr=ptr):
        return ctx.window_gather(ind, data, origins, h, w, (3, 3),
                                 indptr=indptr, cols=cols)
    for kw in (dict(h=0), dict(w=0), dict(cols=()), dict(cols=(2,)),
               dict(cols=(0, -1)),
               dict(h=1 << 15, w=1 << 15, origins=np.zeros((2, 2), np.int32)),
               dict(indptr=np.array([0, 2, 1, 3], dtype=np.int64)),
               dict(indptr=np.array([0, 1, 2, 4], dtype=np.int64))):
        with pytest.raises(_native.H3DError) as e:
            call(**kw)
        assert e.value.code == -1, kw
    # no windows, and no entries: both succeed
    assert call(origins=np.zeros((0, 2), np.int32)).shape == (1, 0, 2, 2)
    got = ctx.window_gather(np.zeros(0, np.int32), np.zeros((0, 2)), org, 2,
                            3, (3, 3), indptr=np.zeros(4, np.int64), fill=7.)
    np.testing.assert_array_equal(got, np.full((2, 1, 2, 3), 7.))
    got = ctx.window_gather(np.zeros(0, np.int32), np.zeros(0), org, 2, 3,
                            (0, 0), row=np.zeros(0, np.int32))
    assert np.isnan(got).all() and got.shape == (1, 1, 2, 3)


def test_window_gather_sentinel_and_far_windows(ctx):
    """A window at INT32_MIN rows is NaN whatever the fill; windows anywhere
    in the int32 plane are harmless (absent cells, no wrapped index)."""
    ind = np.array([0, 2, 1], dtype=np.int32)
    ptr = np.array([0, 2, 3, 3], dtype=np.int64)
    data = np.array([1., 2., 3.])
    lo, hi = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    org = np.array([[lo, 0], [0, 0], [hi - 1, hi - 1], [lo + 1, lo], [-1, -1],
                    [hi, 0], [0, hi]], dtype=np.int32)
    got = ctx.window_gather(ind, data, org, 3, 3, (3, 3), indptr=ptr,
                            fill=-5.)[0]
    assert np.isnan(got[0]).all()
    np.testing.assert_array_equal(got[1], [[1, -5, 2], [-5, 3, -5],
                                           [-5, -5, -5]])
    for k in (2, 3, 5, 6):
        np.testing.assert_array_equal(got[k], np.full((3, 3), -5.))
    np.testing.assert_array_equal(got[4], [[-5, -5, -5], [-5, 1, -5],
                                           [-5, -5, 3]])
    sym = ctx.window_gather(ind, data, org[1:2], 3, 3, (3, 3), indptr=ptr,
                            symmetrize=True)[0, 0]
    np.testing.assert_array_equal(sym, [[1, np.nan, 2], [np.nan, 3, np.nan],
                                        [2, np.nan, np.nan]])


def test_window_gather_dev_equals_host_entry(views, ctx):
    """The device-pointer entry on torch tensors, from row pointers and from
    the sorted rows, = the host entry bit for bit (stack and mean mode)."""
    import torch
    from hic3defdr_amd.util.matrices import check_table
    row, col = check_table(views['sel_row'], views['sel_col'])
    d = views['sel_data']
    data = np.ascontiguousarray(np.stack([d, 2 * d, d + 1], axis=1))
    n_bins, cols = 200, [2, 0]
    org = np.array([[50, 50], [-3, -2], [np.iinfo(np.int32).min, 7],
                    [195, 190], [36, 30]], dtype=np.int32)
    indptr = np.searchsorted(row, np.arange(n_bins + 1)).astype(np.int64)
    dev = torch.device('cuda', 0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in dict(
        row=row, col=col, data=data, org=org, indptr=indptr).items()}
    for mean in (False, True):
        for sym in (False, True):
            want = ctx.window_gather(col, data, org, 9, 13, (n_bins, n_bins),
                                     row=row, cols=cols, symmetrize=sym,
                                     mean=mean)
            for src in ('row', 'indptr'):
                out = torch.full(want.shape, -1., dtype=torch.float64,
                                 device=dev)
                torch.cuda.synchronize(dev)   # (the ctx has its own stream)
                ctx.window_gather_dev(
                    t['col'].data_ptr(), t['data'].data_ptr(), len(row), 3,
                    (n_bins, n_bins), cols, t['org'].data_ptr(), len(org), 9,
                    13, out.data_ptr(), symmetrize=sym, mean=mean,
                    **{'d_' + src: t[src].data_ptr()})
                assert_same_bits(out.cpu().numpy(), want)


# -- get_matrix through the class -------------------------------------------

@pytest.fixture(scope='module')
def small2_run():
    from hic3defdr_amd import HiC3DeFDR
    g, kw = e2e_inputs('small2')
    outdir = tempfile.mkdtemp(prefix='h3d_views_')
    design = pd.DataFrame(kw['design'], index=kw['reps'], columns=kw['conds'])
    h = HiC3DeFDR(raw_npz_patterns=kw['raw_npz_patterns'],
                  bias_patterns=kw['bias_patterns'], chroms=kw['chroms'],
                  design=design, outdir=outdir,
                  dist_thresh_max=kw['dist_thresh_max'],
                  loop_patterns=kw['loop_patterns'], res=10000)
    h.run_to_qvalues(verbose=False)
    yield h, kw
    h.flush()
    shutil.rmtree(outdir, ignore_errors=True)


def gm_args(views):
    r0, r1, c0, c1 = (int(v) for v in views['gm_slices'])
    return str(views['gm_chrom']), slice(r0, r1), slice(c0, c1)


def assert_close_same_nans(got, want, rtol, what):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), what)
    err = rel_err(got, want)    # (equal cells, zeros included, count as 0)
    print('%s: max rel err %.3e over %d cells' % (what, err,
                                                  (~np.isnan(want)).sum()))
    assert err <= rtol, what


def test_get_matrix_matches_reference(views, small2_run):
    h, kw = small2_run
    chrom, rs, cs = gm_args(views)
    rep, cond = str(views['gm_rep']), str(views['gm_cond'])
    raw = h.get_matrix('raw', chrom, rs, cs, rep=rep)
    assert raw.dtype == np.float64
    assert_same_bits(raw, views['gm_raw'])
    assert_same_bits(h.get_matrix('raw_mean', chrom, rs, cs, cond=cond),
                     views['gm_raw_mean'])
    # 1e-12: the bound test_gpu_norms.py holds the size factors to, one
    # order looser for the division
    assert_close_same_nans(h.get_matrix('scaled', chrom, rs, cs, rep=rep),
                           views['gm_scaled'], 1e-12, 'scaled')
    assert_close_same_nans(h.get_matrix('scaled_mean', chrom, rs, cs,
                                        cond=cond),
                           views['gm_scaled_mean'], 1e-12, 'scaled_mean')
    # 1e-6: the project's q bar
    assert_close_same_nans(h.get_matrix('qvalues', chrom, rs, cs),
                           views['gm_qvalues'], 1e-6, 'qvalues')


def test_get_matrix_mean_is_the_replicates_mean(views, small2_run):
    """scaled_mean (one launch, the kernel's mean mode) = np.mean of this
    build's own per-replicate matrices, bit for bit: numpy reduces a leading
    axis sequentially, the kernel's order."""
    h, kw = small2_run
    chrom, rs, cs = gm_args(views)
    for cond in kw['conds']:
        reps = h.design.index[np.asarray(h.design[cond], dtype=bool)]
        assert len(reps) == 2
        for stage in ('scaled', 'raw'):
            per_rep = [h.get_matrix(stage, chrom, rs, cs, rep=r)
                       for r in reps]
            assert_same_bits(h.get_matrix(stage + '_mean', chrom, rs, cs,
                                          cond=cond),
                             np.mean(per_rep, axis=0))


def test_get_matrix_refuses_what_it_cannot_average(views, small2_run):
    h, kw = small2_run
    chrom, rs, cs = gm_args(views)
    for name in ('mu_hat_alt_mean', 'qvalues_mean', '_mean'):
        with pytest.raises(ValueError, match='averaged'):
            h.get_matrix(name, chrom, rs, cs, cond=kw['conds'][0])
    with pytest.raises(ValueError, match='needs cond'):
        h.get_matrix('scaled_mean', chrom, rs, cs)
    with pytest.raises(ValueError, match='rep or cond'):
        h.get_matrix('scaled', chrom, rs, cs)
    # mu_hat_alt: the suffix is removed as a suffix, the stage loads
    m = h.get_matrix('mu_hat_alt', chrom, rs, cs, cond=kw['conds'][0])
    assert m.shape == (rs.stop - rs.start, cs.stop - cs.start)
    assert np.isfinite(m).any()


def test_apa_stack_over_an_outdir_stage(views, small2_run):
    """apa_stack = make_apa_stack on the stage's upper triangle as a scipy
    matrix of the chromosome's size."""
    from hic3defdr_amd.util.apa import make_apa_stack
    from hic3defdr_amd.util.clusters import load_clusters
    h, kw = small2_run
    chrom = kw['chroms'][0]
    cond = kw['conds'][0]
    clusters = load_clusters(kw['loop_patterns'][cond]
                             .replace('<chrom>', chrom))
    clusters = [sorted(c) for c in clusters] + [[(3, 4)], [(1, 30)]]
    n_bins = h.load_bias(chrom).shape[0]
    for name, sel in (('scaled', dict(rep=kw['reps'][0])),
                      ('scaled_mean', dict(cond=cond))):
        got = h.apa_stack(name, chrom, clusters, 7, **sel)
        row, col, data = h.load_data('scaled', chrom, coo=True)
        d = data[:, 0] if name == 'scaled' else \
            np.mean(data[:, np.asarray(h.design[cond], dtype=bool)].T, axis=0)
        m = sparse.coo_matrix((d, (row, col)), shape=(n_bins, n_bins))
        want = make_apa_stack(m, clusters, 7)
        assert got.shape == (len(clusters), 7, 7)
        assert_same_bits(got, want)
        assert np.isnan(got[-1]).all() and np.isnan(got[-2]).all()
        assert np.isfinite(got).any()
    assert h.apa_stack('scaled', chrom, [], 7, rep=kw['reps'][0]).shape == \
        (0, 7, 7)


# -- aggregate --------------------------------------------------------------

def int_stack():
    rng = np.random.default_rng(5)
    st = rng.integers(-50, 1000, (1000, 11, 11)).astype(np.float64)
    st[rng.random(st.shape) < 0.05] = np.nan
    st[rng.random(1000) < 0.1] = np.nan       # whole windows
    st[:, 0, 3] = np.nan                      # cells NaN in every window
    st[:, 10, 10] = np.nan
    return st


def test_apa_mean_exact_on_an_integer_stack():
    from hic3defdr_amd import HiC3DeFDR
    st = int_stack()
    mean, count = HiC3DeFDR.apa_mean(st)
    assert count.dtype == np.int64 and mean.dtype == np.float64
    np.testing.assert_array_equal(count, (~np.isnan(st)).sum(axis=0))
    assert count[0, 3] == 0 and count[10, 10] == 0 and count.max() < 1000
    with np.errstate(all='ignore'), pytest.warns(RuntimeWarning):
        want = np.nanmean(st, axis=0)
    np.testing.assert_array_equal(mean, want)
    assert np.isnan(mean[0, 3]) and np.isnan(mean[10, 10])


def test_apa_mean_float_stack_within_reordering_bound_and_reproducible():
    from hic3defdr_amd.util.apa import apa_mean
    rng = np.random.default_rng(6)
    W = 1000
    st = rng.gamma(2.0, 3.0, (W, 11, 11))
    st[rng.random(st.shape) < 0.05] = np.nan
    mean, count = apa_mean(st)
    want = np.nanmean(st, axis=0)
    rel = np.max(np.abs(mean - want) / want)
    print('apa_mean vs np.nanmean: max rel diff %.3e (bound %.3e)'
          % (rel, W * 2.0 ** -53))
    # the worst case of reordering a positive sum of W terms
    assert rel <= W * 2.0 ** -53
    mean2, count2 = apa_mean(st)
    assert mean.tobytes() == mean2.tobytes()
    assert count.tobytes() == count2.tobytes()
    # no windows
    m0, c0 = apa_mean(np.zeros((0, 3, 5)))
    assert c0.shape == (3, 5) and not c0.any() and np.isnan(m0).all()


# -- one moderate shape: more than a few workgroups --------------------------

def test_moderate_shape_stack_and_mean_bit_equal_to_numpy(ctx):
    """2,000 bins, band 100 (about 2e5 pixels), 3,000 windows of width 21,
    K = 4, against a plain numpy scatter."""
    from hic3defdr_amd.util.matrices import check_table
    rng = np.random.default_rng(7)
    n_bins, band, width, W, K = 2000, 100, 21, 3000, 4
    i = np.repeat(np.arange(n_bins), band + 1)
    j = i + np.tile(np.arange(band + 1), n_bins)
    keep = (j < n_bins) & (rng.random(len(i)) < 0.97)
    row, col = i[keep], j[keep]
    assert 1.9e5 < len(row) < 2.1e5
    data = rng.normal(0, 1, (len(row), 6))
    cols = [4, 0, 5, 2]
    org = np.stack([rng.integers(-30, n_bins + 10, W),
                    rng.integers(-30, n_bins + 10, W)], axis=1)
    org[::50, 0] = np.iinfo(np.int32).min
    # numpy: the padded dense matrices, one per column, sliced per window
    pad = 64
    dense = np.full((K, n_bins + 2 * pad, n_bins + 2 * pad), np.nan)
    for k, c in enumerate(cols):
        dense[k, row + pad, col + pad] = data[:, c]
    want = np.full((K, W, width, width), np.nan)
    for n, (r0, c0) in enumerate(org):
        if r0 != np.iinfo(np.int32).min:
            want[:, n] = dense[:, r0 + pad:r0 + pad + width,
                               c0 + pad:c0 + pad + width]
    r32, c32 = check_table(row, col)
    got = ctx.window_gather(c32, data, org, width, width, (n_bins, n_bins),
                            row=r32, cols=cols)
    assert got.shape == want.shape
    assert_same_bits(got, want)
    got_mean = ctx.window_gather(c32, data, org, width, width,
                                 (n_bins, n_bins), row=r32, cols=cols,
                                 mean=True)
    assert_same_bits(got_mean, np.mean(want, axis=0))
    # symmetrized: the transposed pass on top
    sym = ctx.window_gather(c32, data, org[:200], width, width,
                            (n_bins, n_bins), row=r32, cols=cols[:1],
                            symmetrize=True)[0]
    d0 = dense[0]
    both = np.where(np.isnan(d0.T), d0, d0.T)
    for n, (r0, c0) in enumerate(org[:200]):
        if r0 != np.iinfo(np.int32).min:
            assert_same_bits(sym[n], both[r0 + pad:r0 + pad + width,
                                          c0 + pad:c0 + pad + width])
