"""The evaluation kernels (csrc/h3d_eval.hip) behind util.clusters'
pixel_membership_gpu, util.evaluation's make_y_true_gpu / roc_curve_gpu /
evaluate_gpu, util.diagnostics.distance_bias and the class's
evaluate(gpu=True) / distance_bias_data. Every output is a count or a ratio
of counts, so everything is held to equality with the host code
(tests/eval_cases.py), NaN positions included."""
import os

import numpy as np
import pytest

from conftest import e2e_inputs, golden

import eval_cases as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from hic3defdr_amd import _native
    return _native.context(0)


# -- membership ---------------------------------------------------------------

def _pixels(rng, n, span):
    return rng.integers(0, span, n), rng.integers(0, span, n)


@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 257, 4097])
def test_membership_equals_host(n):
    from hic3defdr_amd.util.clusters import (pixel_membership,
                                             pixel_membership_gpu)
    rng = np.random.default_rng(n)
    # unsorted queries with repeats over a small span, so many hit the set
    row, col = _pixels(rng, n, 40)
    prow, pcol = _pixels(rng, 300, 40)
    pix = np.stack([prow, pcol], axis=1)
    pix = np.concatenate([pix, pix[:50]])            # a set with repeats
    sets = [{(int(a), int(b)) for a, b in zip(*_pixels(rng, 30, 40))},
            {(3, 4)}]
    for lists in ([pix], [sets], [pix, sets], [pix[:1]], [pix[:0]], [[]]):
        want = pixel_membership(row, col, lists)
        got = pixel_membership_gpu(row, col, lists)
        assert got.dtype == np.bool_
        np.testing.assert_array_equal(got, want)
        if n >= 63 and lists[0] is pix:
            assert want.any() and not want.all()
    # sorted unique queries (the host's searchsorted branch), the mask form
    key = np.unique(row * 64 + col)
    srow, scol = key // 64, key % 64
    mask = rng.random(len(key)) < 0.5
    np.testing.assert_array_equal(
        pixel_membership_gpu(srow, scol, [pix]),
        pixel_membership(srow, scol, [pix]))
    np.testing.assert_array_equal(
        pixel_membership_gpu(srow, scol, [pix], mask=mask),
        pixel_membership(srow, scol, [pix], mask=mask))


def test_membership_set_pixels_beyond_range_are_ignored(ctx):
    row = np.array([5, 7, 0, 2 ** 31 - 1], dtype=np.int64)
    col = np.array([6, 8, 0, 2 ** 31 - 1], dtype=np.int64)
    prow = np.array([5, 2 ** 31, -1, 7, 2 ** 31 - 1, 2 ** 40 + 7, 0],
                    dtype=np.int64)
    pcol = np.array([6, 8, 0, 2 ** 32 + 8, 2 ** 31 - 1, 8, -2 ** 32],
                    dtype=np.int64)
    got = ctx.pixel_membership(row, col, prow, pcol)
    np.testing.assert_array_equal(got, [True, False, False, True])
    # a query outside the range is an argument error of the library too
    from hic3defdr_amd._native import H3DError
    with pytest.raises(H3DError) as e:
        ctx.pixel_membership(np.array([1, -1]), np.array([1, 1]), prow, pcol)
    assert e.value.code == -1


def test_membership_small2_loop_idx():
    """small2's real clusters against prepare_data's golden loop_idx."""
    from hic3defdr_amd.util.clusters import (load_cluster_pixels,
                                             load_clusters,
                                             pixel_membership_gpu)
    g, kw = e2e_inputs('small2')
    for c in kw['chroms']:
        files = [p.replace('<chrom>', c)
                 for p in kw['loop_patterns'].values()]
        disp_idx = g['disp_idx__%s' % c]
        row, col = g['row__%s' % c], g['col__%s' % c]
        want = g['loop_idx__%s' % c]
        assert want.any()
        got = pixel_membership_gpu(row, col,
                                   [load_cluster_pixels(f) for f in files],
                                   mask=disp_idx)
        np.testing.assert_array_equal(got, want)
        got = pixel_membership_gpu(row[disp_idx], col[disp_idx],
                                   [load_clusters(f) for f in files])
        np.testing.assert_array_equal(got, want)


def test_membership_dev_equals_host_call(ctx):
    import torch
    rng = np.random.default_rng(7)
    row, col = _pixels(rng, 4097, 50)
    prow, pcol = _pixels(rng, 500, 50)
    want = ctx.pixel_membership(row, col, prow, pcol)
    dev = torch.device('cuda', 0)
    t = [torch.from_numpy(a).to(dev) for a in (row, col, prow, pcol)]
    got = ctx.pixel_membership_dev(*t)
    assert got.dtype == torch.bool
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    empty = torch.zeros(0, dtype=torch.int64, device=dev)
    assert not ctx.pixel_membership_dev(t[0], t[1], empty, empty).any()
    assert ctx.pixel_membership_dev(empty, empty, t[2], t[3]).numel() == 0


def test_make_y_true_gpu_equals_host():
    from hic3defdr_amd.util.evaluation import make_y_true, make_y_true_gpu
    c = ec.small2_eval_case(0)
    for row, col, clusters, labels in c['per_chrom']:
        want = make_y_true(row, col, clusters, labels)
        assert want.any()
        np.testing.assert_array_equal(
            make_y_true_gpu(row, col, clusters, labels), want)


# -- ROC / FDR ----------------------------------------------------------------

@pytest.mark.parametrize('kind', ec.KINDS)
@pytest.mark.parametrize('n', ec.N_LIST + (20011,))
def test_evaluate_gpu_equals_host(n, kind):
    from hic3defdr_amd.util.evaluation import evaluate_gpu
    y, q = ec.case(n, kind)
    want = ec.host_evaluate(y, q)
    got = evaluate_gpu(y, q)
    ec.assert_same(got, want, 'n=%d %s' % (n, kind))
    if kind == 'unique' and n >= 257:
        # most interior points are collinear: the drop pass did its work
        assert len(got[3]) < n / 2
    if kind == 'run5000' and n > 5000:
        assert np.count_nonzero(q == 0.25) == 5000


@pytest.mark.parametrize('points', [1, 7, 1000])
def test_evaluate_gpu_fdr_point_counts(points):
    from hic3defdr_amd.util.evaluation import evaluate_gpu
    y, q = ec.case(4097, 'grid', seed=3)
    ec.assert_same(evaluate_gpu(y, q, points),
                   ec.host_evaluate(y, q, points))


def test_evaluate_gpu_million(ctx):
    """n = 1,000,003 against the restatement; the counts ascend; a rerun
    and a second context give the same bits."""
    from hic3defdr_amd import _native
    y, q = ec.case(1000003, 'grid', seed=1)
    q = np.round(q, 4)
    want = ec.curve_ref(y, 1 - q)
    res, flags = ctx.roc_curve(y, q, 100, True, complement=True)
    assert flags == 0
    got = tuple(res[k] for k in ctx.ROC_FIELDS)
    ec.assert_same(got, want)
    assert (np.diff(res['fps']) >= 0).all() and \
        (np.diff(res['tps']) >= 0).all()
    assert res['fps'][-1] + res['tps'][-1] == len(y)
    again, _ = ctx.roc_curve(y, q, 100, True, complement=True)
    other = _native.Context(0)
    try:
        third, _ = other.roc_curve(y, q, 100, True, complement=True)
    finally:
        other.close()
    for k in ctx.ROC_FIELDS:
        assert again[k].tobytes() == res[k].tobytes(), k
        assert third[k].tobytes() == res[k].tobytes(), k


@pytest.mark.parametrize('kind', ['unique', 'grid', 'allpos'])
@pytest.mark.parametrize('drop', [False, True])
def test_roc_curve_gpu_equals_sklearn(kind, drop):
    import warnings
    from sklearn.metrics import roc_curve
    from hic3defdr_amd.util.evaluation import roc_curve_gpu
    y, q = ec.case(4097, kind, seed=5)
    score = 1 - q
    score[:3] = [0.0, -0.0, -1.5]      # signed zeros are one score
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fpr, tpr, thresh = roc_curve(y, score, drop_intermediate=drop)
    thresh = thresh.copy()
    thresh[0] = thresh[1] + 1           # scikit-learn 0.24's opening
    got = roc_curve_gpu(y, score, drop_intermediate=drop)
    ec.assert_same(got, (fpr, tpr, thresh), '%s drop=%s' % (kind, drop))
    if not drop:
        assert len(got[2]) == len(np.unique(score)) + 1


def test_roc_curve_dev_equals_host_call_and_flags_nan(ctx):
    import torch
    y, q = ec.case(4097, 'grid', seed=9)
    want, _ = ctx.roc_curve(y, q, 50, True, complement=True)
    dev = torch.device('cuda', 0)
    t_y, t_q = torch.from_numpy(y).to(dev), torch.from_numpy(q).to(dev)
    got, flags = ctx.roc_curve_dev(t_y, t_q, 50, True, complement=True)
    assert flags == 0
    for k in ctx.ROC_FIELDS:
        assert got[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    # a NaN score: rc 0 and the status flag, from both entries
    q[17] = np.nan
    assert ctx.roc_curve(y, q, 50, True)[1] == 16
    assert ctx.roc_curve_dev(t_y, torch.from_numpy(q).to(dev), 50,
                             True)[1] == 16


# -- order statistics / bin fractions -----------------------------------------

BINS = [(None, 10), (5, 30), (11, 20), (21, None), (None, None), (1000, 2000),
        (7, 7), (30, 5)]


@pytest.mark.parametrize('n', [1, 65, 4097])
@pytest.mark.parametrize('threshold', [0.05, 0.0, 1.0, 0.37])
def test_distance_bias_equals_numpy(n, threshold):
    from hic3defdr_amd.util.diagnostics import distance_bias
    rng = np.random.default_rng(n)
    p = np.round(rng.random(n), 3)
    dist = rng.integers(0, 60, n)
    for bins in (BINS, BINS[:1], [(k, k + 3) for k in range(64)]):
        want_p, want_f = ec.distance_bias_ref(p, dist, bins, threshold)
        got_p, got_f = distance_bias(p, dist, bins, threshold)
        assert np.float64(got_p).tobytes() == np.float64(want_p).tobytes()
        np.testing.assert_array_equal(got_f, want_f)
    if n > 1:
        _, f = distance_bias(p, dist, BINS, threshold)
        assert np.isnan(f[5]) and np.isnan(f[7]) and not np.isnan(f[:5]).any()


def test_distance_bias_nan_pvalues(ctx):
    from hic3defdr_amd.util.diagnostics import distance_bias
    rng = np.random.default_rng(3)
    p = rng.random(4097)
    p[[5, 77, 4000]] = np.nan
    dist = rng.integers(0, 60, 4097)
    want_p, want_f = ec.distance_bias_ref(p, dist, BINS)
    got_p, got_f = distance_bias(p, dist, BINS)
    assert np.isnan(want_p) and np.isnan(got_p)
    np.testing.assert_array_equal(got_f, want_f)
    assert (got_f[:5] == 0).all()
    vals, n_nan = ctx.order_stats(p, [0, 4093, 4094, 4096])
    assert n_nan == 3
    s = np.sort(p)
    np.testing.assert_array_equal(vals, s[[0, 4093, 4094, 4096]])
    # a finite p_star over p-values with NaN: a NaN is never below it
    lo = np.array([np.iinfo(np.int64).min, 10])
    hi = np.array([np.iinfo(np.int64).max, 20])
    members, below = ctx.bin_fractions(p, dist, lo, hi, 0.5)
    np.testing.assert_array_equal(
        members, [4097, np.count_nonzero((dist >= 10) & (dist <= 20))])
    with np.errstate(invalid='ignore'):
        np.testing.assert_array_equal(
            below, [np.count_nonzero(p < 0.5),
                    np.count_nonzero((p < 0.5) & (dist >= 10) &
                                     (dist <= 20))])


# -- the class ----------------------------------------------------------------

@pytest.mark.parametrize('which', [0, 1, 2, 3])
def test_class_evaluate_gpu(which, tmp_path):
    """evaluate(gpu=True) on the reference's simulated-analysis arrays, set
    up as test_simulation.py::test_evaluate_matches_reference: the default
    path's arrays exactly, the goldens at that test's rtol."""
    g = golden('sim_small2.npz')
    h, lab = ec.small2_analysis(str(tmp_path))
    a, b, rr = (int(v) for v in g['meta_evals'][which])
    a = None if a < 0 else a
    b = None if b < 0 else b
    fn = 'eval' if a is None and b is None else 'eval_%s_%s' % (a, b)
    h.evaluate('ES', lab, min_dist=a, max_dist=b, rerun_bh=bool(rr))
    host = dict(np.load(os.path.join(str(tmp_path), 'out', fn + '.npz')))
    os.remove(os.path.join(str(tmp_path), 'out', fn + '.npz'))
    h.evaluate('ES', lab, min_dist=a, max_dist=b, rerun_bh=bool(rr),
               gpu=True)
    e = np.load(os.path.join(str(tmp_path), 'out', fn + '.npz'))
    assert sorted(e.files) == ['fdr', 'fpr', 'thresh', 'tpr']
    for k in ('fdr', 'fpr', 'tpr', 'thresh'):
        np.testing.assert_array_equal(e[k], host[k], k)
        ref = g['eval__%s__%s' % (fn, k)]
        np.testing.assert_array_equal(np.isnan(e[k]), np.isnan(ref))
        np.testing.assert_allclose(e[k], ref, rtol=1e-12, atol=0)


@pytest.mark.parametrize('idx', ['disp', 'loop'])
def test_class_distance_bias_data(idx, tmp_path):
    h, _ = ec.small2_analysis(str(tmp_path))
    bins = [(None, 15), (16, 30), (31, None), (None, None), (500, None)]
    disp_idx, _ = h.load_data('disp_idx', 'all')
    loop_idx, _ = h.load_data('loop_idx', 'all')
    rc_idx = (disp_idx, loop_idx) if idx == 'loop' else disp_idx
    row, _ = h.load_data('row', 'all', idx=rc_idx)
    col, _ = h.load_data('col', 'all', idx=rc_idx)
    p, _ = h.load_data('pvalues', 'all',
                       idx=loop_idx if idx == 'loop' else None)
    assert len(p) == len(row) > 100
    for threshold in (0.05, 0.5):
        want_p, want_f = ec.distance_bias_ref(p, col - row, bins, threshold)
        labels, got_p, got_f = h.distance_bias_data(bins, idx=idx,
                                                    threshold=threshold)
        assert labels == ec.bias_labels_ref(bins)
        assert np.float64(got_p).tobytes() == np.float64(want_p).tobytes()
        np.testing.assert_array_equal(got_f, want_f)
        assert np.isnan(got_f[4]) and not np.isnan(got_f[:4]).any()
