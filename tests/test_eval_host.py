"""CPU checks behind the GPU evaluation operators (csrc/h3d_eval.hip): the
integer restatement of the ROC / FDR curve (tests/eval_cases.py) against the
host evaluate() and the reference's eval.npz arrays, bit for bit; the
percentile interpolation against np.percentile; the signatures and the
argument rejections of the new functions, which must happen before a device
is touched; rates_at_threshold against the reference's expression."""
import inspect

import numpy as np
import pytest

import eval_cases as ec


@pytest.mark.parametrize('kind', ec.KINDS)
@pytest.mark.parametrize('n', ec.N_LIST + (100003,))
def test_restatement_equals_host_evaluate(n, kind):
    y, q = ec.case(n, kind)
    ec.assert_same(ec.evaluate_ref(y, q), ec.host_evaluate(y, q),
                   'n=%d %s' % (n, kind))


@pytest.mark.parametrize('points', [1, 7, 1000])
def test_restatement_fdr_point_counts(points):
    y, q = ec.case(4097, 'grid', seed=3)
    ec.assert_same(ec.evaluate_ref(y, q, points),
                   ec.host_evaluate(y, q, points))


@pytest.mark.parametrize('which', [0, 1, 2, 3])
def test_restatement_equals_reference_eval_files(which):
    from hic3defdr_amd import _native
    c = ec.small2_eval_case(which)
    q = _native.bh(c['values']) if c['rerun'] else c['values']
    got = dict(zip(('fdr', 'fpr', 'tpr', 'thresh'),
                   ec.evaluate_ref(c['y_true'], q)))
    ec.assert_same([got[k] for k in sorted(got)],
                   [c['golden'][k] for k in sorted(got)], c['fn'])


def test_drop_intermediate_flag_matches_sklearn():
    from sklearn.metrics import roc_curve
    for kind in ('unique', 'grid'):
        y, q = ec.case(4097, kind, seed=5)
        for drop in (False, True):
            fpr, tpr, thresh = roc_curve(y, 1 - q, drop_intermediate=drop)
            thresh = thresh.copy()
            thresh[0] = thresh[1] + 1
            ref = ec.curve_ref(y, 1 - q, drop_intermediate=drop)
            ec.assert_same((ref[1], ref[2], ref[3]), (fpr, tpr, thresh))


def test_percentile_interpolation_equals_numpy():
    from hic3defdr_amd.util.diagnostics import (percentile_lerp,
                                                percentile_ranks)
    rng = np.random.default_rng(11)
    pairs = [(1, 0.05), (1, 0.), (1, 1.), (2, 0.05), (2, 0.), (2, 1.),
             (2, 0.5), (3, 0.5), (65, 0.05), (4097, 0.05), (100, 1.),
             (100, 0.)]
    while len(pairs) < 1200:
        pairs.append((int(rng.integers(1, 3000)),
                      float(rng.choice([rng.random(), rng.random(), 0.05,
                                        0.5, 0., 1.]))))
    for t, (n, threshold) in enumerate(pairs):
        x = rng.random(n)
        if t % 3 == 0:
            x = np.round(x, 1)          # repeated values
        if t % 7 == 0:
            x = x * 1e-300              # tiny values: no intermediate fuse
        s = np.sort(x)
        lo, hi, gamma = percentile_ranks(n, threshold)
        assert 0 <= lo < n and 0 <= hi < n
        got = np.float64(percentile_lerp(s[lo], s[hi], gamma))
        want = np.float64(np.percentile(x, 100 * threshold))
        assert got.tobytes() == want.tobytes(), (n, threshold, got, want)


def test_signatures():
    from hic3defdr_amd import HiC3DeFDR
    from hic3defdr_amd.util import clusters, diagnostics, evaluation

    def sig(fn):
        return str(inspect.signature(fn))
    assert sig(clusters.pixel_membership_gpu) == \
        '(row, col, clusters_lists, mask=None)'
    assert sig(evaluation.make_y_true_gpu) == '(row, col, clusters, labels)'
    assert sig(evaluation.roc_curve_gpu) == \
        '(y_true, y_score, drop_intermediate=True)'
    assert sig(evaluation.evaluate_gpu) == \
        '(y_true, qvalues, n_fdr_points=100)'
    assert sig(evaluation.rates_at_threshold) == \
        '(eval_result, threshold=0.15)'
    assert sig(diagnostics.distance_bias) == \
        '(pvalues, dist, bins, threshold=0.05)'
    assert sig(HiC3DeFDR.distance_bias_data) == \
        "(self, bins, idx='disp', threshold=0.05)"
    p = inspect.signature(HiC3DeFDR.evaluate).parameters
    assert p['gpu'].default is False
    assert list(p)[-1] == 'gpu'
    # the evaluation module's GPU path does not pull scikit-learn in
    src = inspect.getsource(evaluation)
    gpu_part = src[src.index('def make_y_true_gpu'):]
    assert 'from sklearn' not in gpu_part and 'import sklearn' not in gpu_part
    assert 'sklearn' not in vars(evaluation)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to load the library or open a context fails the test."""
    from hic3defdr_amd import _native

    def touched(*a, **k):
        raise AssertionError('a device was touched before the rejection')
    monkeypatch.setattr(_native, 'context', touched)
    monkeypatch.setattr(_native, 'load_library', touched)
    monkeypatch.setattr(_native, 'Context', touched)


def test_rejections_before_a_device_is_touched(no_device):
    from hic3defdr_amd.util import clusters, diagnostics, evaluation
    y = np.array([True, False, True])
    q = np.array([0.1, 0.2, 0.3])
    # a NaN score
    with pytest.raises(ValueError, match='NaN'):
        evaluation.evaluate_gpu(y, np.array([0.1, np.nan, 0.3]))
    with pytest.raises(ValueError, match='NaN'):
        evaluation.roc_curve_gpu(y, np.array([np.nan, 0.2, 0.3]))
    # n = 0
    with pytest.raises(ValueError):
        evaluation.evaluate_gpu(np.zeros(0, dtype=bool), np.zeros(0))
    with pytest.raises(ValueError):
        evaluation.roc_curve_gpu(np.zeros(0, dtype=bool), np.zeros(0))
    # label / score lengths that differ
    with pytest.raises(ValueError):
        evaluation.evaluate_gpu(y, q[:2])
    with pytest.raises(ValueError):
        evaluation.roc_curve_gpu(y[:2], q)
    with pytest.raises(ValueError):
        evaluation.evaluate_gpu(y, q, n_fdr_points=0)
    with pytest.raises(TypeError):
        evaluation.evaluate_gpu(y, np.array(['a', 'b', 'c']))
    # B > 64, B = 0, shapes, threshold
    p = np.array([0.1, 0.5, 0.9])
    d = np.array([1, 2, 3])
    with pytest.raises(ValueError, match='65'):
        diagnostics.distance_bias(p, d, [(None, k) for k in range(65)])
    with pytest.raises(ValueError):
        diagnostics.distance_bias(p, d, [])
    with pytest.raises(ValueError):
        diagnostics.distance_bias(p, d[:2], [(None, None)])
    with pytest.raises(TypeError):
        diagnostics.distance_bias(p, d.astype(float), [(None, None)])
    with pytest.raises(ValueError):
        diagnostics.distance_bias(p, d, [(None, None)], threshold=1.5)
    # a negative query coordinate, one beyond 2^31, shapes, dtypes
    pix = np.array([[1, 2], [3, 4]])
    with pytest.raises(ValueError, match='2\\^31'):
        clusters.pixel_membership_gpu(np.array([1, -1]), np.array([2, 4]),
                                      [pix])
    with pytest.raises(ValueError, match='2\\^31'):
        clusters.pixel_membership_gpu(np.array([1, 3]),
                                      np.array([2, 2 ** 31]), [pix])
    with pytest.raises(ValueError):
        clusters.pixel_membership_gpu(np.array([1, 3]), np.array([2]), [pix])
    with pytest.raises(TypeError):
        clusters.pixel_membership_gpu(np.array([1., 3.]), np.array([2, 4]),
                                      [pix])
    with pytest.raises(ValueError):
        clusters.pixel_membership_gpu(np.array([1, 3]), np.array([2, 4]),
                                      [pix], mask=np.array([True]))
    with pytest.raises(ValueError):
        evaluation.make_y_true_gpu(np.array([1]), np.array([2]),
                                   [{(1, 2)}], ['up', 'down'])
    # nothing to look up: answered without a device
    out = clusters.pixel_membership_gpu(np.array([1, 3]), np.array([2, 4]),
                                        [[], np.zeros((0, 2), dtype=int)])
    assert out.dtype == np.bool_ and not out.any() and out.shape == (2,)
    out = clusters.pixel_membership_gpu(np.zeros(0, dtype=int),
                                        np.zeros(0, dtype=int), [pix])
    assert out.dtype == np.bool_ and out.shape == (0,)
    p_star, frac = diagnostics.distance_bias(np.zeros(0),
                                             np.zeros(0, dtype=int),
                                             [(None, None), (1, 2)])
    assert np.isnan(p_star) and np.isnan(frac).all() and frac.shape == (2,)


def test_class_rejections_before_a_device_is_touched(no_device, tmp_path):
    h, _ = ec.small2_analysis(str(tmp_path))
    with pytest.raises(ValueError):
        h.distance_bias_data([(None, None)], idx='all')
    with pytest.raises(ValueError):
        h.distance_bias_data([(None, k) for k in range(65)])


@pytest.mark.parametrize('which', [0, 1, 2, 3])
def test_rates_at_threshold(which):
    from hic3defdr_amd.util.evaluation import rates_at_threshold
    res = ec.small2_eval_case(which)['golden']
    for threshold in (0.15, 0.05, 0.0, 1.0, 0.5):
        # plotting/fn_vs_fp.py:63-68
        fpr = res['fpr']
        fnr = 1 - res['tpr']
        thresh = 1 - res['thresh']
        idx = np.argmin(np.abs(thresh - threshold))
        got = rates_at_threshold(res, threshold)
        assert got == (fpr[idx], fnr[idx])
        again = rates_at_threshold((res['fdr'], res['fpr'], res['tpr'],
                                    res['thresh']), threshold)
        assert again == got
    assert rates_at_threshold(res) == rates_at_threshold(res, 0.15)
    with pytest.raises(ValueError):
        rates_at_threshold({'fpr': np.zeros(2), 'tpr': np.zeros(3),
                            'thresh': np.zeros(2)})


def test_distance_bias_labels():
    bins = [(None, 10), (11, 20), (21, None), (None, None)]
    assert ec.bias_labels_ref(bins) == ['<= 10', '11 to 20', '>= 21', 'all']
