"""Yardsticks and inputs shared by test_eval_host.py (CPU) and
test_gpu_eval.py: an integer restatement of the ROC / FDR curve of
util.evaluation.evaluate, the distance-bias expressions of the reference's
plotting/distance_bias.py:101-112, and the inputs of sim_small2.npz's four
evaluate() runs."""
import os

import numpy as np

from conftest import e2e_inputs, golden

N_LIST = (1, 2, 3, 63, 64, 65, 257, 4097)
KINDS = ('unique', 'grid', 'run5000', 'equal', 'allneg', 'allpos')


def curve_ref(y_true, y_score, n_fdr_points=100, drop_intermediate=True):
    """(fdr, fpr, tpr, thresh, fps, tps) in integers: a stable descending
    sort, the last element of every run of equal scores, the cumulative
    positives there, the second-difference drop, the origin, the ratios of
    the counts and the sampled FDR."""
    y = np.asarray(y_true, dtype=bool)
    s = np.asarray(y_score, dtype=np.float64)
    assert y.shape == s.shape and s.ndim == 1 and len(s) > 0
    assert not np.isnan(s).any()
    order = np.argsort(-s, kind='stable')
    ss, yy = s[order], y[order]
    ends = np.flatnonzero(np.r_[ss[1:] != ss[:-1], True])
    tps = np.cumsum(yy.astype(np.int64))[ends]
    fps = 1 + ends.astype(np.int64) - tps
    thresh = ss[ends]
    if drop_intermediate and len(fps) > 2:
        keep = np.r_[True, (np.diff(fps, 2) != 0) | (np.diff(tps, 2) != 0),
                     True]
        fps, tps, thresh = fps[keep], tps[keep], thresh[keep]
    fps = np.r_[np.int64(0), fps]
    tps = np.r_[np.int64(0), tps]
    thresh = np.r_[thresh[0] + 1, thresh]
    m = len(thresh)
    with np.errstate(divide='ignore', invalid='ignore'):
        fpr = fps / np.float64(fps[-1])
        tpr = tps / np.float64(tps[-1])
        rate = max(int(m / n_fdr_points), 1)
        pos = np.flatnonzero(tps > 0)
        start = int(pos[0]) if len(pos) else 0
        fdr = np.full(m, np.nan)
        idx = np.arange(start, m, rate)
        fdr[idx] = fps[idx] / (fps[idx] + tps[idx]).astype(np.float64)
    return fdr, fpr, tpr, thresh, fps, tps


def evaluate_ref(y_true, qvalues, n_fdr_points=100):
    """curve_ref on the scores ``1 - q``: (fdr, fpr, tpr, thresh)."""
    return curve_ref(y_true, 1 - np.asarray(qvalues, dtype=np.float64),
                     n_fdr_points)[:4]


def host_evaluate(y_true, qvalues, n_fdr_points=100):
    """util.evaluation.evaluate with scikit-learn's one-class and numpy's
    0 / 0 warnings silenced."""
    import warnings
    from hic3defdr_amd.util.evaluation import evaluate
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        return evaluate(y_true, qvalues, n_fdr_points)


def case(n, kind, seed=0):
    """(y_true bool, q-values) of one shape of input."""
    rng = np.random.default_rng(1000 * seed + n % 997 + len(kind))
    q = rng.random(n)
    y = rng.random(n) < np.where(q < 0.2, 0.5, 0.02)
    if kind == 'grid':
        q = np.round(q, 2)
    elif kind == 'run5000':
        at = rng.choice(n, size=min(5000, n), replace=False)
        q[at] = 0.25
    elif kind == 'equal':
        q[:] = 0.5
    elif kind == 'allneg':
        y[:] = False
    elif kind == 'allpos':
        y[:] = True
    elif kind != 'unique':
        raise ValueError(kind)
    return y, q


def assert_same(got, want, what=''):
    """assert_array_equal on each pair of arrays, NaN positions included."""
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, '%s[%d]: %s vs %s' % (what, i, a.shape,
                                                          b.shape)
        np.testing.assert_array_equal(a, b, '%s[%d]' % (what, i))


# -- distance bias ------------------------------------------------------------

def distance_bias_ref(pvalues, dist, bins, threshold=0.05):
    """plotting/distance_bias.py:101-112 on arrays: (p_star, fractions)."""
    pvalues, dist = np.asarray(pvalues), np.asarray(dist)
    with np.errstate(all='ignore'):
        p_star = np.percentile(pvalues, 100 * threshold)
        out = []
        for min_dist, max_dist in bins:
            dist_idx = np.ones(len(dist), dtype=bool)
            if min_dist is not None:
                dist_idx[dist < min_dist] = False
            if max_dist is not None:
                dist_idx[dist > max_dist] = False
            sel = pvalues[dist_idx] < p_star
            out.append(np.mean(sel) if sel.size else np.nan)
    return p_star, np.array(out, dtype=np.float64)


def bias_labels_ref(bins):
    """plotting/distance_bias.py:73-84."""
    out = []
    for min_dist, max_dist in bins:
        if min_dist is None and max_dist is not None:
            out.append('<= %s' % max_dist)
        elif min_dist is not None and max_dist is None:
            out.append('>= %s' % min_dist)
        elif min_dist is None and max_dist is None:
            out.append('all')
        else:
            out.append('%s to %s' % (min_dist, max_dist))
    return out


# -- sim_small2's evaluate() runs ---------------------------------------------

def small2_eval_case(which):
    """The inputs of evaluate() run ``which`` of sim_small2.npz, gathered as
    SimulatingHiC3DeFDR.evaluate does: dict(row, col per chromosome after
    the distance filter, clusters, labels, y_true, values, rerun, fn)."""
    from hic3defdr_amd.util.clusters import load_clusters
    from hic3defdr_amd.util.evaluation import make_y_true
    g = golden('sim_small2.npz')
    _, kw = e2e_inputs('small2')
    a, b, rr = (int(v) for v in g['meta_evals'][which])
    a = None if a < 0 else a
    b = None if b < 0 else b
    restrict = a is not None or b is not None
    per_chrom, y_true, values = [], [], []
    for c in kw['chroms']:
        disp_idx = g['simrun__disp_idx__%s' % c]
        loop_idx = g['simrun__loop_idx__%s' % c]
        row = g['simrun__row__%s' % c][disp_idx][loop_idx]
        col = g['simrun__col__%s' % c][disp_idx][loop_idx]
        dist = col - row
        keep = np.ones(len(dist), dtype=bool)
        if a is not None:
            keep[dist < a] = False
        if b is not None:
            keep[dist > b] = False
        clusters = load_clusters(
            kw['loop_patterns']['ES'].replace('<chrom>', c))
        labels = np.atleast_1d(g['labels__%s' % c])
        per_chrom.append((row[keep], col[keep], clusters, labels))
        y_true.append(make_y_true(row[keep], col[keep], clusters, labels))
        if restrict and rr:
            values.append(g['simrun__pvalues__%s' % c][loop_idx][keep])
        elif restrict:
            values.append(g['simrun__qvalues__%s' % c][keep])
        else:
            values.append(g['simrun__qvalues__%s' % c])
    fn = 'eval' if not restrict else 'eval_%s_%s' % (a, b)
    return dict(per_chrom=per_chrom, y_true=np.concatenate(y_true),
                values=np.concatenate(values), rerun=bool(restrict and rr),
                fn=fn, min_dist=a, max_dist=b, rr=bool(rr),
                golden={k: g['eval__%s__%s' % (fn, k)]
                        for k in ('fdr', 'fpr', 'tpr', 'thresh')})


def small2_analysis(tmp):
    """A HiC3DeFDR over sim_small2.npz's simulated-analysis arrays, set up as
    test_simulation.py::test_evaluate_matches_reference does; returns
    (analysis, label pattern)."""
    import pandas as pd
    from hic3defdr_amd import HiC3DeFDR
    g = golden('sim_small2.npz')
    _, kw = e2e_inputs('small2')
    lab = os.path.join(tmp, 'labels_<chrom>.txt')
    reps = ['A1', 'A2', 'B1', 'B2']
    design = pd.DataFrame({'A': [1, 1, 0, 0], 'B': [0, 0, 1, 1]},
                          dtype=bool, index=reps)
    h = HiC3DeFDR(raw_npz_patterns=['x_<chrom>'] * 4,
                  bias_patterns=['y_<chrom>'] * 4, chroms=kw['chroms'],
                  design=design, outdir=os.path.join(tmp, 'out'),
                  dist_thresh_max=kw['dist_thresh_max'],
                  loop_patterns={'ES': kw['loop_patterns']['ES']})
    for c in kw['chroms']:
        np.savetxt(lab.replace('<chrom>', c), g['labels__%s' % c], fmt='%s')
        for st in ('pvalues', 'qvalues', 'disp_idx', 'loop_idx', 'row',
                   'col'):
            h.save_data(g['simrun__%s__%s' % (st, c)], st, c)
    return h, lab

