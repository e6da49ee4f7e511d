"""Generates tests/golden/annotate.npz by running the REFERENCE's
``add_columns_to_cluster_table`` (cluster_table.py:192-332).

Run like make_golden_views.py (same interpreter, same refshim, the reference
checkout on PYTHONPATH):

    PYTHONPATH=tests/golden/refshim:<reference checkout> \
        PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=agg \
        python tests/golden/make_golden_annotate.py

A record ``<r>`` is a cluster table, a sequence of calls on it and the
resulting frame:

    <r>_chrom, <r>_pts, <r>_starts   the frame's rows: us_chrom (= ds_chrom)
                                     and the ``cluster`` cells in row order
    <r>_ncalls, <r>_c<j>_{pattern, table, labels, has_labels, reducer,
                          chrom}     call j ('' chrom = None); its table is
                                     <r>_c<table>_{row, col, data}
    <r>_names, <r>_out               the new columns and their values
                                     (rows, names) after the last call

Records: the three doctest calls of the reference's docstring; random banded
tables of about 300 pixels in shuffled order with K in {1, 2, 3, 9}, NaN,
+-inf and -0.0 among the data, clusters with absent pixels and a pixel listed
twice, all three reducers; and the reference's own collect() table of the
committed small2 dataset annotated per chromosome with qvalues / min and
mu_hat_alt / mean (the results file it read is calls_small2.npz's; the stage
tables are the run's own outdir arrays and are not stored).
"""
import os
import shutil
import tempfile

import numpy as np
import pandas as pd

import hic3defdr.util.scaling as scaling


def equal_bin_stable(data, n_bins):
    idx = np.linspace(0, n_bins, data.size, endpoint=0, dtype=int)
    return idx[data.argsort(kind='stable').argsort(kind='stable')]


scaling.equal_bin = equal_bin_stable

from hic3defdr import HiC3DeFDR  # noqa: E402
from hic3defdr.util.cluster_table import clusters_to_table, \
    add_columns_to_cluster_table, load_cluster_table  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = ['us_chrom', 'us_start', 'us_end', 'ds_chrom', 'ds_start', 'ds_end',
        'cluster_size', 'cluster', 'classification']


def record(out, r, df, calls, inputs=True):
    """Stores the frame's rows, runs ``calls`` on it and stores the result
    (``inputs=False``: not the calls' tables)."""
    cells = [[list(map(int, p)) for p in c] for c in df['cluster']]
    out[r + '_chrom'] = np.array(list(df['us_chrom']))
    assert list(df['us_chrom']) == list(df['ds_chrom'])
    out[r + '_pts'] = np.array([p for c in cells for p in c],
                               dtype=np.int64).reshape(-1, 2)
    out[r + '_starts'] = np.concatenate(
        [[0], np.cumsum([len(c) for c in cells])]).astype(np.int64)
    out[r + '_ncalls'] = np.array(len(calls))
    for j, c in enumerate(calls):
        add_columns_to_cluster_table(
            df, c['pattern'], c['row'], c['col'], c['data'],
            labels=c.get('labels'), reducer=c.get('reducer', 'mean'),
            chrom=c.get('chrom'))
        if not inputs:
            continue
        p = '%s_c%d_' % (r, j)
        out[p + 'pattern'] = np.array(c['pattern'])
        # the first call with this very table holds it
        first = [i for i in range(j + 1) if all(
            calls[i][a] is c[a] for a in ('row', 'col', 'data'))][0]
        out[p + 'table'] = np.array(first)
        if first == j:
            out[p + 'row'] = np.asarray(c['row'], dtype=np.int64)
            out[p + 'col'] = np.asarray(c['col'], dtype=np.int64)
            out[p + 'data'] = np.asarray(c['data'], dtype=np.float64)
        out[p + 'labels'] = np.array(c.get('labels') or [''])
        out[p + 'has_labels'] = np.array(c.get('labels') is not None)
        out[p + 'reducer'] = np.array(c.get('reducer', 'mean'))
        out[p + 'chrom'] = np.array(c.get('chrom') or '')
    names = [n for n in df.columns if n not in BASE]
    out[r + '_names'] = np.array(names)
    out[r + '_out'] = df[names].to_numpy(dtype=np.float64)
    return df


def doctest_records(out):
    clusters = [[(1, 2), (1, 1)], [(4, 4), (3, 4)]]
    res = 10000
    row, col = zip(*sum(clusters, []))
    data = np.array([[1, 2], [3, 4], [5, 6], [7, 8]], dtype=float)
    df = record(out, 'doc0', clusters_to_table(clusters, 'chrX', res), [
        dict(pattern='%s_mean', row=row, col=col, data=data,
             labels=['rep1', 'rep2'])])
    assert df.iloc[0]['rep1_mean'] == 2 and df.iloc[0]['rep2_mean'] == 3
    df = pd.concat([clusters_to_table(clusters, 'chr1', res),
                    clusters_to_table(clusters, 'chr2', res)], axis=0)
    df = record(out, 'doc1', df, [
        dict(pattern='%s_mean', row=row, col=col, data=data,
             labels=['rep1', 'rep2'], chrom='chr1'),
        dict(pattern='%s_mean', row=row, col=col, data=data[::-1, :],
             labels=['rep1', 'rep2'], chrom='chr2')])
    assert df.iloc[2]['rep1_mean'] == 6 and df.iloc[2]['rep2_mean'] == 7
    # the state between the two calls: chr2 still NaN
    df = pd.concat([clusters_to_table(clusters, 'chr1', res),
                    clusters_to_table(clusters, 'chr2', res)], axis=0)
    df = record(out, 'doc1a', df, [
        dict(pattern='%s_mean', row=row, col=col, data=data,
             labels=['rep1', 'rep2'], chrom='chr1')])
    assert np.isnan(df.iloc[2]['rep1_mean'])
    df = record(out, 'doc2', clusters_to_table(clusters, 'chrX', res), [
        dict(pattern='value', row=row, col=col, data=data[:, 0])])
    assert df.iloc[0]['value'] == 2


def random_records(out):
    rng = np.random.default_rng(30)
    for t, K in enumerate((1, 2, 3, 9)):
        n_bins, band = 60, 8
        i = rng.integers(0, n_bins, 1500)
        j = np.minimum(i + rng.integers(0, band, len(i)), n_bins - 1)
        key = rng.permutation(np.unique(i * n_bins + j))[:300]
        # the table's corner pixel fixes its shape
        key = np.unique(np.concatenate([key, [n_bins * n_bins - 1]]))
        key = rng.permutation(key)
        row, col = key // n_bins, key % n_bins
        data = rng.normal(1.0, 2.0, (len(row), K))
        for v in (np.nan, np.inf, -np.inf, -0.0):
            data[rng.integers(0, len(row), 4), rng.integers(0, K, 4)] = v
        clusters = []
        for c in range(25):
            m = int(rng.integers(1, 12))
            k = rng.integers(0, len(row), m)
            pts = [(int(row[a]), int(col[a])) for a in k]
            if c % 3 == 0:   # pixels the table may lack, inside its shape
                pts += [(int(rng.integers(0, n_bins)),
                         int(rng.integers(0, n_bins))) for _ in range(3)]
            if c % 4 == 1:   # a pixel listed twice
                pts.append(pts[0])
            clusters.append(pts)
        # a cluster wholly absent from the table
        gone = [(a, b) for a in range(3) for b in range(40, 43)
                if a * n_bins + b not in set(key.tolist())]
        clusters.append(gone)
        df = clusters_to_table(clusters, 'chrR', 10000)
        labels = ['c%d' % c for c in range(K)]
        calls = []
        for red in ('mean', 'max', 'min'):
            if K == 1:
                calls.append(dict(pattern='v_' + red, row=row, col=col,
                                  data=data[:, 0], reducer=red))
            else:
                calls.append(dict(pattern='%s_' + red, row=row, col=col,
                                  data=data, labels=labels, reducer=red))
        df = record(out, 'rnd%d' % t, df, calls)
        vals = out['rnd%d_out' % t]
        assert np.isnan(vals).any() and np.isinf(vals).any()
        print('rnd%d: K=%d, %d pixels, %d clusters' % (t, K, len(row),
                                                       len(df)))


def small2_record(out, fdr=0.05, size=3):
    g = np.load(os.path.join(HERE, 'e2e_small2.npz'), allow_pickle=False)
    base = os.path.join(HERE, 'data', 'small2')
    reps = [str(r) for r in g['meta_reps']]
    conds = [str(c) for c in g['meta_conds']]
    chroms = [str(c) for c in g['meta_chroms']]
    design = pd.DataFrame(g['meta_design'].astype(bool), index=reps,
                          columns=conds)
    outdir = tempfile.mkdtemp(prefix='h3golden_annotate_')
    try:
        h = HiC3DeFDR(
            raw_npz_patterns=[os.path.join(base, r, '<chrom>_raw.npz')
                              for r in reps],
            bias_patterns=[os.path.join(base, r, '<chrom>_kr.bias')
                           for r in reps],
            chroms=chroms, design=design, outdir=outdir,
            dist_thresh_max=int(g['meta_dist_thresh_max']),
            loop_patterns={c: os.path.join(base, 'clusters',
                                           '%s_<chrom>.json' % c)
                           for c in conds}, res=10000)
        h.run_to_qvalues(n_threads=0, verbose=False)
        for c in chroms:
            assert np.array_equal(np.load('%s/qvalues_%s.npy' % (outdir, c)),
                                  g['qvalues__%s' % c], equal_nan=True)
        h.collect(fdr=fdr, cluster_size=size, n_threads=0)
        path = '%s/results_%g_%i.tsv' % (outdir, fdr, size)
        # the results file is the one calls_small2.npz holds
        with open(path, 'rb') as fh:
            calls_g = np.load(os.path.join(HERE, 'calls_small2.npz'))
            assert fh.read() == bytes(
                calls_g['file__results_%g_%i.tsv' % (fdr, size)])
        out['small2_fdr'], out['small2_size'] = np.array(fdr), np.array(size)
        calls = []
        for c in chroms:
            row, col, q = h.load_data('qvalues', c, coo=True)
            calls.append(dict(pattern='qvalues_min', row=row, col=col, data=q,
                              reducer='min', chrom=c))
            row, col, mu = h.load_data('mu_hat_alt', c, coo=True)
            calls.append(dict(pattern='mu_hat_alt_%s_mean', row=row, col=col,
                              data=mu, labels=conds, reducer='mean', chrom=c))
        df = record(out, 'small2', load_cluster_table(path), calls,
                    inputs=False)
        assert not df[list(out['small2_names'])].isna().any().any()
        print('small2: %d rows, columns %s' % (len(df), out['small2_names']))
    finally:
        shutil.rmtree(outdir, ignore_errors=True)


if __name__ == '__main__':
    records = {}
    doctest_records(records)
    random_records(records)
    small2_record(records)
    path = os.path.join(HERE, 'annotate.npz')
    np.savez_compressed(path, **records)
    print('%s: %d bytes' % (path, os.path.getsize(path)))
