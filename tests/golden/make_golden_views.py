"""Generates tests/golden/views.npz by running the REFERENCE's dense views:
``select_matrix``, ``make_apa_stack``, ``cluster_to_slices`` and
``HiC3DeFDR.get_matrix``.

Run like make_golden.py (same interpreter, same refshim, the reference
checkout on PYTHONPATH):

    PYTHONPATH=tests/golden/refshim:<reference checkout> \
        PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=agg \
        python3.9 tests/golden/make_golden_views.py

Every record holds the inputs (tables, clusters, slices) and the reference's
output. The get_matrix records come from the reference's own run_to_qvalues
on the committed small2 dataset (tests/golden/data/small2), with
``equal_bin`` pinned to the stable tie order as in make_golden.py.

Kept out on purpose: an APA cluster whose centre of mass is exactly
``size - int(width / 2)``; the reference raises a broadcast ValueError there
(checked below), the product returns an all-NaN window.
"""
import os
import shutil
import tempfile

import numpy as np
import pandas as pd
import scipy.sparse as sparse

import hic3defdr.util.scaling as scaling


def equal_bin_stable(data, n_bins):
    idx = np.linspace(0, n_bins, data.size, endpoint=0, dtype=int)
    return idx[data.argsort(kind='stable').argsort(kind='stable')]


scaling.equal_bin = equal_bin_stable

from hic3defdr import HiC3DeFDR  # noqa: E402
from hic3defdr.util.apa import make_apa_stack  # noqa: E402
from hic3defdr.util.clusters import cluster_to_slices  # noqa: E402
from hic3defdr.util.matrices import select_matrix  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def select_records(out):
    """A 200-bin upper-triangular table of band 12 with empty rows, rows of
    one entry, a NaN, an inf and a -0.0 among the data."""
    rng = np.random.default_rng(20)
    n_bins, band = 200, 12
    rows, cols = [], []
    empty = {0, 1, 17, 54, 120, 121, 198}
    single = {5, 33, 57, 102, 150}
    for i in range(n_bins):
        if i in empty:
            continue
        js = np.arange(i, min(i + band, n_bins - 1) + 1)
        if i in single:
            js = js[[int(rng.integers(len(js)))]]
        else:
            js = js[rng.random(len(js)) < 0.6]
        rows += [i] * len(js)
        cols += js.tolist()
    # the last bin's diagonal pixel closes the table
    if (rows[-1], cols[-1]) != (n_bins - 1, n_bins - 1):
        rows.append(n_bins - 1)
        cols.append(n_bins - 1)
    row = np.array(rows, dtype=np.int64)
    col = np.array(cols, dtype=np.int64)
    data = rng.normal(3.0, 2.0, len(row))

    def plant(lo, hi, value, diag=None):
        ok = (row >= lo) & (row < hi) & (col >= lo) & (col < hi)
        if diag is not None:
            ok &= (col - row > 0) == diag
        k = np.flatnonzero(ok)[3]
        data[k] = value
        return k

    k_nan = plant(50, 60, np.nan, diag=True)
    k_inf = plant(30, 46, np.inf, diag=True)
    k_nz = plant(100, 110, -0.0)
    k1 = np.flatnonzero((col - row == 4) & (row > 70))[0]
    # (row start, row stop, col start, col stop, symmetrize)
    windows = [
        (50, 60, 50, 60, 1),        # on the diagonal: both passes hit
        (30, 40, 36, 46, 1),        # above the diagonal
        (36, 46, 30, 40, 1),        # below: only the transposed pass fills
        (100, 105, 103, 110, 1),    # 5 x 7
        (60, 125, 90, 93, 1),       # 65 x 3
        (int(row[k1]), int(row[k1]) + 1, int(col[k1]), int(col[k1]) + 1, 1),
        (int(col[k1]), int(col[k1]) + 1, int(row[k1]), int(row[k1]) + 1, 1),
        (int(col[k1]), int(col[k1]) + 1, int(row[k1]), int(row[k1]) + 1, 0),
        (int(row[0]) - 2, int(row[0]) + 4, int(col[0]) - 1, int(col[0]) + 5,
         1),                        # the first stored entry
        (192, 200, 193, 200, 1),    # the last stored entry
        (-3, 4, -2, 6, 1),          # negative starts
        (195, 206, 190, 204, 1),    # past the last bin
        (300, 305, 310, 316, 1),    # wholly outside
        (-20, -10, 4, 9, 1),        # wholly outside, negative stops
        (50, 60, 50, 60, 0),        # the first again, not symmetrized
        (36, 46, 30, 40, 0),        # below the diagonal, not symmetrized
    ]
    out['sel_row'], out['sel_col'], out['sel_data'] = row, col, data
    out['sel_planted'] = np.array([k_nan, k_inf, k_nz])
    out['sel_windows'] = np.array(windows, dtype=np.int64)
    for i, (r0, r1, c0, c1, sym) in enumerate(windows):
        m = select_matrix(slice(r0, r1), slice(c0, c1), row, col, data,
                          symmetrize=bool(sym))
        out['sel_out_%d' % i] = m
    seen = np.concatenate([out['sel_out_%d' % i].ravel()
                           for i in range(len(windows))])
    assert np.isinf(seen).any() and np.isnan(seen).any()
    assert (np.signbit(seen) & (seen == 0)).any()
    print('select_matrix: %d pixels, %d windows' % (len(row), len(windows)))


def apa_records(out):
    """A 300-bin matrix with entries in both triangles and repeated COO
    entries (summed by tocsr; dyadic values, so the sums are exact in any
    order), about 60 clusters, widths 5 and 11."""
    rng = np.random.default_rng(21)
    size = 300
    i = rng.integers(0, size, 6000)
    j = np.clip(i + rng.integers(-45, 46, len(i)), 0, size - 1)
    v = rng.integers(1, 4000, len(i)) / 8.0
    i = np.concatenate([i, i[:400]])
    j = np.concatenate([j, j[:400]])
    v = np.concatenate([v, rng.integers(1, 4000, 400) / 8.0])
    coo = sparse.coo_matrix((v, (i, j)), shape=(size, size))
    clusters = [
        [(100, 103), (101, 104)],            # nearer the diagonal than min_dist
        [(1, 20), (2, 21)],                  # com[0] = 1.5 < r at width 5
        [(250, 297)],                        # width 5 ends at the last bin
        [(20, 100), (21, 101)],              # half-integer com 20.5 -> 20
        [(240, 294), (241, 294), (240, 295), (239, 293)],
        [(150, 120), (151, 121), (151, 120)],  # below the diagonal
        [(2, 40)],                           # com[0] = r at width 5
        [(5, 60), (5, 61), (6, 61)],         # com[0] = r at width 11
        [(294, 250)],                        # width 11 ends at the last bin
    ]
    while len(clusters) < 60:
        ci, cj = int(rng.integers(0, size)), int(rng.integers(0, size))
        pts = {(int(np.clip(ci + di, 0, size - 1)),
                int(np.clip(cj + dj, 0, size - 1)))
               for di, dj in rng.integers(-2, 3, (int(rng.integers(1, 7)), 2))}
        com = np.mean(list(pts), axis=0)
        if any(c == size - r for c in com for r in (2, 5)):
            continue                         # the reference raises there
        clusters.append(sorted(pts))
    out['apa_row'], out['apa_col'], out['apa_data'] = i, j, v
    out['apa_size'] = np.array(size)
    out['apa_points'] = np.array([p for c in clusters for p in c],
                                 dtype=np.int64)
    out['apa_starts'] = np.concatenate(
        [[0], np.cumsum([len(c) for c in clusters])]).astype(np.int64)
    empty = sparse.coo_matrix((size, size))
    for width in (5, 11):
        st = make_apa_stack(coo, clusters, width)
        out['apa_stack_w%d' % width] = st
        out['apa_slices_w%d' % width] = np.array(
            [[s.start, s.stop] for c in clusters
             for s in cluster_to_slices(c, width)],
            dtype=np.int64).reshape(len(clusters), 4)
        out['apa_none_w%d' % width] = make_apa_stack(coo, [], width)
        out['apa_nnz0_w%d' % width] = make_apa_stack(empty, clusters, width)
        print('apa width %d: %d of %d windows kept' % (
            width, int((~np.isnan(st[:, 0, 0])).sum()), len(clusters)))
    out['apa_stack_w5_min3'] = make_apa_stack(coo, clusters, 5, min_dist=3)
    # the position kept out of the goldens: the reference raises
    m40 = sparse.coo_matrix((np.ones(1), ([10], [38])), shape=(40, 40))
    try:
        make_apa_stack(m40, [[(10, 38)]], 5)
        raise AssertionError('the reference no longer raises at size - r')
    except ValueError:
        pass


def get_matrix_records(out):
    g = np.load(os.path.join(HERE, 'e2e_small2.npz'), allow_pickle=False)
    base = os.path.join(HERE, 'data', 'small2')
    reps = [str(r) for r in g['meta_reps']]
    conds = [str(c) for c in g['meta_conds']]
    chroms = [str(c) for c in g['meta_chroms']]
    design = pd.DataFrame(g['meta_design'].astype(bool), index=reps,
                          columns=conds)
    outdir = tempfile.mkdtemp(prefix='h3golden_views_')
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
        chrom = chroms[0]
        # the run must be the one the e2e golden recorded
        assert np.array_equal(np.load('%s/qvalues_%s.npy' % (outdir, chrom)),
                              g['qvalues__%s' % chrom], equal_nan=True)
        rs, cs = slice(100, 140), slice(90, 135)
        out['gm_chrom'] = np.array(chrom)
        out['gm_slices'] = np.array([rs.start, rs.stop, cs.start, cs.stop])
        out['gm_rep'] = np.array(reps[1])
        out['gm_cond'] = np.array(conds[1])
        out['gm_raw'] = h.get_matrix('raw', chrom, rs, cs, rep=reps[1])
        out['gm_scaled'] = h.get_matrix('scaled', chrom, rs, cs, rep=reps[1])
        out['gm_scaled_mean'] = h.get_matrix('scaled_mean', chrom, rs, cs,
                                             cond=conds[1])
        out['gm_raw_mean'] = h.get_matrix('raw_mean', chrom, rs, cs,
                                          cond=conds[1])
        out['gm_qvalues'] = h.get_matrix('qvalues', chrom, rs, cs)
        print('get_matrix: %s, %d finite q cells' % (
            chrom, int(np.isfinite(out['gm_qvalues']).sum())))
    finally:
        shutil.rmtree(outdir, ignore_errors=True)


if __name__ == '__main__':
    # the reference's doctest of cluster_to_slices
    assert cluster_to_slices([(4, 5), (3, 4), (3, 5), (3, 6)], width=5) == \
        (slice(1, 6), slice(3, 8))
    records = {}
    select_records(records)
    apa_records(records)
    get_matrix_records(records)
    path = os.path.join(HERE, 'views.npz')
    np.savez_compressed(path, **records)
    print('%s: %d bytes' % (path, os.path.getsize(path)))
