"""Numpy restatement of the reference's add_columns_to_cluster_table
(cluster_table.py:298-332) and the shared inputs of the annotate tests.

``gather`` evaluates the table at a cluster's pixels as the reference's CSR
indexing does (an absent pixel is 0, a pixel beyond the shape an IndexError);
``reduce_clusters`` applies np.mean / np.max / np.min to each cluster's
values. The only arithmetic is numpy's own. tests/golden/annotate.npz (the
reference's output, make_golden_annotate.py) holds it to the reference
exactly (test_annotate_host.py)."""
import numpy as np

REDUCERS = {'mean': np.mean, 'max': np.max, 'min': np.min}
CHUNK = 2048     # h3d_cstat.h kChunk
SIZES = (1, 2, 3, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)
KS = (1, 2, 3, 8, 9, 17)


def gather(row, col, data, prow, pcol):
    """(m, K) values of the table at the pixels (prow, pcol), in order."""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    data = np.asarray(data, dtype=np.float64)
    if data.ndim == 1:
        data = data[:, None]
    prow = np.asarray(prow, dtype=np.int64)
    pcol = np.asarray(pcol, dtype=np.int64)
    shape = (int(row.max()) + 1, int(col.max()) + 1) if len(row) else (0, 0)
    if len(prow) and (prow.max() >= shape[0] or pcol.max() >= shape[1]):
        raise IndexError('index out of bounds of shape %r' % (shape,))
    out = np.zeros((len(prow), data.shape[1]))
    if not len(row):
        return out
    key = row * shape[1] + col
    order = np.argsort(key, kind='stable')
    ks = key[order]
    q = prow * shape[1] + pcol
    pos = np.minimum(np.searchsorted(ks, q), len(ks) - 1)
    hit = ks[pos] == q
    out[hit] = data[order[pos[hit]]]
    return out


def reduce_clusters(row, col, data, prow, pcol, starts, reducer):
    """(k, K): ``reducer`` of every cluster's gathered values per column,
    and found (k,): the cluster's pixels the table holds."""
    vals = gather(row, col, data, prow, pcol)
    present = gather(row, col, np.ones(len(np.asarray(row))), prow, pcol)[:, 0]
    fn = REDUCERS[reducer]
    k = len(starts) - 1
    out = np.empty((k, vals.shape[1]))
    found = np.empty(k, dtype=np.int64)
    with np.errstate(invalid='ignore'):
        for j in range(k):
            a, b = int(starts[j]), int(starts[j + 1])
            for c in range(vals.shape[1]):
                out[j, c] = fn(vals[a:b, c])
            found[j] = int(present[a:b].sum())
    return out, found


def mean_bound(row, col, data, prow, pcol, starts):
    """(k, K): (2m + 2) * 2^-53 * (sum |v| / m) -- two summation orders of m
    terms plus the division."""
    v = np.abs(gather(row, col, data, prow, pcol))
    out = np.empty((len(starts) - 1, v.shape[1]))
    with np.errstate(invalid='ignore'):
        for j in range(len(starts) - 1):
            a, b = int(starts[j]), int(starts[j + 1])
            m = b - a
            out[j] = (2 * m + 2) * 2.0 ** -53 * (v[a:b].sum(axis=0) / m)
    return out


def assert_means(got, ref, bound):
    """NaN and inf where the reference has them, the rest within ``bound``;
    returns the largest share of the bound used (0 where nothing is)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(got[~fin & ~np.isnan(ref)],
                                  ref[~fin & ~np.isnan(ref)])
    err = np.abs(got[fin] - ref[fin])
    b = bound[fin]
    assert np.all(err <= b), (err.max(), b[err > b][:4])
    pos = b > 0
    return float((err[pos] / b[pos]).max()) if pos.any() else 0.0


def assert_extrema(got, ref):
    """Equal values (0.0 == -0.0) and NaN in the same places."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    np.testing.assert_array_equal(got[ok], ref[ok])


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and \
        a.tobytes() == b.tobytes()


def banded_table(rng, n_bins=400, band=30, n=6000, K=3, special=True):
    """A shuffled banded table of distinct pixels with NaN, +-inf and -0.0
    among the data."""
    i = rng.integers(0, n_bins, 4 * n)
    j = np.minimum(i + rng.integers(0, band, len(i)), n_bins - 1)
    key = np.unique(i * n_bins + j)
    key = rng.permutation(key)[:n]
    row, col = key // n_bins, key % n_bins
    data = rng.normal(2.0, 3.0, (len(row), K))
    if special:
        for v in (np.nan, np.inf, -np.inf, -0.0, 0.0):
            data[rng.integers(0, len(row), 3), rng.integers(0, K, 3)] = v
    return row.astype(np.int64), col.astype(np.int64), data


def sized_clusters(rng, row, col, sizes, absent=0.2):
    """One cluster per size: pixels drawn from the table (repeats allowed),
    a share of them replaced by pixels the table may lack (inside its
    shape)."""
    n_rows, n_cols = int(row.max()) + 1, int(col.max()) + 1
    prow, pcol = [], []
    for m in sizes:
        k = rng.integers(0, len(row), m)
        r, c = row[k].copy(), col[k].copy()
        gone = rng.random(m) < absent
        r[gone] = rng.integers(0, n_rows, int(gone.sum()))
        c[gone] = rng.integers(0, n_cols, int(gone.sum()))
        prow.append(r)
        pcol.append(c)
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.concatenate(prow), np.concatenate(pcol), starts


def load_hosttest():
    """libh3d_hosttest.so's h3dt_cluster_stats as a Python function: returns
    (flags, dict mean / max / min / found)."""
    import ctypes
    from hic3defdr_amd import build
    lib = ctypes.CDLL(build.build_hosttest())
    P, I64, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    fn = lib.h3dt_cluster_stats
    fn.restype = I
    fn.argtypes = [P, P, P, I64, I, I, I64, I64, P, P, P, I64, P, P, P, P]

    def run(row, col, data, prow, pcol, starts, sorted=False, shape=None):
        row = np.ascontiguousarray(row, dtype=np.int64)
        col = np.ascontiguousarray(col, dtype=np.int64)
        data = np.ascontiguousarray(data, dtype=np.float64)
        if data.ndim == 1:
            data = data[:, None]
        prow = np.ascontiguousarray(prow, dtype=np.int64)
        pcol = np.ascontiguousarray(pcol, dtype=np.int64)
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        if shape is None:
            shape = (int(row.max()) + 1, int(col.max()) + 1) if len(row) \
                else (0, 0)
        k, K = len(starts) - 1, data.shape[1]
        out = {r: np.full((k, K), -7.0) for r in ('mean', 'max', 'min')}
        out['found'] = np.full(k, -7, dtype=np.int32)

        def p(a):
            return a.ctypes.data_as(P)
        rc = fn(p(row), p(col), p(data), len(row), K, int(sorted), shape[0],
                shape[1], p(prow), p(pcol), p(starts), k, p(out['mean']),
                p(out['max']), p(out['min']), p(out['found']))
        return rc, out
    return run
