"""CPU checks behind the per-cluster statistics (csrc/h3d_cstat.h,
csrc/h3d_cstat.hip, util.cluster_table.add_columns_to_cluster_table,
HiC3DeFDR.annotate): the numpy restatement (tests/annotate_cases.py) against
the reference's own output (tests/golden/annotate.npz); the host twin
h3dt_cluster_stats -- the device's keys, lookup, tasks, lane striding and
folds written serially -- against the restatement; the signatures and the
rejections, which happen before a device is touched; the extra columns of
ClusterTable through the TSV."""
import inspect

import numpy as np
import pytest

import annotate_cases as ac
from conftest import golden


@pytest.fixture(scope='module')
def twin():
    return ac.load_hosttest()


# -- the restatement against the reference -----------------------------------

def golden_calls(g, r):
    for j in range(int(g[r + '_ncalls'])):
        p = '%s_c%d_' % (r, j)
        t = '%s_c%d_' % (r, int(g[p + 'table']))
        yield dict(pattern=str(g[p + 'pattern']), row=g[t + 'row'],
                   col=g[t + 'col'], data=g[t + 'data'],
                   labels=[str(x) for x in g[p + 'labels']]
                   if bool(g[p + 'has_labels']) else None,
                   reducer=str(g[p + 'reducer']),
                   chrom=str(g[p + 'chrom']) or None)


GOLDEN_RECORDS = ['doc0', 'doc1', 'doc1a', 'doc2', 'rnd0', 'rnd1', 'rnd2',
                  'rnd3']


@pytest.mark.parametrize('r', GOLDEN_RECORDS)
def test_restatement_equals_reference_output(r):
    g = golden('annotate.npz')
    chroms = np.array([str(c) for c in g[r + '_chrom']])
    pts, starts = g[r + '_pts'], g[r + '_starts']
    cols = {}
    for c in golden_calls(g, r):
        data = c['data'] if c['data'].ndim == 2 else c['data'][:, None]
        rows = np.ones(len(chroms), dtype=bool) if c['chrom'] is None \
            else chroms == c['chrom']
        for i in range(data.shape[1]):
            name = c['pattern'] % c['labels'][i] if c['labels'] is not None \
                else c['pattern']
            v = cols.setdefault(name, np.full(len(chroms), np.nan))
            out, _ = ac.reduce_clusters(c['row'], c['col'], data[:, i],
                                        pts[:, 0], pts[:, 1], starts,
                                        c['reducer'])
            v[rows] = out[rows, 0]
    assert list(cols) == [str(n) for n in g[r + '_names']]
    want = g[r + '_out']
    for i, name in enumerate(cols):
        np.testing.assert_array_equal(cols[name], want[:, i], err_msg=name)


# -- the host twin against the restatement -----------------------------------

def check_twin(twin, row, col, data, prow, pcol, starts, sorted=False):
    rc, out = twin(row, col, data, prow, pcol, starts, sorted=sorted)
    assert rc == 0
    share = 0.0
    for red in ('max', 'min'):
        ref, found = ac.reduce_clusters(row, col, data, prow, pcol, starts,
                                        red)
        ac.assert_extrema(out[red], ref)
        np.testing.assert_array_equal(out['found'], found)
    ref, _ = ac.reduce_clusters(row, col, data, prow, pcol, starts, 'mean')
    share = ac.assert_means(out['mean'], ref,
                            ac.mean_bound(row, col, data, prow, pcol, starts))
    return share, out


@pytest.mark.parametrize('K', ac.KS)
def test_host_twin_equals_restatement(twin, K):
    """Cluster sizes around the lane count and the task size, absent pixels
    and repeats, NaN / inf / -0.0 among the data: max, min and found equal,
    mean within (2m + 2) 2^-53 mean|v|. The largest share of the bound seen
    over these cases is 0.41."""
    rng = np.random.default_rng(1100 + K)
    row, col, data = ac.banded_table(rng, K=K)
    prow, pcol, starts = ac.sized_clusters(rng, row, col, ac.SIZES)
    share, _ = check_twin(twin, row, col, data, prow, pcol, starts)
    print('K=%d: largest share of the mean bound %.3g' % (K, share))
    assert share <= 1.0
    # the same table in (row, col) order under the sorted promise: the same
    # bits (the lookup finds the same table rows)
    order = np.lexsort((col, row))
    rc, a = twin(row, col, data, prow, pcol, starts)
    rc2, b = twin(row[order], col[order], data[order], prow, pcol, starts,
                  sorted=True)
    assert rc == 0 and rc2 == 0
    for f in ('mean', 'max', 'min', 'found'):
        assert ac.bits_equal(a[f], b[f]), f


def test_host_twin_finite_data_mean_share(twin):
    """No special values: every mean is finite and held to the bound."""
    rng = np.random.default_rng(77)
    row, col, data = ac.banded_table(rng, K=4, special=False)
    prow, pcol, starts = ac.sized_clusters(rng, row, col, ac.SIZES)
    share, out = check_twin(twin, row, col, data, prow, pcol, starts)
    assert np.isfinite(out['mean']).all() and 0 < share <= 1.0


def test_host_twin_cluster_is_pure(twin):
    """A cluster alone = the same cluster among others, bit for bit."""
    rng = np.random.default_rng(5)
    row, col, data = ac.banded_table(rng, K=3)
    prow, pcol, starts = ac.sized_clusters(rng, row, col, ac.SIZES)
    _, allc = twin(row, col, data, prow, pcol, starts)
    for k in (0, 5, 9):
        a, b = starts[k], starts[k + 1]
        _, one = twin(row, col, data, prow[a:b], pcol[a:b], [0, b - a])
        for f in ('mean', 'max', 'min', 'found'):
            assert ac.bits_equal(one[f][0], allc[f][k]), (k, f)


def test_host_twin_empty_table_and_flags(twin):
    z = np.zeros(0, dtype=np.int64)
    rc, out = twin(z, z, np.zeros((0, 2)), [0, 1], [0, 3], [0, 2],
                   shape=(4, 4))
    assert rc == 0
    for f in ('mean', 'max', 'min'):
        np.testing.assert_array_equal(out[f], np.zeros((1, 2)))
    assert out['found'][0] == 0
    row, col = np.array([0, 0, 1]), np.array([1, 2, 1])
    data = np.ones((3, 1))
    one = ([0], [1], [0, 1])
    assert twin(row, col, data, *one)[0] == 0
    # a repeated table pixel, sorted or not
    assert twin([0, 0, 0], [1, 2, 1], data, *one)[0] & 1
    assert twin([0, 0, 1], [1, 1, 1], data, *one, sorted=True)[0] & 1
    assert twin([0, -1, 1], [1, 1, 1], data, *one)[0] & 1
    # a broken promise
    assert twin([0, 1, 0], [1, 1, 2], data, *one, sorted=True)[0] == 2
    # a cluster pixel outside the shape, a negative one
    assert twin(row, col, data, [2], [1], [0, 1])[0] == 4
    assert twin(row, col, data, [0], [-1], [0, 1])[0] == 4
    # an empty cluster
    assert twin(row, col, data, [0], [1], [0, 0, 1])[0] == 8


# -- the Python surface: signatures and rejections without a device ----------

def test_signatures():
    from hic3defdr_amd.util import cluster_table, clusters
    from hic3defdr_amd.analysis.constructor import HiC3DeFDR
    sig = inspect.signature(cluster_table.add_columns_to_cluster_table)
    assert list(sig.parameters) == ['cluster_table', 'name_pattern', 'row',
                                    'col', 'data', 'labels', 'reducer',
                                    'chrom']
    assert [p.default for p in sig.parameters.values()][5:] == \
        [None, 'mean', None]
    sig = inspect.signature(clusters.cluster_stats_gpu)
    assert list(sig.parameters)[:6] == ['clusters', 'row', 'col', 'data',
                                        'reducers', 'ctx']
    assert sig.parameters['reducers'].default == ('mean',)
    sig = inspect.signature(HiC3DeFDR.annotate)
    assert list(sig.parameters) == ['self', 'fdr', 'cluster_size', 'columns',
                                    'outfile']
    assert sig.parameters['columns'].default == (('qvalues', 'min'),
                                                 ('mu_hat_alt', 'mean'))
    assert sig.parameters['fdr'].default == 0.05
    assert sig.parameters['cluster_size'].default == 3


@pytest.fixture
def no_device(monkeypatch):
    from hic3defdr_amd import _native

    def boom(*a, **k):
        raise AssertionError('a device was touched')
    for name in ('context', 'load_library', 'Context'):
        monkeypatch.setattr(_native, name, boom)


def test_rejections_happen_before_a_device_is_touched(no_device):
    from hic3defdr_amd.util.clusters import cluster_stats_gpu as f
    row, col = np.array([0, 0, 1]), np.array([1, 2, 1])
    data = np.arange(3.0)
    cl = [[(0, 1), (1, 1)]]
    with pytest.raises(AssertionError, match='device'):
        f(cl, row, col, data)                      # valid: reaches the ctx
    with pytest.raises(ValueError):
        f(cl, row, col, data, reducers=('median',))
    with pytest.raises(ValueError):
        f(cl, row, col, data, reducers=())
    with pytest.raises(ValueError):
        f(cl, row, col[:2], data)                  # lengths
    with pytest.raises(ValueError):
        f(cl, row, col, np.zeros((2, 2)))
    with pytest.raises(ValueError):
        f(cl, row, col, np.zeros((3, 2, 2)))       # dimensions
    with pytest.raises(ValueError):
        f(cl, row.reshape(3, 1), col, data)
    with pytest.raises(TypeError):
        f(cl, row.astype(float), col, data)        # dtypes
    with pytest.raises(TypeError):
        f(cl, row, col, np.array(['a', 'b', 'c']))
    with pytest.raises(TypeError):
        f([[(0.5, 1.0)]], row, col, data)
    with pytest.raises(ValueError):
        f(cl, row, col, np.zeros((3, 257)))        # K
    with pytest.raises(ValueError):
        f(cl, row, col, np.zeros((3, 0)))
    with pytest.raises(ValueError):
        f([[(0, 1)], []], row, col, data)          # an empty cluster
    with pytest.raises(ValueError):
        f([[(0, -1)]], row, col, data)             # negative cluster pixel
    with pytest.raises(IndexError):
        f([[(2, 1)]], row, col, data)              # beyond the shape
    with pytest.raises(IndexError):
        f([[(0, 3)]], row, col, data)
    with pytest.raises(ValueError):
        f(cl, np.array([0, 0, 2 ** 31]), col, data)  # coordinates
    with pytest.raises(ValueError):
        f(cl, np.array([0, -1, 1]), col, data)
    with pytest.raises(IndexError):
        f(cl, row[:0], col[:0], data[:0])          # an empty table: (0, 0)
    # no clusters: nothing to run
    out = f([], row, col, np.zeros((3, 2), dtype=int), reducers=('max',))
    assert out['max'].shape == (0, 2) and out['found'].shape == (0,)


def test_frame_function_rejections_and_bookkeeping(no_device):
    pd = pytest.importorskip('pandas')
    from hic3defdr_amd.util.cluster_table import \
        add_columns_to_cluster_table as add
    df = pd.DataFrame({'us_chrom': ['chr1', 'chr2'],
                       'ds_chrom': ['chr1', 'chr2'],
                       'cluster': ['[[1, 2], [1, 1]]', [[4, 4], [3, 4]]]})
    row, col, data = [1, 1, 4, 3], [2, 1, 4, 4], np.arange(8.).reshape(4, 2)
    with pytest.raises(ValueError):
        add(df, 'x', row, col, data[:, 0], reducer='median')
    with pytest.raises(ValueError):
        add(df, 'x', row, col, data[:3, 0])
    # a chromosome without rows: the columns appear as NaN, the string cell
    # is corrected in place, and no device is needed
    add(df, '%s_max', row, col, data, labels=['a', 'b'], reducer='max',
        chrom='chr9')
    assert list(df.columns[-2:]) == ['a_max', 'b_max']
    assert df[['a_max', 'b_max']].isna().all().all()
    assert df['cluster'][0] == [[1, 2], [1, 1]]
    with pytest.raises(AssertionError, match='device'):
        add(df, '%s_max', row, col, data, labels=['a', 'b'], chrom='chr1')


def test_annotate_rejects_before_loading(no_device, tmp_path):
    from hic3defdr_amd.analysis.constructor import HiC3DeFDR
    h = HiC3DeFDR.__new__(HiC3DeFDR)
    h.outdir = str(tmp_path)     # empty: any load would fail otherwise
    with pytest.raises(ValueError, match='stage'):
        h.annotate(columns=(('nonsense', 'min'),))
    with pytest.raises(ValueError, match='stage'):
        h.annotate(columns=(('row', 'min'),))
    with pytest.raises(ValueError, match='reducer'):
        h.annotate(columns=(('qvalues', 'median'),))
    with pytest.raises(ValueError):
        h.annotate(fdr=[0.05, 0.1], outfile=str(tmp_path / 'x.tsv'))
    assert list(tmp_path.iterdir()) == []


# -- ClusterTable extras ---------------------------------------------------

def small2_results():
    g = golden('calls_small2.npz')
    return bytes(g['file__results_0.05_3.tsv']).decode('ascii')


def test_table_without_extras_writes_todays_bytes(tmp_path):
    from hic3defdr_amd.util.cluster_table import ClusterTable
    text = small2_results()
    src, dst = tmp_path / 'in.tsv', tmp_path / 'out.tsv'
    src.write_text(text)
    t = ClusterTable.read_tsv(str(src))
    assert t.extras == {}
    t.to_tsv(str(dst))
    assert dst.read_text() == text
    # through take / sorted / concat / with_classification as well
    t2 = ClusterTable.concat([t.take(np.arange(len(t)))]).sorted()
    t2.to_tsv(str(dst))
    assert dst.read_text() == text


def test_extras_round_trip_through_tsv(tmp_path):
    pytest.importorskip('pandas')
    from hic3defdr_amd.util.cluster_table import ClusterTable, \
        load_cluster_table
    text = small2_results()
    src, dst = tmp_path / 'in.tsv', tmp_path / 'out.tsv'
    src.write_text(text)
    t = ClusterTable.read_tsv(str(src))
    n = len(t)
    rng = np.random.default_rng(3)
    a = rng.normal(size=n) * 10.0 ** rng.integers(-12, 12, n)
    a[[1, 7]] = np.nan
    a[2], a[3], a[4], a[5] = np.inf, -np.inf, -0.0, 5e-324
    b = np.arange(n, dtype=float)
    t.extras = {'q_min': a, 'mu_ES_mean': b}
    with pytest.raises(ValueError):
        ClusterTable(t.us_chrom, t.us_start, t.us_end, t.ds_chrom,
                     t.ds_start, t.ds_end, t.size, t.cluster,
                     extras={'x': np.zeros(n + 1)})
    # carried through take, sorted, concat and with_classification
    perm = rng.permutation(n)
    back = ClusterTable.concat([t.take(perm[:10]), t.take(perm[10:])]) \
        .sorted().with_classification('x')
    assert list(back.extras) == ['q_min', 'mu_ES_mean']
    assert ac.bits_equal(back.extras['q_min'], a)
    assert ac.bits_equal(back.extras['mu_ES_mean'], b)
    # a table without a column gets NaN there
    plain = ClusterTable.read_tsv(str(src))
    both = ClusterTable.concat([t, plain])
    assert np.isnan(both.extras['mu_ES_mean'][n:]).all()
    t.to_tsv(str(dst))
    lines = dst.read_text().split('\n')
    assert lines[0].split('\t')[-3:] == ['classification', 'q_min',
                                         'mu_ES_mean']
    # the leading columns are the plain table's own
    assert [ln.rsplit('\t', 2)[0] for ln in lines] == text.split('\n')
    assert lines[2].split('\t')[-2] == ''           # NaN: an empty field
    # the file is pandas' own text of the frame, so load_cluster_table reads
    # it as it reads a frame the reference wrote (pandas' default float
    # parser keeps some 15 significant digits; ClusterTable.read_tsv, below,
    # is exact)
    assert dst.read_text() == t.to_frame().to_csv(sep='\t')
    df = load_cluster_table(str(dst))
    np.testing.assert_array_equal(np.isnan(df['q_min'].to_numpy()),
                                  np.isnan(a))
    np.testing.assert_allclose(df['q_min'].to_numpy(), a, rtol=1e-12, atol=0)
    assert ac.bits_equal(df['mu_ES_mean'].to_numpy(), b)
    assert df['cluster'].iloc[0] == \
        load_cluster_table(str(src))['cluster'].iloc[0]
    # read_tsv ignores the columns unless asked
    assert ClusterTable.read_tsv(str(dst)).extras == {}
    got = ClusterTable.read_tsv(str(dst), extras=True)
    assert list(got.extras) == ['q_min', 'mu_ES_mean']
    assert ac.bits_equal(got.extras['q_min'], a)
    got = ClusterTable.read_tsv(str(dst), extras=['mu_ES_mean'])
    assert list(got.extras) == ['mu_ES_mean']
    assert list(t.to_frame().columns[-2:]) == ['q_min', 'mu_ES_mean']


def test_cluster_text_pixels():
    from hic3defdr_amd.util.clusters import cluster_text_pixels
    r, c, s = cluster_text_pixels(['[[1, 2], [1, 1]]', '[[40, 4]]'])
    np.testing.assert_array_equal(r, [1, 1, 40])
    np.testing.assert_array_equal(c, [2, 1, 4])
    np.testing.assert_array_equal(s, [0, 2, 3])
