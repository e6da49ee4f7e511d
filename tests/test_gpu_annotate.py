"""Per-cluster statistics on the GPU (csrc/h3d_cstat.hip) behind
cluster_stats_gpu, add_columns_to_cluster_table and HiC3DeFDR.annotate. The
yardstick of the arithmetic is the host twin h3dt_cluster_stats (the same
h3d_cstat.h folds written serially, held to the numpy restatement by
test_annotate_host.py): means, max, min and found are compared bit for bit.
The frames are held to the reference's own output (tests/golden/annotate.npz)
under the derived bound (2m + 2) 2^-53 mean|v| for the means and to equality
for max and min."""
import hashlib
import os
import shutil
import tempfile

import numpy as np
import pytest

from conftest import golden

import annotate_cases as ac

pytestmark = pytest.mark.gpu

FIELDS = ('mean', 'max', 'min', 'found')
ALL = ('mean', 'max', 'min')


@pytest.fixture(scope='module')
def ctx():
    from hic3defdr_amd import _native
    return _native.context(0)


@pytest.fixture(scope='module')
def twin():
    return ac.load_hosttest()


def assert_gpu_is_twin(ctx, twin, row, col, data, prow, pcol, starts, what):
    order = np.lexsort((col, row))
    rc, want = twin(row, col, data, prow, pcol, starts)
    assert rc == 0, what
    for sorted_ in (False, True):
        t = (row[order], col[order], data[order]) if sorted_ else \
            (row, col, data)
        got = ctx.cluster_stats(*t, prow, pcol, starts, reducers=ALL,
                                sorted=sorted_)
        for f in FIELDS:
            assert got[f].dtype == want[f].dtype, (what, f)
            assert ac.bits_equal(got[f].reshape(want[f].shape), want[f]), \
                (what, f, sorted_)
    return want


@pytest.mark.parametrize('total', [1, 63, 64, 65, 257, 4097])
def test_pixel_totals_equal_the_host_twin(ctx, twin, total):
    """The cluster pixels of a call split over clusters at random: either
    side of a wave, of a workgroup and of a second grid-stride block."""
    rng = np.random.default_rng(total)
    row, col, data = ac.banded_table(rng, K=3)
    cuts = np.unique(rng.integers(1, total, min(total, 40))) if total > 1 \
        else np.zeros(0, dtype=np.int64)
    sizes = np.diff(np.concatenate([[0], cuts, [total]]))
    sizes = sizes[sizes > 0]
    prow, pcol, starts = ac.sized_clusters(rng, row, col, sizes)
    assert starts[-1] == total
    assert_gpu_is_twin(ctx, twin, row, col, data, prow, pcol, starts, total)


def test_no_clusters_and_an_empty_table(ctx):
    row, col, data = ac.banded_table(np.random.default_rng(0), K=2)
    z = np.zeros(0, dtype=np.int64)
    out = ctx.cluster_stats(row, col, data, z, z, [0], reducers=ALL)
    assert out['mean'].shape == (0, 2) and out['found'].shape == (0,)
    # n == 0 at the ABI (the Python rule refuses it: the shape is (0, 0))
    import torch
    dev = torch.device('cuda', ctx.device)
    e = torch.zeros(0, dtype=torch.int64, device=dev)
    p = torch.tensor([0, 3, 1], dtype=torch.int64, device=dev)
    out = ctx.cluster_stats_dev(
        e, e, torch.zeros((0, 2), dtype=torch.float64, device=dev), 4, 4,
        p, p, torch.tensor([0, 2, 3], dtype=torch.int64, device=dev),
        reducers=ALL)
    for f in ALL:
        assert out[f].cpu().numpy().tobytes() == np.zeros((2, 2)).tobytes()
    assert out['found'].cpu().tolist() == [0, 0]


@pytest.mark.parametrize('K', ac.KS)
def test_cluster_sizes_and_column_counts_equal_the_host_twin(ctx, twin, K):
    """Sizes around the lane count and the task size, every column blocking
    (1, 2, 4, 8 columns, the paired loads for even K, two and three blocks),
    absent and repeated pixels, NaN / inf / -0.0."""
    rng = np.random.default_rng(1100 + K)
    row, col, data = ac.banded_table(rng, K=K)
    prow, pcol, starts = ac.sized_clusters(rng, row, col, ac.SIZES)
    want = assert_gpu_is_twin(ctx, twin, row, col, data, prow, pcol, starts,
                              K)
    assert np.isnan(want['max']).any() and (want['found'] > 0).any()
    # one reducer at a time gives the same bits
    for red in ALL:
        got = ctx.cluster_stats(row, col, data, prow, pcol, starts,
                                reducers=(red,))
        assert sorted(got) == sorted([red, 'found'])
        assert ac.bits_equal(got[red], want[red]), red


def test_4097_three_pixel_clusters_and_purity(ctx, twin):
    """4,097 clusters of three pixels in one call = the host twin; a cluster
    computed alone = the same cluster among the 4,096 others, also next to a
    cluster of many tasks; reruns and a second ctx repeat the bits."""
    from hic3defdr_amd import _native
    rng = np.random.default_rng(4097)
    row, col, data = ac.banded_table(rng, K=4)
    sizes = np.full(4097, 3)
    prow, pcol, starts = ac.sized_clusters(rng, row, col, sizes)
    want = assert_gpu_is_twin(ctx, twin, row, col, data, prow, pcol, starts,
                              'triples')
    for k in (0, 2048, 4096):
        a, b = starts[k], starts[k + 1]
        one = ctx.cluster_stats(row, col, data, prow[a:b], pcol[a:b], [0, 3],
                                reducers=ALL)
        for f in FIELDS:
            assert ac.bits_equal(one[f][0], want[f][k]), (k, f)
    # a large cluster alone and between the triples
    big_r, big_c, _ = ac.sized_clusters(rng, row, col, [3 * ac.CHUNK + 5])
    alone = ctx.cluster_stats(row, col, data, big_r, big_c,
                              [0, len(big_r)], reducers=ALL)
    mixed = ctx.cluster_stats(
        row, col, data, np.concatenate([prow[:300], big_r, prow[300:]]),
        np.concatenate([pcol[:300], big_c, pcol[300:]]),
        np.concatenate([starts[:101], starts[100:] + len(big_r)]),
        reducers=ALL)
    for f in FIELDS:
        assert ac.bits_equal(mixed[f][100], alone[f][0]), f
        assert ac.bits_equal(np.delete(mixed[f], 100, axis=0), want[f]), f
    other = _native.Context(0)
    for c in (ctx, ctx, other):
        again = c.cluster_stats(row, col, data, prow, pcol, starts,
                                reducers=ALL)
        for f in FIELDS:
            assert ac.bits_equal(again[f], want[f]), f


def test_dev_tensors_equal_the_host_array_call(ctx):
    import torch
    dev = torch.device('cuda', ctx.device)
    rng = np.random.default_rng(12)
    for K in (1, 2, 5):
        row, col, data = ac.banded_table(rng, K=K)
        prow, pcol, starts = ac.sized_clusters(rng, row, col,
                                               [1, 3, 65, ac.CHUNK + 1])
        want = ctx.cluster_stats(row, col, data, prow, pcol, starts,
                                 reducers=ALL)
        t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
             for a in (row, col, data, prow, pcol, starts)]
        got = ctx.cluster_stats_dev(t[0], t[1], t[2], int(row.max()) + 1,
                                    int(col.max()) + 1, t[3], t[4], t[5],
                                    reducers=ALL)
        for f in FIELDS:
            assert ac.bits_equal(got[f].cpu().numpy(), want[f]), (K, f)
        # data whose base is 8 bytes off a 16-byte boundary: the unpaired loads
        if K == 2:
            pad = torch.zeros(len(row) * K + 1, dtype=torch.float64,
                              device=dev)
            off = pad[1:].view(len(row), K)
            off.copy_(t[2])
            assert off.data_ptr() % 16 == 8
            got = ctx.cluster_stats_dev(t[0], t[1], off, int(row.max()) + 1,
                                        int(col.max()) + 1, t[3], t[4], t[5],
                                        reducers=ALL)
            for f in FIELDS:
                assert ac.bits_equal(got[f].cpu().numpy(), want[f]), f


def test_the_device_sets_its_own_flags(ctx):
    """Through the _dev form, which the Python checks do not cover: the flag
    bits come from compares on the device, and nothing reads out of bounds."""
    import torch
    from hic3defdr_amd import _native
    dev = torch.device('cuda', ctx.device)

    def run(row, col, prow, pcol, starts, sorted=False, check=False,
            shape=(8, 8)):
        def t(a):
            return torch.tensor(a, dtype=torch.int64, device=dev)
        data = torch.ones((len(row), 1), dtype=torch.float64, device=dev)
        return ctx.cluster_stats_dev(t(row), t(col), data, shape[0],
                                     shape[1], t(prow), t(pcol), t(starts),
                                     sorted=sorted, check=check)
    ok = ([0, 0, 1], [1, 2, 1])
    one = ([0], [1], [0, 1])
    out = run(*ok, *one, sorted=True)
    assert out['flags'] == 0 and out['mean'].cpu().tolist() == [[1.0]]
    # a repeated table pixel, unsorted and under the promise; a coordinate
    # outside [0, 2^31)
    assert run([0, 1, 0], [1, 1, 1], *one)['flags'] & _native.CSTAT_REPEAT
    assert run([0, 0, 1], [1, 1, 1], *one, sorted=True)['flags'] \
        & _native.CSTAT_REPEAT
    assert run([0, 2 ** 31, 1], [1, 1, 1], *one)['flags'] \
        & _native.CSTAT_REPEAT
    assert run([0, -1, 1], [1, 1, 1], *one, sorted=True)['flags'] \
        & _native.CSTAT_REPEAT
    # a broken promise
    assert run([0, 1, 0], [1, 1, 2], *one, sorted=True)['flags'] \
        == _native.CSTAT_ORDER
    # cluster pixels outside [0, n_rows) x [0, n_cols), far outside included
    for r, c in ((8, 1), (1, 8), (-1, 1), (1, -1), (2 ** 40, 1),
                 (1, -2 ** 62)):
        assert run(*ok, [0, r], [1, c], [0, 2])['flags'] \
            == _native.CSTAT_PIXEL, (r, c)
    # an empty cluster; starts that do not begin at 0
    assert run(*ok, [0], [1], [0, 0, 1])['flags'] == _native.CSTAT_STARTS
    assert run(*ok, [0, 0], [1, 1], [1, 2])['flags'] == _native.CSTAT_STARTS
    # the exceptions of the flags
    with pytest.raises(ValueError, match='repeats'):
        run([0, 1, 0], [1, 1, 1], *one, check=True)
    with pytest.raises(ValueError, match='order'):
        run([0, 1, 0], [1, 1, 2], *one, sorted=True, check=True)
    with pytest.raises(IndexError):
        run(*ok, [8], [1], [0, 1], check=True)
    # the host-array call raises the same for what only the device can see
    with pytest.raises(ValueError, match='repeats'):
        ctx.cluster_stats([0, 1, 0], [1, 1, 1], np.ones(3), *one)
    with pytest.raises(ValueError, match='order'):
        ctx.cluster_stats([0, 1, 0], [1, 1, 2], np.ones(3), *one, sorted=True)


# -- the frames against the reference ---------------------------------------

def golden_frame(g, r):
    import pandas as pd
    chroms = [str(c) for c in g[r + '_chrom']]
    pts, starts = g[r + '_pts'], g[r + '_starts']
    cells = [pts[a:b].tolist() for a, b in zip(starts[:-1], starts[1:])]
    return pd.DataFrame({'us_chrom': chroms, 'ds_chrom': chroms,
                         'cluster': cells})


def assert_frame(df, g, r, calls):
    """Columns, NaN cells and values: max / min equal, means within the
    bound of the call that wrote the cell."""
    names = [str(n) for n in g[r + '_names']]
    assert list(df.columns[3:]) == names
    want = g[r + '_out']
    chroms = np.array([str(c) for c in g[r + '_chrom']])
    pts, starts = g[r + '_pts'], g[r + '_starts']
    bound = {}
    for c in calls:
        data = c['data'] if c['data'].ndim == 2 else c['data'][:, None]
        rows = np.ones(len(chroms), dtype=bool) if c['chrom'] is None \
            else chroms == c['chrom']
        b = ac.mean_bound(c['row'], c['col'], data, pts[:, 0], pts[:, 1],
                          starts)
        for i in range(data.shape[1]):
            name = c['pattern'] % c['labels'][i] if c['labels'] is not None \
                else c['pattern']
            bound.setdefault(name, np.zeros(len(chroms)))[rows] = \
                b[rows, i] if c['reducer'] == 'mean' else 0.0
    for i, name in enumerate(names):
        got = df[name].to_numpy(dtype=np.float64)
        if bound[name].any():
            ac.assert_means(got, want[:, i], bound[name])
        else:
            ac.assert_extrema(got, want[:, i])


@pytest.mark.parametrize('r', ['doc0', 'doc1', 'doc1a', 'doc2', 'rnd0',
                               'rnd1', 'rnd2', 'rnd3'])
def test_add_columns_equals_the_reference(r):
    from test_annotate_host import golden_calls
    from hic3defdr_amd.util.cluster_table import add_columns_to_cluster_table
    g = golden('annotate.npz')
    df = golden_frame(g, r)
    if r == 'doc2':   # string cells are corrected in place
        df['cluster'] = [str(c) for c in df['cluster']]
    calls = list(golden_calls(g, r))
    for c in calls:
        ret = add_columns_to_cluster_table(
            df, c['pattern'], c['row'], c['col'], c['data'],
            labels=c['labels'], reducer=c['reducer'], chrom=c['chrom'])
        assert ret is None
    assert all(isinstance(c, list) for c in df['cluster'])
    assert_frame(df, g, r, calls)


# -- the class on small2 -----------------------------------------------------

def sha_of_files(outdir, skip=()):
    out = {}
    for f in sorted(os.listdir(outdir)):
        if f not in skip:
            with open(os.path.join(outdir, f), 'rb') as fh:
                out[f] = hashlib.sha256(fh.read()).hexdigest()
    return out


@pytest.fixture(scope='module')
def small2_outdir():
    """The reference's outdir arrays of small2 and its results file."""
    from test_calls import fill_outdir_from_golden
    outdir = tempfile.mkdtemp(prefix='h3d_annotate_')
    h = fill_outdir_from_golden('small2', outdir)
    text = bytes(golden('calls_small2.npz')['file__results_0.05_3.tsv'])
    with open(os.path.join(outdir, 'results_0.05_3.tsv'), 'wb') as fh:
        fh.write(text)
    yield h, outdir, text.decode('ascii')
    h.flush()
    shutil.rmtree(outdir, ignore_errors=True)


def test_annotate_on_small2(small2_outdir):
    from hic3defdr_amd.util.cluster_table import ClusterTable
    from hic3defdr_amd.util.clusters import cluster_text_pixels, \
        cluster_stats_gpu
    h, outdir, text = small2_outdir
    g = golden('annotate.npz')
    before = sha_of_files(outdir)
    h.annotate()
    made = os.path.join(outdir, 'results_0.05_3_annotated.tsv')
    assert sha_of_files(outdir, skip=['results_0.05_3_annotated.tsv']) \
        == before
    with open(made, 'rb') as fh:
        first = fh.read()
    names = ['qvalues_min', 'mu_hat_alt_ES_mean', 'mu_hat_alt_NPC_mean']
    assert [str(n) for n in g['small2_names']] == names
    lines = first.decode('ascii').split('\n')
    assert lines[0].split('\t')[-3:] == names
    # rows and leading columns are the results file's own
    assert [ln.rsplit('\t', 3)[0] for ln in lines] == text.split('\n')
    t = ClusterTable.read_tsv(made, extras=True)
    assert list(t.extras) == names
    # against the restatement on what load_data returns, and found = size
    prow, pcol, starts = cluster_text_pixels(t.cluster)
    us = np.array(t.us_chrom)
    assert [str(c) for c in g['small2_chrom']] == t.us_chrom
    for ch in h.chroms:
        rows = np.flatnonzero(us == ch)
        assert len(rows)
        # this chromosome's clusters alone (the other's pixels may lie
        # beyond its tables' shape)
        sz = np.diff(starts)[rows]
        st = np.concatenate([[0], np.cumsum(sz)])
        pix = np.repeat(starts[rows] - st[:-1], sz) + np.arange(st[-1])
        pr, pc = prow[pix], pcol[pix]
        for stage, red, cols in (('qvalues', 'min', names[:1]),
                                 ('mu_hat_alt', 'mean', names[1:])):
            row, col, data = h.load_data(stage, ch, coo=True)
            ref, found = ac.reduce_clusters(row, col, data, pr, pc, st, red)
            np.testing.assert_array_equal(found, t.size[rows])
            got = np.column_stack([t.extras[n] for n in cols])[rows]
            if red == 'min':
                ac.assert_extrema(got, ref)
            else:
                b = ac.mean_bound(row, col, data, pr, pc, st)
                ac.assert_means(got, ref, b)
                # the reference's annotated table (the same outdir arrays)
                ac.assert_means(got, g['small2_out'][rows, 1:], b)
        cl = [np.column_stack([pr[a:b], pc[a:b]]).tolist()
              for a, b in zip(st[:-1], st[1:])]
        row, col, q = h.load_data('qvalues', ch, coo=True)
        out = cluster_stats_gpu(cl, row, col, q, reducers=('min',),
                                sorted=True)
        np.testing.assert_array_equal(out['found'], t.size[rows])
    ac.assert_extrema(t.extras['qvalues_min'], g['small2_out'][:, 0])
    assert not np.isnan(g['small2_out']).any()
    # a second call writes the same bytes; outfile and other columns
    h.annotate()
    with open(made, 'rb') as fh:
        assert fh.read() == first
    other = os.path.join(outdir, 'custom.tsv')
    h.annotate(fdr=0.05, cluster_size=3, outfile=other,
               columns=(('qvalues', 'max'), ('qvalues', 'min'),
                        ('loop_idx', 'mean')))
    t2 = ClusterTable.read_tsv(other, extras=True)
    assert list(t2.extras) == ['qvalues_max', 'qvalues_min', 'loop_idx_mean']
    assert ac.bits_equal(t2.extras['qvalues_min'], t.extras['qvalues_min'])
    assert np.all(t2.extras['qvalues_max'] >= t2.extras['qvalues_min'])
    assert np.all(t2.extras['loop_idx_mean'] == 1.0)
    os.remove(other)
    os.remove(made)


def test_annotate_collects_a_missing_results_file(small2_outdir):
    h, outdir, text = small2_outdir
    path = os.path.join(outdir, 'results_0.2_1.tsv')
    assert not os.path.exists(path)
    h.annotate(fdr=0.2, cluster_size=1, columns=(('mu_hat_alt', 'max'),))
    with open(path) as fh:
        plain = fh.read()
    with open(path.replace('.tsv', '_annotated.tsv')) as fh:
        lines = fh.read().split('\n')
    assert lines[0].endswith(
        '\tclassification\tmu_hat_alt_ES_max\tmu_hat_alt_NPC_max')
    assert [ln.rsplit('\t', 2)[0] for ln in lines] == plain.split('\n')
