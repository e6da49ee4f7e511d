"""The connected-component calls on the GPU (csrc/h3d_clusters.hip) behind
ClusterList.find_gpu, threshold_clusters_gpu, classify_clusters_gpu and the
class's threshold / classify / collect(gpu=True). The yardstick is
scipy.ndimage.label per class, renumbered by first member
(tests/cluster_cases.py): labels, sizes, classes, bounding boxes, members and
starts are integers and are held to equality; the scale cases have answers
in closed form."""
import json
import os
import shutil
import tempfile

import numpy as np
import pytest

from conftest import e2e_inputs, golden

import cluster_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from hic3defdr_amd import _native
    return _native.context(0)


def _assert_lists(got, want, what):
    for k in ('size', 'cls_of', 'bounds', 'members', 'starts'):
        assert got[k].dtype == want[k].dtype, (what, k)
        np.testing.assert_array_equal(got[k], want[k],
                                      err_msg='%s %s' % (what, k))


def _check(ctx, row, col, cls, what, sizes=(1, 3)):
    for conn in (1, 2):
        want, nc = cc.labels_ref(row, col, cls, conn)
        got, gc = ctx.label_components(row, col, cls, conn)
        assert got.dtype == np.int32
        assert gc == nc, (what, conn)
        np.testing.assert_array_equal(got, want,
                                      err_msg='%s conn %d' % (what, conn))
        for ms in sizes:
            _assert_lists(ctx.cluster_lists(got, cls, row, col, gc, ms),
                          cc.lists_ref(want, nc, row, col, cls, ms),
                          '%s conn %d min_size %d' % (what, conn, ms))
    return nc


@pytest.mark.parametrize('n', cc.N_LIST)
def test_random_band_sets_equal_the_restatement(ctx, n):
    for classes, absent in ((1, 0.), (2, 0.), (2, 0.2), (3, 0.1)):
        row, col, cls = cc.random_band(n, 11, classes=classes, absent=absent)
        _check(ctx, row, col, cls, 'n%d c%d a%g' % (n, classes, absent))
    if n:
        row, col, cls = cc.random_band(n, 12)
        got, gc = ctx.label_components(row, col, np.full(n, 255, np.uint8), 1)
        assert gc == 0 and np.all(got == -1)
        out = ctx.cluster_lists(got, cls, row, col, 0)
        assert len(out['members']) == 0 and out['starts'].tolist() == [0]


@pytest.mark.parametrize('name', sorted(cc.STRUCTURED))
def test_structured_cases_equal_the_restatement(ctx, name):
    row, col, cls = cc.STRUCTURED[name]()
    nc = _check(ctx, row, col, cls, name)
    if name == 'serpentine_cut':
        assert nc == 150
    if name == 'serpentine':
        assert ctx.label_components(row, col, cls, 2)[1] == 1
        assert ctx.label_components(row, col, cls, 1)[1] == 76


def test_stripes_of_4097_runs_over_17_workgroups(ctx):
    row, col, cls = cc.stripes(4097)
    assert len(row) == 4097
    _check(ctx, row, col, cls, 'stripes 4097')


def test_scale_full_band_is_one_cluster(ctx):
    bins, band = 5100, 200
    row, col = cc.band_pixels(bins, band)
    n = len(row)
    assert 10 ** 6 <= n < 1.02 * 10 ** 6
    cls = np.zeros(n, dtype=np.uint8)
    for conn in (1, 2):
        label, nc = ctx.label_components(row, col, cls, conn)
        assert nc == 1 and not label.any()
    out = ctx.cluster_lists(label, cls, row, col, 1, 3)
    assert out['size'].tolist() == [n] and out['cls_of'].tolist() == [0]
    assert out['bounds'].ravel().tolist() == [0, bins - 1, 0, bins - 1]
    assert out['starts'].tolist() == [0, n]
    np.testing.assert_array_equal(out['members'], np.arange(n, dtype=np.int32))


def test_scale_checkerboard_is_all_singletons(ctx):
    row, col, cls = cc.checkerboard(10100, 200)
    n = len(row)
    assert 10 ** 6 <= n < 1.02 * 10 ** 6
    label, nc = ctx.label_components(row, col, cls, 1)
    assert nc == n
    np.testing.assert_array_equal(label, np.arange(n, dtype=np.int32))
    out = ctx.cluster_lists(label, cls, row, col, n, 1)
    assert np.all(out['size'] == 1) and not out['cls_of'].any()
    np.testing.assert_array_equal(out['bounds'],
                                  np.stack([row, row, col, col]))
    np.testing.assert_array_equal(out['members'], np.arange(n, dtype=np.int32))
    np.testing.assert_array_equal(out['starts'], np.arange(n + 1))
    out = ctx.cluster_lists(label, cls, row, col, n, 2)
    assert len(out['members']) == 0 and out['starts'].tolist() == [0]
    assert ctx.label_components(row, col, cls, 2)[1] == 1


def test_reruns_and_a_second_ctx_are_bit_identical(ctx):
    from hic3defdr_amd import _native
    other = _native.Context(0)
    cases = [cc.stripes(4097), cc.serpentine(),
             cc.random_band(4097, 3, classes=3, absent=0.1)]
    for row, col, cls in cases:
        for conn in (1, 2):
            first, nc = ctx.label_components(row, col, cls, conn)
            lists = ctx.cluster_lists(first, cls, row, col, nc, 2)
            for c in (ctx, ctx, other):
                again, nc2 = c.label_components(row, col, cls, conn)
                assert nc2 == nc and again.tobytes() == first.tobytes()
                l2 = c.cluster_lists(again, cls, row, col, nc, 2)
                for k in lists:
                    assert l2[k].tobytes() == lists[k].tobytes(), k


def test_dev_tensors_equal_the_host_array_call(ctx):
    import torch
    dev = torch.device('cuda', ctx.device)
    row, col, cls = cc.random_band(4097, 5, classes=2, absent=0.2)
    t_row, t_col = (torch.from_numpy(a).to(dev) for a in (row, col))
    t_cls = torch.from_numpy(cls).to(dev)
    for conn in (1, 2):
        label, nc = ctx.label_components(row, col, cls, conn)
        t_label, t_nc = ctx.label_components_dev(t_row, t_col, t_cls, conn)
        assert t_nc == nc and t_label.dtype == torch.int32
        np.testing.assert_array_equal(t_label.cpu().numpy(), label)
        want = ctx.cluster_lists(label, cls, row, col, nc, 2)
        got = ctx.cluster_lists_dev(t_label, t_cls, t_row, t_col, nc, 2)
        _assert_lists({k: v.cpu().numpy() for k, v in got.items()}, want,
                      'dev conn %d' % conn)
    # the class bytes on the device against numpy
    rng = np.random.default_rng(4)
    q = rng.random(4097)
    q[::5] = np.nan
    got = ctx.threshold_classes_dev(torch.from_numpy(q).to(dev), 0.3)
    np.testing.assert_array_equal(
        got.cpu().numpy(), np.where(q < 0.3, 0, np.where(q >= 0.3, 1, 255)))
    value = np.round(rng.random((4097, 3)), 1)
    value[rng.random((4097, 3)) < 0.1] = np.nan
    member = rng.random(4097) < 0.7
    got = ctx.argmax_classes_dev(torch.from_numpy(value).to(dev),
                                 torch.from_numpy(member).to(dev))
    np.testing.assert_array_equal(
        got.cpu().numpy(), np.where(member, np.argmax(value, axis=1), 255))


def test_the_device_checks_the_input_rule(ctx):
    import torch
    from hic3defdr_amd._native import H3DError
    dev = torch.device('cuda', ctx.device)
    row, col, cls = cc.random_band(257, 9)
    for what in ('swap', 'repeat', 'negative', 'wide'):
        r, c = row.copy(), col.copy()
        if what == 'swap':
            r[[100, 101]], c[[100, 101]] = r[[101, 100]], c[[101, 100]]
        elif what == 'repeat':
            r[200], c[200] = r[199], c[199]
        elif what == 'negative':
            c[0] = -1
        else:
            r[256] = 2 ** 31
        with pytest.raises(ValueError):
            ctx.label_components(r, c, cls)
        with pytest.raises(ValueError):
            ctx.label_components_dev(torch.from_numpy(r).to(dev),
                                     torch.from_numpy(c).to(dev),
                                     torch.from_numpy(cls).to(dev))
    with pytest.raises(H3DError):
        ctx.label_components(row, col, cls, connectivity=3)
    with pytest.raises(H3DError):                        # a label out of range
        ctx.cluster_lists(np.full(257, 5, np.int32), cls, row, col, 5)
    # and the call after a rejected one is sound
    _check(ctx, row, col, cls, 'after rejections')


def test_find_gpu_and_find_clusters_gpu(ctx):
    import scipy.sparse as sparse
    from hic3defdr_amd.util.clusters import (ClusterList, find_clusters,
                                             find_clusters_gpu)
    row, col, _ = cc.random_band(4097, 21)
    for conn in (1, 2):
        got = ClusterList.find_gpu(row, col, conn)
        want = ClusterList.find(row, col, conn)
        assert cc.frozen(got) == cc.frozen(want) and len(got) == len(want)
        cc.assert_canonical(got)
        b = got.bounds()
        got._bounds = None
        for x, y in zip(b, got.bounds()):
            np.testing.assert_array_equal(x, y)
    m = sparse.coo_matrix((np.ones(len(row), bool), (row, col)))
    got = find_clusters_gpu(m, 2)
    assert {frozenset(s) for s in got} == \
        {frozenset(s) for s in find_clusters(m, 2)}
    assert find_clusters_gpu(sparse.coo_matrix((4, 4), dtype=bool)) == []


# -- small2: the utilities against the host path ------------------------------

def _small2_calls():
    ref = golden('calls_small2.npz')
    return ([float(x) for x in ref['meta_fdrs']],
            [int(x) for x in ref['meta_sizes']])


def test_threshold_clusters_gpu_equals_host_on_small2():
    from hic3defdr_amd.util.thresholding import (threshold_clusters,
                                                 threshold_clusters_gpu)
    g, kw = e2e_inputs('small2')
    fdrs, _ = _small2_calls()
    n_sig = 0
    for c in kw['chroms']:
        sel = g['disp_idx__%s' % c]
        row, col = g['row__%s' % c][sel], g['col__%s' % c][sel]
        sel = g['loop_idx__%s' % c]
        row, col = row[sel], col[sel]
        q = g['qvalues__%s' % c].copy()
        assert len(q) == len(row)
        q[::11] = np.nan                                  # planted NaNs
        pairs = threshold_clusters_gpu(q, row, col, fdrs, [1, 3])
        assert len(pairs) == len(fdrs)
        for f, (sig, insig) in zip(fdrs, pairs):
            hs, hi = threshold_clusters(q, row, col, f)
            for size in (1, 3):
                for got, want in ((sig, hs), (insig, hi)):
                    got, want = got.size_filter(size), want.size_filter(size)
                    assert len(got) == len(want)
                    assert cc.frozen(got) == cc.frozen(want)
                    cc.assert_canonical(got)
            one = threshold_clusters_gpu(q, row, col, f, 3)
            assert cc.frozen(one[0]) == cc.frozen(hs.size_filter(3))
            assert cc.frozen(one[1]) == cc.frozen(hi.size_filter(3))
        n_sig += sum(len(s) for s, _ in pairs)
    assert n_sig


def test_classify_clusters_gpu_equals_host_on_small2():
    from hic3defdr_amd.util.classification import (classify_clusters,
                                                   classify_clusters_gpu)
    from hic3defdr_amd.util.thresholding import threshold_clusters
    g, kw = e2e_inputs('small2')
    fdrs, _ = _small2_calls()
    seen = 0
    for c in kw['chroms']:
        sel = g['disp_idx__%s' % c]
        row, col = g['row__%s' % c][sel], g['col__%s' % c][sel]
        sel = g['loop_idx__%s' % c]
        row, col = row[sel], col[sel]
        q = g['qvalues__%s' % c].copy()
        q[::11] = np.nan
        value = g['mu_hat_alt__%s' % c][sel].copy()
        assert value.shape[0] == len(row)
        value[::7, 0] = np.nan                            # a NaN wins
        value[::5, 1] = value[::5, 0]                     # ties: the first wins
        for f in fdrs:
            for size in (1, 3):
                sig = threshold_clusters(q, row, col, f)[0].size_filter(size)
                want = classify_clusters(row, col, value, sig)
                got = classify_clusters_gpu(row, col, value, sig)
                assert len(got) == len(want) == value.shape[1]
                for a, b in zip(got, want):
                    assert len(a) == len(b) and cc.frozen(a) == cc.frozen(b)
                    cc.assert_canonical(a)
                    seen += len(a)
    assert seen


# -- the class: threshold / classify / collect(gpu=True) ------------------------

def _tsv(path):
    with open(path) as fh:
        lines = [ln.split('\t') for ln in fh.read().split('\n') if ln]
    return lines[0], lines[1:]


def _compare_tsv(a_path, b_path):
    """Every column but 'cluster' equal, 'cluster' equal as a pixel set; the
    row order equal outside groups of rows with identical sort keys (lexsort
    is stable, so ties follow input order, which differs): those groups are
    compared as multisets. Returns the number of rows in such groups."""
    ha, ra = _tsv(a_path)
    hb, rb = _tsv(b_path)
    assert ha == hb and len(ra) == len(rb)
    if not ra:
        return 0
    ci = ha.index('cluster')
    keys = [ha.index(k) for k in ('us_chrom', 'us_start', 'us_end',
                                  'ds_chrom', 'ds_start', 'ds_end')]

    def norm(r):
        return tuple(r[:ci]) + (frozenset(map(tuple, json.loads(r[ci]))),) \
            + tuple(r[ci + 1:])

    def groups(rows):
        out = []
        for r in rows:
            k = tuple(r[i] for i in keys)
            if out and out[-1][0] == k:
                out[-1][1].append(norm(r))
            else:
                out.append((k, [norm(r)]))
        return out
    ga, gb = groups(ra), groups(rb)
    assert [k for k, _ in ga] == [k for k, _ in gb]
    tied_a = sum(len(v) for _, v in ga if len(v) > 1)
    tied_b = sum(len(v) for _, v in gb if len(v) > 1)
    assert tied_a == tied_b
    for (k, va), (_, vb) in zip(ga, gb):
        if len(va) == 1:
            assert va == vb, k
        else:
            assert sorted(va, key=repr) == sorted(vb, key=repr), k
    return tied_a


def test_class_calls_gpu_equal_the_default_path():
    from test_calls import fill_outdir_from_golden
    fdrs, sizes = _small2_calls()
    host_dir = tempfile.mkdtemp(prefix='h3d_calls_host_')
    gpu_dir = tempfile.mkdtemp(prefix='h3d_calls_gpu_')
    try:
        hh = fill_outdir_from_golden('small2', host_dir)
        hg = fill_outdir_from_golden('small2', gpu_dir)
        before = set(os.listdir(gpu_dir))
        # the steps on their own, then collect for what is still missing
        hg.threshold(fdr=fdrs[0], cluster_size=sizes[0], gpu=True)
        hg.classify(fdr=fdrs[0], cluster_size=sizes[0], gpu=True)
        hg.collect(fdr=fdrs, cluster_size=sizes, gpu=True)
        hh.collect(fdr=fdrs, cluster_size=sizes)
        made = sorted(set(os.listdir(gpu_dir)) - before)
        assert made == sorted(set(os.listdir(host_dir)) - before)
        assert any(f.startswith('results_') for f in made)
        n_json = n_clusters = 0
        for fn in made:
            a, b = os.path.join(gpu_dir, fn), os.path.join(host_dir, fn)
            if fn.endswith('.json'):
                with open(a) as fh:
                    got = json.load(fh)
                with open(b) as fh:
                    want = json.load(fh)
                assert len(got) == len(want), fn
                assert {frozenset(map(tuple, c)) for c in got} == \
                    {frozenset(map(tuple, c)) for c in want}, fn
                # canonical: clusters by first pixel, pixels in order
                assert all(c == sorted(c) for c in got), fn
                assert [c[0] for c in got] == sorted(c[0] for c in got), fn
                n_json += 1
                n_clusters += len(got)
            elif fn.endswith('.tsv'):
                tied = _compare_tsv(a, b)
                print('%s: %d rows in groups of equal sort keys' % (fn, tied))
        assert n_json and n_clusters
    finally:
        shutil.rmtree(host_dir, ignore_errors=True)
        shutil.rmtree(gpu_dir, ignore_errors=True)
