"""CPU checks behind the connected-component calls (csrc/h3d_ccl.h,
csrc/h3d_clusters.hip): the scipy.ndimage.label restatement
(tests/cluster_cases.py) against the host ClusterList.find partition; the
host twin h3dt_ccl_labels -- the device's run predicates and link enumeration
under a serial union-find -- against the restatement, label for label; the
class bytes against numpy; the signatures and the rejections of the new
functions, which happen before a device is touched."""
import ctypes
import inspect

import numpy as np
import pytest

import cluster_cases as cc


def test_restatement_equals_host_find_partition():
    """790 random banded pixel sets, connectivity 1 and 2: the clusters of
    the DirectedDisjointSet replay are the connected components."""
    from hic3defdr_amd.util.clusters import ClusterList
    rng = np.random.default_rng(790)
    multi = 0
    for t in range(790):
        n = int(rng.integers(1, 400))
        row, col, cls = cc.random_band(n, t, band=int(rng.integers(2, 30)))
        conn = 1 + t % 2
        want, nc = cc.labels_ref(row, col, cls, conn)
        cl = ClusterList.find(row, col, conn)
        got, gc = cc.list_labels(cl, n)
        assert gc == nc == len(cl), (t, n, conn)
        np.testing.assert_array_equal(got, want, err_msg='case %d' % t)
        multi += nc > 1
    assert multi > 700


def _check_twin(row, col, cls, what):
    for conn in (1, 2):
        want, nc = cc.labels_ref(row, col, cls, conn)
        got, gc, rc = cc.twin_labels(row, col, cls, conn)
        assert rc == 0, what
        assert gc == nc, (what, conn)
        np.testing.assert_array_equal(got, want,
                                      err_msg='%s conn %d' % (what, conn))
    return nc


def test_twin_equals_restatement_on_random_sets():
    seen = 0
    for name, (row, col, cls) in cc.random_cases():
        _check_twin(row, col, cls, name)
        seen += 1
    assert seen == 4 * len(cc.N_LIST)
    rng = np.random.default_rng(3)
    for t in range(300):
        n = int(rng.integers(1, 500))
        row, col, cls = cc.random_band(
            n, 1000 + t, band=int(rng.integers(2, 30)),
            classes=1 + t % 3, absent=(0., 0.15)[t % 2])
        _check_twin(row, col, cls, 'random %d' % t)


@pytest.mark.parametrize('name', sorted(cc.STRUCTURED))
def test_twin_equals_restatement_on_structured_cases(name):
    row, col, cls = cc.STRUCTURED[name]()
    _check_twin(row, col, cls, name)


def test_structured_cases_are_what_they_say():
    row, col, cls = cc.checkerboard()
    assert cc.labels_ref(row, col, cls, 1)[1] == len(row)
    assert cc.labels_ref(row, col, cls, 2)[1] == 1
    row, col, cls = cc.full_band()
    assert cc.labels_ref(row, col, cls, 1)[1] == 1
    row, col, cls = cc.stripes(4097)
    assert len(row) == 4097
    # every run has length 1: no two neighbours in a row share a class
    assert np.all((np.diff(col) != 1) | (np.diff(cls.astype(int)) != 0))
    row, col, cls = cc.serpentine()
    assert 9000 < len(row) < 11000
    assert cc.labels_ref(row, col, cls, 2)[1] == 1
    # connectivity 1: each of the 75 connectors at r + 63 (r = 3, 7, .. 299)
    # touches only the row below and so starts a component; rows 0-2 are one
    assert cc.labels_ref(row, col, cls, 1)[1] == 76
    row, col, cls = cc.serpentine(connectors=False)
    assert cc.labels_ref(row, col, cls, 1)[1] == 150
    assert cc.labels_ref(row, col, cls, 2)[1] == 150


def test_twin_edge_sizes_and_all_absent():
    z = np.zeros(0, dtype=np.int64)
    label, nc, rc = cc.twin_labels(z, z, z.astype(np.uint8), 1)
    assert (rc, nc, len(label)) == (0, 0, 0)
    one = np.array([5], dtype=np.int64)
    label, nc, rc = cc.twin_labels(one, one, np.zeros(1, np.uint8), 2)
    assert (rc, nc, label.tolist()) == (0, 1, [0])
    label, nc, rc = cc.twin_labels(one, one, np.full(1, 255, np.uint8), 2)
    assert (rc, nc, label.tolist()) == (0, 0, [-1])
    row, col, cls = cc.random_band(257, 2)
    label, nc, rc = cc.twin_labels(row, col, np.full(257, 255, np.uint8), 1)
    assert (rc, nc) == (0, 0) and np.all(label == -1)
    # the largest coordinates: the widened span stays inside the key's low word
    top = 2 ** 31 - 1
    row = np.array([top - 1, top - 1, top, top], dtype=np.int64)
    col = np.array([top - 1, top, top - 1, top], dtype=np.int64)
    label, nc, rc = cc.twin_labels(row, col, np.array([0, 1, 1, 0], np.uint8),
                                   2)
    assert (rc, nc, label.tolist()) == (0, 2, [0, 1, 1, 0])


@pytest.mark.parametrize('what', ['unsorted', 'repeat', 'negative', 'wide',
                                  'col_back'])
def test_twin_flags_a_broken_input_rule(what):
    row = np.array([0, 0, 1, 2, 2], dtype=np.int64)
    col = np.array([0, 1, 1, 2, 5], dtype=np.int64)
    if what == 'unsorted':
        row[2], row[3] = 2, 1
    elif what == 'repeat':
        col[1] = 0
    elif what == 'negative':
        row[0] = -1
    elif what == 'wide':
        col[4] = 2 ** 31
    else:
        col[4] = 1
    label, nc, rc = cc.twin_labels(row, col, np.zeros(5, np.uint8), 1)
    assert rc == 16 and nc == 0 and np.all(label == -1)
    assert cc.twin_labels(row[:1] * 0, col[:1] * 0, np.zeros(1, np.uint8),
                          3)[2] == -1


def test_class_bytes_equal_numpy():
    lib = cc.host_lib()
    rng = np.random.default_rng(8)
    n, C = 3000, 5
    value = np.round(rng.random((n, C)), 1)            # ties
    value[rng.random((n, C)) < 0.1] = np.nan           # NaNs, often several
    value[:4] = [[np.nan] * C, [1.] * C, [-np.inf] * C,
                 [0., np.inf, np.inf, np.nan, np.nan]]
    member = (rng.random(n) < 0.8).astype(np.uint8)
    member[:4] = 1
    cls = np.zeros(n, dtype=np.uint8)
    lib.h3dt_argmax_class(ctypes.c_int64(n), ctypes.c_int(C), cc._p(value),
                          cc._p(member), cc._p(cls))
    want = np.where(member != 0, np.argmax(value, axis=1), 255)
    np.testing.assert_array_equal(cls, want)
    assert len(np.unique(cls)) == C + 1
    one = np.ascontiguousarray(value[:, :1])
    lib.h3dt_argmax_class(ctypes.c_int64(n), ctypes.c_int(1), cc._p(one),
                          cc._p(member), cc._p(cls))
    np.testing.assert_array_equal(cls, np.where(member != 0, 0, 255))
    q = rng.random(n)
    q[::7] = np.nan
    q[1], q[2] = 0.05, np.nextafter(0.05, 0)
    lib.h3dt_q_class(ctypes.c_int64(n), cc._p(q), ctypes.c_double(0.05),
                     cc._p(cls))
    want = np.where(q < 0.05, 0, np.where(q >= 0.05, 1, 255))
    np.testing.assert_array_equal(cls, want)
    assert cls[1] == 1 and cls[2] == 0 and cls[7] == 255


def test_signatures():
    from hic3defdr_amd import HiC3DeFDR, _native
    from hic3defdr_amd.util import classification, clusters, thresholding

    def params(fn):
        return list(inspect.signature(fn).parameters)
    assert params(clusters.ClusterList.find_gpu) == ['row', 'col',
                                                     'connectivity']
    assert params(clusters.find_clusters_gpu)[:1] == ['sig_points']
    assert params(thresholding.threshold_clusters_gpu)[:4] == [
        'qvalues', 'row', 'col', 'fdr']
    assert params(classification.classify_clusters_gpu)[:4] == [
        'row', 'col', 'value', 'clusters']
    for fn in (HiC3DeFDR.threshold, HiC3DeFDR.classify, HiC3DeFDR.collect):
        p = inspect.signature(fn).parameters
        assert p['gpu'].default is False, fn
    for name in ('h3d_label_components', 'h3d_label_components_dev',
                 'h3d_threshold_classes_dev', 'h3d_argmax_classes_dev',
                 'h3d_cluster_lists', 'h3d_cluster_lists_dev'):
        assert name in _native.EXPORTS
    for name in ('label_components', 'label_components_dev',
                 'threshold_classes_dev', 'argmax_classes_dev',
                 'cluster_lists', 'cluster_lists_dev'):
        assert callable(getattr(_native.Context, name))


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a context fails the test."""
    from hic3defdr_amd import _native

    def boom(*a, **k):
        raise AssertionError('a device was touched')
    monkeypatch.setattr(_native, 'context', boom)


def _good():
    return (np.array([0, 0, 1, 2], dtype=np.int64),
            np.array([0, 1, 1, 5], dtype=np.int64))


BROKEN = {
    'unsorted': lambda r, c: (r[[0, 1, 3, 2]], c[[0, 1, 3, 2]]),
    'repeat': lambda r, c: (r[[0, 1, 1, 2, 3]], c[[0, 1, 1, 2, 3]]),
    'negative': lambda r, c: (r - 1, c),
    'wide': lambda r, c: (r, np.where(c == 5, 2 ** 31, c)),
    'length': lambda r, c: (r, c[:-1]),
    'two_d': lambda r, c: (r.reshape(2, 2), c.reshape(2, 2)),
}


@pytest.mark.parametrize('what', sorted(BROKEN))
def test_rejections_before_a_device_is_touched(no_device, what):
    from hic3defdr_amd.util.classification import classify_clusters_gpu
    from hic3defdr_amd.util.clusters import ClusterList
    from hic3defdr_amd.util.thresholding import threshold_clusters_gpu
    row, col = BROKEN[what](*_good())
    n = len(row)
    with pytest.raises(ValueError):
        ClusterList.find_gpu(row, col)
    with pytest.raises(ValueError):
        threshold_clusters_gpu(np.zeros(n), row, col, 0.05)
    with pytest.raises(ValueError):
        classify_clusters_gpu(row, col, np.zeros((n, 2)), [{(0, 0)}])


def test_more_rejections_before_a_device_is_touched(no_device):
    import scipy.sparse as sparse
    from hic3defdr_amd.util.classification import classify_clusters_gpu
    from hic3defdr_amd.util.clusters import ClusterList, find_clusters_gpu
    from hic3defdr_amd.util.thresholding import threshold_clusters_gpu
    row, col = _good()
    for conn in (0, 3, True, 1.5):
        with pytest.raises(ValueError):
            ClusterList.find_gpu(row, col, connectivity=conn)
        with pytest.raises(ValueError):
            find_clusters_gpu(sparse.eye(3, dtype=bool), connectivity=conn)
    with pytest.raises(TypeError):
        ClusterList.find_gpu(row.astype(float), col)
    with pytest.raises(ValueError):                      # q of another length
        threshold_clusters_gpu(np.zeros(3), row, col, 0.05)
    with pytest.raises(TypeError):
        threshold_clusters_gpu(np.zeros(4, dtype=np.int64), row, col, 0.05)
    with pytest.raises(ValueError):
        threshold_clusters_gpu(np.zeros(4), row, col, 0.05, cluster_size=[])
    with pytest.raises(ValueError):                      # value of another length
        classify_clusters_gpu(row, col, np.zeros((3, 2)), [{(0, 0)}])
    with pytest.raises(ValueError):                      # value not (n, C)
        classify_clusters_gpu(row, col, np.zeros(4), [{(0, 0)}])
    with pytest.raises(ValueError, match='254'):         # C > 254
        classify_clusters_gpu(row, col, np.zeros((4, 255)), [{(0, 0)}])
    with pytest.raises(ValueError):                      # C = 0
        classify_clusters_gpu(row, col, np.zeros((4, 0)), [{(0, 0)}])
    # nothing to do is no device work either
    z = np.zeros(0, dtype=np.int64)
    assert len(ClusterList.find_gpu(z, z)) == 0
    sig, insig = threshold_clusters_gpu(np.zeros(0), z, z, 0.05)
    assert len(sig) == 0 and len(insig) == 0
    assert [len(p) for p in threshold_clusters_gpu(np.zeros(0), z, z,
                                                   [0.01, 0.05])] == [2, 2]
    assert [len(c) for c in classify_clusters_gpu(
        row, col, np.zeros((4, 3)), [])] == [0, 0, 0]


def test_cluster_list_carries_bounds():
    from hic3defdr_amd.util.clusters import ClusterList
    row = np.array([0, 0, 3, 4, 4], dtype=np.int64)
    col = np.array([1, 2, 7, 7, 9], dtype=np.int64)
    plain = ClusterList(row, col, np.arange(5), [0, 2, 4, 5])
    want = [a.tolist() for a in plain.bounds()]
    assert want == [[0, 3, 4], [0, 4, 4], [1, 7, 9], [2, 7, 9]]
    carried = ClusterList(row, col, np.arange(5), [0, 2, 4, 5], bounds=want)
    assert [a.tolist() for a in carried.bounds()] == want
    keep = np.array([True, False, True])
    assert [a.tolist() for a in carried.select(keep).bounds()] == \
        [a.tolist() for a in plain.select(keep).bounds()]
    assert [a.tolist() for a in carried.size_filter(2).bounds()] == \
        [a.tolist() for a in plain.size_filter(2).bounds()]
