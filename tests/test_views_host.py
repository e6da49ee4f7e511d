"""CPU checks of the dense views (get_matrix / select_matrix / APA): the
host-side window placement against the reference goldens (views.npz,
tests/golden/make_golden_views.py), the argument checks that must fire
before any device is touched, and the new ABI names."""
import numpy as np
import pytest
import scipy.sparse as sparse

from conftest import golden

from hic3defdr_amd import _native
from hic3defdr_amd import build as h3dbuild
from hic3defdr_amd.util.apa import apa_windows, make_apa_stack
from hic3defdr_amd.util.clusters import ClusterList, cluster_to_slices
from hic3defdr_amd.util.matrices import NAN_WINDOW, select_matrix

NEW_EXPORTS = ('h3d_window_gather', 'h3d_window_gather_dev',
               'h3d_stack_aggregate')


@pytest.fixture(scope='module')
def views():
    return golden('views.npz')


def golden_clusters(g):
    pts, starts = g['apa_points'], g['apa_starts']
    return [[tuple(int(v) for v in p) for p in pts[a:b]]
            for a, b in zip(starts[:-1], starts[1:])]


def test_cluster_to_slices_reference_doctest():
    assert cluster_to_slices([(4, 5), (3, 4), (3, 5), (3, 6)], width=5) == \
        (slice(1, 6, None), slice(3, 8, None))


@pytest.mark.parametrize('width', [5, 11])
def test_cluster_to_slices_matches_golden(views, width):
    ref = views['apa_slices_w%d' % width]
    for c, want in zip(golden_clusters(views), ref):
        rs, cs = cluster_to_slices(c, width=width)
        assert (rs.start, rs.stop, cs.start, cs.stop) == tuple(want)
        assert rs.step is None and cs.step is None


@pytest.mark.parametrize('width,min_dist,key', [
    (5, None, 'apa_stack_w5'), (11, None, 'apa_stack_w11'),
    (5, 3, 'apa_stack_w5_min3')])
def test_apa_windows_match_golden(views, width, min_dist, key):
    """Origins and validity of every cluster's window = the reference's:
    valid where its slice is not all NaN, placed where its cluster_to_slices
    starts."""
    clusters = golden_clusters(views)
    size = int(views['apa_size'])
    origins, valid = apa_windows(clusters, width, size, min_dist)
    ref_valid = ~np.isnan(views[key][:, 0, 0])
    np.testing.assert_array_equal(valid, ref_valid)
    sl = views['apa_slices_w%d' % width]
    np.testing.assert_array_equal(origins[valid], sl[valid][:, [0, 2]])
    assert (origins[~valid, 0] == NAN_WINDOW).all()
    assert origins.dtype == np.int32 and origins.shape == (len(clusters), 2)
    # the same from the array form of the clusters
    o2, v2 = apa_windows(ClusterList.from_sets(clusters), width, size,
                         min_dist)
    np.testing.assert_array_equal(o2, origins)
    np.testing.assert_array_equal(v2, valid)


def test_apa_window_validity_cases(views):
    """The golden's named cases: nearer the diagonal than min_dist, com[0] =
    1.5 < r, a window ending exactly at the last bin, a half-integer centre
    of mass; and the one deliberate deviation (com = size - r: NaN here)."""
    size = int(views['apa_size'])
    clusters = golden_clusters(views)
    assert clusters[:4] == [[(100, 103), (101, 104)], [(1, 20), (2, 21)],
                            [(250, 297)], [(20, 100), (21, 101)]]
    origins, valid = apa_windows(clusters[:4], 5, size)
    np.testing.assert_array_equal(valid, [False, False, True, True])
    assert tuple(origins[2]) == (248, 295) and origins[2, 1] + 5 == size
    assert tuple(origins[3]) == (18, 98)
    _, v = apa_windows([[(10, 38)], [(10, 37)], [(10, 39)]], 5, 40)
    np.testing.assert_array_equal(v, [False, True, False])
    o, v = apa_windows([], 5, size)
    assert o.shape == (0, 2) and v.shape == (0,)


def test_new_abi_names_exported():
    h3dbuild.build_native()
    lib = _native.load_library()
    for name in NEW_EXPORTS:
        assert name in _native.EXPORTS
        assert hasattr(lib, name), name
    for name in ('window_gather', 'window_gather_dev', 'stack_aggregate'):
        assert callable(getattr(_native.Context, name))


def test_no_device_raises_not_fakes(views):
    h3dbuild.build_native()
    if _native.load_library().h3d_device_count() > 0:
        pytest.skip('a GPU is visible')
    with pytest.raises(_native.H3DError):
        select_matrix(slice(0, 4), slice(0, 4), views['sel_row'],
                      views['sel_col'], views['sel_data'])
    m = sparse.coo_matrix((np.ones(2), ([3, 30], [30, 3])), shape=(60, 60))
    with pytest.raises(_native.H3DError):
        make_apa_stack(m, [[(3, 30)]], 5)


def test_select_matrix_refuses_bad_input(views):
    row, col, data = views['sel_row'], views['sel_col'], views['sel_data']
    rs, cs = slice(10, 20), slice(10, 20)
    perm = np.arange(len(row))
    perm[[3, 4]] = [4, 3]
    with pytest.raises(ValueError, match='sorted'):
        select_matrix(rs, cs, row[perm], col[perm], data[perm])
    with pytest.raises(ValueError, match='sorted'):   # a repeated pixel
        select_matrix(rs, cs, row[[0, 0, 1]], col[[0, 0, 1]], data[:3])
    k = np.flatnonzero(col > row)
    with pytest.raises(ValueError, match='row > col'):
        select_matrix(rs, cs, col[k], row[k], data[k])
    with pytest.raises(ValueError, match='integer start and stop'):
        select_matrix(slice(None, 20), cs, row, col, data)
    with pytest.raises(ValueError, match='integer start and stop'):
        select_matrix(rs, slice(10, None), row, col, data)
    with pytest.raises(ValueError, match='step'):
        select_matrix(slice(10, 20, 2), cs, row, col, data)
    with pytest.raises(ValueError, match='rep or cond'):
        select_matrix(rs, cs, row, col, np.stack([data, data], axis=1))


def test_make_apa_stack_refuses_even_width():
    m = sparse.coo_matrix((np.ones(1), ([3], [30])), shape=(60, 60))
    for width in (4, 0, 10):
        with pytest.raises(ValueError, match='odd'):
            make_apa_stack(m, [[(3, 30)]], width)
    with pytest.raises(ValueError, match='odd'):
        apa_windows([[(3, 30)]], 6, 60)


def test_class_surface_present():
    from hic3defdr_amd import HiC3DeFDR
    for name in ('get_matrix', 'apa_stack', 'apa_mean'):
        assert callable(getattr(HiC3DeFDR, name))
