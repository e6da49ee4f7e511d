"""The yardstick and the cases of the connected-component calls
(csrc/h3d_ccl.h, csrc/h3d_clusters.hip; tests/test_clusters_ccl_host.py on
the CPU, tests/test_gpu_clusters.py on the GPU).

The yardstick is scipy.ndimage.label with generate_binary_structure(2,
connectivity) on the dense matrix of each class, the components renumbered by
their first member in (row, col) order. A case is (row, col, cls): int64
pixels in strictly increasing (row, col) order inside an upper band, and a
class byte per pixel (255 = no pixel)."""
import ctypes

import numpy as np

ABSENT = 255
BAND = 40
N_LIST = (0, 1, 63, 64, 65, 257, 4097)


# -- the restatement ----------------------------------------------------------

def canonical(raw):
    """Component ids (any integers, -1 = none) -> int32 labels numbered by
    first occurrence, and their count."""
    raw = np.asarray(raw)
    label = np.full(len(raw), -1, dtype=np.int32)
    present = np.flatnonzero(raw >= 0)
    if not len(present):
        return label, 0
    uniq, first = np.unique(raw[present], return_index=True)
    rank = np.empty(len(uniq), dtype=np.int32)
    rank[np.argsort(first, kind='stable')] = np.arange(len(uniq),
                                                       dtype=np.int32)
    label[present] = rank[np.searchsorted(uniq, raw[present])]
    return label, len(uniq)


def labels_ref(row, col, cls, connectivity):
    """(label int32 (n), n_clusters): scipy.ndimage.label per class."""
    from scipy import ndimage
    row, col, cls = np.asarray(row), np.asarray(col), np.asarray(cls)
    raw = np.full(len(row), -1, dtype=np.int64)
    if len(row):
        r0, c0 = row.min(), col.min()
        shape = (int(row.max() - r0) + 1, int(col.max() - c0) + 1)
        struct = ndimage.generate_binary_structure(2, connectivity)
        offset = 0
        for k in np.unique(cls[cls != ABSENT]):
            sel = np.flatnonzero(cls == k)
            dense = np.zeros(shape, dtype=bool)
            dense[row[sel] - r0, col[sel] - c0] = True
            lab, m = ndimage.label(dense, structure=struct)
            raw[sel] = lab[row[sel] - r0, col[sel] - c0] - 1 + offset
            offset += m
    return canonical(raw)


def lists_ref(label, n_clusters, row, col, cls, min_size=1):
    """The arrays of h3d_cluster_lists from labels, in numpy."""
    label = np.asarray(label)
    idx = np.flatnonzero(label >= 0)
    lab = label[idx]
    size = np.bincount(lab, minlength=n_clusters).astype(np.int32)
    first = np.full(n_clusters, len(label), dtype=np.int64)
    np.minimum.at(first, lab, idx)
    bounds = np.empty((4, n_clusters), dtype=np.int32)
    bounds[0::2] = np.iinfo(np.int32).max
    bounds[1::2] = -1
    np.minimum.at(bounds[0], lab, row[idx])
    np.maximum.at(bounds[1], lab, row[idx])
    np.minimum.at(bounds[2], lab, col[idx])
    np.maximum.at(bounds[3], lab, col[idx])
    keep = size >= max(min_size, 1)
    kept = idx[keep[lab]]
    members = kept[np.argsort(label[kept], kind='stable')].astype(np.int32)
    starts = np.concatenate([[0], np.cumsum(size[keep])]).astype(np.int64)
    return dict(size=size, cls_of=np.asarray(cls)[first].astype(np.uint8),
                bounds=bounds, members=members, starts=starts)


def list_labels(cl, n):
    """A ClusterList over n pixels (members index them) -> canonical labels."""
    raw = np.full(n, -1, dtype=np.int64)
    raw[cl.members] = np.repeat(np.arange(len(cl)), cl.sizes())
    return canonical(raw)


def frozen(cl):
    """A ClusterList as a set of frozensets of (row, col)."""
    return {frozenset(s) for s in cl.to_sets()}


def assert_canonical(cl):
    """Clusters by first pixel, pixels in (row, col) order."""
    r, c = cl.pixels()
    key = r * 2 ** 32 + c
    firsts = []
    for a, b in zip(cl.starts[:-1], cl.starts[1:]):
        assert b > a
        assert np.all(np.diff(key[a:b]) > 0)
        firsts.append(key[a])
    assert np.all(np.diff(firsts) > 0)


# -- the host twin ------------------------------------------------------------

_host = []


def host_lib():
    if not _host:
        from hic3defdr_amd import build as h3dbuild
        _host.append(ctypes.CDLL(h3dbuild.build_hosttest()))
    return _host[0]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def twin_labels(row, col, cls, connectivity):
    """(label, n_clusters, rc) of h3dt_ccl_labels (libh3d_hosttest.so)."""
    lib = host_lib()
    row = np.ascontiguousarray(row, dtype=np.int64)
    col = np.ascontiguousarray(col, dtype=np.int64)
    cls = np.ascontiguousarray(cls, dtype=np.uint8)
    label = np.full(len(row), -7, dtype=np.int32)
    nc = ctypes.c_int64(-7)
    lib.h3dt_ccl_labels.restype = ctypes.c_int
    rc = lib.h3dt_ccl_labels(_p(row), _p(col), _p(cls),
                             ctypes.c_int64(len(row)),
                             ctypes.c_int(connectivity), _p(label),
                             ctypes.byref(nc))
    return label, nc.value, rc


# -- cases --------------------------------------------------------------------

def band_pixels(bins, band):
    """Every pixel of the upper band 0 <= col - row < band, col < bins, in
    (row, col) order."""
    r = np.repeat(np.arange(bins, dtype=np.int64), band)
    c = r + np.tile(np.arange(band, dtype=np.int64), bins)
    ok = c < bins
    return r[ok], c[ok]


def random_band(n, seed, band=BAND, classes=1, absent=0.):
    """n pixels drawn from a band about 1.6 n pixels large; the class bytes
    uniform over ``classes``, a fraction ``absent`` of them 255."""
    rng = np.random.default_rng([seed, n, classes])
    bins = band
    while True:
        row, col = band_pixels(bins, band)
        if len(row) >= 1.6 * n:
            break
        bins += 1 + bins // 8
    pick = np.sort(rng.choice(len(row), size=n, replace=False))
    cls = rng.integers(0, classes, n).astype(np.uint8)
    cls[rng.random(n) < absent] = ABSENT
    return row[pick], col[pick], cls


def full_band(bins=30, band=12):
    """Every run ends at the band edge, where the pixel above does not
    exist; one component."""
    row, col = band_pixels(bins, band)
    return row, col, np.zeros(len(row), dtype=np.uint8)


def rows_missing(seed=5):
    """A random set without the rows 3, 4, 9, 10, 15, ...: nothing links
    across a missing row."""
    row, col, cls = random_band(600, seed, classes=2, absent=0.1)
    ok = (row % 6 != 3) & (row % 6 != 4)
    return row[ok], col[ok], cls[ok]


def checkerboard(bins=40, band=16):
    """All singletons at connectivity 1, one component at connectivity 2."""
    row, col = band_pixels(bins, band)
    ok = (row + col) % 2 == 0
    return row[ok], col[ok], np.zeros(int(ok.sum()), dtype=np.uint8)


def stripes(n=None, band=BAND, classes=2):
    """Vertical class stripes over a full band: every run has length 1 and
    every component is a column segment. ``n``: the first n pixels."""
    bins = band if n is None else n // band + band + 1
    row, col = band_pixels(bins, band)
    if n is not None:
        row, col = row[:n], col[:n]
    return row, col, (col % classes).astype(np.uint8)


def serpentine(connectors=True, bins=300, band=64):
    """Even rows full, odd rows one connector pixel, alternately at column
    r + 1 and r + 63: about 10 k pixels. At connectivity 2 it is one
    component of maximal diameter; at connectivity 1 the r + 63 connectors
    touch only the row below (the band's edge: (r - 1, r + 63) is outside
    it), so a component is two full rows and their connectors. With the connectors
    absent (class 255) every full row is a component: 150 of them."""
    rows, cols, cls = [], [], []
    for r in range(bins):
        if r % 2 == 0:
            c = np.arange(r, r + band)
            k = np.zeros(band, dtype=np.uint8)
        else:
            c = np.array([r + 1 if r % 4 == 1 else r + band - 1])
            k = np.array([0 if connectors else ABSENT], dtype=np.uint8)
        rows.append(np.full(len(c), r))
        cols.append(c)
        cls.append(k)
    return (np.concatenate(rows).astype(np.int64),
            np.concatenate(cols).astype(np.int64), np.concatenate(cls))


STRUCTURED = {
    'full_band': full_band,
    'rows_missing': rows_missing,
    'checkerboard': checkerboard,
    'stripes': stripes,
    'stripes3': lambda: stripes(classes=3),
    'serpentine': serpentine,
    'serpentine_cut': lambda: serpentine(connectors=False),
}


def random_cases():
    """The random banded sets: 1, 2 and 3 classes, with and without absent
    pixels, at the sizes of N_LIST."""
    for n in N_LIST:
        for classes, absent in ((1, 0.), (2, 0.), (2, 0.2), (3, 0.1)):
            yield ('n%d_c%d_a%g' % (n, classes, absent),
                   random_band(n, 11, classes=classes, absent=absent))
