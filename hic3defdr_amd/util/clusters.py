"""Clusters of pixels (reference hic3defdr/util/clusters.py).

Two forms:

- the reference's: a list of sets of ``(i, j)`` tuples (``find_clusters``,
  ``load_clusters``, ``save_clusters`` keep that API);
- ``ClusterList``: the same clusters as arrays (pixel coordinates, a member
  permutation and cluster start offsets), which the pipeline steps use so a
  chromosome with millions of thresholded pixels never becomes millions of
  Python tuples. Cluster numbering follows the reference's group order, and
  within a cluster the pixels come in the iteration order of the reference's
  Python set (h3d_find_clusters_ordered replays CPython's set table over the
  DirectedDisjointSet's adds and merges), so the JSON / TSV text is the
  reference's byte for byte.

Clustering itself is ``h3d_find_clusters`` in libh3d (host C++ restatement of
the DirectedDisjointSet, clusters.py:15-97).

``ClusterList.find_gpu`` / ``find_clusters_gpu`` give the same clusters as
sets of pixels from the GPU (h3d_label_components, a run-based connected-
component labelling) in a canonical order instead of the reference's:
clusters by their first pixel in (row, col) order, pixels inside a cluster in
(row, col) order (deviation 10).
"""
import json
import re

import numpy as np

from hic3defdr_amd import _native


class ClusterList(object):
    """Cluster k = pixels ``(row[m], col[m])`` for
    ``m in members[starts[k]:starts[k + 1]]``."""

    def __init__(self, row, col, members, starts, bounds=None):
        self.row = np.asarray(row, dtype=np.int64)
        self.col = np.asarray(col, dtype=np.int64)
        self.members = np.asarray(members, dtype=np.int64)
        self.starts = np.asarray(starts, dtype=np.int64)
        # (4, len(self)) min row, max row, min col, max col when the clusters
        # came with them (find_gpu computes them on the device), else None
        self._bounds = None if bounds is None else \
            np.asarray(bounds, dtype=np.int64).reshape(4, len(self.starts) - 1)

    @classmethod
    def empty(cls):
        z = np.zeros(0, dtype=np.int64)
        return cls(z, z, z, np.zeros(1, dtype=np.int64))

    @classmethod
    def from_labels(cls, row, col, labels, n_clusters):
        """Group pixels by label (stable: input order inside a cluster)."""
        members = np.argsort(labels, kind='stable')
        counts = np.bincount(labels, minlength=n_clusters)
        starts = np.zeros(n_clusters + 1, dtype=np.int64)
        np.cumsum(counts, out=starts[1:])
        return cls(row, col, members, starts)

    @classmethod
    def find(cls, row, col, connectivity=1):
        """Clusters of the pixel list (row, col) in the reference's order
        (``find_clusters`` on the COO of these pixels)."""
        row = np.asarray(row, dtype=np.int64)
        col = np.asarray(col, dtype=np.int64)
        if len(row) == 0:
            return cls.empty()
        try:
            lab, nc, order = _native.cluster_order(row, col, connectivity)
        except _native.H3DError:
            # repeated pixels (a COO with duplicates): the sets' order is not
            # defined by the pixel list; input order inside each cluster
            lab, nc = _native.cluster_labels(row, col, connectivity)
            return cls.from_labels(row, col, lab, nc)
        counts = np.bincount(lab, minlength=nc)
        starts = np.zeros(nc + 1, dtype=np.int64)
        np.cumsum(counts, out=starts[1:])
        return cls(row, col, order, starts)

    @classmethod
    def find_gpu(cls, row, col, connectivity=1):
        """The clusters of ``find`` as sets of pixels, labelled on the GPU
        (h3d_label_components), in canonical order: clusters by their first
        pixel, pixels in (row, col) order. The pixels must be distinct, in
        (row, col) order, with coordinates in [0, 2^31) (ValueError
        otherwise, before a device is touched). There is no CPU fallback."""
        row, col = check_pixels(row, col, connectivity)
        if len(row) == 0:
            return cls.empty()
        return components_gpu(row, col, np.zeros(len(row), dtype=np.uint8),
                              1, connectivity=connectivity)[0]

    @classmethod
    def from_sets(cls, clusters):
        """From the reference form (list of iterables of (i, j))."""
        rows, cols, sizes = [], [], []
        for c in clusters:
            c = list(c)
            sizes.append(len(c))
            for i, j in c:
                rows.append(int(i))
                cols.append(int(j))
        starts = np.zeros(len(sizes) + 1, dtype=np.int64)
        np.cumsum(sizes, out=starts[1:])
        return cls(np.array(rows, dtype=np.int64),
                   np.array(cols, dtype=np.int64),
                   np.arange(len(rows), dtype=np.int64), starts)

    def __len__(self):
        return len(self.starts) - 1

    def sizes(self):
        return np.diff(self.starts)

    def select(self, keep):
        """Sub-list of the clusters where ``keep`` (bool per cluster)."""
        keep = np.asarray(keep, dtype=bool)
        sz = self.sizes()[keep]
        idx = np.repeat(keep, self.sizes())
        starts = np.zeros(len(sz) + 1, dtype=np.int64)
        np.cumsum(sz, out=starts[1:])
        return ClusterList(self.row, self.col, self.members[idx], starts,
                           None if self._bounds is None
                           else self._bounds[:, keep])

    def size_filter(self, cluster_size):
        """thresholding.py:44-61: keep clusters with >= cluster_size pixels."""
        return self.select(self.sizes() >= cluster_size)

    def pixels(self):
        """(row, col) of all member pixels, cluster by cluster."""
        return self.row[self.members], self.col[self.members]

    def bounds(self):
        """Per-cluster (min row, max row, min col, max col)."""
        if not len(self):
            z = np.zeros(0, dtype=np.int64)
            return z, z, z, z
        if self._bounds is not None:
            return tuple(self._bounds)
        r, c = self.pixels()
        s = self.starts[:-1]
        return (np.minimum.reduceat(r, s), np.maximum.reduceat(r, s),
                np.minimum.reduceat(c, s), np.maximum.reduceat(c, s))

    def texts(self):
        """Per-cluster text ``[[i, j], [i, j]]`` as a list of str."""
        if not len(self):
            return []
        buf, ends = _native.format_clusters(self.row, self.col, self.members,
                                            self.starts)
        b = np.concatenate([[0], ends])
        s = buf.decode('ascii')
        return [s[b[k]:b[k + 1]] for k in range(len(self))]

    def json_text(self):
        """save_clusters text (clusters.py:129-130, json.dump defaults)."""
        if not len(self):
            return '[]'
        buf, _ = _native.format_clusters(self.row, self.col, self.members,
                                         self.starts)
        # clusters are adjacent "[...]" blocks: join them with ", "
        return '[' + buf.decode('ascii').replace(']][[', ']], [[') + ']'

    def to_sets(self):
        r, c = self.pixels()
        return [set(zip(r[a:b].tolist(), c[a:b].tolist()))
                for a, b in zip(self.starts[:-1], self.starts[1:])]


def find_clusters(sig_points, connectivity=1):
    """Reference ``clusters.py:73-97``: clusters of the True entries of a
    boolean matrix (scipy sparse or dense), as a list of sets of tuples."""
    import scipy.sparse as sparse
    m = sparse.coo_matrix(sig_points)
    return ClusterList.find(m.row, m.col, connectivity).to_sets()


def check_pixels(row, col, connectivity=1):
    """The input rule of the GPU labelling, checked on the host before a
    device is touched: integer (n,) arrays of one length, n <= 2^31 - 2,
    coordinates in [0, 2^31), strictly increasing in (row, col) order (so
    distinct); connectivity 1 or 2. Returns (row, col) as int64."""
    row, col = np.asarray(row), np.asarray(col)
    for a, what in ((row, 'row'), (col, 'col')):
        if a.dtype.kind not in 'iu':
            raise TypeError('%s must be integers, not %s' % (what, a.dtype))
        if a.ndim != 1:
            raise ValueError('%s must have 1 dimension' % what)
    if row.shape != col.shape:
        raise ValueError('row and col must have one length')
    if isinstance(connectivity, bool) or connectivity not in (1, 2):
        raise ValueError('connectivity must be 1 or 2, got %r'
                         % (connectivity,))
    if len(row) > _native.CCL_MAX_N:
        raise ValueError('at most 2^31 - 2 pixels')
    if len(row):
        if min(row.min(), col.min()) < 0 or \
                max(row.max(), col.max()) >= 2 ** 31:
            raise ValueError(_native.BAD_PIXELS)
        dr = row[1:] > row[:-1]
        same = row[1:] == row[:-1]
        if not np.all(dr | (same & (col[1:] > col[:-1]))):
            raise ValueError(_native.BAD_PIXELS)
    return row.astype(np.int64, copy=False), col.astype(np.int64, copy=False)


def components_dev(ctx, row, col, t_row, t_col, t_cls, n_classes,
                   connectivity=1, min_size=1):
    """One ``ClusterList`` per class 0 .. n_classes - 1 from the device:
    ``t_row`` / ``t_col`` (int64) and the class bytes ``t_cls`` (uint8, 255 =
    no pixel) are torch tensors of ``ctx``'s device holding the host pixels
    ``row`` / ``col``. Clusters below ``min_size`` pixels are not listed. The
    lists share ``row`` / ``col`` and carry the device's bounding boxes."""
    label, nc = ctx.label_components_dev(t_row, t_col, t_cls, connectivity)
    out = ctx.cluster_lists_dev(label, t_cls, t_row, t_col, nc, min_size)
    kept = out['size'].cpu().numpy() >= max(int(min_size), 1)
    cls_of = out['cls_of'].cpu().numpy()[kept]
    whole = ClusterList(row, col, out['members'].cpu().numpy(),
                        out['starts'].cpu().numpy(),
                        out['bounds'].cpu().numpy()[:, kept])
    return [whole.select(cls_of == k) for k in range(n_classes)]


def components_gpu(row, col, cls, n_classes, connectivity=1, min_size=1,
                   ctx=None):
    """``components_dev`` for host arrays (checked by ``check_pixels``)."""
    import torch
    ctx = ctx or _native.context()
    dev = torch.device('cuda', ctx.device)
    t_row = torch.from_numpy(np.ascontiguousarray(row)).to(dev)
    t_col = torch.from_numpy(np.ascontiguousarray(col)).to(dev)
    t_cls = torch.from_numpy(np.ascontiguousarray(cls, dtype=np.uint8)).to(dev)
    return components_dev(ctx, row, col, t_row, t_col, t_cls, n_classes,
                          connectivity, min_size)


def find_clusters_gpu(sig_points, connectivity=1):
    """``find_clusters`` on the GPU: a boolean matrix (scipy sparse or
    dense) -> the canonical CSR pixel order -> ``ClusterList.find_gpu``; a
    list of sets of tuples, clusters ordered by their first pixel."""
    import scipy.sparse as sparse
    m = sparse.csr_matrix(sig_points, dtype=bool)
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    m = m.tocoo()
    return ClusterList.find_gpu(m.row.astype(np.int64),
                                m.col.astype(np.int64),
                                connectivity).to_sets()


def cluster_pixels(clusters):
    """(prow, pcol, starts) of ``clusters`` -- a ``ClusterList`` or a list of
    pixel lists -- in list order, repeats kept."""
    if isinstance(clusters, ClusterList):
        prow, pcol = clusters.pixels()
        return prow, pcol, clusters.starts
    sizes = np.fromiter((len(c) for c in clusters), dtype=np.int64,
                        count=len(clusters))
    starts = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=starts[1:])
    pix = np.array([p for c in clusters for p in c])
    if pix.size == 0:
        pix = np.zeros((0, 2), dtype=np.int64)
    if pix.ndim != 2 or pix.shape[1] != 2:
        raise ValueError('a cluster is a list of (row, col) pixels')
    return pix[:, 0], pix[:, 1], starts


def cluster_text_pixels(texts):
    """(prow, pcol, starts) of the ``cluster`` cells of a cluster table
    (``[[i, j], [i, j]]`` per row, the text ``ClusterTable.read_tsv`` keeps),
    parsed by numpy's text reader over all rows at once."""
    sizes = np.array([t.count('[') - 1 for t in texts], dtype=np.int64)
    starts = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=starts[1:])
    body = ' '.join(texts).encode('ascii').translate(_PIXEL_TEXT) \
        .replace(b',', b' ').strip()
    pix = np.fromstring(body.decode('ascii'), dtype=np.int64, sep=' ') \
        if body else np.zeros(0, dtype=np.int64)
    if len(pix) != 2 * starts[-1]:
        raise ValueError('a cluster cell is not a list of [row, col] pairs')
    pix = pix.reshape(-1, 2)
    return pix[:, 0], pix[:, 1], starts


def cluster_stats_gpu(clusters, row, col, data, reducers=('mean',), ctx=None,
                      sorted=False):
    """The sparse table ``(row, col, data)`` evaluated at the pixels of every
    cluster and reduced per cluster (reference ``cluster_table.py:298-332``'s
    arithmetic, h3d_cluster_stats): a pixel the table lacks counts as 0.0, a
    pixel listed twice counts twice, 'mean' divides by the number of listed
    pixels, 'max' / 'min' are NaN where a value is. ``clusters`` is a
    ``ClusterList`` or a list of pixel lists; ``data`` is (n,) or (n, K).
    Returns a dict from each of ``reducers`` to a (k, K) float64 array, plus
    'found' (k,): how many of a cluster's pixels the table holds. The table
    may come in any order (``sorted=True`` promises strictly increasing
    (row, col) and saves the sort); a repeated table pixel, an empty cluster
    or a negative cluster coordinate is a ValueError, a cluster pixel beyond
    the table's shape an IndexError. There is no CPU fallback;
    the arguments are checked before a device is touched."""
    reducers, _ = _native.cstat_want(reducers)
    prow, pcol, starts = cluster_pixels(clusters)
    args = _native.check_cluster_stats(row, col, data, prow, pcol, starts)
    if len(starts) == 1:
        K = args[2].shape[1]
        out = {r: np.zeros((0, K)) for r in reducers}
        out['found'] = np.zeros(0, dtype=np.int32)
        return out
    ctx = ctx or _native.context()
    return ctx.cluster_stats(*args[:6], reducers=reducers, sorted=sorted)


def load_clusters(infile):
    """Reference ``clusters.py:176-193``: list of sets of (i, j) tuples."""
    with open(infile, 'r') as handle:
        return [set([tuple(e) for e in cluster]) for cluster in
                json.load(handle)]


_PIXEL_TEXT = bytes.maketrans(b'[]', b'  ')
_PAIR = rb'\[\d+,\d+\]'
_CLUSTER = rb'\[(?:%s(?:,%s)*)?\]' % (_PAIR, _PAIR)
_CLUSTER_FILE = re.compile(rb'\[(?:%s(?:,%s)*)?\]' % (_CLUSTER, _CLUSTER))


def load_cluster_pixels(infile):
    """Every pixel of a cluster JSON (reference clusters.py:176-193's file:
    a list of clusters, each a list of [i, j]) as one (k, 2) int64 array,
    parsed in C (numpy's text reader over the numbers) instead of as
    Python sets of tuples -- what prepare_data's loop_idx needs (the union
    of the clusters' pixels, analysis.py:117-125). Files that are not pure
    nested lists of integer pairs go through json (load_clusters)."""
    with open(infile, 'rb') as handle:
        text = handle.read()
    compact = text.translate(None, b' \t\r\n')
    if _CLUSTER_FILE.fullmatch(compact):
        body = compact.translate(_PIXEL_TEXT).replace(b',', b' ').strip()
        if not body:
            return np.zeros((0, 2), dtype=np.int64)
        return np.fromstring(body.decode('ascii'), dtype=np.int64,
                             sep=' ').reshape(-1, 2)
    # anything else as the reference reads it; a pixel with a non-integer
    # coordinate can match no (row, col) of the union
    pix = np.array([p for cl in load_clusters(infile) for p in cl],
                   dtype=np.float64).reshape(-1, 2)
    pix = pix[np.all(pix == np.floor(pix), axis=1)]
    return pix.astype(np.int64)


def load_cluster_list(infile):
    """A cluster JSON as a ``ClusterList`` (file order kept)."""
    with open(infile, 'r') as handle:
        data = json.load(handle)
    return ClusterList.from_sets(data)


def save_clusters(clusters, outfile):
    """Reference ``clusters.py:116-136`` (list of sets or a ClusterList)."""
    with open(outfile, 'w') as handle:
        if isinstance(clusters, ClusterList):
            handle.write(clusters.json_text())
        else:
            json.dump([[[int(i), int(j)] for i, j in cluster]
                       for cluster in clusters], handle)


def cluster_to_loop_id(cluster, chrom, resolution):
    """Reference ``clusters.py:300-330``: "chr:start-end_chr:start-end"."""
    x, y = zip(*cluster)
    return '%s:%s-%s_%s:%s-%s' % (chrom, min(x) * resolution,
                                  (max(x) + 1) * resolution, chrom,
                                  min(y) * resolution,
                                  (max(y) + 1) * resolution)


def cluster_to_slices(cluster, width=21):
    """Reference ``clusters.py:253-289``: the (row, column) slices of the
    ``width`` x ``width`` square centred on the cluster's centre of mass
    (truncated to a bin per axis); ``width`` should be odd.

    >>> cluster_to_slices([(4, 5), (3, 4), (3, 5), (3, 6)], width=5)
    (slice(1, 6, None), slice(3, 8, None))
    """
    half = int((width - 1) / 2)
    rows, cols = zip(*cluster)
    r, c = int(np.mean(rows)), int(np.mean(cols))
    return slice(r - half, r + half + 1), slice(c - half, c + half + 1)


def cluster_from_string(cluster_string):
    """Reference ``clusters.py:333-360``."""
    return json.loads(cluster_string.replace('(', '[').replace('{', '[')
                      .replace(')', ']').replace('}', ']'))


def pixel_membership(row, col, clusters_lists, n_bins=None, mask=None):
    """Boolean vector: (row[k], col[k]) in the union of all clusters
    (reference ``analysis.py:117-125``, a Python set lookup per pixel),
    vectorised with 64-bit pixel keys. ``clusters_lists``: per condition a
    list of pixel sets (load_clusters) or a (k, 2) pixel array
    (load_cluster_pixels)."""
    arrs = [c for c in clusters_lists if isinstance(c, np.ndarray)]
    sets = [c for c in clusters_lists if not isinstance(c, np.ndarray)]
    if sets:
        pixels = set().union(*sum(sets, []))
        if pixels:
            arrs.append(np.array(sorted(pixels), dtype=np.int64))
    arrs = [a.reshape(-1, 2) for a in arrs if len(a)]
    if not arrs or len(row) == 0:
        return np.zeros(len(row) if mask is None else
                        int(np.count_nonzero(mask)), dtype=bool)
    pix = np.concatenate(arrs)
    return pixel_in(row, col, pix[:, 0], pix[:, 1], mask=mask)


def pixel_in(row, col, prow, pcol, mask=None):
    """(row[k], col[k]) in the pixel set {(prow, pcol)} (vectorised), for
    the k where ``mask`` (when given) is set -- the keys are formed over all
    of row / col in place and masked once (prepare_data's loop_idx over the
    disp pixels of a chromosome's union)."""
    row = np.asarray(row)
    col = np.asarray(col)
    if mask is not None and len(row):
        n_out = int(np.count_nonzero(mask))
    else:
        n_out = len(row)
    if n_out == 0 or len(prow) == 0:
        return np.zeros(n_out, dtype=bool)
    prow = np.asarray(prow, dtype=np.int64)
    pcol = np.asarray(pcol, dtype=np.int64)
    base = int(max(pcol.max(), col.max())) + 1
    keys = row.astype(np.int64)
    keys *= base
    keys += col
    if mask is not None:
        keys = keys[mask]
    pk = prow * base + pcol
    if len(keys) > 1 and not np.all(keys[1:] > keys[:-1]):
        return np.isin(keys, pk)
    # the union's pixels come in (row, col) order with unique keys: each set
    # pixel is found by binary search (no sort of the chromosome's keys)
    out = np.zeros(len(keys), dtype=bool)
    pos = np.searchsorted(keys, pk)
    ok = pos < len(keys)
    pos, pk = pos[ok], pk[ok]
    out[pos[keys[pos] == pk]] = True
    return out


def _set_pixels(clusters_lists):
    """The pixels of ``pixel_membership``'s ``clusters_lists`` as one (k, 2)
    int64 array (repeats kept)."""
    arrs = []
    for c in clusters_lists:
        if isinstance(c, np.ndarray):
            a = c
        else:
            pix = [p for cluster in c for p in cluster]
            a = np.array(pix, dtype=np.int64) if pix else \
                np.zeros((0, 2), dtype=np.int64)
        if a.dtype.kind not in 'iu':
            raise TypeError('cluster pixels must be integers, not %s'
                            % a.dtype)
        if a.size:
            arrs.append(a.reshape(-1, 2).astype(np.int64, copy=False))
    if not arrs:
        return np.zeros((0, 2), dtype=np.int64)
    return np.concatenate(arrs)


def pixel_membership_gpu(row, col, clusters_lists, mask=None):
    """``pixel_membership`` on the GPU (h3d_pixel_membership): the set's
    64-bit pixel keys are sorted once on the device and every query pixel is
    found by a binary search, so the queries may come in any order. Returns
    a bool vector, one entry per pixel (per pixel where ``mask`` is set).
    There is no CPU fallback; the arguments are checked before a device is
    touched."""
    row, col = np.asarray(row), np.asarray(col)
    for a, what in ((row, 'row'), (col, 'col')):
        if a.dtype.kind not in 'iu':
            raise TypeError('%s must be integers, not %s' % (what, a.dtype))
        if a.ndim != 1:
            raise ValueError('%s must have 1 dimension' % what)
    if row.shape != col.shape:
        raise ValueError('row and col must have one length')
    if mask is not None:
        mask = np.asarray(mask)
        if mask.dtype != np.bool_ or mask.shape != row.shape:
            raise ValueError('mask must be a boolean vector of row\'s length')
        row, col = row[mask], col[mask]
    if len(row) >= 2 ** 31:
        raise ValueError('at most 2^31 - 1 pixels')
    if len(row) and (min(row.min(), col.min()) < 0 or
                     max(row.max(), col.max()) >= 2 ** 31):
        raise ValueError('row and col must be in [0, 2^31)')
    pix = _set_pixels(clusters_lists)
    if len(pix) >= 2 ** 31:
        raise ValueError('at most 2^31 - 1 set pixels')
    if len(row) == 0 or len(pix) == 0:
        return np.zeros(len(row), dtype=bool)
    return _native.context().pixel_membership(row, col, pix[:, 0], pix[:, 1])
