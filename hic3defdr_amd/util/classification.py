"""Classification (reference hic3defdr/util/classification.py)."""
import numpy as np

from hic3defdr_amd.util.clusters import ClusterList, pixel_in


def classify_clusters(row, col, value, clusters):
    """``ClusterList`` form of ``classify`` (classification.py:7-49): the
    pixels of ``clusters`` (matched against (row, col)) get the class
    argmax(value[pixel]) (first maximum; NaN wins as in np.argmax), then each
    class's pixels are re-clustered in (row, col) order. Returns one
    ``ClusterList`` per column of ``value``."""
    row = np.asarray(row, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    value = np.asarray(value)
    if not isinstance(clusters, ClusterList):
        clusters = ClusterList.from_sets(clusters)
    pr, pc = clusters.pixels()
    idx = pixel_in(row, col, pr, pc)
    classes = np.argmax(value[idx, :], axis=1) if idx.any() else \
        np.zeros(0, dtype=np.int64)
    r, c = row[idx], col[idx]
    return [ClusterList.find(r[classes == k], c[classes == k])
            for k in range(value.shape[1])]


def classify_clusters_gpu(row, col, value, clusters, connectivity=1,
                          ctx=None):
    """``classify_clusters`` on the GPU: the same per-class clusters as sets
    of pixels, in canonical order (clusters by their first pixel, pixels in
    (row, col) order). Membership in ``clusters`` is
    h3d_pixel_membership_dev, the class byte of a member np.argmax of its
    row of ``value`` (h3d_argmax_classes_dev), and every class is labelled
    in the one pass (h3d_label_components_dev). The pixels must be distinct,
    in (row, col) order, with coordinates in [0, 2^31), and ``value`` (n, C)
    with C <= 254 (ValueError otherwise, before a device is touched). There
    is no CPU fallback."""
    from hic3defdr_amd import _native
    from hic3defdr_amd.util.clusters import check_pixels, components_dev
    row, col = check_pixels(row, col, connectivity)
    value = np.asarray(value)
    if value.ndim != 2 or value.shape[0] != len(row):
        raise ValueError('value must be (n, C) with one row per pixel')
    if value.dtype.kind not in 'fiu':
        raise TypeError('value must be numeric, not %s' % value.dtype)
    C = value.shape[1]
    _native.check_class_count(C)
    if not isinstance(clusters, ClusterList):
        clusters = ClusterList.from_sets(clusters)
    pr, pc = clusters.pixels()
    if len(row) == 0 or len(pr) == 0:
        return [ClusterList.empty() for _ in range(C)]
    import torch
    ctx = ctx or _native.context()
    dev = torch.device('cuda', ctx.device)

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)

    t_row, t_col = up(row, np.int64), up(col, np.int64)
    member = ctx.pixel_membership_dev(t_row, t_col, up(pr, np.int64),
                                      up(pc, np.int64))
    t_cls = ctx.argmax_classes_dev(up(value, np.float64), member)
    return components_dev(ctx, row, col, t_row, t_col, t_cls, C, connectivity)


def classify(row, col, value, clusters):
    """Reference ``classification.py:7-49``: list (per class) of lists of
    sets of (i, j)."""
    return [cl.to_sets() for cl in classify_clusters(row, col, value,
                                                     clusters)]
