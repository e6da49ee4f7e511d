"""Thresholding (reference hic3defdr/util/thresholding.py)."""
import numpy as np

from hic3defdr_amd.util.clusters import ClusterList


def threshold_clusters(qvalues, row, col, fdr):
    """``ClusterList`` form of ``threshold_and_cluster``: pixels with
    q < fdr and with q >= fdr (NaN in neither), each clustered in pixel
    order (thresholding.py:7-41)."""
    q = np.asarray(qvalues)
    row = np.asarray(row)
    col = np.asarray(col)
    sig = q < fdr
    insig = q >= fdr
    return (ClusterList.find(row[sig], col[sig]),
            ClusterList.find(row[insig], col[insig]))


def threshold_clusters_gpu(qvalues, row, col, fdr, cluster_size=1,
                           connectivity=1, ctx=None):
    """``threshold_clusters`` on the GPU: the same ``(sig, insig)`` clusters
    as sets of pixels, in canonical order (clusters by their first pixel,
    pixels in (row, col) order). Both sets are labelled in one pass over a
    class byte per pixel (h3d_threshold_classes_dev,
    h3d_label_components_dev, h3d_cluster_lists_dev).

    ``fdr`` may be a list: row, col and the q-values are uploaded once and
    a list of ``(sig, insig)`` pairs comes back. ``cluster_size`` (or the
    smallest of a list) is the size below which clusters are not listed;
    ``size_filter`` does the rest. The pixels must be distinct, in (row, col)
    order, with coordinates in [0, 2^31) (ValueError otherwise, before a
    device is touched). There is no CPU fallback."""
    from hic3defdr_amd import _native
    from hic3defdr_amd.util.clusters import check_pixels, components_dev
    row, col = check_pixels(row, col, connectivity)
    q = np.asarray(qvalues)
    if q.dtype.kind != 'f':
        raise TypeError('qvalues must be floating point, not %s' % q.dtype)
    if q.shape != row.shape:
        raise ValueError('qvalues, row and col must have one length')
    many = hasattr(fdr, '__len__')
    fdrs = [float(f) for f in fdr] if many else [float(fdr)]
    sizes = list(cluster_size) if hasattr(cluster_size, '__len__') \
        else [cluster_size]
    if not sizes or any(isinstance(s, bool) or int(s) != s for s in sizes):
        raise ValueError('cluster_size must be an integer or a list of them')
    min_size = max(int(min(sizes)), 1)
    if len(row) == 0:
        out = [(ClusterList.empty(), ClusterList.empty()) for _ in fdrs]
        return out if many else out[0]
    import torch
    ctx = ctx or _native.context()
    dev = torch.device('cuda', ctx.device)
    t_row = torch.from_numpy(np.ascontiguousarray(row)).to(dev)
    t_col = torch.from_numpy(np.ascontiguousarray(col)).to(dev)
    t_q = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float64)).to(dev)
    out = []
    for f in fdrs:
        t_cls = ctx.threshold_classes_dev(t_q, f)
        out.append(tuple(components_dev(ctx, row, col, t_row, t_col, t_cls, 2,
                                        connectivity, min_size)))
    return out if many else out[0]


def threshold_and_cluster(qvalues, row, col, fdr):
    """Reference ``thresholding.py:7-41``: lists of sets of (i, j)."""
    sig, insig = threshold_clusters(qvalues, row, col, fdr)
    return sig.to_sets(), insig.to_sets()


def size_filter(clusters, cluster_size):
    """Reference ``thresholding.py:44-61``."""
    if isinstance(clusters, ClusterList):
        return clusters.size_filter(cluster_size)
    return [c for c in clusters if len(c) >= cluster_size]
