"""Aggregate peak analysis stacks (reference hic3defdr/util/apa.py:6-44).

The reference slices a scipy matrix once per cluster in a Python loop; here
the window of every cluster is found on the host in one vectorised pass
(``apa_windows``) and all of them are gathered on the GPU in one launch
(``h3d_window_gather``). ``apa_mean`` aggregates a stack on the GPU
(``h3d_stack_aggregate``). There is no CPU fallback.
"""
import numpy as np

from hic3defdr_amd import _native
from hic3defdr_amd.util.clusters import ClusterList
from hic3defdr_amd.util.matrices import NAN_WINDOW, float_data


def check_width(width):
    """The window width as an int; ``ValueError`` unless it is a positive odd
    integer (the reference fails with a broadcast ValueError on even ones:
    its stack is ``width`` wide, its slices ``width + 1``)."""
    if isinstance(width, bool) or not isinstance(width, (int, np.integer)) \
            or width < 1 or width % 2 == 0:
        raise ValueError('width must be a positive odd integer, got %r'
                         % (width,))
    return int(width)


def apa_windows(clusters, width, size, min_dist=None):
    """Window of every cluster, as the reference places and filters them
    (``apa.py:31-43``, ``clusters.py:284-289``): ``(origins, valid)`` with
    ``origins`` (W, 2) int32 -- the window's first row and column, the centre
    being the centre of mass truncated per axis -- and ``valid`` (W,) bool.
    A cluster closer to the diagonal than ``min_dist`` (default ``width +
    1``), or whose centre of mass is less than ``r = int(width / 2)`` from
    either end of ``[0, size]``, is not valid; its row origin is
    ``NAN_WINDOW`` (an all-NaN window).

    Deviation: at a centre of mass of exactly ``size - r`` the reference's
    test passes, its slice is clipped by the matrix and the assignment raises
    a broadcast ValueError; here that window does not fit and is not valid.

    ``clusters``: a list of clusters (iterables of ``(i, j)``) or a
    ``ClusterList``."""
    width = check_width(width)
    if min_dist is None:
        min_dist = width + 1
    cl = clusters if isinstance(clusters, ClusterList) \
        else ClusterList.from_sets(clusters)
    n = cl.sizes()
    if len(n) == 0:
        return np.zeros((0, 2), dtype=np.int32), np.zeros(0, dtype=bool)
    if n.min() < 1:
        raise ValueError('a cluster without points has no centre')
    r = int(width / 2)
    pr, pc = cl.pixels()
    starts = cl.starts[:-1]
    # integer point sums (below 2^53), so sum / len is np.mean exactly
    com0 = np.add.reduceat(pr, starts) / n
    com1 = np.add.reduceat(pc, starts) / n
    c0, c1 = com0.astype(np.int64), com1.astype(np.int64)
    valid = ~((np.abs(com1 - com0) < min_dist) | (com0 < r) | (com1 < r) |
              (size - com0 < r) | (size - com1 < r))
    valid &= (c0 + r + 1 <= size) & (c1 + r + 1 <= size)
    origins = np.empty((len(n), 2), dtype=np.int32)
    origins[:, 0] = np.where(valid, c0 - r, NAN_WINDOW)
    origins[:, 1] = np.where(valid, c1 - r, 0)
    return origins, valid


def make_apa_stack(matrix, clusters, width, min_dist=None):
    """Reference ``apa.py:6-44``: the stack (clusters, width, width) of the
    square slices of ``matrix`` (any scipy sparse matrix) centred on each
    cluster; slices of clusters that ``apa_windows`` does not keep are NaN,
    cells the matrix does not store are 0."""
    width = check_width(width)
    m = matrix.tocsr()
    if m is matrix:
        m = m.copy()
    m.sum_duplicates()
    m.sort_indices()
    origins, _ = apa_windows(clusters, width, max(m.shape), min_dist)
    if len(origins) == 0:
        return np.zeros((0, width, width))
    return _native.context().window_gather(
        m.indices, float_data(m.data), origins, width, width, m.shape,
        indptr=m.indptr, symmetrize=False, fill=0.0)[0]


def apa_mean(stack):
    """``(mean, count)`` of a stack (W, h, w) over its windows: ``count``
    (int64) the windows whose cell is not NaN, ``mean`` their mean, NaN where
    ``count`` is 0 -- ``np.nanmean(stack, axis=0)`` with a fixed summation
    order on the GPU, so a rerun gives the same bits."""
    count, total = _native.context().stack_aggregate(stack)
    with np.errstate(invalid='ignore', divide='ignore'):
        return total / count, count
