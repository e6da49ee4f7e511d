"""Dense views of COO-format sparse data (reference
hic3defdr/util/matrices.py:132-160 ``select_matrix``).

The reference masks the whole table once per window; here the table -- the
lexsorted ``(row, col)`` pixel list of an outdir stage -- is read as a CSR
matrix on the GPU and any number of windows is gathered in one launch
(``h3d_window_gather``). There is no CPU fallback.
"""
import numpy as np

from hic3defdr_amd import _native

_I32_MIN = int(np.iinfo(np.int32).min)
_I32_MAX = int(np.iinfo(np.int32).max)
# window origin of an all-NaN window (h3d.h)
NAN_WINDOW = _I32_MIN


def check_table(row, col):
    """``(row, col)`` as int32 arrays after checking, once and vectorised,
    that the pixels are sorted by (row, col) with no repeats and lie in the
    upper triangle (``row <= col``) -- the layout of every outdir table, and
    what lets the device find a pixel by binary search. ``ValueError``
    otherwise (a deviation: the reference accepts any COO order)."""
    row = np.asarray(row)
    col = np.asarray(col)
    if row.ndim != 1 or row.shape != col.shape:
        raise ValueError('row and col must be vectors of one length')
    if len(row) == 0:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    if not (np.issubdtype(row.dtype, np.integer) and
            np.issubdtype(col.dtype, np.integer)):
        raise ValueError('row and col must be integer arrays')
    if row.min() < 0 or col.max() > _I32_MAX:
        raise ValueError('row / col outside [0, 2^31)')
    if np.any(row > col):
        raise ValueError('pixels below the diagonal (row > col): the table '
                         'must hold the upper triangle')
    r0, r1, c0, c1 = row[:-1], row[1:], col[:-1], col[1:]
    if not np.all((r1 > r0) | ((r1 == r0) & (c1 > c0))):
        raise ValueError('pixels are not sorted by (row, col), or repeat')
    return (np.ascontiguousarray(row, dtype=np.int32),
            np.ascontiguousarray(col, dtype=np.int32))


def slice_bounds(s, what='slice'):
    """(start, stop) of a slice with integer bounds and step None or 1."""
    if not isinstance(s, slice):
        raise ValueError('%s must be a slice' % what)
    for v in (s.start, s.stop):
        if v is None or isinstance(v, bool) or \
                not isinstance(v, (int, np.integer)):
            raise ValueError('%s needs integer start and stop, got %r'
                             % (what, s))
    if s.step is not None and s.step != 1:
        raise ValueError('%s must have step None or 1, got %r' % (what, s))
    return int(s.start), int(s.stop)


def float_data(data):
    """Stage data as float64 (integer and boolean stages converted on the
    host, as the reference's assignment into a float matrix does)."""
    data = np.asarray(data)
    if data.dtype.kind not in 'fiub':
        raise ValueError('data of dtype %s cannot fill a float matrix'
                         % data.dtype)
    return np.ascontiguousarray(data, dtype=np.float64)


def table_windows(row, col, data, origins, h, w, cols=None, n_bins=None,
                  symmetrize=True, mean=False, fill=np.nan):
    """Dense ``h`` x ``w`` windows at ``origins`` (W, 2) of the lexsorted
    table ``(row, col, data)``, ``data`` (n,) or (n, columns): (K, W, h, w),
    or (W, h, w) with ``mean`` (the listed columns averaged in list order).
    One launch of ``h3d_window_gather``."""
    row, col = check_table(row, col)
    data = float_data(data)
    if data.shape[0] != len(row):
        raise ValueError('data must have one row per pixel')
    if n_bins is None:
        n_bins = int(col.max()) + 1 if len(col) else 0
    return _native.context().window_gather(
        col, data, origins, h, w, (n_bins, n_bins), row=row, cols=cols,
        symmetrize=symmetrize, mean=mean, fill=fill)


def slice_window(row_slice, col_slice):
    """(origin (1, 2) int32, h, w) of the window two slices select."""
    r0, r1 = slice_bounds(row_slice, 'row_slice')
    c0, c1 = slice_bounds(col_slice, 'col_slice')
    h, w = r1 - r0, c1 - c0
    if h < 0 or w < 0:
        raise ValueError('negative dimensions are not allowed')
    if not (_I32_MIN < r0 <= _I32_MAX and _I32_MIN < c0 <= _I32_MAX):
        raise ValueError('slice start outside the int32 range')
    return np.array([[r0, c0]], dtype=np.int32), h, w


def select_matrix(row_slice, col_slice, row, col, data, symmetrize=True):
    """Reference ``matrices.py:132-160``: the dense float64 matrix that
    ``row_slice`` x ``col_slice`` selects from COO data, NaN where nothing is
    stored; ``symmetrize`` also fills ``(j, i)`` from a stored ``(i, j)``
    (written second, so it wins where both are stored).

    Slices need integer bounds and a step of None or 1; negative starts and
    stops beyond the matrix are allowed (those cells are NaN). Deviation:
    ``(row, col)`` must be sorted by (row, col) without repeats, with
    ``row <= col`` (the layout of every outdir table); the reference accepts
    any COO order."""
    origin, h, w = slice_window(row_slice, col_slice)
    data = np.asarray(data)
    if data.ndim != 1:
        raise ValueError('data must be one value per pixel (pass rep or cond '
                         'for a stage with several columns)')
    if h == 0 or w == 0:
        check_table(row, col)
        return np.full((h, w), np.nan)
    return table_windows(row, col, data, origin, h, w,
                         symmetrize=symmetrize)[0, 0]
