"""ctypes binding of libh3d.so (include/h3d.h).

The product path has no CPU fallback: if the library or a gfx950 device is
missing, every entry point raises ``H3DError``.
"""
import ctypes
import os
import threading

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('H3D_LIB', os.path.join(PKG, 'lib', 'libh3d.so'))

H3D_EST = {'qcml': 0, 'cml': 1, 'mme': 2}
# size-factor methods (util/scaling.py), h3d.h H3D_NORM_*
H3D_NORM = {'conditional_mor': 0, 'conditional_scaling': 1,
            'median_of_ratios': 2, 'simple_scaling': 3, 'no_scaling': 4}

ERRORS = {-1: 'bad argument', -2: 'HIP runtime error',
          -3: 'numerical failure', -4: 'out of device memory',
          -5: 'invalid numeric input', -6: 'no gfx950 device'}

EXPORTS = [
    'h3d_version', 'h3d_device_count', 'h3d_open', 'h3d_close',
    'h3d_last_error', 'h3d_set_stream', 'h3d_union_count', 'h3d_union_fill',
    'h3d_size_factors_cmor', 'h3d_size_factors', 'h3d_disp_per_dist', 'h3d_disp_per_dist_dev',
    'h3d_disp_table', 'h3d_disp_tables', 'h3d_lrt', 'h3d_lrt_dev', 'h3d_bh',
    'h3d_profile_enable', 'h3d_profile_read', 'h3d_profile_reset',
    'h3d_find_clusters', 'h3d_find_clusters_ordered', 'h3d_format_clusters', 'h3d_lrt_poisson',
    'h3d_lrt_poisson_dev', 'h3d_mme_per_pixel', 'h3d_lrt_wide', 'h3d_cml',
    'h3d_bh_ctx', 'h3d_bh_dev', 'h3d_npz_csr_info', 'h3d_npz_csr_read',
    'h3d_disp_tables_dev', 'h3d_disp_tables_wait', 'h3d_lrt_dev_tab',
    'h3d_estimate_disp_dev', 'h3d_bh_sort_dev', 'h3d_bh_scan_dev',
    'h3d_bh_finish_dev', 'h3d_union_fill_dev', 'h3d_size_factors_dev',
    'h3d_disp_pixels_dev', 'h3d_table_gather_dev', 'h3d_disp_seg_stats',
    'h3d_scale_disp_dev', 'h3d_npz_backend', 'h3d_npz_csr_read_slack',
    'h3d_pixel_f_dev', 'h3d_read_text_column', 'h3d_set_qcml_tol',
    'h3d_window_gather', 'h3d_window_gather_dev', 'h3d_stack_aggregate',
    'h3d_filter_sparse_rows', 'h3d_kr_balance',
    'h3d_nb_fit_mu', 'h3d_nb_fit_mu_dev', 'h3d_nb_equalize',
    'h3d_nb_equalize_dev', 'h3d_nb_quantile_map', 'h3d_nb_logpmf',
    'h3d_group_sums', 'h3d_group_sums_dev', 'h3d_histogram',
    'h3d_histogram_dev', 'h3d_ma_stats', 'h3d_density_grid',
    'h3d_rank_average', 'h3d_corr_matrix', 'h3d_pixel_moments',
    'h3d_balance_pixels',
    'h3d_pixel_membership', 'h3d_pixel_membership_dev', 'h3d_roc_curve',
    'h3d_roc_curve_dev', 'h3d_order_stats', 'h3d_bin_fractions',
    'h3d_nb_sample', 'h3d_nb_sample_dev', 'h3d_simulate_dev',
    'h3d_label_components', 'h3d_label_components_dev',
    'h3d_threshold_classes_dev', 'h3d_argmax_classes_dev',
    'h3d_cluster_lists', 'h3d_cluster_lists_dev',
    'h3d_cluster_stats', 'h3d_cluster_stats_dev',
]


# entry points a library built from an older tree may lack; callers check
OPTIONAL = ('h3d_find_clusters_ordered', 'h3d_npz_backend',
            'h3d_npz_csr_read_slack', 'h3d_read_text_column',
            'h3d_disp_tables', 'h3d_npz_csr_info', 'h3d_npz_csr_read',
            'h3d_disp_tables_dev', 'h3d_disp_tables_wait', 'h3d_lrt_dev_tab',
            'h3d_estimate_disp_dev')


class H3DError(RuntimeError):
    """A libh3d call failed (the reference would have raised too, or the
    native library / GPU is unavailable). ``code``: the library's return
    code (``ERRORS``), None when the failure was not a libh3d return."""

    def __init__(self, msg, code=None):
        RuntimeError.__init__(self, msg)
        self.code = code


H3D_EINPUT = -5
H3D_FLAG_BADIN = 16
# the calls as connected components (h3d_label_components): the class byte of
# "no pixel", the largest class count and pixel count, the input rule
CLS_ABSENT = 255
CCL_MAX_CLASSES = 254
CCL_MAX_N = 2 ** 31 - 2
BAD_PIXELS = ('pixels must be distinct, in (row, col) order, with '
              'coordinates in [0, 2^31)')


# per-cluster statistics (h3d_cluster_stats): the reducers as `want` bits, the
# largest K, the flag bits of h3d.h
CSTAT_WANT = {'mean': 1, 'max': 2, 'min': 4}
CSTAT_MAX_K = 256
CSTAT_REPEAT, CSTAT_ORDER, CSTAT_PIXEL, CSTAT_STARTS = 1, 2, 4, 8


def cstat_want(reducers):
    """The `want` bits of an iterable of reducer names (ValueError for a name
    that is not 'mean', 'max' or 'min', or for none at all)."""
    if isinstance(reducers, str):
        reducers = (reducers,)
    reducers = tuple(reducers)
    for r in reducers:
        if r not in CSTAT_WANT:
            raise ValueError("reducer must be 'mean', 'max' or 'min', got %r"
                             % (r,))
    if not reducers:
        raise ValueError('no reducer')
    want = 0
    for r in reducers:
        want |= CSTAT_WANT[r]
    return reducers, want


def cstat_raise(flags):
    """The exceptions of h3d_cluster_stats' flag bits."""
    if flags & CSTAT_REPEAT:
        raise ValueError('the table repeats a pixel, or has a coordinate '
                         'outside [0, 2^31)')
    if flags & CSTAT_ORDER:
        raise ValueError('sorted=True, but the table is not in strictly '
                         'increasing (row, col) order')
    if flags & CSTAT_STARTS:
        raise ValueError('starts must begin at 0 and every cluster must have '
                         'a pixel')
    if flags & CSTAT_PIXEL:
        raise IndexError('a cluster pixel is outside the table\'s shape')


def check_cluster_stats(row, col, data, prow, pcol, starts):
    """The input rule of h3d_cluster_stats for host arrays, checked before a
    device is touched. Table: integer ``row`` / ``col`` (n,) with coordinates
    in [0, 2^31), n <= 2^31 - 2, ``data`` (n,) or (n, K) float, integer or
    bool (converted to float64), 1 <= K <= 256. Clusters: integer ``prow`` /
    ``pcol`` (p,), ``starts`` (k + 1,) from 0 to p, strictly increasing (an
    empty cluster is a ValueError). A negative cluster coordinate is a
    ValueError, one beyond the table's shape ``(max(row) + 1, max(col) + 1)``
    an IndexError. Returns (row, col, data (n, K), prow, pcol, starts, n_rows,
    n_cols) as contiguous int64 / float64."""
    row, col, data = np.asarray(row), np.asarray(col), np.asarray(data)
    prow, pcol, starts = np.asarray(prow), np.asarray(pcol), np.asarray(starts)
    for a, what in ((row, 'row'), (col, 'col'), (prow, 'cluster rows'),
                    (pcol, 'cluster columns'), (starts, 'starts')):
        if a.dtype.kind not in 'iu' and a.size:
            raise TypeError('%s must be integers, not %s' % (what, a.dtype))
        if a.ndim != 1:
            raise ValueError('%s must have 1 dimension' % what)
    if data.dtype.kind not in 'fiub':
        raise TypeError('data must be float, integer or bool, not %s'
                        % data.dtype)
    if data.ndim == 1:
        data = data[:, None]
    if data.ndim != 2:
        raise ValueError('data must have 1 or 2 dimensions')
    n = len(row)
    if col.shape != row.shape or data.shape[0] != n:
        raise ValueError('row, col and data must have one length')
    if not 1 <= data.shape[1] <= CSTAT_MAX_K:
        raise ValueError('between 1 and %d data columns, got %d'
                         % (CSTAT_MAX_K, data.shape[1]))
    if n > CCL_MAX_N or len(prow) > CCL_MAX_N:
        raise ValueError('at most 2^31 - 2 pixels')
    if pcol.shape != prow.shape:
        raise ValueError('cluster rows and columns must have one length')
    if len(starts) < 1 or starts[0] != 0 or starts[-1] != len(prow):
        raise ValueError('starts must run from 0 to the number of cluster '
                         'pixels')
    if np.any(starts[1:] <= starts[:-1]):
        raise ValueError('an empty cluster')
    n_rows = n_cols = 0
    if n:
        if min(row.min(), col.min()) < 0 or \
                max(row.max(), col.max()) >= 2 ** 31:
            raise ValueError('row and col must be in [0, 2^31)')
        n_rows, n_cols = int(row.max()) + 1, int(col.max()) + 1
    if len(prow):
        if min(prow.min(), pcol.min()) < 0:
            raise ValueError('a cluster pixel has a negative coordinate')
        if prow.max() >= n_rows or pcol.max() >= n_cols:
            raise IndexError('a cluster pixel is outside the table\'s shape '
                             '(%d, %d)' % (n_rows, n_cols))
    return (_c(row, np.int64), _c(col, np.int64), _c(data, np.float64),
            _c(prow, np.int64), _c(pcol, np.int64), _c(starts, np.int64),
            n_rows, n_cols)


def check_class_count(C):
    if not 1 <= int(C) <= CCL_MAX_CLASSES:
        raise ValueError('between 1 and %d classes, got %d'
                         % (CCL_MAX_CLASSES, C))


_P = ctypes.c_void_p
_INT_MAX = 2 ** 31 - 1
_I64 = ctypes.c_int64
_I = ctypes.c_int
_D = ctypes.c_double
_U64 = ctypes.c_uint64
_U32 = ctypes.c_uint32
ALLREDUCE_FN = ctypes.CFUNCTYPE(_I, ctypes.POINTER(_D), _I64, _P)

_lib = None
_lock = threading.RLock()  # context() -> Context() -> load_library()


def load_library(path=None):
    """Loads libh3d.so (once) and declares every prototype of h3d.h."""
    global _lib
    with _lock:
        if _lib is not None and path is None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise H3DError('libh3d.so not found at %s: run '
                           '`python -c "import __graft_entry__ as g; g.build()"`'
                           % p)
        # One HIP runtime per process: torch (when installed) ships its own
        # libamdhip64.so.7 under the same SONAME as the /opt/rocm one libh3d
        # links, and whichever loads first serves both. Loading torch's first
        # keeps torch.cuda working next to libh3d (the other order leaves
        # torch without devices) and lets torch tensors / streams be handed
        # to the *_dev entry points.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = ctypes.CDLL(p)
        sig = {
            'h3d_version': (_I, []),
            'h3d_device_count': (_I, []),
            'h3d_open': (_P, [_I]),
            'h3d_close': (None, [_P]),
            'h3d_last_error': (ctypes.c_char_p, []),
            'h3d_set_stream': (_I, [_P, _P]),
            'h3d_set_qcml_tol': (_I, [_P, _D]),
            'h3d_union_count': (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _I, _P]),
            'h3d_union_fill': (_I, [_P, _P, _P, _P, _P, _I64]),
            'h3d_union_fill_dev': (_I, [_P, _P, _P, _P, _P, _I64, _P, _P, _P,
                                        _P]),
            'h3d_size_factors_dev': (_I, [_P, _P, _P, _I64, _I, _I, _I, _P,
                                          _P]),
            'h3d_disp_pixels_dev': (_I, [_P, _P, _P, _P, _P, _I, _P, _I, _P,
                                         _I64, _I, _I64, _P, _P, _P]),
            'h3d_table_gather_dev': (_I, [_P, _P, _I, _I, _P, _I64, _P]),
            'h3d_pixel_f_dev': (_I, [_P, _P, _P, _P, _P, _I64, _I, _P, _P, _P,
                                     _P, _I, _P]),
            'h3d_scale_disp_dev': (_I, [_P, _P, _P, _I, _P, _P, _I64, _I, _I,
                                        _P, ctypes.c_double, _I, _P, _P, _P,
                                        _P]),
            'h3d_disp_seg_stats': (_I, [_P, _I, _P, _P]),
            'h3d_size_factors_cmor': (_I, [_P, _P, _P, _I64, _I, _I, _P]),
            'h3d_size_factors': (_I, [_P, _P, _P, _I64, _I, _I, _I, _P]),
            'h3d_disp_per_dist': (_I, [_P, _P, _P, _P, _I64, _I, _I, _P, _I,
                                       _I, _P, _P]),
            'h3d_disp_per_dist_dev': (_I, [_P, _P, _P, _P, _I64, _I, _I, _P,
                                           _I, _I, _P, _P, ALLREDUCE_FN, _P]),
            'h3d_disp_table': (_I, [_P, _I, _I, _D, _D, _P]),
            'h3d_disp_tables': (_I, [_P, _I, _I, _I, _D, _D, _P]),
            'h3d_lrt': (_I, [_P, _P, _P, _P, _P, _I64, _I, _I, _P, _I, _I, _P,
                             _P, _P, _P, _P]),
            'h3d_lrt_dev': (_I, [_P, _P, _P, _P, _P, _I64, _I, _I, _P, _I, _I,
                                 _P, _P, _P, _P, _P]),
            'h3d_bh': (_I, [_P, _I64, _P]),
            'h3d_bh_ctx': (_I, [_P, _P, _I64, _P]),
            'h3d_bh_dev': (_I, [_P, _P, _I64, _P]),
            'h3d_bh_sort_dev': (_I, [_P, _P, _P, _I64, _P, _P, _P]),
            'h3d_bh_scan_dev': (_I, [_P, _P, _I64, _I64, _I64, _P, _P]),
            'h3d_bh_finish_dev': (_I, [_P, _P, _I64, _D, _P]),
            'h3d_profile_enable': (_I, [_P, _I]),
            'h3d_profile_read': (_I, [_P, ctypes.c_char_p, _P, _P, _P]),
            'h3d_profile_reset': (_I, [_P]),
            'h3d_find_clusters': (_I, [_P, _P, _I64, _I, _P, _P]),
            'h3d_find_clusters_ordered': (_I, [_P, _P, _I64, _I, _P, _P, _P]),
            'h3d_format_clusters': (_I, [_P, _P, _P, _P, _I64, _P, _I64, _P,
                                         _P]),
            'h3d_lrt_poisson': (_I, [_P, _P, _P, _I64, _I, _I, _P, _P, _P,
                                     _P, _P]),
            'h3d_lrt_poisson_dev': (_I, [_P, _P, _P, _I64, _I, _I, _P, _P,
                                         _P, _P, _P]),
            'h3d_mme_per_pixel': (_I, [_P, _P, _P, _I64, _I, _I, _P, _D,
                                       _P]),
            'h3d_lrt_wide': (_I, [_P, _P, _P, _P, _I64, _I, _I, _P, _I, _P,
                                  _P, _P, _P]),
            'h3d_cml': (_I, [_P, _P, _I64, _I, _P]),
            'h3d_disp_tables_dev': (_I, [_P, _P, _I, _I, _I, _D, _D, _P]),
            'h3d_disp_tables_wait': (_I, [_P]),
            'h3d_estimate_disp_dev': (_I, [_P, _P, _P, _P, _I64, _I, _I, _P, _I,
                                           _I, _D, _D, _P, _P, _P]),
            'h3d_lrt_dev_tab': (_I, [_P, _P, _P, _P, _P, _I64, _I, _I, _P, _I,
                                     _I, _P, _P, _P, _P, _P]),
            'h3d_npz_csr_info': (_I, [ctypes.c_char_p, _P, _P, _P]),
            'h3d_npz_backend': (_I, []),
            'h3d_read_text_column': (_I, [ctypes.c_char_p, _P, _I64, _P]),
            'h3d_npz_csr_read_slack': (_I, [ctypes.c_char_p, _I64, _I64, _P,
                                            _P, _P, _I64, _P]),
            'h3d_npz_csr_read': (_I, [ctypes.c_char_p, _I64, _I64, _P, _P, _P,
                                      _P]),
            'h3d_window_gather': (_I, [_P, _P, _P, _P, _P, _I64, _I, _I, _I,
                                       _P, _I, _P, _I64, _I, _I, _I, _I, _D,
                                       _P]),
            'h3d_window_gather_dev': (_I, [_P, _P, _P, _P, _P, _I64, _I, _I,
                                           _I, _P, _I, _P, _I64, _I, _I, _I,
                                           _I, _D, _P]),
            'h3d_stack_aggregate': (_I, [_P, _P, _I64, _I, _I, _P, _P]),
            'h3d_filter_sparse_rows': (_I, [_P, _P, _P, _P, _I, _I64, _I, _I,
                                            _P, _P, _P, _P, _P]),
            'h3d_kr_balance': (_I, [_P, _P, _P, _P, _I, _I64, _I, _I, _D, _D,
                                    _D, _I, _P, _P, _P, _P, _P, _P, _I]),
            'h3d_nb_fit_mu': (_I, [_P, _P, _P, _P, _I64, _I64, _I64, _I, _P,
                                   _P]),
            'h3d_nb_fit_mu_dev': (_I, [_P, _P, _P, _P, _I64, _I64, _I64, _I,
                                       _P, _P]),
            'h3d_nb_equalize': (_I, [_P, _P, _P, _D, _P, _I64, _I, _P, _P,
                                     _P]),
            'h3d_nb_equalize_dev': (_I, [_P, _P, _P, _D, _P, _I64, _I, _P, _P,
                                         _P]),
            'h3d_nb_quantile_map': (_I, [_P, _P, _P, _P, _D, _P, _I64, _P]),
            'h3d_nb_logpmf': (_I, [_P, _P, _P, _P, _I64, _P]),
            'h3d_nb_sample': (_I, [_P, _P, _P, _I64, _U64, _U32, _U32, _I64,
                                   _P, _P, _P]),
            'h3d_nb_sample_dev': (_I, [_P, _P, _P, _I64, _U64, _U32, _U32,
                                       _I64, _P, _P, _P]),
            'h3d_simulate_dev': (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _I,
                                      _I64, _I, _I, _U64, _U32, _I64, _P,
                                      _P]),
            'h3d_group_sums': (_I, [_P, _P, _P, _I64, _I, _I, _P, _P]),
            'h3d_group_sums_dev': (_I, [_P, _P, _P, _I64, _I, _I, _P, _P]),
            'h3d_histogram': (_I, [_P, _P, _I64, _P, _I, _P]),
            'h3d_histogram_dev': (_I, [_P, _P, _I64, _P, _I, _P]),
            'h3d_ma_stats': (_I, [_P, _P, _I64, _I, _I, _P, _I, _I, _P, _P,
                                  _I64, _D, _P, _P, _P, _P]),
            'h3d_density_grid': (_I, [_P, _P, _P, _P, _I64, _I, _P, _I, _P,
                                      _I, _P]),
            'h3d_rank_average': (_I, [_P, _P, _I64, _I, _P, _P]),
            'h3d_corr_matrix': (_I, [_P, _P, _I64, _I, _I, _P]),
            'h3d_pixel_moments': (_I, [_P, _P, _I64, _I, _P, _I, _P, _P]),
            'h3d_balance_pixels': (_I, [_P, _P, _P, _P, _P, _I64, _I, _I,
                                        _P]),
            'h3d_pixel_membership': (_I, [_P, _P, _P, _I64, _P, _P, _I64,
                                          _P]),
            'h3d_pixel_membership_dev': (_I, [_P, _P, _P, _I64, _P, _P, _I64,
                                              _P]),
            'h3d_roc_curve': (_I, [_P, _P, _P, _I64, _I64, _I, _I, _P, _P, _P,
                                   _P, _P, _P, _P, _P]),
            'h3d_roc_curve_dev': (_I, [_P, _P, _P, _I64, _I64, _I, _I, _P, _P,
                                       _P, _P, _P, _P, _P, _P]),
            'h3d_order_stats': (_I, [_P, _P, _I64, _P, _I, _P, _P]),
            'h3d_bin_fractions': (_I, [_P, _P, _P, _I64, _P, _P, _I, _D, _P,
                                       _P]),
            'h3d_label_components': (_I, [_P, _P, _P, _P, _I64, _I, _P, _P,
                                          _P]),
            'h3d_label_components_dev': (_I, [_P, _P, _P, _P, _I64, _I, _P,
                                              _P, _P]),
            'h3d_threshold_classes_dev': (_I, [_P, _P, _I64, _D, _P]),
            'h3d_argmax_classes_dev': (_I, [_P, _P, _I64, _I, _P, _P]),
            'h3d_cluster_lists': (_I, [_P, _P, _P, _P, _P, _I64, _I64, _I64,
                                       _P, _P, _P, _P, _P, _P, _P]),
            'h3d_cluster_lists_dev': (_I, [_P, _P, _P, _P, _P, _I64, _I64,
                                           _I64, _P, _P, _P, _P, _P, _P, _P]),
            'h3d_cluster_stats': (_I, [_P, _P, _P, _P, _I64, _I, _I, _I64,
                                       _I64, _P, _P, _P, _I64, _I, _P, _P, _P,
                                       _P, _P]),
            'h3d_cluster_stats_dev': (_I, [_P, _P, _P, _P, _I64, _I, _I, _I64,
                                           _I64, _P, _P, _P, _I64, _I, _P, _P,
                                           _P, _P, _P]),
        }
        for name, (res, args) in sig.items():
            if name in OPTIONAL and not hasattr(lib, name):
                continue   # an older libh3d (A/B runs against past builds)
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if path is None:
            _lib = lib
        return lib


def _check(rc, what):
    if rc != 0:
        msg = load_library().h3d_last_error().decode(errors='replace')
        raise H3DError('%s: %s (%d: %s)' % (what, msg, rc,
                                            ERRORS.get(rc, '?')), code=rc)


def _wmode(weighted):
    """The smoother's ``weighted`` argument at the ABI: 0 plain lowess, 1
    weighted lowess with the smallest scaled weight pinned to 1 (the
    product's default), 2 (``weighted='reference'``) weighted
    lowess with the reference's own ``w * (1 / w)`` scaling, which floors a
    minimum weight that rounds to 1 - 2^-53 to zero copies
    (lowess.py:183-201)."""
    if isinstance(weighted, str):
        if weighted != 'reference':
            raise ValueError('weighted must be a bool or "reference"')
        return 2
    return int(bool(weighted))


def check_stream(seed, stream=0, rep=0, pixel0=0):
    """The coordinates of the sampling stream (h3d_nb_sample) as Python ints:
    ``seed`` an integer in [0, 2^63), ``stream`` and ``rep`` in [0, 2^32),
    ``pixel0`` in [0, 2^62); ValueError otherwise (bool is not an integer
    here)."""
    out = []
    for name, v, hi in (('seed', seed, 2 ** 63), ('stream', stream, 2 ** 32),
                        ('rep', rep, 2 ** 32), ('pixel0', pixel0, 2 ** 62)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or \
                not 0 <= int(v) < hi:
            raise ValueError('%s must be an integer in [0, 2^%d), got %r'
                             % (name, hi.bit_length() - 1, v))
        out.append(int(v))
    return tuple(out)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


class CSR(object):
    """The three arrays of a CSR matrix as the union kernels take them
    (indptr int64, indices int32, data float64; the attribute names of
    scipy.sparse.csr_matrix)."""

    def __init__(self, indptr, indices, data, shape):
        self.indptr, self.indices, self.data = indptr, indices, data
        self.shape = shape


def read_text_column(path):
    """A one-column text file (a replicate's bias vector) as np.loadtxt
    reads it, parsed by libh3d (h3d_read_text_column) without holding the
    GIL -- prepare_data's reader thread parses the next chromosome's bias
    files while the main thread drives the device, and np.loadtxt held the
    GIL for all of it. None when libh3d does not take the file (anything but
    one decimal number per line, or an older library): the caller reads it
    with np.loadtxt."""
    try:
        lib = load_library()
        size = os.path.getsize(path)
    except (H3DError, OSError):
        return None
    if not hasattr(lib, 'h3d_read_text_column'):
        return None
    cap = size // 2 + 1          # a value takes at least a digit and a newline
    out = np.empty(cap)
    n = ctypes.c_int64(0)
    if lib.h3d_read_text_column(os.fsencode(path), _ptr(out), cap,
                                ctypes.byref(n)) != 0:
        return None
    return out[:n.value]


_NPZ_SLACK = 4096


def load_npz_csr(path, alloc=None):
    """A scipy.sparse.save_npz CSR archive read by libh3d's reader
    (h3d_npz_csr_info / _read; the reference loads it with
    scipy.sparse.load_npz, analysis.py:94,100). Rows whose columns are not
    strictly increasing are canonicalised as scipy's sum_duplicates does.
    Raises H3DError for archives the reader does not take (other sparse
    formats, unsupported dtypes); the caller decides whether to use scipy.
    ``alloc(nbytes)``: the uint8 buffers indices and data are inflated into
    (default numpy; prepare_data passes pinned host memory, so the union's
    uploads of them run at DMA speed)."""
    lib = load_library()
    if not hasattr(lib, 'h3d_npz_csr_read'):
        raise H3DError('libh3d.so predates h3d_npz_csr_read')
    bp = os.fsencode(path)
    n_rows, n_cols, nnz = _I64(0), _I64(0), _I64(0)
    _check(lib.h3d_npz_csr_info(bp, ctypes.byref(n_rows), ctypes.byref(n_cols),
                                ctypes.byref(nnz)), 'h3d_npz_csr_info')
    indptr = np.empty(n_rows.value + 1, dtype=np.int64)
    canon = _I(0)
    # (not for nnz 0: numpy places an empty slice at its base's start)
    if hasattr(lib, 'h3d_npz_csr_read_slack') and nnz.value > 0:
        # _NPZ_SLACK bytes ahead of indices / data: the members are inflated
        # in place, their .npy headers landing in the slack
        mk = alloc or (lambda k: np.empty(k, dtype=np.uint8))
        ib = mk(_NPZ_SLACK + 4 * nnz.value)
        db = mk(_NPZ_SLACK + 8 * nnz.value)
        indices = ib[_NPZ_SLACK:].view(np.int32)
        data = db[_NPZ_SLACK:].view(np.float64)
        _check(lib.h3d_npz_csr_read_slack(
            bp, n_rows.value, nnz.value, _ptr(indptr), _ptr(indices),
            _ptr(data), _NPZ_SLACK, ctypes.byref(canon)),
            'h3d_npz_csr_read_slack')
    else:
        indices = np.empty(nnz.value, dtype=np.int32)
        data = np.empty(nnz.value, dtype=np.float64)
        _check(lib.h3d_npz_csr_read(bp, n_rows.value, nnz.value,
                                    _ptr(indptr), _ptr(indices), _ptr(data),
                                    ctypes.byref(canon)), 'h3d_npz_csr_read')
    shape = (n_rows.value, n_cols.value)
    if canon.value:
        return CSR(indptr, indices, data, shape)
    import scipy.sparse as sparse
    m = sparse.csr_matrix((data, indices, indptr), shape=shape)
    m.sum_duplicates()
    return CSR(_c(m.indptr, np.int64), _c(m.indices, np.int32),
               _c(m.data, np.float64), shape)


class Context(object):
    """One libh3d context bound to one GPU (``h3d_open``)."""

    def __init__(self, device=0):
        self.lib = load_library()
        self.device = device
        h = self.lib.h3d_open(device)
        if not h:
            raise H3DError('h3d_open(%d): %s' % (
                device, self.lib.h3d_last_error().decode(errors='replace')))
        self.handle = h

    def close(self):
        if self.handle:
            self.lib.h3d_close(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle):
        _check(self.lib.h3d_set_stream(self.handle, stream_handle),
               'h3d_set_stream')

    def set_qcml_tol(self, tol):
        """qcml's convergence tolerance for this ctx's later estimate_disp
        calls (h3d_set_qcml_tol; dispersion.py:10's tol, default 1e-4)."""
        _check(self.lib.h3d_set_qcml_tol(self.handle, float(tol)),
               'h3d_set_qcml_tol')

    # -- prepare_data -------------------------------------------------------
    def sparse_union(self, csrs, bias, dist_max, device_alloc=None,
                     host_balanced=True, host_raw=True):
        """csrs: list of canonical CSR matrices (scipy or `CSR`, n_bins x
        n_bins); bias
        (n_bins, R) filtered. Returns row, col (int32), raw (int64 (n, R)),
        balanced (float64 (n, R)). ``device_alloc(n, R)``, when given,
        returns device pointers (row, col, raw int32, balanced; any may be
        None) that also receive the union (h3d_union_fill_dev); with a device
        balanced, ``host_balanced=False`` skips its host copy (balanced is
        then None)."""
        R = len(csrs)
        n_bins = bias.shape[0]
        keep = []
        ip = (ctypes.c_void_p * R)()
        ix = (ctypes.c_void_p * R)()
        dt = (ctypes.c_void_p * R)()
        nnz = np.zeros(R, dtype=np.int64)
        for r, m in enumerate(csrs):
            a = _c(m.indptr, np.int64)
            b = _c(m.indices, np.int32)
            c = _c(m.data, np.float64)
            keep += [a, b, c]
            ip[r], ix[r], dt[r] = a.ctypes.data, b.ctypes.data, c.ctypes.data
            nnz[r] = len(c)
        bias = _c(bias, np.float64)
        n_px = ctypes.c_int64(0)
        _check(self.lib.h3d_union_count(
            self.handle, R, n_bins, ip, ix, dt, _ptr(nnz), _ptr(bias),
            int(dist_max), ctypes.byref(n_px)), 'h3d_union_count')
        n = n_px.value
        row = np.empty(n, dtype=np.int32)
        col = np.empty(n, dtype=np.int32)
        # host_raw=False with a device raw copy: raw is None (fetched from
        # the device copy in the background by the caller)
        raw = np.empty((n, R), dtype=np.int64) \
            if host_raw or device_alloc is None else None
        bal = np.empty((n, R), dtype=np.float64) \
            if host_balanced or device_alloc is None else None
        if device_alloc is None:
            _check(self.lib.h3d_union_fill(self.handle, _ptr(row), _ptr(col),
                                           _ptr(raw), _ptr(bal), n),
                   'h3d_union_fill')
        else:
            d = device_alloc(n, R)
            if bal is None and n and not d[3]:
                raise ValueError('host_balanced=False needs a device balanced')
            if raw is None and n and not d[2]:
                raise ValueError('host_raw=False needs a device raw')
            _check(self.lib.h3d_union_fill_dev(
                self.handle, _ptr(row), _ptr(col), _ptr(raw),
                _ptr(bal) if bal is not None else None, n,
                *[_P(v) if v else None for v in d]), 'h3d_union_fill_dev')
        return row, col, raw, bal

    def size_factors_dev(self, d_balanced, dist, n, R, norm='conditional_mor',
                         n_bins=0, d_sf_out=None, host_out=True):
        """size_factors on a device balanced (n, R); the result on the host
        and, with ``d_sf_out``, in that device buffer ((n, R) or (R,))."""
        if norm not in H3D_NORM:
            raise ValueError('unknown norm %r' % (norm,))
        cond = norm.startswith('conditional')
        dist = _c(dist, np.int32) if cond else None
        # host_out=False (conditional norms with a device copy): no host
        # copy, None is returned (the caller fetches the device one)
        out = np.empty((n, R) if cond else R, dtype=np.float64) \
            if (host_out or not cond or not d_sf_out) else None
        _check(self.lib.h3d_size_factors_dev(
            self.handle, _P(d_balanced), _ptr(dist), n, R, H3D_NORM[norm],
            int(n_bins or 0), _ptr(out), _P(d_sf_out) if d_sf_out else None),
            'h3d_size_factors_dev')
        return out

    def scale_disp_dev(self, d_balanced, d_sf, sf_per_rep, d_row, d_col, n,
                       R, design, mean_thresh, dist_thresh_min,
                       d_flag_out=None, d_scaled_out=None):
        """prepare_data's scaled (n, R) and disp_idx flags (n; 0 / 1, or 2
        where numpy's product decides) on the device (h3d_scale_disp_dev);
        returns the host copies (scaled, flag) -- scaled None when it goes to
        the device buffer ``d_scaled_out`` instead."""
        design = np.ascontiguousarray(design, dtype=np.uint8)
        if design.ndim != 2 or design.shape[0] != R:
            raise ValueError('design must be (R, C)')
        scaled = np.empty((n, R), dtype=np.float64) if not d_scaled_out \
            else None
        flag = np.empty(n, dtype=np.uint8)
        _check(self.lib.h3d_scale_disp_dev(
            self.handle, _P(d_balanced), _P(d_sf), int(bool(sf_per_rep)),
            _P(d_row), _P(d_col), n, R, design.shape[1], _ptr(design),
            float(mean_thresh), int(dist_thresh_min), _ptr(scaled),
            _ptr(flag), _P(d_flag_out) if d_flag_out else None,
            _P(d_scaled_out) if d_scaled_out else None),
            'h3d_scale_disp_dev')
        return scaled, flag

    def disp_pixels_dev(self, d_row, d_col, d_raw, d_sf, sf_per_rep, bias,
                        d_disp_idx, n, R, n_disp, d_raw_out, d_f_out,
                        d_dist_out):
        """A chromosome's disp pixels on the device (h3d_disp_pixels_dev):
        raw (n_disp, R) int32, f = bias[row] * bias[col] * sf, dist."""
        bias = _c(bias, np.float64)
        _check(self.lib.h3d_disp_pixels_dev(
            self.handle, _P(d_row), _P(d_col), _P(d_raw), _P(d_sf),
            int(bool(sf_per_rep)), _ptr(bias), bias.shape[0], _P(d_disp_idx),
            n, R, n_disp, _P(d_raw_out) if d_raw_out else None,
            _P(d_f_out) if d_f_out else None,
            _P(d_dist_out) if d_dist_out else None), 'h3d_disp_pixels_dev')

    def pixel_f_dev(self, d_row, d_dist, d_chrom, d_sfi, n, R, d_bias, d_boff,
                    d_sf, d_soff, nchrom, d_f_out):
        """f of re-sharded pixels from their keys (h3d_pixel_f_dev): device
        pointers in and out, synchronous."""
        _check(self.lib.h3d_pixel_f_dev(
            self.handle, _P(d_row), _P(d_dist), _P(d_chrom), _P(d_sfi), n, R,
            _P(d_bias), _P(d_boff), _P(d_sf), _P(d_soff), nchrom,
            _P(d_f_out)), 'h3d_pixel_f_dev')

    def disp_seg_stats(self, D, C):
        """(qcml iterations, Brent NLL evaluations) per segment (D, C) of
        the last estimate_disp call on this ctx."""
        qi = np.zeros((D, C), dtype=np.int32)
        ev = np.zeros((D, C), dtype=np.int32)
        _check(self.lib.h3d_disp_seg_stats(self.handle, D * C, _ptr(qi),
                                           _ptr(ev)), 'h3d_disp_seg_stats')
        return qi, ev

    def table_gather_dev(self, d_tables, D, C, d_dist, n, d_out):
        """disp = tables[dist] on the device (h3d_table_gather_dev)."""
        _check(self.lib.h3d_table_gather_dev(self.handle, _P(d_tables), D, C,
                                             _P(d_dist), n, _P(d_out)),
               'h3d_table_gather_dev')

    def size_factors_cmor(self, balanced, dist, n_bins):
        balanced = _c(balanced, np.float64)
        dist = _c(dist, np.int32)
        n, R = balanced.shape
        out = np.empty((n, R), dtype=np.float64)
        _check(self.lib.h3d_size_factors_cmor(
            self.handle, _ptr(balanced), _ptr(dist), n, R,
            int(n_bins or 0), _ptr(out)), 'h3d_size_factors_cmor')
        return out

    def size_factors(self, balanced, dist, norm='conditional_mor', n_bins=0):
        """Any norm of util/scaling.py: the conditional ones give (n, R)
        (``n_bins`` equal-number distance bins, 0/None = exact distances),
        the others (R,)."""
        if norm not in H3D_NORM:
            raise ValueError('unknown norm %r' % (norm,))
        balanced = _c(balanced, np.float64)
        n, R = balanced.shape
        cond = norm.startswith('conditional')
        dist = _c(dist, np.int32) if cond else None
        out = np.empty((n, R) if cond else R, dtype=np.float64)
        _check(self.lib.h3d_size_factors(
            self.handle, _ptr(balanced), _ptr(dist), n, R, H3D_NORM[norm],
            int(n_bins or 0), _ptr(out)), 'h3d_size_factors')
        return out

    # -- estimate_disp ------------------------------------------------------
    def disp_per_dist(self, raw, f, dist, cond_of_rep, C, D,
                      estimator='qcml'):
        raw = _c(raw, np.int64)
        f = _c(f, np.float64)
        dist = _c(dist, np.int32)
        cond = _c(cond_of_rep, np.int32)
        n, R = raw.shape
        out = np.empty((D, C), dtype=np.float64)
        flags = np.zeros((D, C), dtype=np.int32)
        _check(self.lib.h3d_disp_per_dist(
            self.handle, _ptr(raw), _ptr(f), _ptr(dist), n, R, C, _ptr(cond),
            D, H3D_EST[estimator], _ptr(out), _ptr(flags)),
            'h3d_disp_per_dist')
        return out

    def disp_per_dist_dev(self, d_raw, d_f, d_dist, n, R, cond_of_rep, C, D,
                          reduce=None):
        """Device-pointer variant; ``reduce(ptr, count)`` all-reduces a device
        buffer of doubles in place (multi-GPU)."""
        cond = _c(cond_of_rep, np.int32)
        out = np.empty((D, C), dtype=np.float64)
        flags = np.zeros((D, C), dtype=np.int32)
        if reduce is not None:
            def _cb(ptr, count, user):
                try:
                    reduce(ctypes.cast(ptr, ctypes.c_void_p).value, count)
                    return 0
                except Exception:  # surfaced as H3D_EHIP by the library
                    return 1
            cb = ALLREDUCE_FN(_cb)
        else:
            cb = ALLREDUCE_FN()
        _check(self.lib.h3d_disp_per_dist_dev(
            self.handle, d_raw, d_f, d_dist, n, R, C, _ptr(cond), D, 0,
            _ptr(out), _ptr(flags), cb, None), 'h3d_disp_per_dist_dev')
        return out

    # -- lrt -----------------------------------------------------------------
    def lrt(self, raw, f, dist, disp_table, cond_of_rep, refit_mu=True,
            want_disp=True):
        """``dist=None``: ``disp_table`` is the per-pixel dispersion (n, C)."""
        raw = _c(raw, np.int64)
        f = _c(f, np.float64)
        dist = _c(dist, np.int32) if dist is not None else None
        tab = _c(disp_table, np.float64)
        cond = _c(cond_of_rep, np.int32)
        n, R = raw.shape
        D, C = tab.shape
        if dist is None:
            if D != n:
                raise ValueError('per-pixel disp must be (n, C)')
            D = 0
        p = np.empty(n)
        llr = np.empty(n)
        mu0 = np.empty(n)
        mu1 = np.empty((n, C))
        disp = np.empty((n, C)) if want_disp else None
        _check(self.lib.h3d_lrt(
            self.handle, _ptr(raw), _ptr(f), _ptr(dist), _ptr(tab), n, R, C,
            _ptr(cond), D, int(bool(refit_mu)), _ptr(p), _ptr(llr), _ptr(mu0),
            _ptr(mu1), _ptr(disp)), 'h3d_lrt')
        return p, llr, mu0, mu1, disp

    def lrt_wide(self, raw, f, disp_wide, cond_of_rep, C, refit_mu=True):
        """lrt.py's own call: per pixel and replicate dispersions (n, R)."""
        raw = _c(raw, np.int64)
        f = _c(f, np.float64)
        dw = _c(disp_wide, np.float64)
        cond = _c(cond_of_rep, np.int32)
        n, R = raw.shape
        if f.shape != (n, R) or dw.shape != (n, R):
            raise ValueError('raw, f and disp must all be (n, R)')
        p, llr, mu0 = np.empty(n), np.empty(n), np.empty(n)
        mu1 = np.empty((n, C))
        _check(self.lib.h3d_lrt_wide(
            self.handle, _ptr(raw), _ptr(f), _ptr(dw), n, R, C, _ptr(cond),
            int(bool(refit_mu)), _ptr(p), _ptr(llr), _ptr(mu0), _ptr(mu1)),
            'h3d_lrt_wide')
        return p, llr, mu0, mu1

    def cml(self, data):
        """cml on (n, r) data already divided by f."""
        data = _c(data, np.float64)
        n, r = data.shape
        out = ctypes.c_double(0)
        _check(self.lib.h3d_cml(self.handle, _ptr(data), n, r,
                                ctypes.byref(out)), 'h3d_cml')
        return out.value

    def bh(self, pvalues):
        """BH q-values on this ctx's GPU (h3d_bh_ctx; same bits as bh())."""
        p = _c(pvalues, np.float64)
        q = np.empty_like(p)
        _check(self.lib.h3d_bh_ctx(self.handle, _ptr(p), len(p), _ptr(q)),
               'h3d_bh_ctx')
        return q

    def bh_dev(self, d_p, n, d_q):
        _check(self.lib.h3d_bh_dev(self.handle, _P(d_p), n, _P(d_q)),
               'h3d_bh_dev')

    # pieces of the rank-sharded BH (parallel.bh_sharded, h3d.h)
    def bh_sort_dev(self, d_p, d_val, n, d_key_out, d_val_out):
        m = ctypes.c_int64(0)
        _check(self.lib.h3d_bh_sort_dev(self.handle, _P(d_p), _P(d_val), n,
                                        _P(d_key_out), _P(d_val_out),
                                        ctypes.byref(m)), 'h3d_bh_sort_dev')
        return m.value

    def bh_scan_dev(self, d_ps, mb, offset, m, d_scanned):
        lo = ctypes.c_double(0)
        _check(self.lib.h3d_bh_scan_dev(self.handle, _P(d_ps), mb, offset, m,
                                        _P(d_scanned), ctypes.byref(lo)),
               'h3d_bh_scan_dev')
        return lo.value

    def bh_finish_dev(self, d_scanned, mb, higher_min, d_q):
        _check(self.lib.h3d_bh_finish_dev(self.handle, _P(d_scanned), mb,
                                          float(higher_min), _P(d_q)),
               'h3d_bh_finish_dev')

    def lrt_dev(self, d_raw, d_f, d_dist, disp_table, n, R, cond_of_rep,
                d_p, d_llr, d_mu0, d_mu1, d_disp=None, refit_mu=True):
        tab = _c(disp_table, np.float64)
        cond = _c(cond_of_rep, np.int32)
        D, C = tab.shape
        _check(self.lib.h3d_lrt_dev(
            self.handle, d_raw, d_f, d_dist, _ptr(tab), n, R, C, _ptr(cond),
            D, int(bool(refit_mu)), d_p, d_llr, d_mu0, d_mu1, d_disp),
            'h3d_lrt_dev')

    def disp_tables_dev(self, d_dpd, D, C, d_tables, weighted=True,
                        frac=None, auto_frac_factor=15.):
        """disp_tables on the GPU: device (D, C) float64 in and out, enqueued
        without waiting (settled by lrt_dev_tab or disp_tables_wait)."""
        _check(self.lib.h3d_disp_tables_dev(
            self.handle, d_dpd, D, C, _wmode(weighted),
            -1.0 if frac is None else float(frac), float(auto_frac_factor),
            d_tables), 'h3d_disp_tables_dev')

    def estimate_disp_dev(self, d_raw, d_f, d_dist, n, R, cond_of_rep, C, D,
                          d_tables, weighted=True, frac=None,
                          auto_frac_factor=15.):
        """disp_per_dist_dev whose smoothed (D, C) tables are computed on
        the device into ``d_tables`` (settled by lrt_dev_tab /
        disp_tables_wait); returns disp_per_dist on the host."""
        cond = _c(cond_of_rep, np.int32)
        out = np.empty((D, C), dtype=np.float64)
        flags = np.zeros((D, C), dtype=np.int32)
        _check(self.lib.h3d_estimate_disp_dev(
            self.handle, d_raw, d_f, d_dist, n, R, C, _ptr(cond), D,
            _wmode(weighted), -1.0 if frac is None else float(frac),
            float(auto_frac_factor), _ptr(out), _ptr(flags), d_tables),
            'h3d_estimate_disp_dev')
        return out

    def disp_tables_wait(self):
        _check(self.lib.h3d_disp_tables_wait(self.handle),
               'h3d_disp_tables_wait')

    def lrt_dev_tab(self, d_raw, d_f, d_dist, d_table, D, n, R, cond_of_rep,
                    d_p, d_llr, d_mu0, d_mu1, d_disp=None, refit_mu=True):
        """lrt_dev with the (D, C) table in device memory."""
        cond = _c(cond_of_rep, np.int32)
        C = int(cond.max()) + 1
        _check(self.lib.h3d_lrt_dev_tab(
            self.handle, d_raw, d_f, d_dist, d_table, n, R, C, _ptr(cond),
            D, int(bool(refit_mu)), d_p, d_llr, d_mu0, d_mu1, d_disp),
            'h3d_lrt_dev_tab')

    # -- scaled NB operators (util/scaled_nb.py) ------------------------------
    @staticmethod
    def _alpha_strides(alpha, n, R):
        """alpha as the four broadcast forms of fit_mu_hat
        (scaled_nb.py:110-127) -> (contiguous values, pixel stride, replicate
        stride), never a materialised (n, R) copy of a smaller form."""
        a = np.asarray(alpha, dtype=np.float64)
        if a.ndim == 0 or a.shape in ((1,), (1, 1)):
            return _c(a.reshape(1), np.float64), 0, 0
        if a.shape in ((R,), (1, R)):
            return _c(a.reshape(R), np.float64), 0, 1
        if a.shape == (n, 1):
            return _c(a.reshape(n), np.float64), 1, 0
        if a.shape == (n, R):
            return _c(a, np.float64), R, 1
        raise ValueError('alpha of shape %s does not broadcast against '
                         '(%d, %d)' % (a.shape, n, R))

    def nb_fit_mu(self, x, b, alpha):
        """fit_mu_hat (scaled_nb.py:71-183) for x, b (n, R) and alpha in any
        of its broadcast forms: (mu (n), flags). A failed pixel's mean is NaN
        and its H3D_FLAG_* bits are in ``flags``."""
        x = _c(x, np.int64)
        b = _c(b, np.float64)
        n, R = x.shape
        if b.shape != (n, R):
            raise ValueError('x and b must both be (n, R)')
        a, spx, srep = self._alpha_strides(alpha, n, R)
        mu = np.empty(n)
        fl = _I(0)
        _check(self.lib.h3d_nb_fit_mu(
            self.handle, _ptr(x), _ptr(b), _ptr(a), spx, srep, n, R, _ptr(mu),
            ctypes.byref(fl)), 'h3d_nb_fit_mu')
        return mu, fl.value

    def nb_fit_mu_dev(self, d_x, d_b, d_alpha, alpha_strides, n, R, d_mu):
        """nb_fit_mu on device pointers (x int32, the rest float64);
        ``alpha_strides`` = (pixel, replicate) element strides of d_alpha,
        each 0 or the natural one. Returns the flags."""
        fl = _I(0)
        _check(self.lib.h3d_nb_fit_mu_dev(
            self.handle, d_x, d_b, d_alpha, alpha_strides[0],
            alpha_strides[1], n, R, d_mu, ctypes.byref(fl)),
            'h3d_nb_fit_mu_dev')
        return fl.value

    def nb_equalize(self, x, f, alpha, want_mu=False):
        """equalize (scaled_nb.py:186-214) for x, f (n, R) at a scalar alpha
        or one per pixel (n,): (pseudodata (n, R), mu_hat (n) or None,
        flags)."""
        x = _c(x, np.int64)
        f = _c(f, np.float64)
        n, R = x.shape
        if f.shape != (n, R):
            raise ValueError('data and f must both be (n, R)')
        a = np.asarray(alpha, dtype=np.float64)
        if a.ndim == 0:
            a_s, a_px = float(a), None
        elif a.shape == (n,):
            a_s, a_px = 0.0, _c(a, np.float64)
        else:
            raise ValueError('alpha must be a scalar or (n,)')
        out = np.empty((n, R))
        mu = np.empty(n) if want_mu else None
        fl = _I(0)
        _check(self.lib.h3d_nb_equalize(
            self.handle, _ptr(x), _ptr(f), a_s, _ptr(a_px), n, R, _ptr(out),
            _ptr(mu), ctypes.byref(fl)), 'h3d_nb_equalize')
        return out, mu, fl.value

    def nb_equalize_dev(self, d_x, d_f, alpha, n, R, d_pseudo, d_alpha_px=None,
                        d_mu_hat=None):
        """nb_equalize on device pointers (x int32, the rest float64); the
        dispersion is ``alpha``, or per pixel from d_alpha_px. Returns the
        flags."""
        fl = _I(0)
        _check(self.lib.h3d_nb_equalize_dev(
            self.handle, d_x, d_f, float(alpha), d_alpha_px, n, R, d_pseudo,
            d_mu_hat, ctypes.byref(fl)), 'h3d_nb_equalize_dev')
        return fl.value

    def nb_quantile_map(self, x, mu_in, mu_out, alpha):
        """q2qnbinom (scaled_nb.py:217-275) over flat float64 arrays of one
        length; alpha a scalar or one per element. ``mu_in`` / ``mu_out`` must
        be contiguous float64 arrays: they are clamped in place, as the
        reference does (:240-242)."""
        x = _c(x, np.float64)
        n = x.size
        for m in (mu_in, mu_out):
            if not (isinstance(m, np.ndarray) and m.dtype == np.float64 and
                    m.flags.c_contiguous and m.flags.writeable and
                    m.size == n):
                raise ValueError('mu_in / mu_out must be writable contiguous '
                                 'float64 arrays of x\'s size')
        a = np.asarray(alpha, dtype=np.float64)
        if a.ndim == 0:
            a_s, a_el = float(a), None
        elif a.size == n:
            a_s, a_el = 0.0, _c(a, np.float64)
        else:
            raise ValueError('alpha must be a scalar or one per element')
        out = np.empty(x.shape)
        _check(self.lib.h3d_nb_quantile_map(
            self.handle, _ptr(x), _ptr(mu_in), _ptr(mu_out), a_s, _ptr(a_el),
            n, _ptr(out)), 'h3d_nb_quantile_map')
        return out

    def nb_logpmf(self, k, m, phi):
        """logpmf (scaled_nb.py:12-33) over float64 arrays of one shape."""
        k = _c(k, np.float64)
        m = _c(m, np.float64)
        phi = _c(phi, np.float64)
        if not (k.shape == m.shape == phi.shape):
            raise ValueError('k, m and phi must have one shape')
        out = np.empty(k.shape)
        _check(self.lib.h3d_nb_logpmf(self.handle, _ptr(k), _ptr(m),
                                      _ptr(phi), k.size, _ptr(out)),
               'h3d_nb_logpmf')
        return out

    # -- negative-binomial sampling (util/simulation.py simulate_gpu) ---------
    def nb_sample(self, bm, disp, seed, stream=0, rep=0, pixel0=0,
                  want_lambda=False):
        """One replicate's negative-binomial draws (h3d_nb_sample) for the
        biased means ``bm`` (n) and dispersions ``disp`` (n): (counts (n)
        int32, the gamma stage's lambda (n) or None, flags). Element i is
        the draw of (seed, stream, rep, pixel0 + i). A bad element's count is
        -1 and sets H3D_FLAG_BADIN (16) in flags."""
        seed, stream, rep, pixel0 = check_stream(seed, stream, rep, pixel0)
        bm = _c(bm, np.float64)
        disp = _c(disp, np.float64)
        if bm.ndim != 1 or disp.shape != bm.shape:
            raise ValueError('bm and disp must both be (n,)')
        counts = np.empty(bm.size, dtype=np.int32)
        lam = np.empty(bm.size) if want_lambda else None
        fl = _I(0)
        _check(self.lib.h3d_nb_sample(
            self.handle, _ptr(bm), _ptr(disp), bm.size, seed, stream, rep,
            pixel0, _ptr(counts), _ptr(lam), ctypes.byref(fl)),
            'h3d_nb_sample')
        return counts, lam, fl.value

    def nb_sample_dev(self, bm, disp, seed, stream=0, rep=0, pixel0=0,
                      want_lambda=False):
        """nb_sample on float64 torch tensors of this ctx's device; counts
        and lambda come back as tensors."""
        import torch
        seed, stream, rep, pixel0 = check_stream(seed, stream, rep, pixel0)
        if bm.dtype != torch.float64 or disp.dtype != torch.float64 or \
                bm.dim() != 1 or disp.shape != bm.shape:
            raise ValueError('bm and disp must both be float64 (n,)')
        bm, disp = bm.contiguous(), disp.contiguous()
        n = bm.numel()
        counts = torch.empty(n, dtype=torch.int32, device=bm.device)
        lam = torch.empty(n, dtype=torch.float64, device=bm.device) \
            if want_lambda else None
        fl = _I(0)
        torch.cuda.current_stream(bm.device).synchronize()
        _check(self.lib.h3d_nb_sample_dev(
            self.handle, _P(bm.data_ptr()), _P(disp.data_ptr()), n, seed,
            stream, rep, pixel0, _P(counts.data_ptr()),
            _P(lam.data_ptr()) if want_lambda else None, ctypes.byref(fl)),
            'h3d_nb_sample_dev')
        return counts, lam, fl.value

    def simulate_dev(self, row, col, mean_a, mean_b, bias, size_factors,
                     table, seed, stream=0, pixel0=0):
        """Every replicate of one chromosome (h3d_simulate_dev) on torch
        tensors of this ctx's device: ``row`` / ``col`` (n) int32, ``mean_a``
        / ``mean_b`` (n), ``bias`` (n_bins, J), ``size_factors`` (J,) or
        (D, J), ``table`` (D,) float64 -> (counts (J, n) int32, flags).
        Replicate j < J // 2 draws from mean_a, the others from mean_b."""
        import torch
        seed, stream, _, pixel0 = check_stream(seed, stream, 0, pixel0)
        n = row.numel()
        f64, i32 = torch.float64, torch.int32
        if row.dtype != i32 or col.dtype != i32 or row.dim() != 1 or \
                col.shape != row.shape:
            raise ValueError('row and col must both be int32 (n,)')
        if any(t.dtype != f64 for t in (mean_a, mean_b, bias, size_factors,
                                        table)):
            raise ValueError('means, bias, size factors and table must be '
                             'float64')
        if mean_a.shape != row.shape or mean_b.shape != row.shape:
            raise ValueError('mean_a and mean_b must be (n,)')
        if bias.dim() != 2 or not 1 <= bias.shape[1] <= 32:
            raise ValueError('bias must be (n_bins, J), 1 <= J <= 32')
        n_bins, J = bias.shape
        if table.dim() != 1 or table.numel() < 1:
            raise ValueError('table must be (D,), D >= 1')
        D = table.numel()
        if tuple(size_factors.shape) == (J,):
            sf_rows = 1
        elif tuple(size_factors.shape) == (D, J):
            sf_rows = D
        else:
            raise ValueError('size_factors must be (J,) or (D, J)')
        row, col, mean_a, mean_b, bias, size_factors, table = (
            t.contiguous() for t in (row, col, mean_a, mean_b, bias,
                                     size_factors, table))
        counts = torch.empty((J, n), dtype=i32, device=row.device)
        fl = _I(0)
        torch.cuda.current_stream(row.device).synchronize()
        _check(self.lib.h3d_simulate_dev(
            self.handle, _P(row.data_ptr()), _P(col.data_ptr()),
            _P(mean_a.data_ptr()), _P(mean_b.data_ptr()),
            _P(bias.data_ptr()), _P(size_factors.data_ptr()), sf_rows,
            _P(table.data_ptr()), D, n, J, n_bins, seed, stream, pixel0,
            _P(counts.data_ptr()), ctypes.byref(fl)), 'h3d_simulate_dev')
        return counts, fl.value

    # -- diagnostics (util/diagnostics.py) -----------------------------------
    def group_sums(self, keys, values, K):
        """(sums (K, C), counts (K) int64) of the rows of ``values`` (n, C)
        grouped by ``keys`` (n) in [0, K); a negative key drops its row
        (h3d_group_sums). The sums have a fixed order."""
        keys = _c(keys, np.int32)
        values = _c(values, np.float64)
        if values.ndim != 2 or keys.shape != (values.shape[0],):
            raise ValueError('values must be (n, C) and keys (n,)')
        n, C = values.shape
        sums = np.empty((K, C), dtype=np.float64)
        counts = np.empty(K, dtype=np.int64)
        _check(self.lib.h3d_group_sums(self.handle, _ptr(keys), _ptr(values),
                                       n, int(K), C, _ptr(sums),
                                       _ptr(counts)), 'h3d_group_sums')
        return sums, counts

    def group_sums_dev(self, keys, values, K):
        """group_sums on torch tensors of this ctx's device: ``keys`` (n)
        int32, ``values`` (n, C) float64; returns tensors (sums, counts)."""
        import torch
        if keys.dtype != torch.int32 or values.dtype != torch.float64 or \
                values.dim() != 2 or tuple(keys.shape) != (values.shape[0],):
            raise ValueError('keys must be int32 (n,), values float64 (n, C)')
        keys, values = keys.contiguous(), values.contiguous()
        n, C = values.shape
        sums = torch.empty((K, C), dtype=torch.float64, device=values.device)
        counts = torch.empty(K, dtype=torch.int64, device=values.device)
        torch.cuda.current_stream(values.device).synchronize()
        _check(self.lib.h3d_group_sums_dev(
            self.handle, _P(keys.data_ptr()), _P(values.data_ptr()), n,
            int(K), C, _P(sums.data_ptr()), _P(counts.data_ptr())),
            'h3d_group_sums_dev')
        return sums, counts

    def histogram(self, values, edges):
        """np.histogram(values, bins=edges)[0] (h3d_histogram)."""
        values = _c(values, np.float64).reshape(-1)
        edges = _c(edges, np.float64)
        counts = np.empty(max(len(edges) - 1, 0), dtype=np.int64)
        _check(self.lib.h3d_histogram(self.handle, _ptr(values), len(values),
                                      _ptr(edges), len(edges), _ptr(counts)),
               'h3d_histogram')
        return counts

    def histogram_dev(self, values, edges):
        """histogram of a float64 torch tensor on this ctx's device; the
        edges stay on the host. Returns an int64 tensor."""
        import torch
        if values.dtype != torch.float64:
            raise ValueError('values must be float64')
        values = values.contiguous().reshape(-1)
        edges = _c(edges, np.float64)
        counts = torch.empty(max(len(edges) - 1, 0), dtype=torch.int64,
                             device=values.device)
        torch.cuda.current_stream(values.device).synchronize()
        _check(self.lib.h3d_histogram_dev(
            self.handle, _P(values.data_ptr()), values.numel(), _ptr(edges),
            len(edges), _P(counts.data_ptr())), 'h3d_histogram_dev')
        return counts

    def ma_stats(self, scaled, cond_of_rep, C, cond0, cond1, qvalues, fdr,
                 loop_idx=None):
        """(mean (n, 2), m, a, label int8) of h3d_ma_stats."""
        scaled = _c(scaled, np.float64)
        cond = _c(cond_of_rep, np.int32)
        q = _c(qvalues, np.float64)
        n, R = scaled.shape
        loop = _c(loop_idx, np.uint8) if loop_idx is not None else None
        mean = np.empty((n, 2))
        m, a = np.empty(n), np.empty(n)
        label = np.empty(n, dtype=np.int8)
        _check(self.lib.h3d_ma_stats(
            self.handle, _ptr(scaled), n, R, int(C), _ptr(cond), int(cond0),
            int(cond1), _ptr(loop), _ptr(q), len(q), float(fdr), _ptr(mean),
            _ptr(m), _ptr(a), _ptr(label)), 'h3d_ma_stats')
        return mean, m, a, label

    def density_grid(self, x, y, label, n_classes, xedges, yedges):
        """counts (L, Ex - 1, Ey - 1) int64 of h3d_density_grid."""
        x, y = _c(x, np.float64), _c(y, np.float64)
        label = _c(label, np.int8)
        xe, ye = _c(xedges, np.float64), _c(yedges, np.float64)
        counts = np.empty((int(n_classes), max(len(xe) - 1, 0),
                           max(len(ye) - 1, 0)), dtype=np.int64)
        _check(self.lib.h3d_density_grid(
            self.handle, _ptr(x), _ptr(y), _ptr(label), len(x),
            int(n_classes), _ptr(xe), len(xe), _ptr(ye), len(ye),
            _ptr(counts)), 'h3d_density_grid')
        return counts

    def rank_average(self, columns):
        """(ranks (R, n), nan flags (R)) of the rows of ``columns`` (R, n)
        (h3d_rank_average)."""
        v = _c(columns, np.float64)
        R, n = v.shape
        ranks = np.empty((R, n))
        flags = np.zeros(R, dtype=np.int32)
        _check(self.lib.h3d_rank_average(self.handle, _ptr(v), n, R,
                                         _ptr(ranks), _ptr(flags)),
               'h3d_rank_average')
        return ranks, flags

    def corr_matrix(self, columns, ranked=False):
        """(R, R) Pearson matrix of the rows of ``columns`` (R, n), of their
        average ranks with ``ranked`` (h3d_corr_matrix)."""
        v = _c(columns, np.float64)
        R, n = v.shape
        out = np.empty((R, R))
        _check(self.lib.h3d_corr_matrix(self.handle, _ptr(v), n, R,
                                        int(bool(ranked)), _ptr(out)),
               'h3d_corr_matrix')
        return out

    def pixel_moments(self, scaled, reps):
        """(mean, var ddof=1) per pixel over the columns ``reps`` of
        ``scaled`` (n, R) (h3d_pixel_moments)."""
        scaled = _c(scaled, np.float64)
        reps = _c(reps, np.int32)
        n, R = scaled.shape
        mean, var = np.empty(n), np.empty(n)
        _check(self.lib.h3d_pixel_moments(self.handle, _ptr(scaled), n, R,
                                          _ptr(reps), len(reps), _ptr(mean),
                                          _ptr(var)), 'h3d_pixel_moments')
        return mean, var

    def balance_pixels(self, row, col, raw, bias):
        """raw / (bias[row] * bias[col]) per replicate (h3d_balance_pixels):
        raw (n, R) integers, bias (n_bins, R)."""
        row, col = _c(row, np.int32), _c(col, np.int32)
        raw = _c(raw, np.int64)
        bias = _c(bias, np.float64)
        n, R = raw.shape
        if bias.ndim != 2 or bias.shape[1] != R or row.shape != (n,) or \
                col.shape != (n,):
            raise ValueError('raw (n, R), bias (n_bins, R), row and col (n,)')
        out = np.empty((n, R))
        _check(self.lib.h3d_balance_pixels(
            self.handle, _ptr(row), _ptr(col), _ptr(raw), _ptr(bias), n, R,
            bias.shape[0], _ptr(out)), 'h3d_balance_pixels')
        return out

    # -- evaluation (util/evaluation.py, util/clusters.py) --------------------
    def pixel_membership(self, row, col, prow, pcol):
        """bool (n): (row[i], col[i]) in the pixel set {(prow, pcol)}
        (h3d_pixel_membership); int64 host arrays."""
        row, col = _c(row, np.int64), _c(col, np.int64)
        prow, pcol = _c(prow, np.int64), _c(pcol, np.int64)
        if row.ndim != 1 or col.shape != row.shape or prow.ndim != 1 or \
                pcol.shape != prow.shape:
            raise ValueError('row, col (n,) and prow, pcol (k,)')
        out = np.zeros(len(row), dtype=np.uint8)
        _check(self.lib.h3d_pixel_membership(
            self.handle, _ptr(row), _ptr(col), len(row), _ptr(prow),
            _ptr(pcol), len(prow), _ptr(out)), 'h3d_pixel_membership')
        return out.view(np.bool_)

    def pixel_membership_dev(self, row, col, prow, pcol):
        """pixel_membership on int64 torch tensors of this ctx's device;
        returns a bool tensor."""
        import torch
        for t in (row, col, prow, pcol):
            if t.dtype != torch.int64 or t.dim() != 1:
                raise ValueError('row, col, prow, pcol must be int64 (n,)')
        if col.shape != row.shape or pcol.shape != prow.shape:
            raise ValueError('row, col (n,) and prow, pcol (k,)')
        row, col = row.contiguous(), col.contiguous()
        prow, pcol = prow.contiguous(), pcol.contiguous()
        out = torch.zeros(row.numel(), dtype=torch.uint8, device=row.device)
        torch.cuda.current_stream(row.device).synchronize()
        _check(self.lib.h3d_pixel_membership_dev(
            self.handle, _P(row.data_ptr()), _P(col.data_ptr()), row.numel(),
            _P(prow.data_ptr()), _P(pcol.data_ptr()), prow.numel(),
            _P(out.data_ptr())), 'h3d_pixel_membership_dev')
        return out.to(torch.bool)

    # -- the calls as connected components (util/clusters.py) -----------------
    def label_components(self, row, col, cls, connectivity=1):
        """(label int32 (n), n_clusters) of h3d_label_components: int64 host
        pixels in (row, col) order, ``cls`` a class byte per pixel (255 = no
        pixel). ValueError where the library reports H3D_FLAG_BADIN."""
        row, col = _c(row, np.int64), _c(col, np.int64)
        cls = _c(cls, np.uint8)
        if row.ndim != 1 or col.shape != row.shape or cls.shape != row.shape:
            raise ValueError('row, col and cls must be (n,)')
        label = np.empty(len(row), dtype=np.int32)
        nc, fl = _I64(0), _I(0)
        _check(self.lib.h3d_label_components(
            self.handle, _ptr(row), _ptr(col), _ptr(cls), len(row),
            int(connectivity), _ptr(label), ctypes.byref(nc),
            ctypes.byref(fl)), 'h3d_label_components')
        if fl.value & H3D_FLAG_BADIN:
            raise ValueError(BAD_PIXELS)
        return label, nc.value

    def label_components_dev(self, row, col, cls, connectivity=1):
        """label_components on torch tensors of this ctx's device (row, col
        int64, cls uint8); returns (int32 label tensor, n_clusters)."""
        import torch
        if row.dtype != torch.int64 or col.dtype != torch.int64 or \
                cls.dtype != torch.uint8:
            raise ValueError('row, col must be int64 and cls uint8')
        if row.dim() != 1 or col.shape != row.shape or cls.shape != row.shape:
            raise ValueError('row, col and cls must be (n,)')
        row, col, cls = row.contiguous(), col.contiguous(), cls.contiguous()
        label = torch.empty(row.numel(), dtype=torch.int32, device=row.device)
        nc, fl = _I64(0), _I(0)
        torch.cuda.current_stream(row.device).synchronize()
        _check(self.lib.h3d_label_components_dev(
            self.handle, _P(row.data_ptr()), _P(col.data_ptr()),
            _P(cls.data_ptr()), row.numel(), int(connectivity),
            _P(label.data_ptr()), ctypes.byref(nc), ctypes.byref(fl)),
            'h3d_label_components_dev')
        if fl.value & H3D_FLAG_BADIN:
            raise ValueError(BAD_PIXELS)
        return label, nc.value

    def threshold_classes_dev(self, q, fdr):
        """uint8 class tensor of float64 q-values on this ctx's device: 0
        where q < fdr, 1 where q >= fdr, 255 for NaN
        (h3d_threshold_classes_dev)."""
        import torch
        if q.dtype != torch.float64 or q.dim() != 1:
            raise ValueError('q must be float64 (n,)')
        q = q.contiguous()
        cls = torch.empty(q.numel(), dtype=torch.uint8, device=q.device)
        torch.cuda.current_stream(q.device).synchronize()
        _check(self.lib.h3d_threshold_classes_dev(
            self.handle, _P(q.data_ptr()), q.numel(), float(fdr),
            _P(cls.data_ptr())), 'h3d_threshold_classes_dev')
        return cls

    def argmax_classes_dev(self, value, member):
        """uint8 class tensor: np.argmax of each row of ``value`` (n, C)
        float64 where ``member`` (n) uint8 / bool is set, 255 elsewhere
        (h3d_argmax_classes_dev)."""
        import torch
        if value.dtype != torch.float64 or value.dim() != 2:
            raise ValueError('value must be float64 (n, C)')
        if member.dtype == torch.bool:
            member = member.to(torch.uint8)
        if member.dtype != torch.uint8 or member.shape != value.shape[:1]:
            raise ValueError('member must be uint8 / bool (n,)')
        check_class_count(value.shape[1])
        value, member = value.contiguous(), member.contiguous()
        n = value.shape[0]
        cls = torch.empty(n, dtype=torch.uint8, device=value.device)
        torch.cuda.current_stream(value.device).synchronize()
        _check(self.lib.h3d_argmax_classes_dev(
            self.handle, _P(value.data_ptr()), n, int(value.shape[1]),
            _P(member.data_ptr()), _P(cls.data_ptr())),
            'h3d_argmax_classes_dev')
        return cls

    CLUSTER_FIELDS = ('size', 'cls_of', 'bounds', 'members', 'starts')

    def cluster_lists(self, label, cls, row, col, n_clusters, min_size=1):
        """dict of CLUSTER_FIELDS of h3d_cluster_lists on host arrays: size
        (n_clusters) int32, cls_of (n_clusters) uint8, bounds (4, n_clusters)
        int32 (min row, max row, min col, max col), and of the clusters with
        size >= min_size members (int32 pixel indices) and starts (int64)."""
        label, cls = _c(label, np.int32), _c(cls, np.uint8)
        row, col = _c(row, np.int64), _c(col, np.int64)
        n, nc = len(label), int(n_clusters)
        if label.ndim != 1 or any(a.shape != label.shape
                                  for a in (cls, row, col)):
            raise ValueError('label, cls, row and col must be (n,)')
        size = np.empty(nc, dtype=np.int32)
        cls_of = np.empty(nc, dtype=np.uint8)
        bounds = np.empty((4, nc), dtype=np.int32)
        members = np.empty(n, dtype=np.int32)
        starts = np.zeros(nc + 1, dtype=np.int64)
        nk, nm = _I64(0), _I64(0)
        _check(self.lib.h3d_cluster_lists(
            self.handle, _ptr(label), _ptr(cls), _ptr(row), _ptr(col), n, nc,
            int(min_size), _ptr(size), _ptr(cls_of), _ptr(bounds),
            _ptr(members), _ptr(starts), ctypes.byref(nk), ctypes.byref(nm)),
            'h3d_cluster_lists')
        return dict(size=size, cls_of=cls_of, bounds=bounds,
                    members=members[:nm.value].copy(),
                    starts=starts[:nk.value + 1].copy())

    def cluster_lists_dev(self, label, cls, row, col, n_clusters, min_size=1):
        """cluster_lists on torch tensors of this ctx's device (label int32,
        cls uint8, row / col int64); returns a dict of tensors."""
        import torch
        if label.dtype != torch.int32 or cls.dtype != torch.uint8 or \
                row.dtype != torch.int64 or col.dtype != torch.int64:
            raise ValueError('label int32, cls uint8, row / col int64')
        if label.dim() != 1 or any(t.shape != label.shape
                                   for t in (cls, row, col)):
            raise ValueError('label, cls, row and col must be (n,)')
        label, cls = label.contiguous(), cls.contiguous()
        row, col = row.contiguous(), col.contiguous()
        n, nc, dev = label.numel(), int(n_clusters), label.device
        size = torch.empty(nc, dtype=torch.int32, device=dev)
        cls_of = torch.empty(nc, dtype=torch.uint8, device=dev)
        bounds = torch.empty((4, nc), dtype=torch.int32, device=dev)
        members = torch.empty(n, dtype=torch.int32, device=dev)
        starts = torch.zeros(nc + 1, dtype=torch.int64, device=dev)
        nk, nm = _I64(0), _I64(0)
        torch.cuda.current_stream(dev).synchronize()
        _check(self.lib.h3d_cluster_lists_dev(
            self.handle, _P(label.data_ptr()), _P(cls.data_ptr()),
            _P(row.data_ptr()), _P(col.data_ptr()), n, nc, int(min_size),
            _P(size.data_ptr()), _P(cls_of.data_ptr()),
            _P(bounds.data_ptr()), _P(members.data_ptr()),
            _P(starts.data_ptr()), ctypes.byref(nk), ctypes.byref(nm)),
            'h3d_cluster_lists_dev')
        return dict(size=size, cls_of=cls_of, bounds=bounds,
                    members=members[:nm.value], starts=starts[:nk.value + 1])

    # -- per-cluster statistics (util/cluster_table.py) -----------------------
    def cluster_stats(self, row, col, data, prow, pcol, starts,
                      reducers=('mean',), sorted=False):
        """dict reducer -> (k, K) float64, plus 'found' (k,) int32, of
        h3d_cluster_stats on host arrays: the table ``row`` / ``col`` /
        ``data`` (n, K) reduced over the pixels ``prow`` / ``pcol``
        [starts[j], starts[j + 1]) of each of the k clusters; an absent pixel
        counts as 0.0. ``sorted`` promises the table in strictly increasing
        (row, col) order. The arguments are checked by
        ``check_cluster_stats``; the library's flags become its exceptions
        (a repeated table pixel or a broken promise: ValueError)."""
        reducers, want = cstat_want(reducers)
        row, col, data, prow, pcol, starts, n_rows, n_cols = \
            check_cluster_stats(row, col, data, prow, pcol, starts)
        k, K = len(starts) - 1, data.shape[1]
        out = {r: np.empty((k, K), dtype=np.float64) for r in reducers}
        found = np.zeros(k, dtype=np.int32)
        fl = _I(0)
        _check(self.lib.h3d_cluster_stats(
            self.handle, _ptr(row), _ptr(col), _ptr(data), len(row), K,
            int(bool(sorted)), n_rows, n_cols, _ptr(prow), _ptr(pcol),
            _ptr(starts), k, want, _ptr(out.get('mean')),
            _ptr(out.get('max')), _ptr(out.get('min')), _ptr(found),
            ctypes.byref(fl)), 'h3d_cluster_stats')
        cstat_raise(fl.value)
        out['found'] = found
        return out

    def cluster_stats_dev(self, row, col, data, n_rows, n_cols, prow, pcol,
                          starts, reducers=('mean',), sorted=False,
                          check=True):
        """cluster_stats on torch tensors of this ctx's device (row, col,
        prow, pcol, starts int64; data (n, K) float64); ``n_rows`` /
        ``n_cols`` bound the cluster pixels. Returns a dict of tensors.
        ``check=False`` returns the library's flag word under 'flags'
        instead of raising."""
        import torch
        reducers, want = cstat_want(reducers)
        for t in (row, col, prow, pcol, starts):
            if t.dtype != torch.int64 or t.dim() != 1:
                raise ValueError('row, col, prow, pcol and starts must be '
                                 'int64 with 1 dimension')
        if data.dtype != torch.float64 or data.dim() != 2:
            raise ValueError('data must be float64 (n, K)')
        if col.shape != row.shape or data.shape[0] != row.shape[0] or \
                pcol.shape != prow.shape or starts.numel() < 1:
            raise ValueError('row, col, data (n,) and prow, pcol (p,)')
        K = int(data.shape[1])
        if not 1 <= K <= CSTAT_MAX_K:
            raise ValueError('between 1 and %d data columns, got %d'
                             % (CSTAT_MAX_K, K))
        row, col, data = row.contiguous(), col.contiguous(), data.contiguous()
        prow, pcol = prow.contiguous(), pcol.contiguous()
        starts = starts.contiguous()
        k, dev = starts.numel() - 1, row.device
        # the library reads prow / pcol up to starts[k]
        if k and int(starts[-1]) > prow.numel():
            raise ValueError('starts ends beyond the cluster pixels')
        out = {r: torch.empty((k, K), dtype=torch.float64, device=dev)
               for r in reducers}
        found = torch.zeros(k, dtype=torch.int32, device=dev)

        def p(t):
            return _P(t.data_ptr()) if t is not None else None
        fl = _I(0)
        torch.cuda.current_stream(dev).synchronize()
        _check(self.lib.h3d_cluster_stats_dev(
            self.handle, p(row), p(col), p(data), row.numel(), K,
            int(bool(sorted)), int(n_rows), int(n_cols), p(prow), p(pcol),
            p(starts), k, want, p(out.get('mean')), p(out.get('max')),
            p(out.get('min')), p(found), ctypes.byref(fl)),
            'h3d_cluster_stats_dev')
        if check:
            cstat_raise(fl.value)
        else:
            out['flags'] = fl.value
        out['found'] = found
        return out

    ROC_FIELDS = ('fdr', 'fpr', 'tpr', 'thresh', 'fps', 'tps')

    def roc_curve(self, labels, scores, n_fdr_points=100,
                  drop_intermediate=True, complement=False):
        """(dict of ROC_FIELDS -> (m,) arrays, flags) of h3d_roc_curve:
        ``labels`` (n) bool / bytes, ``scores`` (n) float64; ``complement``:
        the score is ``1 - scores``, formed on the device. flags has
        H3D_FLAG_BADIN (16) when a score is NaN."""
        labels = _c(labels, np.uint8)
        scores = _c(scores, np.float64)
        if labels.ndim != 1 or scores.shape != labels.shape:
            raise ValueError('labels and scores must be (n,)')
        n = len(labels)
        out = [np.empty(n + 1, dtype=np.float64) for _ in range(4)] + \
            [np.empty(n + 1, dtype=np.int64) for _ in range(2)]
        m, fl = _I64(0), _I(0)
        _check(self.lib.h3d_roc_curve(
            self.handle, _ptr(labels), _ptr(scores), n, int(n_fdr_points),
            int(bool(drop_intermediate)), int(bool(complement)),
            *([_ptr(a) for a in out] + [ctypes.byref(m), ctypes.byref(fl)])),
            'h3d_roc_curve')
        return (dict((k, a[:m.value].copy())
                     for k, a in zip(self.ROC_FIELDS, out)), fl.value)

    def roc_curve_dev(self, labels, scores, n_fdr_points=100,
                      drop_intermediate=True, complement=False):
        """roc_curve on torch tensors of this ctx's device: ``labels`` (n)
        uint8 or bool, ``scores`` (n) float64; the dict holds tensors."""
        import torch
        if labels.dtype == torch.bool:
            labels = labels.to(torch.uint8)
        if labels.dtype != torch.uint8 or scores.dtype != torch.float64 or \
                labels.dim() != 1 or scores.shape != labels.shape:
            raise ValueError('labels must be uint8 / bool (n,), scores '
                             'float64 (n,)')
        labels, scores = labels.contiguous(), scores.contiguous()
        n = labels.numel()
        out = [torch.empty(n + 1, dtype=torch.float64, device=scores.device)
               for _ in range(4)] + \
            [torch.empty(n + 1, dtype=torch.int64, device=scores.device)
             for _ in range(2)]
        m, fl = _I64(0), _I(0)
        torch.cuda.current_stream(scores.device).synchronize()
        _check(self.lib.h3d_roc_curve_dev(
            self.handle, _P(labels.data_ptr()), _P(scores.data_ptr()), n,
            int(n_fdr_points), int(bool(drop_intermediate)),
            int(bool(complement)),
            *([_P(a.data_ptr()) for a in out] +
              [ctypes.byref(m), ctypes.byref(fl)])), 'h3d_roc_curve_dev')
        return (dict((k, a[:m.value].clone())
                     for k, a in zip(self.ROC_FIELDS, out)), fl.value)

    def order_stats(self, values, ranks):
        """(the values at the 0-based ``ranks`` of ``values`` sorted
        ascending, NaN last; the NaN count) of h3d_order_stats."""
        values = _c(values, np.float64).reshape(-1)
        ranks = _c(ranks, np.int64).reshape(-1)
        out = np.empty(len(ranks), dtype=np.float64)
        nan = _I64(0)
        _check(self.lib.h3d_order_stats(
            self.handle, _ptr(values), len(values), _ptr(ranks), len(ranks),
            _ptr(out), ctypes.byref(nan)), 'h3d_order_stats')
        return out, nan.value

    def bin_fractions(self, p, dist, lo, hi, p_star):
        """(members, below) int64 (B) of h3d_bin_fractions: per inclusive
        range [lo[b], hi[b]] of ``dist`` the pixels, and those of them with
        ``p < p_star``."""
        p = _c(p, np.float64)
        dist = _c(dist, np.int64)
        lo, hi = _c(lo, np.int64), _c(hi, np.int64)
        if p.ndim != 1 or dist.shape != p.shape or lo.ndim != 1 or \
                hi.shape != lo.shape:
            raise ValueError('p, dist (n,) and lo, hi (B,)')
        members = np.zeros(len(lo), dtype=np.int64)
        below = np.zeros(len(lo), dtype=np.int64)
        _check(self.lib.h3d_bin_fractions(
            self.handle, _ptr(p), _ptr(dist), len(p), _ptr(lo), _ptr(hi),
            len(lo), float(p_star), _ptr(members), _ptr(below)),
            'h3d_bin_fractions')
        return members, below

    # -- alternative models (analysis/alternatives.py) -----------------------
    def lrt_poisson(self, raw, f, cond_of_rep, C):
        """Poisson LRT (alternatives.py:25-42, refit_mu=True): p, llr,
        mu_hat_null (n,), mu_hat_alt (n, C)."""
        raw = _c(raw, np.int64)
        f = _c(f, np.float64)
        cond = _c(cond_of_rep, np.int32)
        n, R = raw.shape
        p = np.empty(n)
        llr = np.empty(n)
        mu0 = np.empty(n)
        mu1 = np.empty((n, C))
        _check(self.lib.h3d_lrt_poisson(
            self.handle, _ptr(raw), _ptr(f), n, R, C, _ptr(cond), _ptr(p),
            _ptr(llr), _ptr(mu0), _ptr(mu1)), 'h3d_lrt_poisson')
        return p, llr, mu0, mu1

    def lrt_poisson_dev(self, d_raw, d_f, n, R, cond_of_rep, C, d_p, d_llr,
                        d_mu0, d_mu1):
        cond = _c(cond_of_rep, np.int32)
        _check(self.lib.h3d_lrt_poisson_dev(
            self.handle, d_raw, d_f, n, R, C, _ptr(cond), d_p, d_llr, d_mu0,
            d_mu1), 'h3d_lrt_poisson_dev')

    def mme_per_pixel(self, data, f, cond_of_rep, C, min_disp=-np.inf):
        """Per-pixel MME dispersion of each condition (dispersion.py:83-104)
        floored at ``min_disp`` (NaN stays NaN): (n, C)."""
        data = _c(data, np.float64)
        f = _c(f, np.float64) if f is not None else None
        cond = _c(cond_of_rep, np.int32)
        n, R = data.shape
        out = np.empty((n, C))
        _check(self.lib.h3d_mme_per_pixel(
            self.handle, _ptr(data), _ptr(f), n, R, C, _ptr(cond),
            float(min_disp), _ptr(out)), 'h3d_mme_per_pixel')
        return out

    # -- dense views (get_matrix / select_matrix / APA) ----------------------
    def window_gather(self, indices, data, origins, h, w, shape, indptr=None,
                      row=None, cols=None, symmetrize=False, mean=False,
                      fill=np.nan):
        """W dense h x w windows of a CSR matrix ``shape`` = (n_rows, n_cols)
        in one launch (h3d_window_gather): ``indices`` (nnz), ``data`` (nnz,)
        or (nnz, ld), and either ``indptr`` or the sorted ``row`` (nnz) of a
        lexsorted table; ``origins`` (W, 2) int32 window corners (a row0 of
        INT32_MIN: an all-NaN window); ``cols`` the data columns taken
        (default: all). Returns (K, W, h, w), or (W, h, w) with ``mean``."""
        if (indptr is None) == (row is None):
            raise ValueError('pass exactly one of indptr and row')
        indices = _c(indices, np.int32)
        data = _c(data, np.float64)
        if data.ndim == 1:
            data = data.reshape(-1, 1)
        nnz, ld = data.shape
        if data.ndim != 2 or len(indices) != nnz:
            raise ValueError('data must be (nnz,) or (nnz, ld), indices (nnz,)')
        n_rows, n_cols = int(shape[0]), int(shape[1])
        if indptr is not None:
            indptr = _c(indptr, np.int64)
            if len(indptr) != n_rows + 1:
                raise ValueError('indptr must have n_rows + 1 entries')
        else:
            row = _c(row, np.int32)
            if len(row) != nnz:
                raise ValueError('row must have nnz entries')
        cols = _c(np.arange(ld) if cols is None else cols, np.int32)
        origins = _c(origins, np.int32).reshape(-1, 2)
        W, K = len(origins), len(cols)
        # (an output the library refuses for its size is not allocated)
        out = np.empty((W, h, w) if mean else (K, W, h, w), dtype=np.float64) \
            if K * W * int(h) * int(w) < 2 ** 31 else None
        _check(self.lib.h3d_window_gather(
            self.handle, _ptr(indptr), _ptr(row), _ptr(indices), _ptr(data),
            nnz, ld, n_rows, n_cols, _ptr(cols), K, _ptr(origins), W, int(h),
            int(w), int(bool(symmetrize)), int(bool(mean)), float(fill),
            _ptr(out)), 'h3d_window_gather')
        return out

    def window_gather_dev(self, d_indices, d_data, nnz, ld, shape, cols,
                          d_origins, W, h, w, d_out, d_indptr=None,
                          d_row=None, symmetrize=False, mean=False,
                          fill=np.nan):
        """window_gather on device buffers (h3d_window_gather_dev); ``cols``
        stays on the host. Synchronous."""
        cols = _c(cols, np.int32)
        _check(self.lib.h3d_window_gather_dev(
            self.handle, _P(d_indptr) if d_indptr else None,
            _P(d_row) if d_row else None, _P(d_indices), _P(d_data), nnz, ld,
            int(shape[0]), int(shape[1]), _ptr(cols), len(cols),
            _P(d_origins), W, int(h), int(w), int(bool(symmetrize)),
            int(bool(mean)), float(fill), _P(d_out)),
            'h3d_window_gather_dev')

    def stack_aggregate(self, stack):
        """(count int64, sum float64), each (h, w): per cell of a stack
        (W, h, w) the windows that are not NaN there and their sum, in a
        fixed order (h3d_stack_aggregate)."""
        stack = _c(stack, np.float64)
        if stack.ndim != 3:
            raise ValueError('stack must be (W, h, w)')
        W, h, w = stack.shape
        count = np.empty((h, w), dtype=np.int64)
        total = np.empty((h, w), dtype=np.float64)
        _check(self.lib.h3d_stack_aggregate(self.handle, _ptr(stack), W, h, w,
                                            _ptr(count), _ptr(total)),
               'h3d_stack_aggregate')
        return count, total

    # -- sparse-bin filter and KR balancing ----------------------------------
    @staticmethod
    def _csr_args(indptr, indices, data, n):
        indptr = _c(indptr, np.int64)
        indices = _c(indices, np.int32)
        data = _c(data, np.float64)
        if len(indptr) != n + 1 or len(indices) != len(data):
            raise ValueError('indptr must have n + 1 entries, indices and '
                             'data one per stored entry')
        return indptr, indices, data

    def filter_sparse_rows(self, indptr, indices, data, n, min_nnz=25, k=300):
        """filter_sparse_rows_count on a square CSR matrix of ``n`` bins
        (h3d_filter_sparse_rows): (indptr, indices, data) of the kept entries
        and the number of wiped bins."""
        indptr, indices, data = self._csr_args(indptr, indices, data, n)
        nnz = len(data)
        out_indptr = np.empty(n + 1, dtype=np.int64)
        out_indices = np.empty(nnz, dtype=np.int32)
        out_data = np.empty(nnz, dtype=np.float64)
        kept, wiped = _I64(0), _I64(0)
        _check(self.lib.h3d_filter_sparse_rows(
            self.handle, _ptr(indptr), _ptr(indices), _ptr(data), n, nnz,
            min(int(min_nnz), _INT_MAX), min(int(k), _INT_MAX),
            _ptr(out_indptr), _ptr(out_indices),
            _ptr(out_data), ctypes.byref(kept), ctypes.byref(wiped)),
            'h3d_filter_sparse_rows')
        return (out_indptr, out_indices[:kept.value].copy(),
                out_data[:kept.value].copy(), wiped.value)

    KR_STATS = ('outer', 'inner', 'low_clamps', 'high_clamps', 'wiped',
                'rows')

    def kr_balance(self, indptr, indices, data, n, min_nnz=0, k=0, tol=1e-6,
                   lo=0.1, hi=3, max_iter=3000, x0=None, balanced=False):
        """The sparse-bin filter (skipped at ``min_nnz`` or ``k`` 0) and the
        Knight-Ruiz balancing of an upper-triangular canonical CSR matrix in
        one device pass (h3d_kr_balance). ``x0``: (n,) start vector by bin,
        or None; ``max_iter`` None: no cap. Returns a dict: ``bias`` (n,),
        ``balanced`` (nnz,) the balanced value of every input entry (None
        unless asked for), ``stats`` (KR_STATS -> int), ``inner`` / ``norms``
        the inner steps and residual norm of every outer step."""
        indptr, indices, data = self._csr_args(indptr, indices, data, n)
        nnz = len(data)
        if x0 is not None:
            x0 = _c(x0, np.float64)
            if x0.shape != (n,):
                raise ValueError('x0 must have one value per bin')
        # (the library stops after 10,000 inner steps, so outer steps too)
        cap = 10002 if max_iter is None else min(max(int(max_iter), 0) + 2,
                                                  10002)
        bias = np.empty(n, dtype=np.float64)
        bal = np.empty(nnz, dtype=np.float64) if balanced else None
        stats = np.zeros(6, dtype=np.int64)
        inner = np.zeros(cap, dtype=np.int32)
        norms = np.zeros(cap, dtype=np.float64)
        _check(self.lib.h3d_kr_balance(
            self.handle, _ptr(indptr), _ptr(indices), _ptr(data), n, nnz,
            min(int(min_nnz), _INT_MAX), min(int(k), _INT_MAX), float(tol),
            float(lo), float(hi),
            -1 if max_iter is None else min(int(max_iter), _INT_MAX),
            _ptr(x0), _ptr(bias),
            _ptr(bal), _ptr(stats), _ptr(inner), _ptr(norms), cap),
            'h3d_kr_balance')
        m = min(int(stats[0]), cap)
        return dict(bias=bias, balanced=bal,
                    stats=dict(zip(self.KR_STATS, (int(v) for v in stats))),
                    inner=inner[:m].copy(), norms=norms[:m].copy())

    # -- measurement ---------------------------------------------------------
    def profile(self, on=True, level=2):
        """HIP-event timing on the ctx stream: level 1 = the roofline
        kernels only (disp_work, lrt), 2 = every kernel scope."""
        _check(self.lib.h3d_profile_enable(self.handle,
                                           int(level) if on else 0),
               'h3d_profile_enable')

    def profile_reset(self):
        _check(self.lib.h3d_profile_reset(self.handle), 'h3d_profile_reset')

    def profile_read(self, name):
        ms = ctypes.c_double(0)
        n = ctypes.c_int64(0)
        u = ctypes.c_int64(0)
        _check(self.lib.h3d_profile_read(self.handle, name.encode(),
                                         ctypes.byref(ms), ctypes.byref(n),
                                         ctypes.byref(u)), 'h3d_profile_read')
        return ms.value, n.value, u.value


def disp_table(disp_per_dist_col, weighted=True, frac=None,
               auto_frac_factor=15.):
    """Host-side smoother (libh3d, C++): the fitted dispersion function
    tabulated at every integer distance."""
    lib = load_library()
    col = _c(disp_per_dist_col, np.float64)
    out = np.empty(len(col))
    _check(lib.h3d_disp_table(_ptr(col), len(col), _wmode(weighted),
                              -1.0 if frac is None else float(frac),
                              float(auto_frac_factor), _ptr(out)),
           'h3d_disp_table')
    return out


def disp_tables(disp_per_dist, weighted=True, frac=None, auto_frac_factor=15.):
    """disp_table for every column of ``disp_per_dist`` (D, C), the
    conditions smoothed on concurrent threads inside libh3d (one call)."""
    lib = load_library()
    d = _c(disp_per_dist, np.float64)
    D, C = d.shape
    if not hasattr(lib, 'h3d_disp_tables'):
        return np.stack([disp_table(d[:, c], weighted, frac, auto_frac_factor)
                         for c in range(C)], axis=1)
    out = np.empty((D, C))
    _check(lib.h3d_disp_tables(_ptr(d), D, C, _wmode(weighted),
                               -1.0 if frac is None else float(frac),
                               float(auto_frac_factor), _ptr(out)),
           'h3d_disp_tables')
    return out


def bh(pvalues):
    lib = load_library()
    p = _c(pvalues, np.float64)
    q = np.empty_like(p)
    _check(lib.h3d_bh(_ptr(p), len(p), _ptr(q)), 'h3d_bh')
    return q


def cluster_labels(row, col, connectivity=1):
    """Cluster index of every pixel, clusters numbered in the reference's
    get_groups() order (libh3d host code, clusters.py:73-97)."""
    lib = load_library()
    r = _c(row, np.int64)
    c = _c(col, np.int64)
    lab = np.empty(len(r), dtype=np.int64)
    nc = ctypes.c_int64(0)
    _check(lib.h3d_find_clusters(_ptr(r), _ptr(c), len(r), int(connectivity),
                                 _ptr(lab), ctypes.byref(nc)),
           'h3d_find_clusters')
    return lab, nc.value


def cluster_order(row, col, connectivity=1):
    """(labels, n_clusters, order): cluster_labels plus the pixel indices
    cluster by cluster, each cluster in the iteration order of the
    reference's Python set (h3d_find_clusters_ordered). Pixels distinct."""
    lib = load_library()
    r = _c(row, np.int64)
    c = _c(col, np.int64)
    lab = np.empty(len(r), dtype=np.int64)
    order = np.empty(len(r), dtype=np.int64)
    nc = ctypes.c_int64(0)
    _check(lib.h3d_find_clusters_ordered(
        _ptr(r), _ptr(c), len(r), int(connectivity), _ptr(lab),
        ctypes.byref(nc), _ptr(order)), 'h3d_find_clusters_ordered')
    return lab, nc.value, order


def format_clusters(row, col, members, starts):
    """Text "[[i, j], ...]" of each cluster -> (bytes, end offsets)."""
    lib = load_library()
    r = _c(row, np.int64)
    c = _c(col, np.int64)
    m = _c(members, np.int64)
    s = _c(starts, np.int64)
    k = len(s) - 1
    ln = ctypes.c_int64(0)
    _check(lib.h3d_format_clusters(_ptr(r), _ptr(c), _ptr(m), _ptr(s), k,
                                   None, 0, None, ctypes.byref(ln)),
           'h3d_format_clusters')
    buf = ctypes.create_string_buffer(max(ln.value, 1))
    ends = np.empty(k, dtype=np.int64)
    _check(lib.h3d_format_clusters(_ptr(r), _ptr(c), _ptr(m), _ptr(s), k,
                                   buf, ln.value, _ptr(ends),
                                   ctypes.byref(ln)), 'h3d_format_clusters')
    return buf.raw[:ln.value], ends


_ctx = {}


def context(device=None):
    """Process-wide context for ``device`` (default: LOCAL_RANK or 0)."""
    if device is None:
        device = int(os.environ.get('LOCAL_RANK', '0'))
    with _lock:
        if device not in _ctx:
            _ctx[device] = Context(device)
        return _ctx[device]
