"""The numbers under the reference's QC figures, as plain functions on arrays.

The reference's ``plotting/*.py`` modules reduce over every pixel and then
draw; these functions do the reduction on the GPU (csrc/h3d_diag.hip) and
return the arrays, which the caller draws -- with matplotlib directly or by
handing them to the reference's own plotters.

- ``dd_curves(row, col, before, after)``: distance-dependence curves,
  plotting/distance_dependence.py:34-43;
- ``value_histogram(values, edges)``: plotting/histograms.py's ``plt.hist``;
- ``ma_stats(scaled, design, conds, qvalues, fdr, loop_idx)``:
  analysis/plotting.py:307 and plotting/ma.py:71-72, :131-155;
- ``density_grid(x, y, label, n_classes, xedges, yedges)``: the point cloud of
  plotting/ma.py as per-class 2-D counts;
- ``correlation_matrix(data, correlation)``: scipy.stats.spearmanr / pearsonr
  over the replicate pairs (analysis/plotting.py:369-376);
- ``mvr_data(scaled_cond, dist, disp_fit, disp_per_dist)``: the per-pixel and
  per-distance quantities of plotting/dispersion.py:133-183;
- ``distance_bias(pvalues, dist, bins, threshold)``: the percentile and the
  per-range shares of plotting/distance_bias.py:101-112 (csrc/h3d_eval.hip).

Every floating-point sum has a fixed order: a rerun gives the same bits.
There is no CPU fallback: without libh3d.so or a gfx950 device the functions
raise ``H3DError``. Shapes, dtypes and ranges are checked before anything is
uploaded.
"""
import numpy as np

from hic3defdr_amd import _native

MAX_REPS = 32       # columns of correlation_matrix / replicates per pixel
MAX_EDGES = 4097    # bin edges per axis
MAX_KEYS = 4096     # groups of one group_sums call
MAX_COLS = 64       # value columns of one group_sums call
_DD_TOP = 101       # np.digitize(..., np.linspace(0, 1000, 101)) beyond 1000


def _floats(a, ndim, what):
    a = np.asarray(a)
    if a.dtype.kind not in 'fiub':
        raise TypeError('%s must be numeric, not %s' % (what, a.dtype))
    if a.ndim != ndim:
        raise ValueError('%s must have %d dimension%s, not %d'
                         % (what, ndim, '' if ndim == 1 else 's', a.ndim))
    return np.ascontiguousarray(a, dtype=np.float64)


def _ints(a, what):
    a = np.asarray(a)
    if a.dtype.kind not in 'iu':
        raise TypeError('%s must be integers, not %s' % (what, a.dtype))
    if a.ndim != 1:
        raise ValueError('%s must have 1 dimension, not %d' % (what, a.ndim))
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError('%s must fit 32 bits' % what)
    return a


def _edges(e, what='edges'):
    e = _floats(e, 1, what)
    if len(e) < 2:
        raise ValueError('%s: at least two edges' % what)
    if len(e) > MAX_EDGES:
        raise ValueError('%s: at most %d edges, not %d'
                         % (what, MAX_EDGES, len(e)))
    if not np.all(np.isfinite(e)):
        raise ValueError('%s must be finite' % what)
    if not np.all(e[1:] > e[:-1]):
        raise ValueError('%s must increase strictly' % what)
    return e


def dd_bins(dist):
    """``np.digitize(dist, np.linspace(0, 1000, 101), right=True)`` for
    integer distances (distance_dependence.py:36): ceil(d / 10), 101 beyond
    1000, 0 for the diagonal and below."""
    d = np.asarray(dist, dtype=np.int64)
    return np.where(d <= 0, 0, np.minimum((d + 9) // 10, _DD_TOP))


def dd_curves(row, col, before, after):
    """plotting/distance_dependence.py:34-43: ``(bs, before_means,
    after_means)``, the means (bins, R). Bin b collects the pixels with
    ``dd_bins(col - row) == b`` (the diagonal, bin 0, is dropped);
    ``bs = 1 .. max bin``; ``means[b] = sums[b] / float(n - b)`` with
    ``n = max(row.max(), col.max()) + 1``; a bin without pixels gives 0."""
    row, col = _ints(row, 'row'), _ints(col, 'col')
    before, after = _floats(before, 2, 'before'), _floats(after, 2, 'after')
    n_px, R = before.shape
    if after.shape != (n_px, R) or row.shape != (n_px,) or \
            col.shape != (n_px,):
        raise ValueError('row, col (n,) and before, after (n, R) must agree')
    if not 1 <= 2 * R <= MAX_COLS:
        raise ValueError('between 1 and %d replicates, not %d'
                         % (MAX_COLS // 2, R))
    if n_px == 0:
        return (np.arange(1, 1), np.empty((0, R)), np.empty((0, R)))
    bins = dd_bins(col.astype(np.int64) - row)
    top = int(bins.max())
    bs = np.arange(1, top + 1)
    n = int(max(row.max(), col.max())) + 1
    keys = np.where(bins > 0, bins, -1).astype(np.int32)
    sums, _ = _native.context().group_sums(
        keys, np.concatenate([before, after], axis=1), _DD_TOP + 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        means = sums[1:top + 1] / (n - bs).astype(np.float64)[:, None]
    return bs, means[:, :R].copy(), means[:, R:].copy()


def value_histogram(values, edges=None):
    """``np.histogram(values, bins=edges)`` -> ``(counts, edges)``
    (plotting/histograms.py draws ``plt.hist`` of the p- or q-values);
    ``edges`` defaults to ``np.linspace(0, 1, 21)``. NaN and values outside
    the edges are dropped; the last bin is closed on the right."""
    edges = _edges(np.linspace(0, 1, 21) if edges is None else edges)
    values = _floats(values, 1, 'values')
    return _native.context().histogram(values, edges), edges


def _conditions(design, conds):
    """(cond_of_rep int32, C, the two condition indices)."""
    names = None
    if hasattr(design, 'columns'):
        names = list(design.columns)
    d = np.asarray(design, dtype=bool)
    if d.ndim != 2:
        raise ValueError('design must be (replicates, conditions)')
    if not np.all(d.sum(axis=1) == 1):
        raise ValueError('every replicate must belong to exactly one '
                         'condition')
    if d.shape[0] > MAX_REPS:
        raise ValueError('at most %d replicates, not %d'
                         % (MAX_REPS, d.shape[0]))
    if conds is None:
        conds = (names if names is not None else list(range(d.shape[1])))[:2]
    conds = list(conds)
    if len(conds) != 2:
        raise ValueError('conds must name two conditions')
    idx = []
    for c in conds:
        if names is not None:
            if c not in names:
                raise ValueError('condition %r is not in the design %r'
                                 % (c, names))
            idx.append(names.index(c))
        else:
            if not isinstance(c, (int, np.integer)) or \
                    not 0 <= c < d.shape[1]:
                raise ValueError('condition %r is not in the design' % (c,))
            idx.append(int(c))
    for i in idx:
        if not d[:, i].any():
            raise ValueError('condition %r has no replicate' % (i,))
    return d.argmax(axis=1).astype(np.int32), d.shape[1], idx


def ma_stats(scaled, design, conds, qvalues, fdr, loop_idx=None):
    """The MA plot's numbers. ``scaled`` (n, R): the disp pixels; ``design``
    a boolean (replicates x conditions) DataFrame or array; ``conds`` two
    condition names (indices for an array design; None: the first two);
    ``qvalues`` one per loop pixel in order; ``loop_idx`` (n,) bool, or None
    when every pixel is a loop pixel. Returns a dict: ``mean`` (n, 2)
    (analysis/plotting.py:307), ``m``, ``a`` (plotting/ma.py:71-72) and
    ``label`` (n,) int8: 0 non-loop, 1 loop and not significant
    (``!(q < fdr)``), 2 significant with m > 0, 3 significant with m < 0, -1
    significant with m == 0 or NaN (the reference draws those in no series,
    ma.py:146-155)."""
    scaled = _floats(scaled, 2, 'scaled')
    n, R = scaled.shape
    cond_of_rep, C, idx = _conditions(design, conds)
    if len(cond_of_rep) != R:
        raise ValueError('scaled has %d columns, the design %d replicates'
                         % (R, len(cond_of_rep)))
    qvalues = _floats(qvalues, 1, 'qvalues')
    if loop_idx is not None:
        loop_idx = np.asarray(loop_idx)
        if loop_idx.dtype != np.bool_ or loop_idx.shape != (n,):
            raise ValueError('loop_idx must be a boolean (n,) array')
        n_loop = int(loop_idx.sum())
    else:
        n_loop = n
    if len(qvalues) != n_loop:
        raise ValueError('%d q-values for %d loop pixels'
                         % (len(qvalues), n_loop))
    fdr = float(fdr)
    if n == 0:
        return dict(mean=np.empty((0, 2)), m=np.empty(0), a=np.empty(0),
                    label=np.empty(0, dtype=np.int8))
    mean, m, a, label = _native.context().ma_stats(
        scaled, cond_of_rep, C, idx[0], idx[1], qvalues, fdr, loop_idx)
    return dict(mean=mean, m=m, a=a, label=label)


def density_grid(x, y, label, n_classes, xedges, yedges):
    """Per class l in [0, n_classes): ``np.histogram2d(x[label == l],
    y[label == l], bins=[xedges, yedges])[0]`` as int64 counts
    (n_classes, len(xedges) - 1, len(yedges) - 1). Rows with another label
    (ma_stats' -1) or a non-finite coordinate are dropped."""
    x, y = _floats(x, 1, 'x'), _floats(y, 1, 'y')
    label = np.asarray(label)
    if label.dtype != np.int8:
        raise TypeError('label must be int8, not %s' % label.dtype)
    if label.shape != x.shape or y.shape != x.shape:
        raise ValueError('x, y and label must have one length')
    n_classes = int(n_classes)
    if not 1 <= n_classes <= 127:
        raise ValueError('n_classes must be in [1, 127]')
    xedges, yedges = _edges(xedges, 'xedges'), _edges(yedges, 'yedges')
    if n_classes * (len(xedges) - 1) * (len(yedges) - 1) >= 2 ** 28:
        raise ValueError('the grid must have fewer than 2^28 cells')
    return _native.context().density_grid(x, y, label, n_classes, xedges,
                                          yedges)


def _columns(data):
    data = _floats(data, 2, 'data')
    if not 1 <= data.shape[0] <= MAX_REPS:
        raise ValueError('data must be (replicates, pixels) with 1 to %d '
                         'replicates, not %d' % (MAX_REPS, data.shape[0]))
    return data


def rank_average(data):
    """``scipy.stats.rankdata(data, method='average', axis=1)`` for ``data``
    (replicates, pixels); a row holding a NaN has NaN ranks."""
    data = _columns(data)
    if data.shape[1] == 0:
        return np.empty(data.shape)
    return _native.context().rank_average(data)[0]


def correlation_matrix(data, correlation='spearman'):
    """The (R, R) matrix of pairwise correlations among the rows of ``data``
    (replicates, pixels) -- the orientation analysis/plotting.py:369 passes
    to make_pairwise_correlation_matrix_from_counts_matrix. 'pearson':
    scipy.stats.pearsonr, computed centred; 'spearman': the same on average
    ranks (scipy.stats.spearmanr). A row with a NaN and a constant row give
    NaN in their row and column."""
    if correlation not in ('spearman', 'pearson'):
        raise ValueError("correlation must be 'spearman' or 'pearson', not %r"
                         % (correlation,))
    data = _columns(data)
    return _native.context().corr_matrix(data,
                                         ranked=correlation == 'spearman')


def force_monotone(raw_means):
    """plotting/dispersion.py:135-144: a running minimum over the finite
    per-distance means (inf until the first finite one)."""
    out = np.empty(len(raw_means))
    smallest = np.inf
    for d, v in enumerate(raw_means):
        if np.isfinite(v) and v < smallest:
            smallest = v
        out[d] = smallest
    return out


def mvr_data(scaled_cond, dist, disp_fit, disp_per_dist=None, distance=None):
    """The data of plot_mvr (plotting/dispersion.py:133-183) for one
    condition: ``scaled_cond`` (n, r) its replicates' scaled values at the
    disp pixels, ``dist`` (n,) their distances, ``disp_fit`` (n,) their
    fitted dispersions, ``disp_per_dist`` (D,) the condition's per-distance
    estimates (optional). Returns a dict: ``pixel_mean``, ``pixel_var``
    (ddof=1; NaN for r == 1), ``pixel_disp_fit``, ``dist_range``,
    ``dist_mean`` (per-distance mean of pixel_mean, forced monotone),
    ``dist_disp_fit`` (per-distance mean of disp_fit; NaN where a distance
    has no pixel) and, with ``disp_per_dist``, ``dist_per_bin``,
    ``disp_per_bin``, ``mean_per_bin``.

    ``distance`` (analysis/plotting.py:132-140): only the pixels at that
    distance; pixel_disp_fit is then ``disp_per_dist[distance]`` throughout
    and the per-distance entries are None."""
    scaled_cond = _floats(scaled_cond, 2, 'scaled_cond')
    n, r = scaled_cond.shape
    if not 1 <= r <= MAX_REPS:
        raise ValueError('between 1 and %d replicates, not %d'
                         % (MAX_REPS, r))
    dist = _ints(dist, 'dist')
    disp_fit = _floats(disp_fit, 1, 'disp_fit')
    if dist.shape != (n,) or disp_fit.shape != (n,):
        raise ValueError('dist and disp_fit must have one value per pixel')
    if n and dist.min() < 0:
        raise ValueError('dist must not be negative')
    if n and dist.max() >= MAX_KEYS:
        raise ValueError('dist must be below %d' % MAX_KEYS)
    if disp_per_dist is not None:
        disp_per_dist = _floats(disp_per_dist, 1, 'disp_per_dist')
    if distance is not None:
        if disp_per_dist is None:
            raise ValueError('distance needs disp_per_dist')
        distance = int(distance)
        if not 0 <= distance < len(disp_per_dist):
            raise ValueError('distance %d outside disp_per_dist' % distance)
    ctx = _native.context() if n else None
    if n:
        mean, var = ctx.pixel_moments(scaled_cond, np.arange(r))
    else:
        mean, var = np.empty(0), np.empty(0)
    out = dict(pixel_mean=mean, pixel_var=var, pixel_disp_fit=disp_fit,
               dist_range=None, dist_mean=None, dist_disp_fit=None,
               dist_per_bin=None, disp_per_bin=None, mean_per_bin=None)
    if distance is not None:
        at = dist == distance
        out.update(pixel_mean=mean[at], pixel_var=var[at],
                   pixel_disp_fit=np.ones(int(at.sum())) *
                   disp_per_dist[distance])
        return out
    if n == 0:
        return out
    K = int(dist.max()) + 1
    sums, counts = ctx.group_sums(dist.astype(np.int32),
                                  np.column_stack([mean, disp_fit]), K)
    with np.errstate(divide='ignore', invalid='ignore'):
        per_dist = sums / counts.astype(np.float64)[:, None]
    out['dist_range'] = np.arange(K)
    out['dist_mean'] = force_monotone(per_dist[:, 0])
    out['dist_disp_fit'] = per_dist[:, 1].copy()
    if disp_per_dist is not None:
        ok = np.isfinite(disp_per_dist)
        out['disp_per_bin'] = disp_per_dist[ok]
        out['dist_per_bin'] = np.arange(len(disp_per_dist))[ok]
        out['mean_per_bin'] = np.interp(out['dist_per_bin'],
                                        out['dist_range'], out['dist_mean'])
    return out


MAX_RANGES = 64     # distance ranges of one distance_bias call


def percentile_ranks(n, threshold):
    """The two 0-based ranks ``np.percentile(x, 100 * threshold)`` (method
    'linear') reads from the sorted ``x`` of length ``n``, and its weight:
    ``(previous, next, gamma)``. numpy's own steps: the virtual index
    ``(n - 1) * (100 * threshold / 100)``, its floor and the rank behind it,
    both the last rank at or beyond the end."""
    q = np.true_divide(100 * threshold, 100)
    vi = (n - 1) * q
    prev = np.floor(vi)
    nxt = prev + 1
    if vi >= n - 1:
        prev = nxt = -1.0
    if vi < 0:
        prev = nxt = 0.0
    gamma = np.float64(vi - prev)
    return int(prev) % n, int(nxt) % n, gamma


def percentile_lerp(a, b, t):
    """numpy's ``_lerp``: ``a + (b - a) * t``, and ``b - (b - a) * (1 - t)``
    for ``t >= 0.5``, in float64, one rounding per operation."""
    a, b, t = np.float64(a), np.float64(b), np.float64(t)
    with np.errstate(invalid='ignore'):
        diff = b - a
        if t >= 0.5:
            return b - diff * (1 - t)
        return a + diff * t


def _ranges(bins):
    lo, hi = [], []
    for pair in bins:
        mn, mx = pair
        lo.append(np.iinfo(np.int64).min if mn is None else int(mn))
        hi.append(np.iinfo(np.int64).max if mx is None else int(mx))
    if not 1 <= len(lo) <= MAX_RANGES:
        raise ValueError('between 1 and %d distance ranges, not %d'
                         % (MAX_RANGES, len(lo)))
    return np.array(lo, dtype=np.int64), np.array(hi, dtype=np.int64)


def distance_bias(pvalues, dist, bins, threshold=0.05):
    """plotting/distance_bias.py:101-112: ``(p_star, fractions)``.
    ``p_star = np.percentile(pvalues, 100 * threshold)``; ``fractions[b] =
    np.mean(pvalues[idx] < p_star)`` over the pixels whose ``dist`` is in
    the inclusive range ``bins[b] = (min, max)``, either end None for open;
    the ranges may overlap, an empty one gives NaN. A NaN p-value makes
    ``p_star`` NaN and every fraction 0, as numpy does. The sort and the
    counts run on the GPU (h3d_order_stats, h3d_bin_fractions); the
    percentile is interpolated here from the two order statistics."""
    pvalues = _floats(pvalues, 1, 'pvalues')
    dist = np.asarray(dist)
    if dist.dtype.kind not in 'iu':
        raise TypeError('dist must be integers, not %s' % dist.dtype)
    if dist.shape != pvalues.shape:
        raise ValueError('pvalues and dist must have one length')
    lo, hi = _ranges(bins)
    threshold = float(threshold)
    if not 0 <= threshold <= 1:
        raise ValueError('threshold must be in [0, 1]')
    n = len(pvalues)
    if n >= 2 ** 31:
        raise ValueError('at most 2^31 - 1 pixels')
    if n == 0:
        return np.float64(np.nan), np.full(len(lo), np.nan)
    ctx = _native.context()
    prev, nxt, gamma = percentile_ranks(n, threshold)
    (a, b), n_nan = ctx.order_stats(pvalues, [prev, nxt])
    p_star = np.float64(np.nan) if n_nan else percentile_lerp(a, b, gamma)
    members, below = ctx.bin_fractions(pvalues, dist, lo, hi, p_star)
    with np.errstate(divide='ignore', invalid='ignore'):
        fractions = below / members.astype(np.float64)
    return p_star, fractions
