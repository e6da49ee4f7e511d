"""The yardstick of the diagnostics tests: what the reference's plotting
modules compute before they draw, restated in elementary numpy, and the
fixtures the tests share.

The reference's plotting/*.py only draw and return an axis, and lib5c (whose
make_pairwise_correlation_matrix_from_counts_matrix the correlation figure
calls) is not vendored, so there is nothing to record as a golden: the
numbers ARE numpy / scipy expressions. Each restatement below cites the
reference lines it restates; tests/test_diag_host.py holds them to
np.histogram, np.histogram2d, scipy.stats.rankdata, pearsonr and spearmanr
themselves."""
import numpy as np

U = 2.0 ** -53


# -- restatements -----------------------------------------------------------

def dd_curves_ref(row, col, before, after):
    """plotting/distance_dependence.py:34-43, verbatim."""
    dist = col - row
    n = max(row.max(), col.max()) + 1
    dist_bin_idx = np.digitize(dist, np.linspace(0, 1000, 101), right=True)
    bs = np.arange(1, dist_bin_idx.max() + 1)
    with np.errstate(all='ignore'):
        before_means = np.array(
            [np.sum(before[dist_bin_idx == b, :], axis=0) / float(n - b)
             for b in bs])
        after_means = np.array(
            [np.sum(after[dist_bin_idx == b, :], axis=0) / float(n - b)
             for b in bs])
    members = np.array([(dist_bin_idx == b).sum() for b in bs])
    return bs, before_means, after_means, members


def balanced_ref(raw, bias, row, col):
    """analysis/plotting.py:46-48."""
    balanced = np.zeros_like(raw, dtype=float)
    with np.errstate(all='ignore'):
        for r in range(raw.shape[1]):
            balanced[:, r] = raw[:, r] / (bias[row, r] * bias[col, r])
    return balanced


def bin_of(values, edges):
    """Bin index of every value under np.histogram's rules with explicit
    edges ([e_i, e_i+1), the last bin closed), -1 where it is dropped."""
    values = np.asarray(values, dtype=float)
    with np.errstate(invalid='ignore'):
        keep = (values >= edges[0]) & (values <= edges[-1])
    b = np.searchsorted(edges, values, side='right') - 1
    b[values == edges[-1]] = len(edges) - 2
    return np.where(keep, b, -1)


def histogram_ref(values, edges):
    """plotting/histograms.py: plt.hist(values, bins=edges), i.e.
    np.histogram."""
    b = bin_of(values, edges)
    return np.bincount(b[b >= 0], minlength=len(edges) - 1).astype(np.int64)


def density_ref(x, y, label, n_classes, xedges, yedges):
    """np.histogram2d(x, y, bins=[xedges, yedges])[0] per class."""
    bx, by = bin_of(x, xedges), bin_of(y, yedges)
    out = np.zeros((n_classes, len(xedges) - 1, len(yedges) - 1),
                   dtype=np.int64)
    ok = (bx >= 0) & (by >= 0) & (label >= 0) & (label < n_classes)
    np.add.at(out, (label[ok].astype(int), bx[ok], by[ok]), 1)
    return out


def ma_ref(scaled, design, cond_idx, qvalues, fdr, loop_idx=None):
    """analysis/plotting.py:307-311 and plotting/ma.py:71-72, :131-155.
    label: 0 non-loop, 1 loop and not significant, 2 / 3 significant with
    m > 0 / m < 0, -1 significant and in neither series."""
    design = np.asarray(design, dtype=float)
    mean = np.dot(scaled, design) / np.sum(design, axis=0)
    mean = mean[:, cond_idx]
    with np.errstate(all='ignore'):
        m = np.log2(mean[:, 0]) - np.log2(mean[:, 1])
        a = 0.5 * (np.log2(mean[:, 0]) + np.log2(mean[:, 1]))
        sig_idx = qvalues < fdr
    if loop_idx is None:
        loop_idx = np.ones(len(m), dtype=bool)
    label = np.zeros(len(m), dtype=np.int8)
    loops = np.flatnonzero(loop_idx)
    label[loops[~sig_idx]] = 1
    sig = loops[sig_idx]
    label[sig] = -1
    label[sig[m[sig] > 0]] = 2
    label[sig[m[sig] < 0]] = 3
    return mean, m, a, label


def rank_ref(x):
    """Average ranks, 1-based: positions i .. j - 1 of the sorted order that
    hold one value share (i + 1 + j) / 2. NaN anywhere: all NaN."""
    x = np.asarray(x, dtype=float)
    if np.isnan(x).any():
        return np.full(len(x), np.nan)
    order = np.argsort(x, kind='stable')
    xs = x[order]
    heads = np.flatnonzero(np.r_[True, xs[1:] != xs[:-1]])
    ends = np.r_[heads[1:], len(x)]
    ranks = np.empty(len(x))
    ranks[order] = np.repeat((heads + 1 + ends) / 2.0, ends - heads)
    return ranks


def pearson_ref(x, y):
    """scipy.stats.pearsonr: centred sums; NaN for constant or NaN input."""
    if np.isnan(x).any() or np.isnan(y).any():
        return np.nan
    if (x == x[0]).all() or (y == y[0]).all():
        return np.nan
    xm, ym = x - x.mean(), y - y.mean()
    r = np.sum(xm * ym) / np.sqrt(np.sum(xm * xm) * np.sum(ym * ym))
    return max(min(r, 1.0), -1.0)


def corr_ref(data, correlation):
    """analysis/plotting.py:369-376: the pairwise matrix over the rows of
    ``data`` (replicates, pixels), unlogged."""
    cols = [rank_ref(c) for c in data] if correlation == 'spearman' \
        else list(data)
    R = len(cols)
    out = np.empty((R, R))
    for i in range(R):
        for j in range(R):
            out[i, j] = pearson_ref(cols[i], cols[j])
    return out


def scipy_corr(data, correlation):
    """The same matrix from scipy.stats itself, pair by pair."""
    import warnings
    import scipy.stats as st
    fn = st.spearmanr if correlation == 'spearman' else st.pearsonr
    R = len(data)
    out = np.empty((R, R))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for i in range(R):
            for j in range(i, R):
                if correlation == 'pearson' and \
                        (np.isnan(data[i]).any() or np.isnan(data[j]).any()):
                    r = np.nan    # pearsonr's propagate
                else:
                    r = fn(data[i], data[j])[0]
                out[i, j] = out[j, i] = r
    return out


def mvr_ref(scaled_cond, dist, disp_fit, disp_per_dist=None):
    """analysis/plotting.py:128-129 and plotting/dispersion.py:133-152,
    :182-183."""
    with np.errstate(all='ignore'):
        mean = np.mean(scaled_cond, axis=1)
        var = np.var(scaled_cond, ddof=1, axis=1)
    dist_range = np.arange(dist.max() + 1)
    smallest_seen = np.inf
    dist_mean_list = []
    raw_means = []
    with np.errstate(all='ignore'):
        for d in dist_range:
            currently_seen = np.mean(mean[dist == d])
            raw_means.append(currently_seen)
            if np.isfinite(currently_seen) and currently_seen < smallest_seen:
                smallest_seen = currently_seen
                dist_mean_list.append(currently_seen)
            else:
                dist_mean_list.append(smallest_seen)
        dist_disp_fit = np.array([np.mean(disp_fit[dist == d])
                                  for d in dist_range])
    out = dict(pixel_mean=mean, pixel_var=var, dist_range=dist_range,
               dist_mean=np.array(dist_mean_list),
               dist_disp_fit=dist_disp_fit, raw_means=np.array(raw_means),
               members=np.bincount(dist, minlength=len(dist_range)))
    if disp_per_dist is not None:
        idx = np.isfinite(disp_per_dist)
        out['disp_per_bin'] = disp_per_dist[idx]
        out['dist_per_bin'] = np.arange(len(disp_per_dist))[idx]
        out['mean_per_bin'] = np.interp(out['dist_per_bin'], dist_range,
                                        out['dist_mean'])
    return out


# -- comparisons -------------------------------------------------------------

def assert_sum_bound(got, want, members, what):
    """Sums of non-negative terms in any order are within (k - 1) u of the
    exact sum, so two of them differ by at most 2 k u (the division's
    rounding included); non-finite cells must be the same non-finite
    value."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, what
    k = np.asarray(members, float).reshape((-1,) + (1,) * (got.ndim - 1))
    fin = np.isfinite(want)
    np.testing.assert_array_equal(np.isfinite(got), fin, what)
    np.testing.assert_array_equal(got[~fin], want[~fin], what)
    err = np.abs(got - want)[fin]
    bound = (2 * k * U * np.abs(want))[fin]
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.
    print('%s: worst |err| / bound = %.3f over %d cells'
          % (what, worst, err.size))
    assert np.all(err <= bound), what


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    assert a.tobytes() == b.tobytes()


# -- fixtures ----------------------------------------------------------------

TAILS = (0, 1, 63, 64, 65, 257, 4097)


def dd_table(n_bins, R, seed, n_px=5000, far=False):
    """A lexsorted pixel table of an n_bins chromosome: distances 0, 1, 10,
    11 present, bin 3 (distances 21 .. 30) empty, bin 7's bias zero in every
    replicate (inf and nan in balanced); ``far``: pixels beyond distance
    1000 too."""
    rng = np.random.default_rng(seed)
    row = rng.integers(0, n_bins, n_px)
    span = 1150 if far else 390
    dist = rng.integers(0, span, n_px)
    dist[:8] = [0, 1, 10, 11, 0, 1, 10, 11]
    if far:
        dist[8:12] = [1000, 1001, 1100, 1149]
        row[8:12] = [3, 5, 9, 11]
    row = np.minimum(row, n_bins - 1 - dist)
    ok = (row >= 0) & ~((dist >= 21) & (dist <= 30))
    pix = np.stack([row[ok], row[ok] + dist[ok]], axis=1)
    pix = np.unique(np.concatenate([pix, [[7, 19], [7, 52]]]), axis=0)
    row, col = pix[:, 0].astype(np.int64), pix[:, 1].astype(np.int64)
    raw = rng.poisson(3.0, (len(row), R)).astype(np.int64)
    raw[(row == 7) & (col == 19)] = 0        # 0 / 0
    raw[(row == 7) & (col == 52)] = 5        # 5 / 0
    bias = rng.uniform(0.5, 2.0, (n_bins, R))
    bias[7] = 0.0
    scaled = raw * rng.uniform(0.5, 2.0, (len(row), R))
    return dict(row=row, col=col, raw=raw, bias=bias, scaled=scaled,
                n_bins=n_bins)


def edge_values():
    """p-values on and around every edge of linspace(0, 1, 21), and the
    values np.histogram drops."""
    e = np.linspace(0, 1, 21)
    v = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf),
                        [np.nan, -0.0, 1.0, -0.5, 1.5, np.inf, -np.inf,
                         np.nan]])
    rng = np.random.default_rng(5)
    v = np.concatenate([v, rng.uniform(0, 1, 4097 - len(v))])
    rng.shuffle(v)
    return v


DESIGNS = {
    '2+2': (np.array([[1, 0], [1, 0], [0, 1], [0, 1]], dtype=bool),
            ['A', 'B'], ['A', 'B']),
    # three conditions, comparing two that are not the first two
    '3+1+2': (np.array([[1, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0],
                        [0, 0, 1], [0, 0, 1]], dtype=bool),
              ['A', 'B', 'C'], ['C', 'B']),
}


def ma_case(name, n=4097, seed=11):
    """scaled (n, R), loop_idx, qvalues, fdr for a design of DESIGNS: four
    planted significant loop pixels whose M is 0 or NaN (three exact ties,
    one pixel with both means zero), pixels with one zero mean (M = +-inf),
    NaN q-values."""
    design, names, conds = DESIGNS[name]
    rng = np.random.default_rng(seed)
    R = design.shape[0]
    scaled = rng.gamma(2.0, 3.0, (n, R))
    loop_idx = rng.uniform(size=n) < 0.5
    loop_idx[:16] = True
    q = rng.uniform(0, 1, int(loop_idx.sum()))
    q[rng.uniform(size=len(q)) < 0.02] = np.nan
    q[:16] = 0.001                       # pixels 0 .. 15: significant
    scaled[0:3] = 2.0                    # ties: mean0 == mean1
    scaled[3] = 0.0                      # both zero: M = nan
    c0, c1 = names.index(conds[0]), names.index(conds[1])
    scaled[4][design[:, c0]] = 0.0       # M = -inf
    scaled[5][design[:, c1]] = 0.0       # M = +inf
    return dict(scaled=scaled, design=design, names=names, conds=conds,
                cond_idx=[c0, c1], loop_idx=loop_idx, qvalues=q, fdr=0.3)


def corr_columns(R, kind, n=4097, seed=3):
    """(R, n): 'counts' Poisson(3) columns (heavy ties), 'scaled' continuous
    ones; column 0 holds -0.0 beside 0.0; from R >= 4 the last three are a
    copy of column 0, a constant and a column with a NaN."""
    rng = np.random.default_rng(seed + R)
    base = rng.gamma(2.0, 2.0, n)
    if kind == 'counts':
        data = rng.poisson(3.0 * base / base.mean(), (R, n)).astype(float)
    else:
        data = base * rng.lognormal(0.0, 0.4, (R, n))
    data[0, :6] = [0.0, -0.0, 0.0, -0.0, 1.0, -0.0]
    if R >= 4:
        data[R - 3] = data[0]
        data[R - 2] = 7.0
        data[R - 1, n // 2] = np.nan
    return data


def mvr_case(r, n=4097, seed=21):
    """scaled_cond (n, r), dist, disp_fit, disp_per_dist: distance 5 has no
    pixel and the per-distance means rise again at distances 9 and 12, so
    the monotone pass has work."""
    rng = np.random.default_rng(seed + r)
    dist = rng.integers(0, 24, n)
    dist[dist == 5] = 6
    level = 40.0 / (1.0 + dist)
    level[dist == 9] *= 3.0
    level[dist == 12] *= 2.0
    scaled = rng.gamma(4.0, 1.0, (n, r)) * level[:, None]
    disp_fit = 0.01 + 0.002 * dist + rng.uniform(0, 1e-3, n)
    dpd = 0.01 + 0.002 * np.arange(30)
    dpd[[5, 27]] = np.nan
    return dict(scaled=scaled, dist=dist, disp_fit=disp_fit,
                disp_per_dist=dpd)
