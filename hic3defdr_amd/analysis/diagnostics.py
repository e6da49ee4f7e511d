"""Diagnostics mixin: one method per plot_* method of the reference's
PlottingHiC3DeFDR (hic3defdr/analysis/plotting.py), loading the same outdir
arrays in the same way and returning the data the figure is drawn from
instead of an axis (DESIGN.md §1 rules out drawing; plot_heatmap / plot_grid
are served by get_matrix). The reductions run on the GPU
(util/diagnostics.py, csrc/h3d_diag.hip)."""
import numpy as np

from hic3defdr_amd import _native
from hic3defdr_amd.util import diagnostics as diag


class DiagnosticHiC3DeFDR(object):
    """Mixin: the numbers under the reference's QC figures."""

    def dd_curves(self, chrom):
        """plot_dd_curves (plotting.py:19-51): ``(bs, before_means,
        after_means, repnames)`` -- the curves are drawn at
        ``bs * 10 + 5``. ``balanced = raw / (bias[row] * bias[col])`` is
        formed on the device; a zero-bias bin gives inf / nan as numpy's
        division does."""
        bias = self.load_bias(chrom)
        row = self.load_data('row', chrom)
        col = self.load_data('col', chrom)
        raw = self.load_data('raw', chrom)
        scaled = self.load_data('scaled', chrom)
        if len(row) and max(row.max(), col.max()) >= len(bias):
            raise ValueError('row / col index beyond the bias vector')
        balanced = _native.context().balance_pixels(row, col, raw, bias) \
            if len(row) else np.empty(raw.shape)
        bs, before, after = diag.dd_curves(row, col, balanced, scaled)
        return bs, before, after, list(self.design.index)

    def _pixel_values(self, name, idx):
        if idx == 'loop':
            loop_idx, _ = self.load_data('loop_idx', 'all')
            return self.load_data(name, 'all', idx=loop_idx)[0]
        return self.load_data(name, 'all')[0]

    def pvalue_distribution(self, idx='disp', edges=None):
        """plot_pvalue_distribution (plotting.py:200-229): ``(counts,
        edges)`` of the p-values of the disp pixels or of the loop pixels."""
        if idx not in ('loop', 'disp'):
            raise ValueError('idx must be loop or disp')
        return diag.value_histogram(self._pixel_values('pvalues', idx), edges)

    def qvalue_distribution(self, edges=None):
        """plot_qvalue_distribution (plotting.py:231-249)."""
        return diag.value_histogram(self.load_data('qvalues', 'all')[0],
                                    edges)

    def ma_data(self, fdr=0.05, conds=None, include_non_loops=True,
                grid=None):
        """plot_ma (plotting.py:251-327): the dict of
        ``util.diagnostics.ma_stats`` over the disp pixels (over the loop
        pixels alone with ``include_non_loops=False``, label 0 then never
        occurs), plus ``conds``. ``grid=(xedges, yedges)`` adds ``density``:
        (4, ...) counts of the (a, m) cloud of the series 0 .. 3."""
        if conds is None:
            conds = self.design.columns.tolist()[:2]
        disp_idx, _ = self.load_data('disp_idx', 'all')
        loop_idx, _ = self.load_data('loop_idx', 'all')
        scaled, _ = self.load_data('scaled', 'all', idx=disp_idx)
        qvalues, _ = self.load_data('qvalues', 'all')
        if include_non_loops:
            out = diag.ma_stats(scaled, self.design, conds, qvalues, fdr,
                                loop_idx=np.asarray(loop_idx, dtype=bool))
        else:
            out = diag.ma_stats(scaled[loop_idx], self.design, conds,
                                qvalues, fdr)
        out['conds'] = list(conds)
        if grid is not None:
            out['density'] = diag.density_grid(out['a'], out['m'],
                                               out['label'], 4, *grid)
        return out

    def correlation_matrix(self, stage='scaled', idx='loop',
                           correlation='spearman'):
        """plot_correlation_matrix (plotting.py:329-379): ``(matrix (R, R),
        replicate names)``."""
        if correlation not in ('spearman', 'pearson'):
            raise ValueError("correlation must be 'spearman' or 'pearson'")
        if idx == 'disp':
            idx, _ = self.load_data('disp_idx', 'all')
        elif idx == 'loop':
            idx = (self.load_data('disp_idx', 'all')[0],
                   self.load_data('loop_idx', 'all')[0])
        else:
            raise ValueError('idx must be \'disp\' or \'loop\'')
        data = self.load_data(stage, 'all', idx=idx)[0].T
        return (diag.correlation_matrix(data, correlation=correlation),
                self.design.index.tolist())

    def dispersion_fit_data(self, cond, distance=None):
        """plot_dispersion_fit (plotting.py:53-156) up to the plot_mvr call:
        the dict of ``util.diagnostics.mvr_data`` for the condition, plus
        ``pixel_dist`` (None with ``distance``). Without a saved
        ``disp_per_dist`` the per-bin entries are None (:115-122)."""
        cond_idx = self.design.columns.tolist().index(cond)
        disp_idx, _ = self.load_data('disp_idx', 'all')
        scaled = self.load_data(
            'scaled', 'all', idx=disp_idx)[0][:, np.asarray(self.design[cond],
                                                            dtype=bool)]
        disp = self.load_data('disp', 'all')[0][:, cond_idx]
        try:
            disp_per_dist = self.load_data('disp_per_dist')[:, cond_idx]
        except IOError:
            disp_per_dist = None
        row, _ = self.load_data('row', 'all', idx=disp_idx)
        col, _ = self.load_data('col', 'all', idx=disp_idx)
        dist = col - row
        out = diag.mvr_data(scaled, dist, disp, disp_per_dist,
                            distance=distance)
        out['pixel_dist'] = None if distance is not None else dist
        return out

    def distance_bias_data(self, bins, idx='disp', threshold=0.05):
        """plot_distance_bias (plotting/distance_bias.py:73-112) for this
        analysis: ``(bin_labels, p_star, fractions)``. ``bins``: inclusive
        ``(min, max)`` distance ranges in bin units, either end None for
        open; ``idx``: 'disp' for the p-values of every disp pixel, 'loop'
        for those of the loop pixels; ``fractions[b]``: the share of the
        range's p-values below ``p_star``, the ``100 * threshold``-th
        percentile of them all (``util.diagnostics.distance_bias``)."""
        if idx not in ('loop', 'disp'):
            raise ValueError('idx must be loop or disp')
        bins = [tuple(b) for b in bins]
        bin_labels = []
        for min_dist, max_dist in bins:
            if min_dist is None and max_dist is not None:
                label = '<= %s' % max_dist
            elif min_dist is not None and max_dist is None:
                label = '>= %s' % min_dist
            elif min_dist is None and max_dist is None:
                label = 'all'
            else:
                label = '%s to %s' % (min_dist, max_dist)
            bin_labels.append(label)
        disp_idx, _ = self.load_data('disp_idx', 'all')
        if idx == 'loop':
            loop_idx, _ = self.load_data('loop_idx', 'all')
            rc_idx, p_idx = (disp_idx, loop_idx), loop_idx
        else:
            rc_idx, p_idx = disp_idx, None
        row, _ = self.load_data('row', 'all', idx=rc_idx)
        col, _ = self.load_data('col', 'all', idx=rc_idx)
        pvalues, _ = self.load_data('pvalues', 'all', idx=p_idx)
        p_star, fractions = diag.distance_bias(
            pvalues, col.astype(np.int64) - row, bins, threshold=threshold)
        return bin_labels, p_star, fractions

    def ddr_data(self, cond):
        """plot_ddr (plotting.py:158-198, plotting/dispersion.py:343-346):
        ``dist_per_bin``, ``disp_per_bin``, and the fitted curve ``ys`` on
        ``xs = np.arange(xmin, xmax + 1)``."""
        cond_idx = self.design.columns.tolist().index(cond)
        disp_per_dist = self.load_data('disp_per_dist')[:, cond_idx]
        ok = np.isfinite(disp_per_dist)
        disp_per_bin = disp_per_dist[ok]
        dist_per_bin = np.arange(self.dist_thresh_max + 1)[ok]
        disp_fn = self.load_disp_fn(cond)
        xs = np.arange(dist_per_bin.min(), dist_per_bin.max() + 1)
        return dict(dist_per_bin=dist_per_bin, disp_per_bin=disp_per_bin,
                    xs=xs, ys=disp_fn(xs))
