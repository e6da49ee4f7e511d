"""Persistence mixin (reference hic3defdr/analysis/core.py): the outdir is the
contract between stages — ``<outdir>/<name>_<chrom>.npy`` per chromosome,
``disp_per_dist.npy``, ``disp_fn_<cond>.pickle`` and ``pickle``. What a file
name means lives here; how the files are written behind, cached and told
apart from later versions lives in outdir.py."""
import pickle

import numpy as np

from hic3defdr_amd.analysis.outdir import OutdirStore


def _load_column(fname):
    """np.loadtxt of a one-column text file, parsed by libh3d when it takes
    the file (_native.read_text_column: the same values, no GIL held)."""
    from hic3defdr_amd import _native
    col = _native.read_text_column(fname)
    return np.loadtxt(fname) if col is None else col


def _interp_extrap(xp, yp, x):
    """scipy interp1d(kind='linear', fill_value='extrapolate')."""
    idx = np.clip(np.searchsorted(xp, x), 1, len(xp) - 1)
    lo, hi = idx - 1, idx
    return (yp[hi] - yp[lo]) / (xp[hi] - xp[lo]) * (x - xp[lo]) + yp[lo]


class DispFn(object):
    """Picklable fitted dispersion function of one condition.

    The reference pickles the lowess closure (``core.py:220-253``,
    ``lowess.py:76-92`` / ``229-242``). The smoothed part is piecewise linear
    with knots on integer distances (lowess outputs at the expanded integer
    x), so its tabulation on d = 0..D-1 (``h3d_disp_table``, native) with
    linear interpolation / extrapolation over the integer knots reproduces
    it. On top of that, in the reference's order:

    - ``lowess_fit``'s left boundary (``lowess.py:84-85``): every
      ``x <= left_boundary`` (= the first finite dispersion value,
      ``analysis.py:212``) returns the fit at its leftmost knot;
    - the weighted fit then replaces everything below ``x[inc_idx]`` by
      linear interpolation of the raw (distance, dispersion) points, and below
      the first fitted distance by ``y[0]`` (``lowess.py:229-242``).
    """

    def __init__(self, table, disp_per_dist_col, weighted=True):
        self.table = np.asarray(table, dtype=float)
        col = np.asarray(disp_per_dist_col, dtype=float)
        fin = np.isfinite(col)
        self.x = np.arange(len(col), dtype=float)[fin]
        self.y = col[fin]
        self.weighted = bool(weighted)
        self.inc_idx = int(np.argmax(np.diff(self.y) > 0) + 1) \
            if self.weighted else 0
        self.left_boundary = float(self.y[0])
        # leftmost lowess knot: the first expanded (weighted) or fitted x
        self.left_value = float(self.table[int(self.x[self.inc_idx])])

    def __call__(self, x_star):
        x = np.asarray(x_star, dtype=float)
        t = self.table
        xi = np.rint(x)
        on_knot = (xi == x) & (xi >= 0) & (xi < len(t))
        out = np.empty(x.shape, dtype=float)
        out[on_knot] = t[xi[on_knot].astype(np.int64)]
        off = ~on_knot
        if off.any():
            out[off] = _interp_extrap(np.arange(len(t), dtype=float), t,
                                      x[off])
        out[x <= self.left_boundary] = self.left_value
        if self.weighted:
            below = x < self.x[self.inc_idx]
            if below.any():
                v = _interp_extrap(self.x, self.y, x[below])
                v[x[below] < self.x[0]] = self.y[0]
                out[below] = v
        return out


class CoreHiC3DeFDR(object):
    """Mixin providing saving and loading (reference ``core.py:10-291``)."""

    @property
    def picklefile(self):
        return '%s/pickle' % self.outdir

    @classmethod
    def load(cls, outdir):
        """Reference ``core.py:15-33``."""
        with open('%s/pickle' % outdir, 'rb') as handle:
            return cls(outdir=outdir, **pickle.load(handle))

    def load_bias(self, chrom):
        """Reference ``core.py:35-60``: (n_bins, R); bins failing
        ``bias_thresh`` in any replicate are zeroed."""
        bias = np.column_stack([_load_column(p.replace('<chrom>', chrom))
                                for p in self.bias_patterns])
        lo, hi = self.bias_thresh, 1. / self.bias_thresh
        bias[((bias < lo) | (bias > hi)).any(axis=1)] = 0
        return bias

    # -- outdir arrays --------------------------------------------------
    # Which pixel set a per-chromosome stage array is parallel to, as the mask
    # chain that selects its (row, col) from the union pixel set
    # (reference core.py:117-134). Stages not listed cannot be loaded as COO.
    _PIXEL_SET = dict(
        [(n, ()) for n in ('raw', 'size_factors', 'scaled', 'disp_idx')] +
        [(n, ('disp_idx',)) for n in ('loop_idx', 'disp', 'mu_hat_null',
                                      'mu_hat_alt', 'llr', 'pvalues')] +
        [('qvalues', ('disp_idx', 'loop_idx'))])
    _NOT_COO = frozenset(['row', 'col', 'bias', 'cov_per_bin',
                          'disp_per_bin'])

    def _npy(self, name, chrom=None):
        return '%s/%s.npy' % (self.outdir, name) if chrom is None \
            else '%s/%s_%s.npy' % (self.outdir, name, chrom)

    def _disp_fn_file(self, cond):
        return '%s/disp_fn_%s.pickle' % (self.outdir, cond)

    def _column(self, rep, cond):
        """Column of a (pixels, reps) / (pixels, conds) array, or None."""
        if rep is not None:
            return list(self.design.index).index(rep)
        if cond is not None:
            return list(self.design.columns).index(cond)
        return None

    @staticmethod
    def _narrow(mask, sub):
        """The entries of boolean ``mask`` that ``sub`` (parallel to the True
        entries of ``mask``) keeps: index chaining (reference core.py:141-145)."""
        out = np.zeros_like(mask)
        out[np.flatnonzero(mask)[sub]] = True
        return out

    @property
    def _store(self):
        """This object's outdir.OutdirStore (the write-behind queue and the
        cache of its outdir files), made on first use: the constructor
        pickles the instance attributes as they stand when it ends, and the
        store is none of the constructor's arguments."""
        try:
            return self._outdir_store
        except AttributeError:
            self._outdir_store = OutdirStore()
            return self._outdir_store

    def _save_npy(self, fname, data, owned=False, ready=None):
        """OutdirStore.save: queues ``data`` for ``fname``."""
        self._store.save(fname, data, owned=owned, ready=ready)

    def flush(self):
        """Waits for every queued outdir write of this object (raises the
        first write error)."""
        self._store.flush()

    def is_current(self, fname):
        """True when ``fname`` holds what this object last wrote there."""
        return self._store.is_current(fname)

    def write_generation(self, fname):
        """How many times this object has written ``fname`` (0: never)."""
        return self._store.generation(fname)

    def cache_nbytes(self):
        """Bytes held by the outdir cache."""
        return self._store.cache_nbytes()

    def pending_nbytes(self):
        """Bytes held by this object's queued (not yet landed) writes."""
        return self._store.pending_nbytes()

    def load_npy_file(self, fname, mmap_mode=None):
        """np.load of an outdir file, after this object's queued write of it
        has landed."""
        self._store.wait(fname)
        return np.load(fname, mmap_mode=mmap_mode)

    def load_data(self, name, chrom=None, idx=None, rep=None, cond=None,
                  coo=False):
        """Reference ``core.py:62-196``: one chromosome's array (``chrom``),
        an unchromosomed one (``chrom=None``), or every chromosome
        concatenated plus offsets (``chrom='all'``; ``idx`` then spans the
        genome). ``idx`` may be a (big, small) mask pair, chained. ``coo``
        returns (row, col, data) with row/col taken through the stage's mask
        chain.

        Deviation: without loop_patterns the reference's ``loop_idx``
        short-circuit calls the non-existent ``np.load_data``
        (``core.py:105``); here it returns the all-True vector it intends."""
        if name == 'loop_idx' and self.loop_patterns is None and \
                idx is None and chrom != 'all':
            return np.ones(int(self.load_data('disp_idx', chrom).sum()),
                           dtype=bool)
        col = self._column(rep, cond)
        if coo:
            if chrom == 'all' or idx is not None:
                raise ValueError("cannot pass coo=True with chrom='all' or idx")
            if name in self._NOT_COO:
                raise ValueError('data with name %s cannot be loaded as COO'
                                 % name)
            if name not in self._PIXEL_SET:
                raise ValueError('data name %s not recognized' % name)
            chain = [self.load_data(m, chrom) for m in self._PIXEL_SET[name]]
            sel = None
            if chain:
                sel = chain[0]
                for sub in chain[1:]:
                    sel = self._narrow(sel, sub)
            data = self.load_data(name, chrom)
            return (self.load_data('row', chrom, idx=sel),
                    self.load_data('col', chrom, idx=sel),
                    data if col is None else data[:, col])
        if isinstance(idx, tuple):
            idx = self._narrow(*idx)
        store = self._store
        if chrom != 'all':
            return store.read(self._npy(name, chrom), idx, col)
        pieces, start = [], 0
        for c in self.chroms:
            fname = self._npy(name, c)
            sub = None
            if idx is not None:
                n = store.n_rows(fname)
                sub, start = idx[start:start + n], start + n
            pieces.append(store.read(fname, sub, col))
        offsets = np.concatenate([[0], np.cumsum([len(a) for a in pieces])])
        return np.concatenate(pieces), offsets

    def save_data(self, data, name, chrom=None):
        """Reference ``core.py:198-218``: ``chrom`` is a chromosome name,
        None (unchromosomed), or an offsets array splitting ``data`` over
        ``self.chroms``."""
        if isinstance(chrom, np.ndarray):
            for c, lo, hi in zip(self.chroms, chrom[:-1], chrom[1:]):
                self._save_npy(self._npy(name, c), data[lo:hi])
            return
        self._save_npy(self._npy(name, chrom), data)

    # -- dense views ----------------------------------------------------
    # per-replicate stages the '_mean' suffix averages within a condition
    _MEAN_STAGES = ('raw', 'scaled')

    def _view_table(self, name, chrom, rep, cond):
        """The COO table behind a dense view of stage ``name``: (row, col,
        data, cols, mean). ``name`` + '_mean' averages the condition's
        replicates, in design order, inside the gather (``mean`` True,
        ``cols`` their columns of the (pixels, reps) ``data``)."""
        if name.endswith('_mean'):
            base = name[:-len('_mean')]
            if base not in self._MEAN_STAGES:
                raise ValueError('%s: only %s can be averaged over a '
                                 "condition's replicates"
                                 % (name, ' / '.join(self._MEAN_STAGES)))
            if cond is None:
                raise ValueError('%s needs cond' % name)
            cols = np.flatnonzero(np.asarray(self.design[cond], dtype=bool))
            if len(cols) == 0:
                raise ValueError('condition %s has no replicates' % cond)
            row, col, data = self.load_data(base, chrom, coo=True)
            return row, col, data, cols, True
        row, col, data = self.load_data(name, chrom, rep=rep, cond=cond,
                                        coo=True)
        if data.ndim != 1:
            raise ValueError('stage %s has %d columns: pass rep or cond'
                             % (name, data.shape[1]))
        return row, col, data, None, False

    def get_matrix(self, name, chrom, row_slice, col_slice, rep=None,
                   cond=None):
        """Reference ``core.py:255-291``: stage ``name`` of ``chrom`` as the
        dense float64 matrix ``row_slice`` x ``col_slice`` selects, both
        triangles filled, NaN where no pixel is stored
        (``util.matrices.select_matrix`` on ``load_data(..., coo=True)``).
        ``raw_mean`` / ``scaled_mean`` average the replicates of ``cond`` in
        design order, in the same launch. (The reference removes the suffix
        with ``name.strip('_mean')``, which strips characters; here it is
        removed as a suffix.)"""
        from hic3defdr_amd.util import matrices
        origin, h, w = matrices.slice_window(row_slice, col_slice)
        row, col, data, cols, mean = self._view_table(name, chrom, rep, cond)
        if h == 0 or w == 0:
            matrices.check_table(row, col)
            return np.full((h, w), np.nan)
        out = matrices.table_windows(row, col, data, origin, h, w, cols=cols,
                                     symmetrize=True, mean=mean)
        return out[0] if mean else out[0, 0]

    def apa_stack(self, name, chrom, clusters, width, min_dist=None,
                  rep=None, cond=None):
        """The APA stack (clusters, width, width) of stage ``name`` of
        ``chrom`` straight from the outdir: ``util.apa.make_apa_stack``'s
        windows (centres, ``min_dist`` and edge filtering on the chromosome's
        bin count; NaN slices for clusters it drops) over the stage's upper
        triangle, 0 where no pixel is stored. ``rep`` / ``cond`` and the
        '_mean' suffix as in ``get_matrix``. Not in the reference, whose
        walkthrough rebuilds a scipy matrix first."""
        from hic3defdr_amd.util import apa, matrices
        width = apa.check_width(width)
        row, col, data, cols, mean = self._view_table(name, chrom, rep, cond)
        n_bins = self.load_bias(chrom).shape[0]
        origins, _ = apa.apa_windows(clusters, width, n_bins, min_dist)
        if len(origins) == 0:
            matrices.check_table(row, col)
            return np.zeros((0, width, width))
        out = matrices.table_windows(row, col, data, origins, width, width,
                                     cols=cols, n_bins=n_bins,
                                     symmetrize=False, mean=mean, fill=0.0)
        return out if mean else out[0]

    @staticmethod
    def apa_mean(stack):
        """``(mean, count)`` over the windows of an APA stack
        (``util.apa.apa_mean``: ``np.nanmean(stack, axis=0)`` and the
        non-NaN count per cell, reduced on the GPU in a fixed order)."""
        from hic3defdr_amd.util import apa
        return apa.apa_mean(stack)

    def load_disp_fn(self, cond):
        """Reference ``core.py:220-236`` (after this object's queued write of
        the file has landed)."""
        self._store.wait(self._disp_fn_file(cond))
        with open(self._disp_fn_file(cond), 'rb') as h:
            return pickle.load(h)

    def save_disp_fn(self, cond, disp_fn):
        """Reference ``core.py:238-253``: the object is pickled here (its
        state as of this call), the bytes land on the outdir's write-behind
        queue (flush() / load_disp_fn wait for them; ~0.3 ms per file on the
        GPU box's host otherwise paid inline)."""
        self._store.save_bytes(self._disp_fn_file(cond),
                               pickle.dumps(disp_fn, -1))
