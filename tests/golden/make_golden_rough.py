"""Generates the ``rough1`` fixture by running the REFERENCE on a shallow
dataset whose bias vectors carry NaN lines: tests/golden/data/rough1/ and
tests/golden/e2e_rough1.npz.

Run like make_golden.py (same interpreter, same refshim, the reference
checkout on PYTHONPATH), from the repository root:

    PYTHONPATH=tests/golden/refshim:<reference checkout> \
        PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=agg \
        python3.9 tests/golden/make_golden_rough.py

Recipe (seeds: dataset 3, edits 511 -- see "Seeds" below):

- ``synthetic.write_dataset(base, {'chrA': 300}, dist_thresh_max=40, seed=3,
  clusters_per_chrom=12)``: the clean, deep dataset of the other fixtures;
- with ``default_rng(511)``, replicate after replicate, every stored count x
  becomes ``binomial(x, 0.15)`` and the zeros are dropped: the band is no
  longer stored whole in every replicate, and the surviving pixels sit at a
  few counts;
- then, replicate after replicate, 5 lines of the bias file chosen by
  ``rng.choice(n_bins, 5, replace=False)`` are edited: the first 3 to NaN,
  the 4th to 0.0, the 5th to 20.0. ``load_bias`` keeps the NaN (both of its
  comparisons are false) and zeroes the rows of the other two.

What the reference does with such input (``core.py:56-60``,
``matrices.py:92-129``, ``analysis.py:91-115``): a pixel at which a replicate
with a NaN bias stores a count has a NaN deconvoluted sum and leaves the
union; a pixel at which that replicate stores nothing but another one does
stays, with ``balanced = 0 / NaN = NaN`` in that replicate. Such rows pass
through the size factors (``NaN > 0`` is false: not a valid ratio row),
``scaled`` (NaN) and ``disp_idx`` (``NaN >= mean_thresh`` is false).

e2e_rough1.npz has run_e2e's layout (make_golden.py) with loops on, plus the
reference's ``prepare_data`` alone under ``norm='median_of_ratios'`` as
``mor__size_factors__<chrom>``, ``mor__scaled__<chrom>`` and
``mor__disp_idx__<chrom>``.

Before anything is written into tests/golden the script asserts that the
fixture is not vacuous (not_vacuous below) and that the reference's bounded
dispersion search does not sit on a near-tie: the CPU restatement's
``estimate_disp`` agrees to 1e-8 relative on the prepared pixels in their
order, reversed and under one seeded permutation (a near-tied
Brent step turns a summation-order difference into a 1e-5 move). A failing
seed is replaced by the next one.

Seeds. The edits were first drawn with ``default_rng(1)``. At this depth the
three orders of a clean search already differ by about 1e-8 (segments of some
150 pixels at 3 counts: the NLL is flat, and the last parabolic step of the
search moves with the last bits of its sums), and a near-tied one by 1e-6 to
1e-2; edit seed 1 gave 8.9e-9 reversed and 1.07e-8 permuted, just over the
bar. Edit seeds 1 .. 510 with dataset seed 3 were tried in turn (and dataset
seeds 4 .. 63 with edit seeds 1 and 2): none agreed to 1e-8 except 453, on
which the reference's own lrt stops (its smoothed dispersion is not positive
at one distance, ``scaled_nb.py:139``). Edit seed 511 is the first that
passes every check: 6.0e-9 reversed, 5.6e-9 permuted, bit-equal to the
reference in order. Its counts: 9 NaN bias entries, 20 zeroed bias rows, 9461
union pixels, 72 rows of ``scaled`` with a NaN, 6590 disp pixels (median raw
count 3, 5.4 % zeros), 137 loop pixels, disp_per_dist 1.0e-4 .. 0.17.
"""
import importlib.util
import os
import shutil
import sys
import tempfile

import numpy as np
import pandas as pd
import scipy.sparse as sparse

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

spec = importlib.util.spec_from_file_location(
    'synthetic', os.path.join(REPO, 'hic3defdr_amd', 'synthetic.py'))
synthetic = importlib.util.module_from_spec(spec)
sys.modules['synthetic'] = synthetic
spec.loader.exec_module(synthetic)

import hic3defdr.util.scaling as scaling  # noqa: E402


def equal_bin_stable(data, n_bins):
    idx = np.linspace(0, n_bins, data.size, endpoint=0, dtype=int)
    return idx[data.argsort(kind='stable').argsort(kind='stable')]


scaling.equal_bin = equal_bin_stable

from hic3defdr import HiC3DeFDR  # noqa: E402

sys.path.insert(0, REPO)
from oracle import restatement as orc  # noqa: E402

NAME = 'rough1'
SIZES = {'chrA': 300}
DMAX = 40
DATA_SEED = 3
EDIT_SEED = 511
THIN = 0.15
STAGES = ['row', 'col', 'raw', 'size_factors', 'scaled', 'disp_idx',
          'loop_idx', 'disp', 'pvalues', 'llr', 'mu_hat_null', 'mu_hat_alt',
          'qvalues']
ORDER_RTOL = 1e-8


def write_inputs(base):
    """The recipe of the module docstring; returns write_dataset's kwargs."""
    kw = synthetic.write_dataset(base, SIZES, dist_thresh_max=DMAX,
                                 seed=DATA_SEED, clusters_per_chrom=12)
    rng = np.random.default_rng(EDIT_SEED)
    for chrom in kw['chroms']:
        for pat in kw['raw_npz_patterns']:
            fn = pat.replace('<chrom>', chrom)
            m = sparse.load_npz(fn).tocsr()
            m.data = rng.binomial(m.data, THIN).astype(m.data.dtype)
            m.eliminate_zeros()
            sparse.save_npz(fn, m)
        for pat in kw['bias_patterns']:
            fn = pat.replace('<chrom>', chrom)
            b = np.loadtxt(fn)
            lines = rng.choice(len(b), 5, replace=False)
            b[lines[:3]] = np.nan
            b[lines[3]] = 0.0
            b[lines[4]] = 20.0
            np.savetxt(fn, b)
    return kw


def reference(kw, outdir):
    design = pd.DataFrame(kw['design'], index=kw['reps'], columns=kw['conds'])
    return HiC3DeFDR(raw_npz_patterns=kw['raw_npz_patterns'],
                     bias_patterns=kw['bias_patterns'], chroms=kw['chroms'],
                     design=design, outdir=outdir, dist_thresh_max=DMAX,
                     loop_patterns=kw['loop_patterns'], res=10000)


def collect(kw, tmp):
    """run_e2e's dict (make_golden.py) + the mor__ keys."""
    outdir = os.path.join(tmp, 'out')
    h = reference(kw, outdir)
    h.run_to_qvalues(n_threads=0, verbose=True)
    out = {'meta_equal_bin': np.array('stable'),
           'meta_chroms': np.array(kw['chroms']),
           'meta_reps': np.array(kw['reps']),
           'meta_conds': np.array(kw['conds']),
           'meta_design': kw['design'],
           'meta_dist_thresh_max': np.array(DMAX),
           'meta_loops': np.array(True),
           'meta_data_seed': np.array(DATA_SEED),
           'meta_edit_seed': np.array(EDIT_SEED),
           'meta_thin': np.array(THIN)}
    for chrom in kw['chroms']:
        for st in STAGES:
            out['%s__%s' % (st, chrom)] = np.load(
                os.path.join(outdir, '%s_%s.npy' % (st, chrom)))
    out['disp_per_dist'] = np.load(os.path.join(outdir, 'disp_per_dist.npy'))
    for cond in kw['conds']:
        fn = h.load_disp_fn(cond)
        out['disp_fn_table__%s' % cond] = fn(np.arange(DMAX + 1))
        xs = np.linspace(-3.0, DMAX + 25.0, 997)
        out['disp_fn_xs'] = xs
        out['disp_fn_cont__%s' % cond] = fn(xs)
    outdir2 = os.path.join(tmp, 'out_mor')
    h2 = reference(kw, outdir2)
    h2.prepare_data(norm='median_of_ratios', n_threads=0, verbose=False)
    for chrom in kw['chroms']:
        for st in ('row', 'col', 'raw'):
            assert np.array_equal(
                np.load(os.path.join(outdir2, '%s_%s.npy' % (st, chrom))),
                out['%s__%s' % (st, chrom)])
        for st in ('size_factors', 'scaled', 'disp_idx'):
            out['mor__%s__%s' % (st, chrom)] = np.load(
                os.path.join(outdir2, '%s_%s.npy' % (st, chrom)))
    return out, h


def not_vacuous(out, kw, h):
    """The properties the fixture exists for; returns the counts."""
    stats = {}
    nan_rows = n_px = n_disp = n_loop = 0
    raws = []
    for c in kw['chroms']:
        bias = h.load_bias(c)
        stats['bias NaN entries ' + c] = int(np.isnan(bias).sum())
        stats['bias zeroed rows ' + c] = int(np.all(bias == 0, axis=1).sum())
        scaled = out['scaled__%s' % c]
        nan_rows += int(np.isnan(scaled).any(axis=1).sum())
        n_px += len(scaled)
        assert not np.isnan(out['size_factors__%s' % c]).any()
        assert not np.isnan(out['mor__size_factors__%s' % c]).any()
        di = out['disp_idx__%s' % c]
        n_disp += int(di.sum())
        n_loop += int(out['loop_idx__%s' % c].sum())
        raws.append(out['raw__%s' % c][di])
        assert not np.isnan(out['pvalues__%s' % c]).any()
        assert not np.isnan(out['qvalues__%s' % c]).any()
        assert len(out['qvalues__%s' % c]) == int(out['loop_idx__%s' % c].sum())
    raw = np.concatenate(raws)
    stats.update({'union pixels': n_px, 'scaled rows with a NaN': nan_rows,
                  'disp pixels': n_disp, 'loop pixels': n_loop,
                  'median disp raw count': float(np.median(raw)),
                  'zero share of disp counts': float((raw == 0).mean())})
    assert 50 <= nan_rows <= 0.05 * n_px, stats
    assert n_disp >= 5000 and n_loop >= 100, stats
    assert np.median(raw) <= 5, stats
    assert (raw == 0).mean() >= 0.03, stats
    return stats


def oracle_checks(out, kw):
    """oracle.prepare_chrom reproduces the reference's prepare stage, and
    the dispersion search is not on a near-tie (module docstring)."""
    preps, biases = [], []
    for c in kw['chroms']:
        npz = [p.replace('<chrom>', c) for p in kw['raw_npz_patterns']]
        bfs = [p.replace('<chrom>', c) for p in kw['bias_patterns']]
        loops = [p.replace('<chrom>', c) for p in kw['loop_patterns'].values()]
        with np.errstate(all='ignore'):
            prep = orc.prepare_chrom(npz, bfs, kw['design'],
                                     dist_thresh_max=DMAX, loop_files=loops)
        for st in ('row', 'col', 'raw', 'disp_idx', 'loop_idx'):
            assert np.array_equal(prep[st], out['%s__%s' % (st, c)]), st
        for st in ('size_factors', 'scaled'):
            assert np.array_equal(np.isnan(prep[st]),
                                  np.isnan(out['%s__%s' % (st, c)])), st
        preps.append(prep)
        biases.append(orc.load_bias(bfs))

    def ordered(order_of):
        ps = []
        for p, b in zip(preps, biases):
            di = np.flatnonzero(p['disp_idx'])
            sel = di[order_of(len(di))]
            ps.append(dict(row=p['row'][sel], col=p['col'][sel],
                           raw=p['raw'][sel],
                           size_factors=p['size_factors'][sel],
                           disp_idx=np.ones(len(sel), dtype=bool)))
        return orc.estimate_disp(ps, biases, kw['design'],
                                 dist_thresh_max=DMAX)[1]
    rng = np.random.default_rng(0)
    dpds = [ordered(lambda n: np.arange(n)),
            ordered(lambda n: np.arange(n)[::-1]),
            ordered(lambda n: rng.permutation(n))]
    ref = out['disp_per_dist']
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(dpds[0]))
    spread = [float(np.max(np.abs(d[fin] - dpds[0][fin]) / dpds[0][fin]))
              for d in dpds[1:]]
    for d in dpds[1:]:
        rel = np.where(fin, np.abs(d - dpds[0]) / dpds[0], 0.0)
        at = np.unravel_index(np.argmax(rel), rel.shape)
        print('  widest move at (distance, condition) %s: %.17g -> %.17g'
              % (at, dpds[0][at], d[at]))
    vs_ref = float(np.max(np.abs(dpds[0][fin] - ref[fin]) / ref[fin]))
    print('oracle estimate_disp: reversed / permuted vs in order %s, in '
          'order vs the reference %.3g' % (spread, vs_ref))
    assert max(spread) <= ORDER_RTOL and vs_ref <= ORDER_RTOL, \
        'near-tied search: take the next seed'


def main():
    tmp = tempfile.mkdtemp(prefix='h3golden_rough_')
    try:
        base = os.path.join(tmp, 'data')
        kw = write_inputs(base)
        out, h = collect(kw, tmp)
        stats = not_vacuous(out, kw, h)
        for k in sorted(stats):
            print('%s: %s' % (k, stats[k]))
        print('disp_per_dist range %.3g .. %.3g' % (
            np.nanmin(out['disp_per_dist']), np.nanmax(out['disp_per_dist'])))
        oracle_checks(out, kw)
        dest = os.path.join(HERE, 'data', NAME)
        shutil.rmtree(dest, ignore_errors=True)
        shutil.copytree(base, dest)
        np.savez_compressed(os.path.join(HERE, 'e2e_%s.npz' % NAME), **out)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
