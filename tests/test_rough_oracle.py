"""oracle.prepare_chrom -- the yardstick of tests/test_gpu_rough.py on the
GPU machine -- held to the reference on the ``rough1`` fixture
(tests/golden/make_golden_rough.py): shallow counts, and bias vectors with
NaN lines that differ between the replicates, so that union pixels carry
``balanced = 0 / NaN`` in some replicate. Integer and bool arrays are equal,
the NaN masks are equal, and what is finite agrees within 1e-13, under the
default norm and under ``median_of_ratios``."""
import warnings

import numpy as np
import pytest

import oracle
from conftest import e2e_inputs, rel_err

NAME = 'rough1'


def _files(kw, c):
    npz = [p.replace('<chrom>', c) for p in kw['raw_npz_patterns']]
    bfs = [p.replace('<chrom>', c) for p in kw['bias_patterns']]
    loops = [p.replace('<chrom>', c) for p in kw['loop_patterns'].values()]
    return npz, bfs, loops


def _same_floats(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=what)
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(np.isfinite(got), fin, err_msg=what)
    err = rel_err(got[fin], ref[fin])
    print('%s: rel_err %.3g over %d finite, %d NaN'
          % (what, err, int(fin.sum()), int(np.isnan(ref).sum())))
    assert err < 1e-13, what


@pytest.mark.parametrize('norm', ['conditional_mor', 'median_of_ratios'])
def test_prepare_chrom_matches_the_reference_on_rough1(norm):
    g, kw = e2e_inputs(NAME)
    key = '%s__%s' if norm == 'conditional_mor' else 'mor__%s__%s'
    nan_rows = 0
    for c in kw['chroms']:
        npz, bfs, loops = _files(kw, c)
        with np.errstate(all='ignore'), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            prep = oracle.prepare_chrom(
                npz, bfs, kw['design'],
                dist_thresh_max=kw['dist_thresh_max'], loop_files=loops,
                norm=norm)
        for st in ('row', 'col', 'raw'):
            np.testing.assert_array_equal(prep[st], g['%s__%s' % (st, c)])
        np.testing.assert_array_equal(prep['disp_idx'],
                                      g[key % ('disp_idx', c)])
        assert prep['disp_idx'].dtype == np.bool_
        if norm == 'conditional_mor':
            np.testing.assert_array_equal(prep['loop_idx'],
                                          g['loop_idx__%s' % c])
        for st in ('size_factors', 'scaled'):
            _same_floats(prep[st], g[key % (st, c)], '%s %s %s' % (norm, st, c))
        assert not np.isnan(prep['size_factors']).any()
        nan_rows += int(np.isnan(prep['scaled']).any(axis=1).sum())
    assert nan_rows >= 50       # the fixture's point


def test_rough1_bias_keeps_its_nan_lines(tmp_path):
    """oracle.load_bias (core.py:35-60) keeps a NaN -- both comparisons with
    the threshold are false -- unless another replicate zeroes the row; the
    product's load_bias gives the same array."""
    import pandas as pd
    from hic3defdr_amd import HiC3DeFDR
    g, kw = e2e_inputs(NAME)
    design = pd.DataFrame(kw['design'], index=kw['reps'], columns=kw['conds'])
    h = HiC3DeFDR(raw_npz_patterns=kw['raw_npz_patterns'],
                  bias_patterns=kw['bias_patterns'], chroms=kw['chroms'],
                  design=design, outdir=str(tmp_path),
                  dist_thresh_max=kw['dist_thresh_max'],
                  loop_patterns=kw['loop_patterns'], res=10000)
    for c in kw['chroms']:
        bias = oracle.load_bias(_files(kw, c)[1])
        assert (np.isnan(bias).sum(axis=0) >= 1).all()  # every replicate
        assert len({tuple(np.flatnonzero(np.isnan(b))) for b in bias.T}) \
            == bias.shape[1]                            # its own lines
        assert np.all(bias == 0, axis=1).sum() >= 8
        np.testing.assert_array_equal(h.load_bias(c), bias)
