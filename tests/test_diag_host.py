"""CPU checks of the diagnostics feature: the ABI carries the new entries,
the numpy restatements of tests/diag_cases.py (the yardstick of
tests/test_gpu_diag.py) agree with np.histogram, np.histogram2d and
scipy.stats themselves, and util/diagnostics.py rejects bad input before a
device is touched."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from conftest import REPO

import diag_cases as dc
from hic3defdr_amd import _native
from hic3defdr_amd import build as h3dbuild
from hic3defdr_amd.util import diagnostics as diag

NEW = ['h3d_group_sums', 'h3d_group_sums_dev', 'h3d_histogram',
       'h3d_histogram_dev', 'h3d_ma_stats', 'h3d_density_grid',
       'h3d_rank_average', 'h3d_corr_matrix', 'h3d_pixel_moments',
       'h3d_balance_pixels']


def test_new_entries_are_declared_listed_and_exported():
    h3dbuild.build_native()
    lib = _native.load_library()
    header = open(os.path.join(REPO, 'include', 'h3d.h')).read()
    declared = set(re.findall(r'\b(h3d_[a-z_]+)\s*\(', header))
    for name in NEW:
        assert name in _native.EXPORTS, name
        assert name in declared, name
        assert hasattr(lib, name), name       # dlsym finds it in libh3d.so
    assert ('h3d_diag.hip', 'hipcc') in h3dbuild.NATIVE_SRCS


# -- the yardstick is numpy / scipy ------------------------------------------

def test_digitize_is_ceil_over_ten():
    d = np.array([0, 1, 10, 11, 1000, 1001, 5000, -3])
    want = np.digitize(d, np.linspace(0, 1000, 101), right=True)
    np.testing.assert_array_equal(want[:6], [0, 1, 1, 2, 100, 101])
    np.testing.assert_array_equal(diag.dd_bins(d), want)
    every = np.arange(0, 1300)
    np.testing.assert_array_equal(
        diag.dd_bins(every),
        np.digitize(every, np.linspace(0, 1000, 101), right=True))


def test_histogram_restatement_is_np_histogram():
    assert np.linspace(0, 1, 21)[1] == 0.05
    v = dc.edge_values()
    for edges in (np.linspace(0, 1, 21), np.array([0.25, 0.75]),
                  np.linspace(-1, 2, 4097)):
        np.testing.assert_array_equal(dc.histogram_ref(v, edges),
                                      np.histogram(v, bins=edges)[0])


def test_density_restatement_is_np_histogram2d():
    rng = np.random.default_rng(0)
    x, y = rng.normal(0, 2, 3000), rng.normal(0, 2, 3000)
    xe, ye = np.linspace(-3, 3, 8), np.linspace(-2, 4, 5)
    x[:8] = xe
    y[:5] = ye
    x[10:13] = [np.inf, -np.inf, np.nan]
    label = rng.integers(-1, 4, 3000).astype(np.int8)
    got = dc.density_ref(x, y, label, 4, xe, ye)
    fin = np.isfinite(x) & np.isfinite(y)
    for l in range(4):
        s = fin & (label == l)
        np.testing.assert_array_equal(
            got[l], np.histogram2d(x[s], y[s], bins=[xe, ye])[0])


@pytest.mark.parametrize('kind', ['counts', 'scaled'])
def test_correlation_restatements_are_scipy(kind):
    import scipy.stats as st
    data = dc.corr_columns(4, kind)
    wide = dc.scipy_corr(dc.corr_columns(9, kind)[:3], 'pearson')
    assert np.all(np.abs(wide[0, 1:]) < 0.999)
    for c in data[:3]:
        np.testing.assert_array_equal(dc.rank_ref(c), st.rankdata(c))
    for corr in ('pearson', 'spearman'):
        ours, theirs = dc.corr_ref(data, corr), dc.scipy_corr(data, corr)
        np.testing.assert_array_equal(np.isnan(ours), np.isnan(theirs))
        ok = ~np.isnan(theirs)
        assert np.abs(ours - theirs)[ok].max() <= 4 * data.shape[1] * dc.U
        assert np.isnan(theirs[2]).all() and np.isnan(theirs[3]).all()
        assert abs(theirs[0, 1] - 1) < 1e-12       # identical columns


def test_ma_fixture_keeps_the_uncompared_pixels_under_one_percent():
    for name in dc.DESIGNS:
        c = dc.ma_case(name)
        _, m, _, label = dc.ma_ref(c['scaled'], c['design'], c['cond_idx'],
                                   c['qvalues'], c['fdr'], c['loop_idx'])
        sig = label >= 2
        sig |= label == -1
        left_out = sig & ~(np.abs(m) > 1e-12)
        assert 4 <= left_out.sum() <= 0.01 * sig.sum()
        np.testing.assert_array_equal(label[:6], [-1, -1, -1, -1, 3, 2])
        assert {0, 1, 2, 3, -1} == set(label.tolist())


# -- rejections, with no device ------------------------------------------------

@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('a rejection must not open a device')
    monkeypatch.setattr(_native, 'context', boom)


def test_rejections_fire_before_a_device_is_touched(no_device):
    x = np.ones(10)
    lab = np.zeros(10, dtype=np.int8)
    e = np.linspace(0, 1, 5)
    # wrong rank or dtype
    with pytest.raises(ValueError):
        diag.value_histogram(np.ones((3, 3)), e)
    with pytest.raises(TypeError):
        diag.value_histogram(np.array(['a', 'b']), e)
    with pytest.raises(ValueError):
        diag.correlation_matrix(np.ones(10))
    with pytest.raises(TypeError):
        diag.density_grid(x, x, np.zeros(10, dtype=np.int64), 4, e, e)
    with pytest.raises(ValueError):
        diag.density_grid(x, x[:5], lab, 4, e, e)
    with pytest.raises(TypeError):
        diag.dd_curves(np.ones(4), np.ones(4), np.ones((4, 2)),
                       np.ones((4, 2)))
    with pytest.raises(ValueError):
        diag.dd_curves(np.arange(4), np.arange(4), np.ones((4, 2)),
                       np.ones((4, 3)))
    with pytest.raises(ValueError):
        diag.mvr_data(np.ones((4, 2)), np.arange(3), np.ones(4))
    with pytest.raises(ValueError):
        diag.mvr_data(np.ones((4, 2)), np.array([0, 1, 2, 4096]), np.ones(4))
    # more than 32 replicates
    with pytest.raises(ValueError, match='32'):
        diag.correlation_matrix(np.ones((33, 10)))
    with pytest.raises(ValueError, match='32'):
        diag.dd_curves(np.arange(4), np.arange(4), np.ones((4, 33)),
                       np.ones((4, 33)))
    with pytest.raises(ValueError, match='32'):
        diag.mvr_data(np.ones((4, 33)), np.arange(4), np.ones(4))
    # edges
    for bad in (np.array([0.0, 0.5, 0.5, 1.0]), np.array([0.0, 1.0, 0.5]),
                np.array([0.0, np.nan, 1.0]), np.array([0.0]),
                np.linspace(0, 1, 4098)):
        with pytest.raises(ValueError):
            diag.value_histogram(x, bad)
        with pytest.raises(ValueError):
            diag.density_grid(x, x, lab, 4, bad, e)
        with pytest.raises(ValueError):
            diag.density_grid(x, x, lab, 4, e, bad)
    with pytest.raises(ValueError, match='4097'):
        diag.value_histogram(x, np.linspace(0, 1, 4098))
    # correlation
    with pytest.raises(ValueError, match='kendall'):
        diag.correlation_matrix(np.ones((2, 10)), correlation='kendall')
    # design / conds / q-values
    design = pd.DataFrame(dc.DESIGNS['2+2'][0], columns=['A', 'B'])
    sc = np.ones((10, 4))
    with pytest.raises(ValueError, match="'Z'"):
        diag.ma_stats(sc, design, ('A', 'Z'), np.ones(10), 0.05)
    with pytest.raises(ValueError):
        diag.ma_stats(sc, design.values, (0, 2), np.ones(10), 0.05)
    with pytest.raises(ValueError):
        diag.ma_stats(sc, design, ('A',), np.ones(10), 0.05)
    with pytest.raises(ValueError):
        diag.ma_stats(np.ones((10, 3)), design, None, np.ones(10), 0.05)
    loop = np.arange(10) % 2 == 0
    with pytest.raises(ValueError, match='4 q-values for 5 loop pixels'):
        diag.ma_stats(sc, design, None, np.ones(4), 0.05, loop_idx=loop)
    with pytest.raises(ValueError, match='9 q-values for 10 loop pixels'):
        diag.ma_stats(sc, design, None, np.ones(9), 0.05)
    with pytest.raises(ValueError):
        diag.ma_stats(sc, design, None, np.ones(5), 0.05,
                      loop_idx=loop.astype(np.int64))


def test_class_has_the_methods_and_rejects_idx_before_loading(tmp_path):
    from hic3defdr_amd import HiC3DeFDR
    for name in ('dd_curves', 'pvalue_distribution', 'qvalue_distribution',
                 'ma_data', 'correlation_matrix', 'dispersion_fit_data',
                 'ddr_data'):
        assert callable(getattr(HiC3DeFDR, name)), name
    design = pd.DataFrame(dc.DESIGNS['2+2'][0], index=list('wxyz'),
                          columns=['A', 'B'])
    h = HiC3DeFDR(['%s/<chrom>.npz' % r for r in 'wxyz'],
                  ['%s/<chrom>.bias' % r for r in 'wxyz'], ['chr1'], design,
                  str(tmp_path / 'out'))
    # (nothing was prepared: any load would raise an IOError instead)
    with pytest.raises(ValueError, match='idx must be loop or disp'):
        h.pvalue_distribution(idx='x')
    with pytest.raises(ValueError, match='idx must be'):
        h.correlation_matrix(idx='x')
    with pytest.raises(ValueError, match='correlation'):
        h.correlation_matrix(correlation='kendall')
