"""The GPU balancing operators as far as a machine without a GPU can check
them: the ABI names, the wrappers' argument checks (which fire before any
device call) and the host runs test_gpu_balancing.py compares against."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sparse

from balancing_cases import clamp_matrix, host_run, sim_matrix
from conftest import REPO
from hic3defdr_amd import _native
from hic3defdr_amd import build as h3dbuild

NEW_EXPORTS = ('h3d_kr_balance', 'h3d_filter_sparse_rows')


def test_new_abi_names_declared_listed_exported():
    src = open(os.path.join(REPO, 'include', 'h3d.h')).read()
    declared = set(re.findall(r'\b(h3d_[a-z_]+)\s*\(', src))
    h3dbuild.build_native()
    lib = _native.load_library()
    for name in NEW_EXPORTS:
        assert name in declared
        assert name in _native.EXPORTS
        assert hasattr(lib, name), name
    for name in ('kr_balance', 'filter_sparse_rows'):
        assert callable(getattr(_native.Context, name))
    assert 'h3d_balance.hip' in [s for s, _ in h3dbuild.NATIVE_SRCS]


@pytest.fixture
def no_device_call(monkeypatch):
    """Any attempt to reach the device fails the test."""
    def boom(*a, **k):
        raise AssertionError('device call before the argument check')
    monkeypatch.setattr(_native, 'context', boom)


def test_value_errors_fire_before_any_device_call(no_device_call):
    from hic3defdr_amd.util.balancing import kr_balance_gpu, kr_bias
    from hic3defdr_amd.util.filtering import filter_sparse_rows_count_gpu
    m = sim_matrix('A1', 'chrB')
    wide = sparse.csr_matrix(np.ones((3, 4)))
    for fn in (kr_balance_gpu, kr_bias, filter_sparse_rows_count_gpu):
        with pytest.raises(ValueError):
            fn(wide)
    for fn in (kr_balance_gpu, kr_bias):
        with pytest.raises(ValueError):
            fn(m, tol=-1e-6)
        with pytest.raises(ValueError):
            fn(m, tol=float('nan'))
        with pytest.raises(ValueError):
            fn(m, x0=np.ones((m.shape[0] + 1, 1)))
    # x0 has one value per NON-EMPTY row (after the filter, for kr_bias)
    rows = host_run(m)['rows']
    assert rows.sum() < m.shape[0]
    with pytest.raises(ValueError):
        kr_balance_gpu(m, x0=np.ones((m.shape[0], 1)))
    with pytest.raises(ValueError):
        filter_sparse_rows_count_gpu(m.toarray())
    with pytest.raises(ValueError):
        filter_sparse_rows_count_gpu(m, min_nnz=-1)


def test_x0_is_spread_over_the_rows_of_the_iteration():
    from hic3defdr_amd.util.balancing import _upper_canonical, _x0_by_bin
    from hic3defdr_amd.util.filtering import filter_sparse_rows_count
    m = sim_matrix('A2', 'chrB')
    up, upper = _upper_canonical(m)
    assert upper and (up != m).nnz == 0
    for min_nnz, k in ((0, 0), (25, 300)):
        filt = filter_sparse_rows_count(m, min_nnz, k)
        rows = host_run(filt, max_iter=0)['rows']
        x0 = np.arange(1., rows.sum() + 1)[:, None]
        by_bin = _x0_by_bin(up, x0, min_nnz, k)
        np.testing.assert_array_equal(by_bin[rows], x0.ravel())
        np.testing.assert_array_equal(by_bin[~rows], 1.0)
    # a full symmetric input is balanced from its upper triangle
    full = (m + m.T).tocsr()
    up2, upper2 = _upper_canonical(full)
    assert not upper2 and (up2 != sparse.triu(full)).nnz == 0


def test_filter_refactor_kept_the_host_filter(no_device_call):
    from hic3defdr_amd.util.filtering import (filter_sparse_rows_count,
                                              filter_sparse_rows_count_gpu,
                                              wiped_bins)
    m = sim_matrix('B1', 'chrA')
    wipe = wiped_bins(m)
    filt = filter_sparse_rows_count(m)
    gone = np.asarray(filt.sum(axis=1)).ravel() == 0
    assert wipe.sum() > 0 and np.all(gone[wipe])
    # skipped filter: a copy, no device
    for min_nnz, k in ((0, 300), (25, 0)):
        out = filter_sparse_rows_count_gpu(m, min_nnz, k)
        assert out is not m and (out != m).nnz == 0


def test_no_device_raises_not_fakes():
    lib = _native.load_library()
    if lib.h3d_device_count() > 0:
        pytest.skip('a GPU is visible')
    from hic3defdr_amd.util.balancing import kr_balance_gpu, kr_bias
    from hic3defdr_amd.util.filtering import filter_sparse_rows_count_gpu
    m = sim_matrix('A1', 'chrB')
    for fn in (kr_balance_gpu, kr_bias, filter_sparse_rows_count_gpu):
        with pytest.raises(_native.H3DError):
            fn(m)


@pytest.mark.parametrize('seed,low,high', [(0, 0, 1), (2, 1, 0)])
def test_fixture_guard_host_converges_on_the_clamp_matrices(seed, low, high):
    """The GPU test's comparison target is sound: the host code converges on
    the clamp matrices and takes the clamp the GPU test expects."""
    h = host_run(clamp_matrix(seed))
    assert h['res_sq'] <= 1e-12
    assert (h['low'], h['high']) == (low, high)
    assert h['outer'] <= 20


def test_fixture_guard_stuck_run():
    """Seed 9 from another scattered start vector with delta = 0 stops
    moving: every later Newton step is one CG step that hits the low clamp
    at 0 and returns y = 1. The reference runs to max_iter; without one its
    loop never ends, which is what the GPU code's inner-step guard is for."""
    x0 = 10 ** np.random.default_rng(101).uniform(-2, 2, (96, 1))
    h = host_run(clamp_matrix(9), x0=x0, delta=0, ddelta=1e6, max_iter=60)
    assert h['outer'] == 61 and h['low'] >= 40 and h['res_sq'] > 1
    assert h['norms'][-1] == h['norms'][-20]


def test_fixture_guard_low_clamp_at_zero():
    """Seed 5 from a scattered start vector takes the low clamp with
    delta = 0 (the `lo == 0` return of the box test) and still converges."""
    x0 = 10 ** np.random.default_rng(100).uniform(-2, 2, (96, 1))
    h = host_run(clamp_matrix(5), x0=x0, delta=0, ddelta=1e6)
    assert h['res_sq'] <= 1e-12
    assert (h['low'], h['high']) == (1, 0)
