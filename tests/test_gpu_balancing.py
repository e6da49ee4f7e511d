"""The sparse-bin filter and KR balancing on the GPU (h3d_kr_balance,
h3d_filter_sparse_rows; util.balancing.kr_balance_gpu / kr_bias /
balance_files, util.filtering.filter_sparse_rows_count_gpu) against the
reference's own results (tests/golden/sim_small2.npz) and against the host
code under the same arguments.

The 1e-9 bars are the ones the host code carries against the same goldens
(tests/test_simulation.py): reordering every dot product and mat-vec row of
the host code moves its bias by at most 9.6e-16 on the goldens and 1.4e-15 on
the clamp matrices, and never its step counts, so a difference in the step
counts is a transcription error, not rounding."""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sparse

from balancing_cases import (SIM_KEYS, SIM_SIZES, SIMREPS, clamp_matrix,
                             host_run, sim_matrix)
from conftest import e2e_inputs, golden, rel_err

pytestmark = pytest.mark.gpu


def _ops():
    from hic3defdr_amd.util.balancing import (balance_files, kr_balance,
                                              kr_balance_gpu, kr_bias)
    from hic3defdr_amd.util.filtering import (filter_sparse_rows_count,
                                              filter_sparse_rows_count_gpu)
    return dict(balance_files=balance_files, kr_balance=kr_balance,
                kr_balance_gpu=kr_balance_gpu, kr_bias=kr_bias,
                filt=filter_sparse_rows_count,
                filt_gpu=filter_sparse_rows_count_gpu)


@pytest.fixture(scope='module')
def filtered():
    """The host-filtered golden matrices (left unchanged by the tests)."""
    o = _ops()
    return {key: o['filt'](sim_matrix(*key)) for key in SIM_KEYS}


def _same_as_host(gpu, host):
    """(balanced, bias, history) of the two codes at the 1e-9 / 1e-6 bars."""
    gb, gbias, ghist = gpu
    hb, hbias, hhist = host
    np.testing.assert_array_equal(gbias == 0, hbias == 0)
    assert rel_err(gbias, hbias) < 1e-9
    assert gb.shape == hb.shape and gb.nnz == hb.nnz
    assert rel_err(gb.toarray(), hb.toarray()) < 1e-9
    assert len(ghist) == len(hhist)
    if len(hhist):
        assert rel_err(ghist, hhist) < 1e-6


# ---- 1. reference parity ---------------------------------------------------

@pytest.mark.parametrize('rep,chrom', SIM_KEYS)
def test_reference_parity(rep, chrom, filtered):
    o = _ops()
    g = golden('sim_small2.npz')
    m = sim_matrix(rep, chrom)
    ref = g['bias__%s__%s' % (rep, chrom)]
    host = host_run(filtered[rep, chrom])
    assert host['outer'] == 10 and sum(host['inner']) in (18, 19)

    filt = o['filt_gpu'](m)
    assert filt.nnz == int(g['filt__%s__%s__nnz' % (rep, chrom)])
    np.testing.assert_array_equal(np.asarray(filt.sum(axis=1)).ravel(),
                                  g['filt__%s__%s__rowsum' % (rep, chrom)])
    st_one, st_two = {}, {}
    one = o['kr_bias'](m, stats=st_one)
    _, two, hist = o['kr_balance_gpu'](filt, fl=0, stats=st_two)
    assert len(hist) == 0
    for bias, st in ((one, st_one), (two, st_two)):
        np.testing.assert_array_equal(bias == 0, ref == 0)
        assert rel_err(bias, ref) < 1e-9
        assert st['outer'] == host['outer']
        assert st['inner'] == sum(host['inner'])
        assert (st['low_clamps'], st['high_clamps']) == (0, 0)
        assert st['rows'] == int(host['rows'].sum())
    assert st_one['wiped'] == int((ref == 0).sum()) and st_two['wiped'] == 0


# ---- 2. both clamps ----------------------------------------------------------

@pytest.mark.parametrize('seed,kw,clamps', [
    (0, {}, (0, 1)), (2, {}, (1, 0)), (2, {'delta': 0}, None)])
def test_clamps_match_host(seed, kw, clamps):
    o = _ops()
    m = clamp_matrix(seed)
    host = host_run(m, **kw)
    st = {}
    _same_as_host(o['kr_balance_gpu'](m, fl=0, stats=st, **kw),
                  o['kr_balance'](m, fl=0, **kw))
    assert (st['low_clamps'], st['high_clamps']) == (host['low'], host['high'])
    if clamps is not None:
        assert (st['low_clamps'], st['high_clamps']) == clamps
    assert st['outer'] == host['outer']
    assert st['inner'] == sum(host['inner'])


def test_low_clamp_at_zero_returns_y():
    """The `lo == 0` return taken for real: clamp matrix 5 from a scattered
    start vector with delta = 0 (test_balancing_host.py guards the case)."""
    o = _ops()
    m = clamp_matrix(5)
    kw = dict(delta=0, ddelta=1e6)
    x0 = 10 ** np.random.default_rng(100).uniform(-2, 2, (96, 1))
    host = host_run(m, x0=x0.copy(), **kw)
    assert (host['low'], host['high']) == (1, 0)
    st = {}
    _same_as_host(o['kr_balance_gpu'](m, fl=0, x0=x0.copy(), stats=st, **kw),
                  o['kr_balance'](m, fl=0, x0=x0.copy(), **kw))
    assert (st['low_clamps'], st['high_clamps']) == (1, 0)
    assert st['outer'] == host['outer']
    assert st['inner'] == sum(host['inner'])


def test_inner_step_guard():
    """A run that stops moving (test_balancing_host.py guards the case): the
    reference's loop has no cap without max_iter; here more than 10,000 inner
    steps in total end the call with H3D_ENOCONV. With a max_iter the stuck
    run ends as the host's does."""
    from hic3defdr_amd import _native
    o = _ops()
    m = clamp_matrix(9)
    kw = dict(delta=0, ddelta=1e6)
    x0 = 10 ** np.random.default_rng(101).uniform(-2, 2, (96, 1))
    host = host_run(m, x0=x0.copy(), max_iter=60, **kw)
    st = {}
    _same_as_host(o['kr_balance_gpu'](m, fl=0, x0=x0.copy(), max_iter=60,
                                      stats=st, **kw),
                  o['kr_balance'](m, fl=0, x0=x0.copy(), max_iter=60, **kw))
    assert st['outer'] == host['outer'] == 61
    assert st['low_clamps'] == host['low']
    with pytest.raises(_native.H3DError) as err:
        o['kr_balance_gpu'](m, fl=0, x0=x0.copy(), max_iter=None, **kw)
    assert err.value.code == -3


# ---- 3. arguments --------------------------------------------------------------

@pytest.mark.parametrize('kw,outer', [({'max_iter': 2}, 3), ({'tol': 1e-3}, None),
                                      ({'tol': 1e-9}, None)])
def test_arguments_match_host(kw, outer, filtered):
    o = _ops()
    m = filtered['A1', 'chrA']
    host = host_run(m, **kw)
    st = {}
    _same_as_host(o['kr_balance_gpu'](m, fl=0, stats=st, **kw),
                  o['kr_balance'](m, fl=0, **kw))
    assert st['outer'] == host['outer']
    assert st['inner'] == sum(host['inner'])
    if outer is not None:
        assert st['outer'] == outer


def test_converged_start_vector_takes_no_step(filtered):
    o = _ops()
    m = filtered['B2', 'chrB']
    x = host_run(m)['x']
    st = {}
    _same_as_host(o['kr_balance_gpu'](m, fl=0, x0=x.copy(), stats=st),
                  o['kr_balance'](m, fl=0, x0=x.copy()))
    assert st['outer'] == 0 and st['inner'] == 0
    # the same through kr_bias, whose x0 is over the rows left by the filter
    raw = sim_matrix('B2', 'chrB')
    st = {}
    bias = o['kr_bias'](raw, x0=x.copy(), stats=st)
    assert st['outer'] == 0
    assert rel_err(bias, o['kr_balance'](m, fl=0, x0=x.copy())[1]) < 1e-9


def test_table_and_history_match_host(filtered, capsys):
    o = _ops()
    m = filtered['A2', 'chrA']
    host = o['kr_balance'](m, fl=1)
    host_out = capsys.readouterr().out.split('\n')
    gpu = o['kr_balance_gpu'](m, fl=1)
    gpu_out = capsys.readouterr().out.split('\n')
    _same_as_host(gpu, host)
    assert len(host[2]) == 10
    assert gpu_out[0] == host_out[0] == 'it in. it res'
    assert len(gpu_out) == len(host_out)
    for a, b in zip(gpu_out[1:], host_out[1:]):
        assert a.split()[:2] == b.split()[:2]
        if a:
            assert abs(float(a.split()[2]) / float(b.split()[2]) - 1) < 2e-3


# ---- 4. small shapes -----------------------------------------------------------

def test_small_shapes():
    o = _ops()
    csr = sparse.csr_matrix
    _, bias, _ = o['kr_balance_gpu'](csr(np.array([[4.]])), fl=0)
    np.testing.assert_allclose(bias, [1.], rtol=1e-12)
    d = sparse.diags([[1., 4., 9.]], [0]).tocsr()
    _, bias, _ = o['kr_balance_gpu'](d, fl=0)
    assert rel_err(bias, o['kr_balance'](d, fl=0)[1]) < 1e-9
    # (the expected values as printed, 8 digits)
    np.testing.assert_allclose(bias, [0.46291005, 0.9258201, 1.38873015],
                               rtol=1e-7)
    pair = csr(np.array([[0., 3.], [0., 0.]]))
    bal, bias, _ = o['kr_balance_gpu'](pair, fl=0)
    np.testing.assert_allclose(bias, [1., 1.], rtol=1e-9)
    np.testing.assert_allclose(bal.toarray(), [[0., 3.], [0., 0.]], rtol=1e-9)
    empty = csr((5, 5))
    bal, bias, _ = o['kr_balance_gpu'](empty, fl=0)
    assert bias.shape == (5,) and np.all(np.isnan(bias)) and bal.nnz == 0
    assert np.all(np.isnan(o['kr_bias'](empty)))


def test_embedded_matrix_and_all_wiped(filtered):
    o = _ops()
    m = filtered['A1', 'chrB'].tocoo()
    n = m.shape[0]
    big = sparse.csr_matrix((m.data, (m.row + 7, m.col + 7)),
                            shape=(n + 12, n + 12))
    _, inside, _ = o['kr_balance_gpu'](filtered['A1', 'chrB'], fl=0)
    _, bias, _ = o['kr_balance_gpu'](big, fl=0)
    np.testing.assert_array_equal(bias[:7], 0)
    np.testing.assert_array_equal(bias[n + 7:], 0)
    np.testing.assert_array_equal(bias[7:n + 7] == 0, inside == 0)
    assert rel_err(bias[7:n + 7], inside) < 1e-9
    # a filter that wipes every bin
    raw = sim_matrix('A1', 'chrB')
    st = {}
    bias = o['kr_bias'](raw, min_nnz=10 ** 6, stats=st)
    assert bias.shape == (n,) and np.all(np.isnan(bias))
    assert st['wiped'] == n and st['rows'] == 0 and st['outer'] == 0
    host = o['kr_balance'](o['filt'](raw, min_nnz=10 ** 6), fl=0)[1]
    assert np.all(np.isnan(host))
    assert o['filt_gpu'](raw, min_nnz=10 ** 6).nnz == 0


# ---- 5. the filter alone -------------------------------------------------------

@pytest.mark.parametrize('rep,chrom', SIM_KEYS)
def test_filter_equals_host_on_goldens(rep, chrom):
    o = _ops()
    m = sim_matrix(rep, chrom)
    for min_nnz, k in ((25, 300), (5, 20), (0, 300), (25, 0)):
        a, b = o['filt_gpu'](m, min_nnz, k), o['filt'](m, min_nnz, k)
        assert a.shape == b.shape and a.dtype == b.dtype
        assert (a != b).nnz == 0, (min_nnz, k)


def test_filter_equals_host_on_edge_matrices():
    o = _ops()
    # n < k
    m = clamp_matrix(0)
    for min_nnz, k in ((12, 300), (12, 96), (12, 97), (3, 2)):
        assert (o['filt_gpu'](m, min_nnz, k) != o['filt'](m, min_nnz, k)).nnz \
            == 0
    # explicit zeros and negative values in the band: data > 0 is the test
    rng = np.random.default_rng(7)
    a = np.triu(rng.poisson(0.5, (150, 150)).astype(float))
    i, j = np.nonzero(np.triu(np.ones((150, 150))) * (rng.random((150, 150)) < 0.4))
    vals = a[i, j]
    vals[rng.random(len(vals)) < 0.2] = -2.0
    zeros = sparse.csr_matrix((vals, (i, j)), shape=(150, 150))
    assert (zeros.data == 0).sum() > 100 and (zeros.data < 0).sum() > 100
    for min_nnz, k in ((8, 40), (15, 300)):
        got, want = o['filt_gpu'](zeros, min_nnz, k), o['filt'](zeros, min_nnz, k)
        assert 0 < want.nnz < zeros.nnz
        assert (got != want).nnz == 0
    # entries below the diagonal are wiped with their bins, never counted
    full = (zeros + zeros.T).tocsr()
    assert (o['filt_gpu'](full, 8, 40) != o['filt'](full, 8, 40)).nnz == 0


# ---- 6. determinism -------------------------------------------------------------

def test_reruns_are_bit_identical():
    o = _ops()
    m = sim_matrix('B1', 'chrA')
    first = o['kr_bias'](m)
    o['kr_bias'](clamp_matrix(0), min_nnz=0)   # another shape in between
    np.testing.assert_array_equal(o['kr_bias'](m), first)
    c = clamp_matrix(2)
    a, b = o['kr_balance_gpu'](c, fl=0), o['kr_balance_gpu'](c, fl=0)
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[0].data, b[0].data)


# ---- 7. balance_files ------------------------------------------------------------

def test_balance_files_feeds_the_analysis(tmp_path):
    from hic3defdr_amd import HiC3DeFDR
    o = _ops()
    g = golden('sim_small2.npz')
    _, kw = e2e_inputs('small2')
    sim = str(tmp_path / 'sim')
    os.makedirs(sim)
    chroms = list(SIM_SIZES)
    for rep, chrom in SIM_KEYS:
        sparse.save_npz(os.path.join(sim, '%s_%s_raw.npz' % (rep, chrom)),
                        sim_matrix(rep, chrom))
    written = o['balance_files'](os.path.join(sim, '<rep>_<chrom>_raw.npz'),
                                 SIMREPS, chroms)
    assert len(written) == 8
    for rep, chrom in SIM_KEYS:
        fn = os.path.join(sim, '%s_%s_kr.bias' % (rep, chrom))
        assert fn in written
        ref = g['bias__%s__%s' % (rep, chrom)]
        bias = np.loadtxt(fn)
        np.testing.assert_array_equal(bias == 0, ref == 0)
        assert rel_err(bias, ref) < 1e-9
    design = os.path.join(sim, 'design.csv')
    with open(design, 'wb') as fh:
        fh.write(g['sim_design_csv'].tobytes())
    assert list(pd.read_csv(design, index_col=0).index) == SIMREPS
    hs = HiC3DeFDR(
        raw_npz_patterns=[os.path.join(sim, '%s_<chrom>_raw.npz' % r)
                          for r in SIMREPS],
        bias_patterns=[os.path.join(sim, '%s_<chrom>_kr.bias' % r)
                       for r in SIMREPS],
        chroms=kw['chroms'], design=design,
        outdir=str(tmp_path / 'simout'),
        dist_thresh_max=kw['dist_thresh_max'],
        loop_patterns={'ES': kw['loop_patterns']['ES']})
    hs.run_to_qvalues(verbose=False)
    out = str(tmp_path / 'simout')
    assert rel_err(np.load(os.path.join(out, 'disp_per_dist.npy')),
                   g['simrun__disp_per_dist']) < 1e-6
    for c in kw['chroms']:
        for st in ('pvalues', 'qvalues'):
            got = np.load(os.path.join(out, '%s_%s.npy' % (st, c)))
            assert rel_err(got, g['simrun__%s__%s' % (st, c)]) < 1e-6, st
