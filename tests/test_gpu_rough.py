"""The prepare chain on input that is neither clean nor deep: the ``rough1``
fixture (tests/golden/make_golden_rough.py) -- bias vectors with NaN lines
that differ between the replicates, counts thinned to a median of 3 -- and
size-factor inputs with NaN and +inf entries, against the reference's arrays
and the CPU oracle (oracle.prepare_chrom is held to the same fixture by
tests/test_rough_oracle.py).

A union pixel at which a replicate with a NaN bias stores nothing has
``balanced = 0 / NaN = NaN`` there; the row goes on through the size factors
(not an all-positive row), ``scaled`` and ``disp_idx`` (NaN means fail the
threshold). numpy's ``simple_scaling`` takes its geometric mean with
``nanmean``, so a NaN column sum makes that replicate's factor NaN and no
other; ``np.median`` gives NaN where an all-positive row holds ``+inf`` (its
ratio is inf / inf). Every check compares the NaN masks first, then what is
finite at the project's bars (test_gpu_parity.py, test_gpu_e2e.py)."""
import os
import shutil
import tempfile
import warnings

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sparse

import oracle
from conftest import e2e_inputs, rel_err

pytestmark = pytest.mark.gpu

NAME = 'rough1'
RTOL_SF = 1e-13     # size factors, scaled
RTOL_PQ = 1e-6      # disp_per_dist, disp, p, q
RTOL_MU = 1e-8      # mu_hat_*


@pytest.fixture(scope='module')
def ctx():
    from hic3defdr_amd import _native
    return _native.context(0)


def _dev(a):
    import torch
    # (a copy: the shared fixture's arrays are read-only)
    return torch.from_numpy(np.array(a, order='C')).to('cuda:0')


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float64
    return a.view(np.int64)


def _quiet(fn, *a, **k):
    """The oracle with numpy's warnings off (0 / NaN, the median of
    nothing, the mean of an empty slice)."""
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return fn(*a, **k)


def _same_nan_then_close(got, ref, rtol, what):
    """NaN masks equal, no infinity on either side that the other lacks,
    finite values within rtol; returns the measured distance."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=what)
    np.testing.assert_array_equal(np.isinf(got), np.isinf(ref), err_msg=what)
    fin = np.isfinite(ref)
    err = rel_err(got[fin], ref[fin])
    print('%s: rel_err %.3g over %d finite, %d NaN'
          % (what, err, int(fin.sum()), int(np.isnan(ref).sum())))
    assert err < rtol, what
    return err


def _load_rough():
    """The fixture's one chromosome as the reference's prepare_data sees it
    (analysis.py:84-101): bias with its NaN lines, canonical CSRs, and
    balanced = raw / (bias[row] * bias[col]) at the fixture's union pixels.
    Shared by the tests below; none of them writes into it."""
    g, kw = e2e_inputs(NAME)
    assert len(kw['chroms']) == 1
    c = kw['chroms'][0]
    bias = oracle.load_bias([p.replace('<chrom>', c)
                             for p in kw['bias_patterns']])
    mats = []
    for p in kw['raw_npz_patterns']:
        m = sparse.load_npz(p.replace('<chrom>', c)).tocsr()
        m.sum_duplicates()
        mats.append(m)
    row, col, raw = g['row__' + c], g['col__' + c], g['raw__' + c]
    with np.errstate(all='ignore'):
        bal = raw / (bias[row] * bias[col])
    out = dict(g=g, kw=kw, c=c, bias=bias, mats=mats, row=row, col=col,
               raw=raw, bal=bal, dist=(col - row).astype(np.int32),
               n_bins=int(kw['dist_thresh_max'] / 5))
    for a in (bias, row, col, raw, bal, out['dist']):
        a.setflags(write=False)
    return out


@pytest.fixture(scope='module')
def rough():
    return _load_rough()


# -- union --------------------------------------------------------------------

def test_union_with_nan_bias(ctx, rough):
    row, col, raw, bal = ctx.sparse_union(rough['mats'], rough['bias'],
                                          rough['kw']['dist_thresh_max'])
    np.testing.assert_array_equal(row, rough['row'])
    np.testing.assert_array_equal(col, rough['col'])
    np.testing.assert_array_equal(raw, rough['raw'])
    want = rough['bal']
    nan = np.isnan(want)
    assert nan.sum() > 0
    np.testing.assert_array_equal(np.isnan(bal), nan)
    np.testing.assert_array_equal(_bits(bal)[~nan], _bits(want)[~nan])
    # a NaN only where that replicate stores no count on a NaN-bias bin
    assert np.all(raw[nan] == 0)
    print('union: %d pixels, %d NaN balanced values in %d rows'
          % (len(row), int(nan.sum()), int(nan.any(axis=1).sum())))


# -- size factors -------------------------------------------------------------

def _both_entries(ctx, bal, dist, norm, n_bins):
    """The norm through h3d_size_factors and through h3d_size_factors_dev
    (device balanced in, the caller's device buffer out)."""
    import torch
    cond = norm.startswith('conditional')
    n, R = bal.shape
    host = ctx.size_factors(bal, dist if cond else None, norm, n_bins)
    t_bal = _dev(bal)
    t_sf = torch.full((n, R) if cond else (R,), -7.0, dtype=torch.float64,
                      device='cuda:0')
    torch.cuda.synchronize()
    back = ctx.size_factors_dev(t_bal.data_ptr(), dist, n, R, norm, n_bins,
                                d_sf_out=t_sf.data_ptr(), host_out=not cond)
    dev = t_sf.cpu().numpy()
    if not cond:
        np.testing.assert_array_equal(_bits(back), _bits(dev))
    return host, dev


def _oracle_sf(bal, dist, norm, n_bins):
    if norm.startswith('conditional'):
        return _quiet(getattr(oracle, norm), bal, dist, n_bins=n_bins or None)
    return _quiet(getattr(oracle, norm), bal)


MOR_CASES = [('conditional_mor', 8), ('conditional_mor', 0),
             ('median_of_ratios', 0)]


@pytest.mark.parametrize('norm,n_bins', MOR_CASES)
def test_mor_factors_on_rows_with_nan(ctx, rough, norm, n_bins):
    """Rows with a NaN are no ratio rows (NaN > 0 is false): no factor is
    NaN, and all agree with the oracle."""
    bal, dist = rough['bal'], rough['dist']
    assert np.isnan(bal).any(axis=1).sum() >= 50
    ref = _oracle_sf(bal, dist, norm, n_bins)
    assert not np.isnan(ref).any()
    for entry, got in zip(('host', 'dev'),
                          _both_entries(ctx, bal, dist, norm, n_bins)):
        assert not np.isnan(got).any()
        _same_nan_then_close(got, ref, RTOL_SF,
                             '%s n_bins=%d %s' % (norm, n_bins, entry))
    if norm == 'conditional_mor' and n_bins == rough['n_bins']:
        assert rel_err(ref, rough['g']['size_factors__' + rough['c']]) < 1e-13
    if norm == 'median_of_ratios':
        assert rel_err(ref, rough['g']['mor__size_factors__' + rough['c']]) \
            < 1e-13


SCALING_CASES = [('conditional_scaling', 8), ('conditional_scaling', 0),
                 ('simple_scaling', 0)]


@pytest.mark.parametrize('norm,n_bins', SCALING_CASES)
def test_scaling_factors_nan_stays_in_its_replicate(ctx, rough, norm, n_bins):
    """balanced's NaN confined to replicate 0: its column sums are NaN, and
    gmean's nanmean leaves them out, so replicate 0's factors are NaN there
    and every other replicate's are finite (scaling.py:50-65)."""
    bal = rough['bal'].copy()
    other = np.isnan(bal)
    other[:, 0] = False
    bal[other] = 0.0
    assert np.isnan(bal[:, 0]).any() and not np.isnan(bal[:, 1:]).any()
    dist = rough['dist']
    ref = _oracle_sf(bal, dist, norm, n_bins)
    assert np.all(np.isfinite(ref[..., 1:]))
    assert np.isnan(ref[..., 0]).any()
    for entry, got in zip(('host', 'dev'),
                          _both_entries(ctx, bal, dist, norm, n_bins)):
        _same_nan_then_close(got, ref, RTOL_SF,
                             '%s n_bins=%d %s' % (norm, n_bins, entry))
    print('%s n_bins=%d: NaN share of replicate 0 %.3f'
          % (norm, n_bins, float(np.isnan(ref[..., 0]).mean())))


def _with_inf(rough):
    """balanced with +inf in column 2 of at most 3 all-positive rows of one
    distance (a count over a zero bias, which load_bias' whole-row zeros
    cannot produce but the entry points accept): the first distance at which
    the oracle's NaN share of that replicate stays within 1/3 under both
    binnings. Returns (balanced, {n_bins: oracle factors})."""
    bal0, dist = rough['bal'], rough['dist']
    pos = np.all(bal0 > 0, axis=1)
    for d in np.unique(dist):
        rows = np.flatnonzero(pos & (dist == d))[:3]
        if len(rows) == 0:
            continue
        bal = bal0.copy()
        bal[rows, 2] = np.inf
        refs = {nb: _oracle_sf(bal, dist, 'conditional_mor', nb)
                for nb in (0, 8)}
        shares = {nb: float(np.isnan(r[:, 2]).mean())
                  for nb, r in refs.items()}
        if all(0 < s <= 1.0 / 3 for s in shares.values()):
            print('inf rows %s at distance %d: NaN share of replicate 2 %s'
                  % (list(rows), d, shares))
            return bal, refs
    raise AssertionError('no distance keeps the NaN share within 1/3')


@pytest.fixture(scope='module')
def inf_case(rough):
    return _with_inf(rough)


@pytest.mark.parametrize('n_bins', [0, 8])
def test_mor_median_with_inf_in_a_valid_row(ctx, rough, inf_case, n_bins):
    """An all-positive row holding +inf has gmean inf and the ratio inf / inf
    = NaN in that replicate: np.median is NaN for that replicate in that bin
    (and 0-ratios enter the others' medians)."""
    bal, refs = inf_case
    ref = refs[n_bins]
    assert np.isnan(ref[:, 2]).any() and np.isnan(ref[:, 2]).mean() <= 1. / 3
    assert not np.isnan(ref[:, [0, 1, 3]]).any()
    for entry, got in zip(('host', 'dev'),
                          _both_entries(ctx, bal, rough['dist'],
                                        'conditional_mor', n_bins)):
        _same_nan_then_close(got, ref, RTOL_SF,
                             'inf rows n_bins=%d %s' % (n_bins, entry))


def _micro(what):
    """n = 130, R = 3, 40 distances (test_gpu_entry_paths.SF_EDGES' 'many
    bins per wave': a wave of k_mor_keys spans some twenty bins).
    'only inf rows': every all-positive row of one distance holds +inf in
    replicate 1; 'nan row': one row of a distance with other all-positive
    rows holds a NaN."""
    rng = np.random.default_rng(8)
    n, R = 130, 3
    dist = rng.integers(0, 40, n).astype(np.int32)
    bal = np.exp(rng.normal(1, 1, (n, R))) * (rng.random((n, R)) > 0.05)
    pos = np.all(bal > 0, axis=1)
    counts = np.bincount(dist[pos], minlength=40)
    d = int(np.flatnonzero(counts >= 3)[1])
    rows = np.flatnonzero(pos & (dist == d))
    if what == 'only inf rows':
        bal[rows, 1] = np.inf
    else:
        assert what == 'nan row'
        bal[rows[1], 2] = np.nan
    return bal, dist, d


@pytest.mark.parametrize('n_bins', [0, 40])
@pytest.mark.parametrize('what', ['only inf rows', 'nan row'])
def test_mor_micro_cases(ctx, what, n_bins):
    bal, dist, d = _micro(what)
    ref = _oracle_sf(bal, dist, 'conditional_mor', n_bins)
    at = dist == d
    if n_bins == 0:
        if what == 'only inf rows':     # NaN there and nowhere else; the
            assert np.isnan(ref[at, 1]).all()   # others' medians are of 0s
            assert np.isnan(ref).sum() == at.sum()
            assert np.all(ref[at][:, [0, 2]] == 0.0)
        else:                           # the NaN row is left out
            assert np.all(np.isfinite(ref))
    else:
        assert np.isnan(ref).mean() <= 1.0 / 3
        assert np.isnan(ref).any() == (what == 'only inf rows')
    for entry, got in zip(('host', 'dev'),
                          _both_entries(ctx, bal, dist, 'conditional_mor',
                                        n_bins)):
        _same_nan_then_close(got, ref, RTOL_SF,
                             '%s n_bins=%d %s' % (what, n_bins, entry))


# -- scaled and disp_idx --------------------------------------------------------

def test_scale_disp_on_rows_with_nan(ctx, rough):
    """h3d_scale_disp_dev on the fixture's balanced and the GPU's own
    factors: scaled is numpy's quotient bit for bit, every row with a NaN is
    left to numpy's product (flag 2), and the decided flags -- then all of
    them, through Resident.scale_disp -- are the fixture's disp_idx."""
    import torch
    from hic3defdr_amd.analysis.resident import Resident
    g, kw, c = rough['g'], rough['kw'], rough['c']
    bal, dist = rough['bal'], rough['dist']
    n, R = bal.shape
    design = kw['design']
    want_di = g['disp_idx__' + c]
    t_bal, t_row, t_col = _dev(bal), _dev(rough['row']), _dev(rough['col'])
    t_sf = torch.empty((n, R), dtype=torch.float64, device='cuda:0')
    torch.cuda.synchronize()
    ctx.size_factors_dev(t_bal.data_ptr(), dist, n, R, 'conditional_mor',
                         rough['n_bins'], d_sf_out=t_sf.data_ptr(),
                         host_out=False)
    sf = t_sf.cpu().numpy()
    scaled, flag = ctx.scale_disp_dev(
        t_bal.data_ptr(), t_sf.data_ptr(), False, t_row.data_ptr(),
        t_col.data_ptr(), n, R, design, 1.0, 4)
    with np.errstate(all='ignore'):
        want = bal / sf
    nan = np.isnan(want)
    assert nan.any(axis=1).sum() >= 50
    np.testing.assert_array_equal(np.isnan(scaled), nan)
    np.testing.assert_array_equal(_bits(scaled)[~nan], _bits(want)[~nan])
    _same_nan_then_close(scaled, g['scaled__' + c], RTOL_SF, 'scaled')
    assert np.all(flag[nan.any(axis=1)] == 2)
    decided = flag != 2
    np.testing.assert_array_equal(flag[decided] == 1, want_di[decided])
    assert not want_di[nan.any(axis=1)].any()

    class _H(object):
        def _ctx(self):
            return ctx
    holder = {'bal': t_bal, 'sf': t_sf, 'row': t_row, 'col': t_col}
    scaled2, ready, disp_idx = Resident(_H()).scale_disp(holder, design, 1.0,
                                                         4, dist)
    ready()
    np.testing.assert_array_equal(disp_idx, want_di)
    np.testing.assert_array_equal(holder['di'].cpu().numpy().astype(bool),
                                  want_di)
    np.testing.assert_array_equal(np.isnan(scaled2), nan)
    np.testing.assert_array_equal(_bits(scaled2)[~nan], _bits(want)[~nan])


# -- the product ----------------------------------------------------------------

def test_run_to_qvalues_on_rough1(rough):
    """HiC3DeFDR.run_to_qvalues on data/rough1 against every outdir array of
    the reference, stage by stage as test_gpu_e2e.py does it.

    Measured on an MI355X (this test's output): see DESIGN.md, "Rough
    input"."""
    from hic3defdr_amd import HiC3DeFDR
    g, kw, c = rough['g'], rough['kw'], rough['c']
    design = pd.DataFrame(kw['design'], index=kw['reps'], columns=kw['conds'])
    outdir = tempfile.mkdtemp(prefix='h3d_rough_')
    try:
        h = HiC3DeFDR(raw_npz_patterns=kw['raw_npz_patterns'],
                      bias_patterns=kw['bias_patterns'], chroms=kw['chroms'],
                      design=design, outdir=outdir,
                      dist_thresh_max=kw['dist_thresh_max'],
                      loop_patterns=kw['loop_patterns'], res=10000)
        h.run_to_qvalues(verbose=False)
        ld = lambda st: np.load(os.path.join(outdir, '%s_%s.npy' % (st, c)))  # noqa: E731,E501
        for st in ('row', 'col', 'raw', 'disp_idx', 'loop_idx'):
            a = ld(st)
            assert a.dtype == g['%s__%s' % (st, c)].dtype, st
            np.testing.assert_array_equal(a, g['%s__%s' % (st, c)])
        assert not np.isnan(ld('size_factors')).any()
        assert np.isnan(ld('scaled')).any(axis=1).sum() >= 50
        for st in ('size_factors', 'scaled'):
            _same_nan_then_close(ld(st), g['%s__%s' % (st, c)], RTOL_SF, st)
        dpd = np.load(os.path.join(outdir, 'disp_per_dist.npy'))
        _same_nan_then_close(dpd, g['disp_per_dist'], RTOL_PQ,
                             'disp_per_dist')
        for st in ('disp', 'pvalues', 'qvalues'):
            assert not np.isnan(ld(st)).any(), st
            _same_nan_then_close(ld(st), g['%s__%s' % (st, c)], RTOL_PQ, st)
        for st in ('mu_hat_null', 'mu_hat_alt'):
            _same_nan_then_close(ld(st), g['%s__%s' % (st, c)], RTOL_MU, st)
        q, qr = ld('qvalues'), g['qvalues__' + c]
        for fdr in (0.01, 0.05, 0.1):
            np.testing.assert_array_equal(q < fdr, qr < fdr)
            print('q < %g: %d calls' % (fdr, int((qr < fdr).sum())))
    finally:
        shutil.rmtree(outdir, ignore_errors=True)


def test_lrt_alone_on_rough1(ctx, rough):
    """The LRT through the reference's own fitted table (disp_fn at every
    integer distance), as test_gpu_parity.test_lrt_vs_reference: counts of a
    few per replicate, zeros among them, where the reference's array secant
    leaves pixels to brentq."""
    g, kw, c = rough['g'], rough['kw'], rough['c']
    di = g['disp_idx__' + c]
    row, col = rough['row'][di], rough['col'][di]
    raw = rough['raw'][di]
    f = rough['bias'][row] * rough['bias'][col] * g['size_factors__' + c][di]
    assert np.all(np.isfinite(f)) and np.all(f > 0)
    assert np.median(raw) <= 5 and (raw == 0).mean() >= 0.03
    design = kw['design']
    tab = np.stack([g['disp_fn_table__%s' % cond] for cond in kw['conds']],
                   axis=1)
    p, llr, m0, m1, disp = ctx.lrt(raw, f, (col - row).astype(np.int32), tab,
                                   design.argmax(axis=1))
    assert rel_err(disp, g['disp__' + c]) < 1e-12
    assert not np.isnan(p).any()
    _same_nan_then_close(p, g['pvalues__' + c], RTOL_PQ, 'lrt alone: p')
    _same_nan_then_close(m0, g['mu_hat_null__' + c], RTOL_MU,
                         'lrt alone: mu_hat_null')
    _same_nan_then_close(m1, g['mu_hat_alt__' + c], RTOL_MU,
                         'lrt alone: mu_hat_alt')
