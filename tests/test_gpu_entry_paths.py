"""The host paths of libh3d's entry points that the pipeline tests pass by:
every size-factor norm through both of its entry points and at n = 0, the
union's kept-entry buffers growing while they hold earlier replicates, the
int64 -> int32 count check of each entry point that has one, argument errors
that are only known after a device round trip, and the BH temp buffer shared
by three hipcub operations. Every expectation is the library's behaviour
(checked against the CPU oracle where there is one); the growth cases use a
context of their own, since the suite's shared one has grown its buffers."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sparse

import oracle
from conftest import rel_err

pytestmark = pytest.mark.gpu

EARG, EINPUT = -1, -5


@pytest.fixture(scope='module')
def ctx():
    from hic3defdr_amd import _native
    return _native.context(0)


@pytest.fixture()
def fresh_ctx():
    from hic3defdr_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


# -- size factors -----------------------------------------------------------

def _sf_inputs(R):
    rng = np.random.default_rng(4)
    n = 3000
    dist = rng.integers(0, 40, n).astype(np.int32)
    bal = np.exp(rng.normal(1, 1, (n, R))) * (rng.random((n, R)) > 0.05)
    return n, dist, bal


@pytest.mark.parametrize('R', [3, 6])
@pytest.mark.parametrize('norm,n_bins', [
    ('conditional_mor', 0), ('conditional_mor', 7),
    ('conditional_scaling', 0), ('conditional_scaling', 7),
    ('median_of_ratios', 0), ('simple_scaling', 0)])
def test_size_factors_host_and_device_entry(ctx, norm, n_bins, R):
    import torch
    n, dist, bal = _sf_inputs(R)
    cond = norm.startswith('conditional')
    ref = getattr(oracle, norm)(bal, dist, n_bins=n_bins or None) if cond \
        else getattr(oracle, norm)(bal)
    assert np.all(np.isfinite(ref))   # NaN == NaN must not hide a failure
    got = ctx.size_factors(bal, dist if cond else None, norm, n_bins)
    assert got.shape == ref.shape
    err = rel_err(got, ref)
    print('%s n_bins=%d R=%d rel_err %.3g' % (norm, n_bins, R, err))
    assert err < 1e-13
    # device balanced in, the factors into the caller's device buffer
    t_bal = _dev(bal)
    t_sf = torch.empty(ref.shape, dtype=torch.float64, device='cuda:0')
    torch.cuda.synchronize()
    host = ctx.size_factors_dev(t_bal.data_ptr(), dist, n, R, norm, n_bins,
                                d_sf_out=t_sf.data_ptr(), host_out=not cond)
    if cond:
        assert host is None
    else:
        np.testing.assert_array_equal(host, got)
    np.testing.assert_array_equal(t_sf.cpu().numpy(), got)


# The conditional norms where the shapes above never go: bins much smaller
# than a wave (k_mor_keys counts a bin's valid rows by ballots over the
# wave's bins), a bin without an all-positive row (the median of nothing is
# NaN, and the interpolation carries it to the neighbouring bins' pixels),
# more bins than pixels, one replicate, and a second, partly filled
# grid-stride trip. name: (seed, n, R, n_bins, distances below, emptied).
SF_EDGES = {
    'many bins per wave': (1, 130, 3, 40, 60, False),
    'bin without a valid row': (2, 257, 9, 7, 40, True),
    'distance without a valid row': (4, 193, 8, 0, 40, True),
    'more bins than pixels': (3, 5, 3, 7, 40, False),
    'one replicate, bins': (5, 300, 1, 7, 40, False),
    'one replicate, distances': (6, 300, 1, 0, 40, False),
    'second grid-stride trip': (7, None, 2, 20, 200, False),
}


def _sf_edge_inputs(name, n_full):
    """(bal, dist, n_bins, emptied pixels or None) of an SF_EDGES case,
    drawn as _sf_inputs draws; ``n_full`` stands in for n = None."""
    seed, n, R, n_bins, dmax, emptied = SF_EDGES[name]
    rng = np.random.default_rng(seed)
    n = n or n_full
    if n_bins > n:      # distinct distances: no two bins share their mean
        dist = rng.permutation(dmax)[:n].astype(np.int32)
    else:
        dist = rng.integers(0, dmax, n).astype(np.int32)
    bal = np.exp(rng.normal(1, 1, (n, R))) * (rng.random((n, R)) > 0.05)
    gone = None
    if emptied:     # replicate 0 zeroed throughout one bin / one distance
        gone = oracle.equal_bin(dist, n_bins) == 3 if n_bins else dist == 17
        assert gone.any()
        bal[gone, 0] = 0.0
    return bal, dist, n_bins, gone


def _sf_edge_check(name, norm, got, ref, gone):
    """The NaN masks agree, the finite factors within the project's bound
    for size factors, and the case does what its name says."""
    assert got.shape == ref.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    fin = np.isfinite(ref)
    err = rel_err(got[fin], ref[fin])
    frac = float(np.isnan(ref).mean())
    print('%s %s: rel_err %.3g over %d finite, %.1f %% NaN'
          % (name, norm, err, int(fin.sum()), 100 * frac))
    assert fin.sum() == (~np.isnan(ref)).sum()      # no infinite factor
    assert err < 1e-13
    if norm == 'conditional_mor':
        assert frac <= 1.0 / 3
        if gone is not None:
            assert np.isnan(ref[gone]).all()
    else:
        assert frac == 0.0


@pytest.mark.parametrize('norm', ['conditional_mor', 'conditional_scaling'])
@pytest.mark.parametrize('name', sorted(SF_EDGES))
def test_size_factors_edges(ctx, name, norm):
    import torch
    n_full = torch.cuda.get_device_properties(0).multi_processor_count * \
        8 * 256 + 37    # one more trip than grid_for's widest grid covers
    bal, dist, n_bins, gone = _sf_edge_inputs(name, n_full)
    n, R = bal.shape
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')     # numpy's median of nothing
        ref = getattr(oracle, norm)(bal, dist, n_bins=n_bins or None)
    got = ctx.size_factors(bal, dist, norm, n_bins)
    _sf_edge_check(name, norm, got, ref, gone)
    t_bal = _dev(bal)
    t_sf = torch.empty((n, R), dtype=torch.float64, device='cuda:0')
    torch.cuda.synchronize()
    assert ctx.size_factors_dev(t_bal.data_ptr(), dist, n, R, norm, n_bins,
                                d_sf_out=t_sf.data_ptr(),
                                host_out=False) is None
    _sf_edge_check(name, norm, t_sf.cpu().numpy(), ref, gone)


@pytest.mark.parametrize('R', [3, 6])
def test_size_factors_without_pixels(ctx, R):
    bal = np.empty((0, R))
    dist = np.empty(0, dtype=np.int32)
    for norm in ('conditional_mor', 'conditional_scaling'):
        for nb in (0, 7):
            assert ctx.size_factors(bal, dist, norm, nb).shape == (0, R)
    for norm in ('median_of_ratios', 'simple_scaling'):
        sf = ctx.size_factors(bal, None, norm)
        assert sf.shape == (R,) and np.all(np.isnan(sf))
    np.testing.assert_array_equal(ctx.size_factors(bal, None, 'no_scaling'),
                                  np.ones(R))


@pytest.mark.parametrize('norm', ['conditional_mor', 'conditional_scaling'])
def test_size_factors_one_bin_is_an_argument_error(ctx, norm):
    """One distance bin cannot be interpolated: the library's own error
    (the reference returns NaNs there)."""
    from hic3defdr_amd import _native
    n, dist, bal = _sf_inputs(3)
    with pytest.raises(_native.H3DError) as e:
        ctx.size_factors(bal, dist, norm, 1)
    assert e.value.code == EARG


# -- union ------------------------------------------------------------------

N_BINS = 300


def _random_csr(density, seed, rng):
    m = sparse.random(N_BINS, N_BINS, density=density, random_state=seed,
                      data_rvs=lambda k: rng.integers(0, 6, k)).tocsr()
    m.sort_indices()
    return m


def _union_bias(rng, R):
    bias = np.exp(rng.normal(0, 0.2, (N_BINS, R)))
    bias[rng.random((N_BINS, R)) < 0.03] = 0.0
    return bias


def _check_union(c, mats, bias, dmax):
    row, col, raw, bal = c.sparse_union(mats, bias, dmax)
    with np.errstate(divide='ignore', invalid='ignore'):
        rr, rc = oracle.sparse_union(mats, dist_thresh=dmax, bias=bias.copy())
    np.testing.assert_array_equal(row, rr)
    np.testing.assert_array_equal(col, rc)
    dense = np.stack([m.toarray()[row, col] for m in mats], axis=1)
    np.testing.assert_array_equal(raw, dense)
    with np.errstate(divide='ignore', invalid='ignore'):
        bal_ref = dense / (bias[row] * bias[col])
    np.testing.assert_array_equal(bal, bal_ref)
    assert np.all((col - row >= 0) & (col - row <= dmax))
    return row


def _in_band(m, dmax):
    coo = m.tocoo()
    d = coo.col - coo.row
    return int(np.count_nonzero((d >= 0) & (d <= dmax)))


@pytest.mark.parametrize('middle_empty', [False, True])
def test_union_entry_buffers_grow_with_entries_in_them(fresh_ctx,
                                                       middle_empty):
    """Each replicate at least doubles the in-band entries, so the
    kept-entry buffers are reallocated while they hold the earlier
    replicates' entries (twice; once with an empty middle replicate)."""
    rng = np.random.default_rng(11)
    dmax = 12
    mats = [_random_csr(d, r + 1, rng)
            for r, d in enumerate((0.02, 0.06, 0.2))]
    if middle_empty:
        mats[1] = sparse.csr_matrix((N_BINS, N_BINS))
    band = [_in_band(m, dmax) for m in mats]
    tot = 0
    for b in band:
        assert b == 0 or b >= 2 * tot
        tot += b
    bias = _union_bias(rng, len(mats))
    row = _check_union(fresh_ctx, mats, bias, dmax)
    assert len(row) > 0


def test_union_with_nothing_in_band(fresh_ctx):
    rng = np.random.default_rng(11)
    mats = []
    for r in range(3):
        m = _random_csr(0.05, r + 1, rng).tolil()
        m.setdiag(0)
        m = m.tocsr()
        m.eliminate_zeros()
        m.sort_indices()
        mats.append(m)
    R = len(mats)
    row, col, raw, bal = fresh_ctx.sparse_union(mats, _union_bias(rng, R), 0)
    assert row.shape == (0,) and col.shape == (0,)
    assert raw.shape == (0, R) and bal.shape == (0, R)


# -- counts beyond int32 ----------------------------------------------------

def _count_inputs():
    rng = np.random.default_rng(5)
    n, R, C, D = 2000, 4, 2, 8
    raw = rng.poisson(20, (n, R)).astype(np.int64)
    raw[n // 2, 1] = 2 ** 31
    f = np.exp(rng.normal(0, 0.1, (n, R)))
    dist = rng.integers(0, D, n).astype(np.int32)
    cond = np.array([0, 0, 1, 1], dtype=np.int32)
    return raw, f, dist, cond, C, D


def test_disp_per_dist_rejects_a_count_beyond_int32(ctx):
    from hic3defdr_amd import _native
    raw, f, dist, cond, C, D = _count_inputs()
    with pytest.raises(_native.H3DError) as e:
        ctx.disp_per_dist(raw, f, dist, cond, C, D)
    assert e.value.code == EINPUT


def test_lrt_rejects_a_count_beyond_int32(ctx):
    from hic3defdr_amd import _native
    raw, f, dist, cond, C, D = _count_inputs()
    with pytest.raises(_native.H3DError) as e:
        ctx.lrt(raw, f, dist, np.full((D, C), 0.1), cond)
    assert e.value.code == EINPUT


def test_lrt_poisson_rejects_a_count_beyond_int32(ctx):
    from hic3defdr_amd import _native
    raw, f, dist, cond, C, D = _count_inputs()
    with pytest.raises(_native.H3DError) as e:
        ctx.lrt_poisson(raw, f, cond, C)
    assert e.value.code == EINPUT


def test_union_count_beyond_int32_only_fails_the_device_copy(ctx):
    import torch
    from hic3defdr_amd import _native
    rng = np.random.default_rng(11)
    dmax = 12
    mats = [_random_csr(0.05, r + 1, rng).astype(np.float64)
            for r in range(2)]
    coo = mats[0].tocoo()
    k = np.flatnonzero((coo.col - coo.row >= 0) &
                       (coo.col - coo.row <= dmax) & (coo.data > 0))[0]
    i, j = int(coo.row[k]), int(coo.col[k])
    mats[0][i, j] = float(2 ** 31)
    bias = np.ones((N_BINS, len(mats)))
    row, col, raw, bal = ctx.sparse_union(mats, bias, dmax)
    at = np.flatnonzero((row == i) & (col == j))
    assert len(at) == 1 and raw[at[0], 0] == 2 ** 31
    hold = {}

    def alloc(n, R):
        hold['raw'] = torch.empty((n, R), dtype=torch.int32, device='cuda:0')
        return None, None, hold['raw'].data_ptr(), None
    with pytest.raises(_native.H3DError) as e:
        ctx.sparse_union(mats, bias, dmax, device_alloc=alloc)
    assert e.value.code == EINPUT


# -- argument errors known after a device round trip ------------------------

def test_disp_pixels_dev_checks_the_selected_count(ctx):
    import torch
    from hic3defdr_amd import _native
    rng = np.random.default_rng(6)
    n, R, nb = 2000, 3, 100
    row = rng.integers(0, nb - 20, n).astype(np.int32)
    col = (row + rng.integers(0, 20, n)).astype(np.int32)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    n_disp = int(mask.sum()) + 3
    t = [_dev(row), _dev(col),
         _dev(rng.poisson(5, (n, R)).astype(np.int32)), _dev(np.ones(R)),
         _dev(mask)]
    out = [torch.empty((n_disp, R), dtype=torch.int32, device='cuda:0'),
           torch.empty((n_disp, R), dtype=torch.float64, device='cuda:0'),
           torch.empty(n_disp, dtype=torch.int32, device='cuda:0')]
    torch.cuda.synchronize()
    with pytest.raises(_native.H3DError) as e:
        ctx.disp_pixels_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                            t[3].data_ptr(), True, np.ones((nb, R)),
                            t[4].data_ptr(), n, R, n_disp,
                            *[o.data_ptr() for o in out])
    assert e.value.code == EARG


def test_pixel_f_dev_flags_a_key_outside_the_bias_table(ctx):
    import torch
    from hic3defdr_amd import _native
    rng = np.random.default_rng(6)
    n, R, nb = 2000, 3, 100
    row = rng.integers(0, nb - 20, n).astype(np.int32)
    dist = rng.integers(0, 20, n).astype(np.int32)
    t_chrom = _dev(np.zeros(n, dtype=np.int32))
    t_sfi = _dev(np.zeros(n, dtype=np.int32))
    t_bias = _dev(np.exp(rng.normal(0, 0.2, (nb, R))))
    t_boff = _dev(np.array([0, nb], dtype=np.int64))
    t_sf = _dev(np.ones((1, R)))
    t_soff = _dev(np.array([0, 1], dtype=np.int64))
    t_f = torch.empty((n, R), dtype=torch.float64, device='cuda:0')

    def run(row):
        t_row, t_dist = _dev(row), _dev(dist)
        torch.cuda.synchronize()
        ctx.pixel_f_dev(t_row.data_ptr(), t_dist.data_ptr(),
                        t_chrom.data_ptr(), t_sfi.data_ptr(), n, R,
                        t_bias.data_ptr(), t_boff.data_ptr(), t_sf.data_ptr(),
                        t_soff.data_ptr(), 1, t_f.data_ptr())
    run(row)
    assert np.all(np.isfinite(t_f.cpu().numpy()))
    row[n // 3] = nb   # row + dist >= the chromosome's bias rows
    with pytest.raises(_native.H3DError) as e:
        run(row)
    assert e.value.code == EINPUT


# -- BH temp sizing ---------------------------------------------------------

def test_bh_temp_serves_each_size_in_turn(fresh_ctx):
    """One temp buffer serves the count, the sort and the min-scan: a small
    call, a large one and two small ones again around a block boundary."""
    from hic3defdr_amd import _native
    rng = np.random.default_rng(7)
    for n in (1, 70000, 257, 255):
        p = rng.random(n)
        np.testing.assert_array_equal(fresh_ctx.bh(p), _native.bh(p))
