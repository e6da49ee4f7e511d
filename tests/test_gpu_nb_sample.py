"""The sampling kernels of libh3d.so (csrc/h3d_sim.hip) on the GPU:
h3d_nb_sample / _dev and the fused h3d_simulate_dev.

What holds a count to scipy is tests/test_nb_draw_host.py, through
h3dt_nb_draw of the self-test library. Here the kernels are tied to that
unit bit for bit on the same device, and to the stream contract: a draw is a
function of (seed, stream, replicate, pixel index) and of nothing else, so
launch tails, slices, reruns and a second context all give the same bits.

simulate_dev's biased means are checked through a debug plane of the
self-test library (h3dt_sim_bm: the kernel's sim_bm on the device) against
numpy in the reference's association, bit for bit; its counts then equal
nb_sample fed those numpy means."""
import ctypes

import numpy as np
import pytest

from hic3defdr_amd import _native
from unit_abi import load_gfx950

pytestmark = pytest.mark.gpu

N = 4097
SEED, STREAM, REP = (0x1E3779B9 << 32) | 12345, 3, 5   # a seed with a high word
VP = ctypes.c_void_p


@pytest.fixture(scope='module')
def ctx():
    return _native.context()


@pytest.fixture(scope='module')
def selftest(ctx):
    lib = load_gfx950()
    lib.h3dt_nb_draw.restype = ctypes.c_int
    lib.h3dt_sim_bm.restype = ctypes.c_int
    return lib


@pytest.fixture(scope='module')
def inputs():
    """Means and dispersions over the whole range of tests/test_nb_draw_host's
    grid, mixed lane by lane (every Poisson path inside one wave), with runs
    of equal values as neighbouring pixels of one distance have."""
    rng = np.random.default_rng(17)
    bm = 10 ** rng.uniform(-3, np.log10(2e4), N)
    disp = 10 ** rng.uniform(-4, np.log10(5), N)
    bm[1000:1400] = 30.0
    disp[1000:1400] = 0.02
    bm.setflags(write=False)
    disp.setflags(write=False)
    return bm, disp


@pytest.fixture(scope='module')
def full(ctx, inputs):
    counts, lam, fl = ctx.nb_sample(*inputs, SEED, STREAM, REP,
                                    want_lambda=True)
    assert fl == 0 and counts.dtype == np.int32 and np.all(counts >= 0)
    assert np.all(np.isfinite(lam)) and len(np.unique(counts)) > 50
    counts.setflags(write=False)
    lam.setflags(write=False)
    return counts, lam


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and \
        a.tobytes() == b.tobytes()


def uniforms(lib, seed, stream, rep, pixels):
    n = len(pixels)
    ctr = np.empty((n, 4), dtype=np.uint32)
    px = np.asarray(pixels, dtype=np.uint64)
    ctr[:, 0] = px & np.uint64(0xFFFFFFFF)
    ctr[:, 1] = px >> np.uint64(32)
    ctr[:, 2] = rep
    ctr[:, 3] = stream
    key = np.empty((n, 2), dtype=np.uint32)
    key[:, 0] = seed & 0xFFFFFFFF
    key[:, 1] = seed >> 32
    out = np.empty((n, 4), dtype=np.uint32)
    u = np.empty((n, 2))
    lib.h3dt_philox(ctypes.c_int64(n), ctr.ctypes.data_as(VP),
                    key.ctypes.data_as(VP), out.ctypes.data_as(VP),
                    u.ctypes.data_as(VP))
    return np.ascontiguousarray(u[:, 0]), np.ascontiguousarray(u[:, 1])


def unit_draw(lib, bm, disp, u1, u2):
    n = len(bm)
    lam = np.empty(n)
    k = np.empty(n, dtype=np.int32)
    bm, disp = np.ascontiguousarray(bm), np.ascontiguousarray(disp)
    fl = lib.h3dt_nb_draw(ctypes.c_int64(n), bm.ctypes.data_as(VP),
                          disp.ctypes.data_as(VP), u1.ctypes.data_as(VP),
                          u2.ctypes.data_as(VP), lam.ctypes.data_as(VP),
                          k.ctypes.data_as(VP), None)
    return k, lam, fl


@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 257, N])
def test_launch_tails(ctx, inputs, full, n):
    bm, disp = inputs
    counts, lam, fl = ctx.nb_sample(bm[:n], disp[:n], SEED, STREAM, REP,
                                    want_lambda=True)
    assert fl == 0 and counts.shape == (n,) and lam.shape == (n,)
    assert same_bits(counts, full[0][:n]) and same_bits(lam, full[1][:n])
    only, none, _ = ctx.nb_sample(bm[:n], disp[:n], SEED, STREAM, REP)
    assert none is None and same_bits(only, counts)


@pytest.mark.parametrize('a,b', [(37, 3001), (1, 2), (4033, N), (63, 129)])
def test_slice_with_its_offset_equals_the_slice_of_the_whole(ctx, inputs,
                                                             full, a, b):
    bm, disp = inputs
    counts, lam, fl = ctx.nb_sample(bm[a:b], disp[a:b], SEED, STREAM, REP,
                                    pixel0=a, want_lambda=True)
    assert fl == 0
    assert same_bits(counts, full[0][a:b]) and same_bits(lam, full[1][a:b])


def test_every_coordinate_of_the_stream_matters(ctx, inputs, full):
    bm, disp = inputs
    for kw in (dict(seed=SEED + 1), dict(stream=STREAM + 1),
               dict(rep=REP + 1), dict(pixel0=1),
               dict(seed=SEED ^ (1 << 40))):
        args = dict(seed=SEED, stream=STREAM, rep=REP, pixel0=0)
        args.update(kw)
        _, lam, _ = ctx.nb_sample(bm, disp, want_lambda=True, **args)
        assert np.mean(lam != full[1]) > 0.99, kw


def test_reruns_and_a_second_context(ctx, inputs, full):
    bm, disp = inputs
    for _ in range(2):
        counts, lam, _ = ctx.nb_sample(bm, disp, SEED, STREAM, REP,
                                       want_lambda=True)
        assert same_bits(counts, full[0]) and same_bits(lam, full[1])
    other = _native.Context(ctx.device)
    try:
        counts, lam, _ = other.nb_sample(bm, disp, SEED, STREAM, REP,
                                         want_lambda=True)
    finally:
        other.close()
    assert same_bits(counts, full[0]) and same_bits(lam, full[1])


def test_device_tensors(ctx, inputs, full):
    import torch
    dev = torch.device('cuda', ctx.device)
    bm, disp = (torch.from_numpy(np.array(a)).to(dev) for a in inputs)
    counts, lam, fl = ctx.nb_sample_dev(bm, disp, SEED, STREAM, REP,
                                        want_lambda=True)
    assert fl == 0 and counts.dtype == torch.int32
    assert same_bits(counts.cpu().numpy(), full[0])
    assert same_bits(lam.cpu().numpy(), full[1])
    a, b = 129, 1000
    counts, lam, _ = ctx.nb_sample_dev(bm[a:b], disp[a:b], SEED, STREAM, REP,
                                       pixel0=a)
    assert lam is None and same_bits(counts.cpu().numpy(), full[0][a:b])
    with pytest.raises(ValueError):
        ctx.nb_sample_dev(bm.float(), disp, SEED)
    with pytest.raises(ValueError):
        ctx.nb_sample_dev(bm, disp[:-1], SEED)


@pytest.mark.parametrize('pixel0', [0, 2 ** 31 - 100, 2 ** 33 + 5])
def test_kernel_equals_the_unit_entry(ctx, selftest, inputs, pixel0):
    """Counts and lambda = h3dt_nb_draw on the uniforms h3dt_philox gives for
    the documented counters, on the same device -- also where the pixel index
    crosses 2^31 and where it has a high word."""
    bm, disp = inputs
    counts, lam, fl = ctx.nb_sample(bm, disp, SEED, STREAM, REP,
                                    pixel0=pixel0, want_lambda=True)
    u1, u2 = uniforms(selftest, SEED, STREAM, REP,
                      pixel0 + np.arange(N, dtype=np.uint64))
    k, lam_u, fl_u = unit_draw(selftest, bm, disp, u1, u2)
    assert fl == 0 and fl_u == 0
    assert same_bits(counts, k) and same_bits(lam, lam_u)


def test_bad_elements(ctx, inputs, full):
    bm, disp = (np.array(a) for a in inputs)
    bad = {5: (0.0, None), 64: (None, -1.0), 700: (np.inf, None),
           4096: (None, np.nan), 2000: (1e13, 0.01)}
    for i, (m, d) in bad.items():
        if m is not None:
            bm[i] = m
        if d is not None:
            disp[i] = d
    counts, lam, fl = ctx.nb_sample(bm, disp, SEED, STREAM, REP,
                                    want_lambda=True)
    assert fl == 16
    keep = np.ones(N, dtype=bool)
    keep[list(bad)] = False
    assert np.all(counts[~keep] == -1)
    assert same_bits(counts[keep], full[0][keep])
    assert same_bits(lam[keep], full[1][keep])


def test_argument_errors(ctx, inputs):
    bm, disp = inputs
    with pytest.raises(ValueError):
        ctx.nb_sample(bm, disp[:-1], SEED)
    with pytest.raises(ValueError):
        ctx.nb_sample(bm, disp, -1)
    with pytest.raises(ValueError):
        ctx.nb_sample(bm, disp, SEED, stream=2 ** 32)
    with pytest.raises(ValueError):
        ctx.nb_sample(bm, disp, SEED, pixel0=-1)


# --- the fused form ---------------------------------------------------------

N_BINS, WIDTH = 600, 9      # 600 x 9 band minus the corner: 5364 pixels


@pytest.fixture(scope='module')
def band():
    row, col = np.array([(r, c) for r in range(N_BINS)
                         for c in range(r, min(r + WIDTH, N_BINS))]).T
    row, col = row[:N].astype(np.int32), col[:N].astype(np.int32)
    rng = np.random.default_rng(23)
    dist = col - row
    mean_a = 10 ** rng.uniform(-2, 3, N) / (1 + dist)
    mean_b = mean_a * np.where(rng.uniform(size=N) < 0.1, 1.5, 1.0)
    table = 0.005 + 0.01 * np.arange(WIDTH) ** 1.5
    return row, col, mean_a, mean_b, table


def sim_inputs(band, J, per_dist):
    rng = np.random.default_rng([J, int(per_dist)])
    bias = rng.uniform(0.3, 3, (N_BINS, J))
    sf = rng.uniform(0.5, 2, (WIDTH, J) if per_dist else J)
    return bias, sf


@pytest.mark.parametrize('per_dist', [False, True], ids=['sf1d', 'sf2d'])
@pytest.mark.parametrize('J', [1, 2, 4, 8, 32])
def test_simulate_dev(ctx, selftest, band, J, per_dist):
    import torch
    row, col, mean_a, mean_b, table = band
    bias, sf = sim_inputs(band, J, per_dist)
    dist = col - row
    # numpy in the reference's association (simulation.py:187-194)
    bm = np.empty((J, N))
    for j in range(J):
        m = mean_a if j < J // 2 else mean_b
        s = sf[dist, j] if per_dist else sf[j]
        f = bias[row, j] * bias[col, j] * s
        bm[j] = m * f
    disp = table[dist]
    # the kernel's own product, from the self-test library's debug plane
    bm_dev, disp_dev = np.empty((J, N)), np.empty((J, N))
    rc = selftest.h3dt_sim_bm(
        ctypes.c_int64(N), J, N_BINS, WIDTH, row.ctypes.data_as(VP),
        col.ctypes.data_as(VP), mean_a.ctypes.data_as(VP),
        mean_b.ctypes.data_as(VP), bias.ctypes.data_as(VP),
        sf.ctypes.data_as(VP), WIDTH if per_dist else 1,
        table.ctypes.data_as(VP), bm_dev.ctypes.data_as(VP),
        disp_dev.ctypes.data_as(VP))
    assert rc == 0
    assert same_bits(bm_dev, bm)
    assert same_bits(disp_dev, np.broadcast_to(disp, (J, N)))
    dev = torch.device('cuda', ctx.device)
    t = [torch.from_numpy(a).to(dev)
         for a in (row, col, mean_a, mean_b, bias, sf, table)]
    pixel0 = 11
    counts, fl = ctx.simulate_dev(*t, seed=SEED, stream=STREAM, pixel0=pixel0)
    assert fl == 0 and tuple(counts.shape) == (J, N)
    counts = counts.cpu().numpy()
    for j in range(J):
        want, _, _ = ctx.nb_sample(bm[j], disp, SEED, STREAM, rep=j,
                                   pixel0=pixel0)
        assert same_bits(counts[j], want), j
    # again: the same bits
    again, _ = ctx.simulate_dev(*t, seed=SEED, stream=STREAM, pixel0=pixel0)
    assert same_bits(again.cpu().numpy(), counts)


def test_simulate_dev_bad_pixels_and_arguments(ctx, band):
    import torch
    row, col, mean_a, mean_b, table = band
    J = 4
    bias, sf = sim_inputs(band, J, True)
    dev = torch.device('cuda', ctx.device)

    def run(row_, col_, bias_=bias):
        t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
             for a in (row_, col_, mean_a, mean_b, bias_, sf, table)]
        counts, fl = ctx.simulate_dev(*t, seed=SEED, stream=STREAM)
        return counts.cpu().numpy(), fl

    good, fl = run(row, col)
    assert fl == 0 and np.all(good >= 0)
    r2, c2 = row.copy(), col.copy()
    r2[10], c2[10] = -1, 3                 # row below 0
    c2[100] = N_BINS                       # col beyond the bins
    r2[1000], c2[1000] = 50, 49            # negative distance
    r2[2000], c2[2000] = 5, 5 + WIDTH      # distance beyond the table
    bad = [10, 100, 1000, 2000]
    counts, fl = run(r2, c2)
    assert fl == 16 and np.all(counts[:, bad] == -1)
    keep = np.ones(N, dtype=bool)
    keep[bad] = False
    assert same_bits(counts[:, keep], good[:, keep])
    b2 = bias.copy()
    b2[row[300], 2] = np.nan               # a bias that is not finite
    counts, fl = run(row, col, b2)
    hit = (row == row[300]) | (col == row[300])
    assert fl == 16 and np.all(counts[2, hit] == -1)
    assert same_bits(counts[:, ~hit], good[:, ~hit])
    assert same_bits(counts[[0, 1, 3]], good[[0, 1, 3]])
    t = [torch.from_numpy(a).to(dev)
         for a in (row, col, mean_a, mean_b, bias, sf, table)]
    with pytest.raises(ValueError):
        ctx.simulate_dev(t[0].long(), *t[1:], seed=SEED)
    with pytest.raises(ValueError):
        ctx.simulate_dev(*t[:5], t[5][:3], t[6], seed=SEED)
    with pytest.raises(ValueError):
        ctx.simulate_dev(*t, seed=None)
