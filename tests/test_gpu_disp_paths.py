"""The estimate_disp driver's paths that no other test reaches (GPU).

Every replicate width the driver dispatches on (``mslot`` 2, 4, 8, 16, 32)
through the single-rank and the multi-rank qcml loop, the 64-bit sort keys of
calls with more than 65535 distances, the packed and the tiled gather, a call
without pixels, and distances outside ``[0, D)`` with device-built and with
host-built segment tables. Segment lengths cross ``kChunk`` = 256.

Every case prints a digest of ``(disp_per_dist, flags)`` (``-rP`` shows it):
a change of the driver that is meant to keep the bits is checked by comparing
these lines before and after.

Synthetic NB counts as in test_gpu_nll_paths.py; a context per switch set,
opened in this process; every result and oracle value computed once per
module.
"""
import contextlib
import ctypes
import hashlib
import os

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

# design -> the driver's replicate slot width (the smallest of 2, 4, 8, 16,
# 32 that holds the largest condition); R <= kMaxReps = 32
WIDTHS = (((2, 2), 2), ((3, 4), 4), ((5, 8), 8), ((9, 16), 16),
          ((17, 15), 32))
LENGTHS = (1, 255, 256, 257, 700)   # around kChunk = 256, several chunks
H3D_EARG = -1

_cache = {}
_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731


def _data(design, lengths, dists=None, D=None):
    """NB counts (means 20-200, dispersion 0.02, f in [0.7, 1.4]);
    ``lengths[k]`` pixels at distance ``dists[k]`` (default k) of D."""
    dists = tuple(range(len(lengths))) if dists is None else dists
    D = len(lengths) if D is None else D
    key = ('data', design, lengths, dists, D)
    if key not in _cache:
        rng = np.random.RandomState(4321 + 17 * sum(design) + len(lengths))
        n, R = sum(lengths), sum(design)
        mu = rng.uniform(20., 200., size=(n, 1))
        f = rng.uniform(0.7, 1.4, size=(n, R))
        size = 1. / 0.02
        raw = rng.negative_binomial(size, size / (size + mu * f)).astype(np.int64)
        dist = np.repeat(np.asarray(dists, dtype=np.int32), lengths)
        # (the driver sorts: hand it the pixels in no particular order)
        perm = rng.permutation(n)
        cond = np.repeat(np.arange(len(design), dtype=np.int32), design)
        _cache[key] = (raw[perm], f[perm], dist[perm], cond, D)
    return _cache[key]


@contextlib.contextmanager
def _open(**switches):
    """A context opened with ``switches`` in the environment (h3d_open reads
    them); the environment is restored at once."""
    from hic3defdr_amd import _native
    saved = {k: os.environ.get(k) for k in switches}
    os.environ.update({k: str(v) for k, v in switches.items()})
    try:
        ctx = _native.Context(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        yield ctx
    finally:
        ctx.close()


def _host_call(ctx, data):
    """h3d_disp_per_dist (single rank): (rc, disp_per_dist, flags)."""
    from hic3defdr_amd import _native
    raw, f, dist, cond, D = data
    n, R = raw.shape
    C = int(cond.max()) + 1
    out = np.full((D, C), -7.0)
    flags = np.full((D, C), -7, dtype=np.int32)
    rc = ctx.lib.h3d_disp_per_dist(
        ctx.handle, _p(raw), _p(f), _p(dist), n, R, C, _p(cond), D,
        _native.H3D_EST['qcml'], _p(out), _p(flags))
    return rc, out, flags


def _noop_call(ctx, data):
    """h3d_disp_per_dist_dev with an identity all-reduce: the multi-rank
    driver on one rank. (rc, disp_per_dist, flags, reduce calls)."""
    import torch
    from hic3defdr_amd import _native
    raw, f, dist, cond, D = data
    n, R = raw.shape
    C = int(cond.max()) + 1
    dev = torch.device('cuda', 0)
    t_raw = torch.from_numpy(raw.astype(np.int32)).to(dev).contiguous()
    t_f = torch.from_numpy(f).to(dev).contiguous()
    t_d = torch.from_numpy(dist).to(dev).contiguous()
    torch.cuda.synchronize()
    calls = []

    def _cb(ptr, count, user):
        calls.append(count)
        return 0

    out = np.full((D, C), -7.0)
    flags = np.full((D, C), -7, dtype=np.int32)
    rc = ctx.lib.h3d_disp_per_dist_dev(
        ctx.handle, t_raw.data_ptr(), t_f.data_ptr(), t_d.data_ptr(), n, R, C,
        _p(cond), D, _native.H3D_EST['qcml'], _p(out), _p(flags),
        _native.ALLREDUCE_FN(_cb), None)
    return rc, out, flags, len(calls)


def _digest(what, out, flags):
    h = hashlib.sha256(np.ascontiguousarray(out).tobytes())
    h.update(np.ascontiguousarray(flags).tobytes())
    print('digest %s %s' % (what, h.hexdigest()[:16]))
    return h.hexdigest()


def _ok(rc, what):
    from hic3defdr_amd import _native
    # (-3: a segment's search failed -- its flag says so, the other segments'
    # results stand, as in test_gpu_nll_paths.py)
    if rc != -3:
        _native._check(rc, what)


def _single(design, lengths, dists=None, D=None):
    key = ('single', design, lengths, dists, D)
    if key not in _cache:
        with _open() as ctx:
            rc, out, flags = _host_call(ctx, _data(design, lengths, dists, D))
        _ok(rc, 'h3d_disp_per_dist')
        _cache[key] = (out, flags)
    return _cache[key]


def _oracle(design, lengths, dists=None, D=None):
    """oracle.qcml of every non-empty segment, in (dists, condition) order;
    NaN where the oracle has no value: a one-replicate condition's NLL does
    not depend on the dispersion (see test_gpu_nll_paths._oracle)."""
    key = ('oracle', design, lengths, dists, D)
    if key not in _cache:
        import oracle
        raw, f, dist, cond, _ = _data(design, lengths, dists, D)
        dd = tuple(range(len(lengths))) if dists is None else dists
        want = np.full((len(dd), len(design)), np.nan)
        for k, d in enumerate(dd):
            for c in range(len(design)):
                if design[c] == 1:
                    continue
                m, r = dist == d, cond == c
                want[k, c] = oracle.qcml(raw[m][:, r].astype(float),
                                         f=f[m][:, r])
        _cache[key] = want
    return _cache[key]


def _check_oracle(design, lengths, got, flags, dists=None, D=None):
    """each non-empty segment against the oracle's qcml at
    test_gpu_operators.py's tolerance"""
    want = _oracle(design, lengths, dists, D)
    dd = tuple(range(len(lengths))) if dists is None else dists
    for k, d in enumerate(dd):
        for c in range(len(design)):
            print(design, lengths[k], d, c, got[d, c], want[k, c], flags[d, c],
                  rel_err(got[d, c], want[k, c]))
    for k, d in enumerate(dd):
        for c in range(len(design)):
            if np.isnan(want[k, c]):
                continue
            assert flags[d, c] == 0, (lengths[k], c)
            assert rel_err(got[d, c], want[k, c]) < 1e-6, (lengths[k], c)


@pytest.mark.parametrize('design,mslot', WIDTHS,
                         ids=['%d+%d' % d for d, _ in WIDTHS])
def test_width_single_rank(design, mslot):
    """h3d_disp_per_dist, default switches, every replicate width."""
    out, flags = _single(design, LENGTHS)
    _digest('single %d+%d mslot=%d' % (design + (mslot,)), out, flags)
    _check_oracle(design, LENGTHS, out, flags)


@pytest.mark.parametrize('design,mslot', WIDTHS,
                         ids=['%d+%d' % d for d, _ in WIDTHS])
def test_width_multi_rank(design, mslot):
    """the multi-rank driver (identity all-reduce), every replicate width:
    the oracle's values, and two calls give the same bits."""
    data = _data(design, LENGTHS)
    with _open() as ctx:
        rc, out, flags, ncalls = _noop_call(ctx, data)
        rc2, out2, flags2, _ = _noop_call(ctx, data)
    _ok(rc, 'h3d_disp_per_dist_dev')
    _ok(rc2, 'h3d_disp_per_dist_dev')
    assert ncalls > 10
    _digest('multi %d+%d mslot=%d' % (design + (mslot,)), out, flags)
    np.testing.assert_array_equal(out, out2)
    np.testing.assert_array_equal(flags, flags2)
    _check_oracle(design, LENGTHS, out, flags)


KEY64_D = 70000     # > 65535 distances: the sort keys take 64 bits
KEY64_DISTS = (0, 3, 69999)
KEY64_LEN = (300, 300, 300)


@pytest.mark.parametrize('design', ((2, 2), (3, 4)),
                         ids=lambda d: '%d+%d' % d)
def test_sort_keys_64bit(design):
    """D = 70000: (distance, count) keys of 64 bits. The three segments with
    pixels against the oracle; the empty ones are NaN without a flag (their
    bits are part of the digest)."""
    out, flags = _single(design, KEY64_LEN, KEY64_DISTS, KEY64_D)
    _digest('key64 %d+%d' % design, out, flags)
    _check_oracle(design, KEY64_LEN, out, flags, KEY64_DISTS, KEY64_D)
    empty = np.ones(KEY64_D, dtype=bool)
    empty[list(KEY64_DISTS)] = False
    assert np.isnan(out[empty]).all()
    assert not flags[empty].any()


@pytest.mark.parametrize('design', ((2, 3), (1, 2)),
                         ids=lambda d: '%d+%d' % d)
def test_gather_tiled_and_packed(design):
    """2+3: a condition of three replicates, every condition through the
    tiled gather (k_gather_cond_tile); 1+2: none above two, the packed
    records (k_gather_pack2), one of them with a single replicate."""
    out, flags = _single(design, LENGTHS)
    _digest('gather %d+%d' % design, out, flags)
    _check_oracle(design, LENGTHS, out, flags)


def test_no_pixels():
    """n = 0: the call succeeds; every segment is NaN and carries no flag.
    (Until the driver backed its one reserved chunk slot with an entry, the
    table staging copied 8 bytes out of an empty vector here and the call
    crashed on the host.)"""
    raw, f, dist, cond, _ = _data((2, 2), LENGTHS)
    empty = (raw[:0], f[:0], dist[:0], cond, 7)
    with _open() as ctx:
        rc, out, flags = _host_call(ctx, empty)
    _digest('n=0', out, flags)
    print(out, flags)
    assert rc == 0
    assert np.isnan(out).all()
    assert not flags.any()


@pytest.mark.parametrize('switches', ({}, {'H3D_BRENT': 2}),
                         ids=['device-tables', 'host-tables'])
def test_distance_out_of_range(switches):
    """One pixel at distance D, then one at -1: H3D_EARG both times, and the
    valid call that follows on the same context gives the bits it gave
    before. (Segment bounds are binary searches over [0, n), so the one
    pixel only shortens the last segment or the first.)"""
    raw, f, dist, cond, D = _data((2, 2), LENGTHS)
    with _open(**switches) as ctx:
        rc, out, flags = _host_call(ctx, (raw, f, dist, cond, D))
        _ok(rc, 'h3d_disp_per_dist')
        want = _digest('valid %s' % (switches or 'default'), out, flags)
        for bad in (D, -1):
            d2 = dist.copy()
            d2[17] = bad
            rc, _, _ = _host_call(ctx, (raw, f, d2, cond, D))
            assert rc == H3D_EARG, (bad, rc)
            assert b'dist outside' in ctx.lib.h3d_last_error()
            rc, out, flags = _host_call(ctx, (raw, f, dist, cond, D))
            _ok(rc, 'h3d_disp_per_dist')
            assert _digest('valid after dist=%d' % bad, out, flags) == want
