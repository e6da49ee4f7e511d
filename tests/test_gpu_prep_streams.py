"""estimate_disp's prep on two streams against one (GPU).

``H3D_PREP_STREAMS=2`` sorts and gathers conditions 1 .. C-1 on a side
stream of the context while condition 0's sort, its gather, the segment
bounds and the table kernels run on the context's stream; ``=1`` runs one
condition after the other on that stream. The kernels, their inputs and the
order inside each branch are the same, so every result must have the same
bits: ``disp_per_dist``, the segment flags and ``h3d_disp_seg_stats``' qcml
iterations and evaluations are compared on their raw bytes.

Designs: 2+2 (packed records, 32-bit keys), 1+2 (packed, a condition of one
replicate), 3+4 (the tiled gather, a key pass per condition, so the side
branch has a key buffer of its own), 2 (one condition: nothing forks) and
2+2+2 (two conditions follow each other through the side branch's buffers).
Segment lengths cross kChunk = 256 and the sort's and gathers' blocks; the
pixels arrive in no particular order.

Every (switch, case) is a context of its own, opened one after another in
this process (``h3d_open`` reads the switch); each result is computed once
per module. Nothing runs twice to look for a race: a mismatch is read from
the code.
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = (1, 255, 256, 257, 1023, 1025, 4097)
SMALL = (1, 255, 256, 257)
DESIGNS = ((2, 2), (1, 2), (3, 4), (2,), (2, 2, 2))
KEY64_D = 70000     # > 65535 distances: 64-bit keys, sort_by_condition<u64>
KEY64_DISTS = (0, 3, 65536, 69999)
KEY64_LEN = (300, 257, 100, 300)

_cache = {}
_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
_id = lambda d: '+'.join(str(r) for r in d)  # noqa: E731


def _data(design, lengths, dists=None, D=None):
    """NB counts (means 20-200, dispersion 0.02, f in [0.7, 1.4]);
    ``lengths[k]`` pixels at distance ``dists[k]`` (default k) of D, shuffled."""
    dists = tuple(range(len(lengths))) if dists is None else dists
    D = len(lengths) if D is None else D
    key = ('data', design, lengths, dists, D)
    if key not in _cache:
        rng = np.random.RandomState(977 + 17 * sum(design) + len(lengths))
        n, R = sum(lengths), sum(design)
        mu = rng.uniform(20., 200., size=(n, 1))
        f = rng.uniform(0.7, 1.4, size=(n, R))
        size = 1. / 0.02
        raw = rng.negative_binomial(size, size / (size + mu * f)).astype(np.int64)
        dist = np.repeat(np.asarray(dists, dtype=np.int32), lengths)
        perm = rng.permutation(n)
        cond = np.repeat(np.arange(len(design), dtype=np.int32), design)
        _cache[key] = (np.ascontiguousarray(raw[perm]),
                       np.ascontiguousarray(f[perm]),
                       np.ascontiguousarray(dist[perm]), cond, D)
    return _cache[key]


@contextlib.contextmanager
def _open(streams):
    """A context opened with H3D_PREP_STREAMS=streams; the environment is
    restored at once."""
    from hic3defdr_amd import _native
    saved = os.environ.get('H3D_PREP_STREAMS')
    os.environ['H3D_PREP_STREAMS'] = str(streams)
    try:
        ctx = _native.Context(0)
    finally:
        if saved is None:
            os.environ.pop('H3D_PREP_STREAMS', None)
        else:
            os.environ['H3D_PREP_STREAMS'] = saved
    try:
        yield ctx
    finally:
        ctx.close()


def _call(ctx, data):
    """h3d_disp_per_dist: (disp_per_dist, flags, qcml iterations,
    evaluations)."""
    from hic3defdr_amd import _native
    raw, f, dist, cond, D = data
    n, R = raw.shape
    C = int(cond.max()) + 1
    out = np.full((D, C), -7.0)
    flags = np.full((D, C), -7, dtype=np.int32)
    rc = ctx.lib.h3d_disp_per_dist(
        ctx.handle, _p(raw), _p(f), _p(dist), n, R, C, _p(cond), D,
        _native.H3D_EST['qcml'], _p(out), _p(flags))
    # (-3: a segment's search failed -- its flag says so, the other segments'
    # results stand, as in test_gpu_nll_paths.py)
    if rc != -3:
        _native._check(rc, 'h3d_disp_per_dist')
    qi, ev = ctx.disp_seg_stats(D, C)
    return out, flags, qi, ev


def _run(streams, design, lengths, dists=None, D=None):
    """one call on a fresh context"""
    key = ('run', streams, design, lengths, dists, D)
    if key not in _cache:
        with _open(streams) as ctx:
            _cache[key] = _call(ctx, _data(design, lengths, dists, D))
    return _cache[key]


def _same_bits(got, want, what):
    for name, a, b in zip(('disp_per_dist', 'flags', 'iterations',
                           'evaluations'), got, want):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, name)


@pytest.mark.parametrize('design', DESIGNS, ids=_id)
def test_two_streams_equal_one(design):
    one = _run(1, design, LENGTHS)
    two = _run(2, design, LENGTHS)
    print(_id(design), 'evals', one[3].sum(), 'iters', one[2].sum(),
          'disp', one[0][-1])
    _same_bits(two, one, _id(design))
    # the call did search: every condition of two or more replicates
    # evaluated its segments' NLL
    for c, r in enumerate(design):
        if r > 1:
            assert np.all(one[3][:, c] > 0) and np.all(np.isfinite(one[0][:, c]))


def test_no_pixels():
    """n = 0: nothing is sorted, nothing forks; every segment NaN, no flag"""
    raw, f, dist, cond, _ = _data((2, 2), LENGTHS)
    empty = (raw[:0], f[:0], dist[:0], cond, 7)
    res = []
    for streams in (1, 2):
        with _open(streams) as ctx:
            res.append(_call(ctx, empty))
    _same_bits(res[1], res[0], 'n=0')
    assert np.isnan(res[1][0]).all() and not res[1][1].any()


@pytest.mark.parametrize('design', ((2, 2), (3, 4)), ids=_id)
def test_keys_64bit(design):
    """D = 70000: 64-bit keys, a key pass per condition (no packed records
    beyond 16 distance bits), a few hundred pixels at four distances"""
    one = _run(1, design, KEY64_LEN, KEY64_DISTS, KEY64_D)
    two = _run(2, design, KEY64_LEN, KEY64_DISTS, KEY64_D)
    _same_bits(two, one, 'key64 ' + _id(design))
    d = list(KEY64_DISTS)
    print(one[0][d], one[3][d])
    assert np.isfinite(one[0][d]).all() and np.all(one[3][d] > 0)
    empty = np.ones(KEY64_D, dtype=bool)
    empty[d] = False
    assert np.isnan(one[0][empty]).all()


@pytest.mark.parametrize('design', ((2, 2), (3, 4)), ids=_id)
def test_back_to_back_reuse(design):
    """One two-stream context, three calls with nothing between them: a
    small one, a larger one (every scratch slot of both branches regrows),
    the small one again (both branches work in the front of larger buffers).
    Each equals a fresh single-stream context's call."""
    with _open(2) as ctx:
        got = [_call(ctx, _data(design, ln)) for ln in (SMALL, LENGTHS, SMALL)]
    for g, ln in zip(got, (SMALL, LENGTHS, SMALL)):
        _same_bits(g, _run(1, design, ln), 'reuse %s n=%d' % (_id(design), sum(ln)))


def test_user_stream():
    """the context on a non-default torch stream (h3d_set_stream): the side
    stream forks from and joins that stream"""
    import torch
    stream = torch.cuda.Stream(torch.device('cuda', 0))
    with _open(2) as ctx:
        ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            got = _call(ctx, _data((2, 2), LENGTHS))
        stream.synchronize()
    _same_bits(got, _run(1, (2, 2), LENGTHS), 'user stream')
