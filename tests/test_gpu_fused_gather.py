"""The first equalize launch gathers its own rows (GPU).

On the packed path of the single-rank driver (32-bit sort keys, every
condition at most two replicates) ``H3D_EQ_GATHER=1`` (the default) leaves
the prep with the sorts alone: the first ``k_disp_work`` launch of the call
reads each pixel's packed record through its condition's sort order, works
on it and stores it to the sorted rows, which the later qcml iterations
read. ``H3D_EQ_GATHER=0`` runs a gather kernel per condition in the prep.
Both must give the same bits. The segment bounds come from the sorted keys
on either path.

The pixels arrive in a shuffled order, so no sort order is the identity.
One distance per segment; the lengths cross the 64-pixel wave task, the
256-pixel chunk and, with ``H3D_BRENT_LDS_KB=16``, the Brent block and LDS
head. Designs 2+2 (the kFull instantiations), 1+2 and 1+1 (the general M = 2
ones: a one-replicate condition's record carries a duplicate slot), 4+4 and
3+4 (the unpacked path, where the switch changes nothing).

Every configuration is a context of its own (``h3d_open`` reads the
switches); each result is computed once per module.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import rel_err
from test_gpu_nll_paths import _same

pytestmark = pytest.mark.gpu

LENGTHS = (1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097)
DESIGNS = ((2, 2), (1, 2), (1, 1), (4, 4), (3, 4))
ORACLE_MAX_LEN = 1025

_cache = {}


def _data(design, lengths=LENGTHS):
    """test_gpu_nll_paths._data's NB counts (means 20-200, dispersion 0.02, f
    uniform in [0.7, 1.4]), one distance per segment, the pixels shuffled."""
    key = ('data', design, lengths)
    if key not in _cache:
        rng = np.random.RandomState(4321 + 17 * sum(design) + len(design))
        n, R = sum(lengths), sum(design)
        mu = rng.uniform(20., 200., size=(n, 1))
        f = rng.uniform(0.7, 1.4, size=(n, R))
        size = 1. / 0.02
        mean = mu * f
        raw = rng.negative_binomial(size, size / (size + mean)).astype(np.int64)
        dist = np.repeat(np.arange(len(lengths), dtype=np.int32), lengths)
        order = rng.permutation(n)
        assert np.any(np.diff(dist[order]) < 0)
        cond = np.repeat(np.arange(len(design), dtype=np.int32), design)
        _cache[key] = (np.ascontiguousarray(raw[order]),
                       np.ascontiguousarray(f[order]),
                       np.ascontiguousarray(dist[order]), cond)
    return _cache[key]


def _call(raw, f, dist, cond, D, **switches):
    """(return code, disp_per_dist, segment flags, qcml iterations,
    evaluations) of one h3d_disp_per_dist call on a context opened with
    ``switches`` in the environment. The outputs start as NaN / -1, so what
    a failing call leaves in them compares too."""
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
        n, R = raw.shape
        C = int(cond.max()) + 1
        out = np.full((D, C), np.nan, dtype=np.float64)
        flags = np.full((D, C), -1, dtype=np.int32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        rc = ctx.lib.h3d_disp_per_dist(
            ctx.handle, p(raw), p(f), p(dist), n, R, C, p(cond), D,
            _native.H3D_EST['qcml'], p(out), p(flags))
        if rc in (0, -3):
            qi, ev = ctx.disp_seg_stats(D, C)
        else:
            qi = ev = np.zeros((D, C), dtype=np.int32)
    finally:
        ctx.close()
    return rc, out, flags, qi, ev


def _run(design, gather, streams=2, brent=None):
    key = ('run', design, gather, streams, brent)
    if key not in _cache:
        sw = dict(H3D_EQ_GATHER=gather, H3D_PREP_STREAMS=streams,
                  H3D_BRENT_LDS_KB=16)
        if brent is not None:
            sw['H3D_BRENT'] = brent
        raw, f, dist, cond = _data(design)
        _cache[key] = _call(raw, f, dist, cond, len(LENGTHS), **sw)
    return _cache[key]


@pytest.mark.parametrize('brent', (None, 0), ids=('brent-default', 'brent0'))
@pytest.mark.parametrize('streams', (1, 2), ids=('one-stream', 'two-streams'))
@pytest.mark.parametrize('design', DESIGNS, ids=lambda d: '%d+%d' % d)
def test_fused_equals_gather_kernels(design, streams, brent):
    """H3D_EQ_GATHER=1 against =0: the return code, disp_per_dist, the
    segment flags and the qcml iteration / evaluation counts bit for bit.
    Every segment of >= 64 pixels in a condition of >= 2 replicates ran at
    least two qcml iterations: the later ones read the rows that the fused
    first launch wrote, so the comparison covers them."""
    fused = _run(design, 1, streams, brent)
    plain = _run(design, 0, streams, brent)
    print(design, streams, brent, 'rc', fused[0], plain[0],
          'iters', fused[3].sum(), 'evals', fused[4].sum())
    assert fused[0] == plain[0]
    assert fused[0] in (0, -3)
    _same(fused[1:], plain[1:])
    assert np.all(fused[4] > 0)
    for d, ln in enumerate(LENGTHS):
        for c, nr in enumerate(design):
            if ln >= 64 and nr >= 2:
                assert fused[3][d, c] >= 2, (ln, c, fused[3][d, c])


def test_fused_matches_oracle():
    """2+2 on the fused path: every segment of up to 1025 pixels against
    the oracle's qcml at test_gpu_operators.py's 1e-6."""
    import oracle
    design = (2, 2)
    raw, f, dist, cond = _data(design)
    rc, got, flags = _run(design, 1)[:3]
    assert rc == 0
    checked = 0
    for d, ln in enumerate(LENGTHS):
        if ln > ORACLE_MAX_LEN:
            continue
        for c in range(len(design)):
            m, r = dist == d, cond == c
            want = oracle.qcml(raw[m][:, r].astype(float), f=f[m][:, r])
            err = rel_err(got[d, c], want)
            print(ln, c, got[d, c], want, flags[d, c], err)
            assert flags[d, c] == 0, (ln, c)
            assert err < 1e-6, (ln, c, err)
            checked += 1
    assert checked == 2 * sum(ln <= ORACLE_MAX_LEN for ln in LENGTHS)


def _edge_inputs(name):
    design = (2, 2)
    D = len(LENGTHS)
    raw, f, dist, cond = _data(design)
    if name == 'one-pixel-at-D':
        return raw[:1], f[:1], np.array([D], dtype=np.int32), cond, D
    if name == 'one-pixel-negative':
        return raw[:1], f[:1], np.array([-1], dtype=np.int32), cond, D
    if name == 'pixel-at-D-among-many':
        bad = dist.copy()
        bad[len(bad) // 2] = D
        return raw, f, bad, cond, D
    if name == 'negative-among-many':
        bad = dist.copy()
        bad[len(bad) // 3] = -7
        return raw, f, bad, cond, D
    if name == 'n=0':
        return raw[:0], f[:0], dist[:0], cond, D
    assert name == 'C=1'
    return (np.ascontiguousarray(raw[:, :2]), np.ascontiguousarray(f[:, :2]),
            dist, cond[:2], D)


@pytest.mark.parametrize('name', ('one-pixel-at-D', 'one-pixel-negative',
                                  'pixel-at-D-among-many',
                                  'negative-among-many', 'n=0', 'C=1'))
def test_edge_calls_same_code_and_output(name):
    """calls the segment check rejects (a distance of D, a negative one),
    an empty call and a one-condition call: the same return code and the
    same outputs under both switch values"""
    raw, f, dist, cond, D = _edge_inputs(name)
    fused = _call(raw, f, dist, cond, D, H3D_EQ_GATHER=1)
    plain = _call(raw, f, dist, cond, D, H3D_EQ_GATHER=0)
    print(name, 'rc', fused[0], plain[0])
    assert fused[0] == plain[0]
    _same(fused[1:], plain[1:])
    if 'pixel' in name or 'negative' in name:
        assert fused[0] == -1  # bad argument: dist outside [0, D)
    else:
        assert fused[0] == 0
    if name == 'n=0':
        assert np.all(np.isnan(fused[1]))
    if name == 'C=1':
        assert np.all(np.isfinite(fused[1])) and np.all(fused[3][2:] >= 2)
