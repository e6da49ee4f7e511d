"""The Brent NLL kernels' instantiations and loop paths (GPU).

``k_brent`` / ``k_brent_gang`` (and the equalize pass before them) have a
general form (run-time replicate count) and a "full" one for calls whose
conditions all have exactly M replicates (``H3D_NLL_FULL``, default 1). Both
must give the same bits: the same terms are added in the same order. The
segment lengths cross the kernels' wave, trip and LDS-head / streamed-tail
boundaries. Design 2+2 is full at M = 2 and takes the full instantiations;
4+4 is full at M = 4, for which none are built (they spilled), and 1+2 and
3+4 are not full: those three take the general instantiations whatever the
switch says, and the comparison documents that.

Each configuration is a context of its own (the switches are read by
``h3d_open``), opened one after another in this process; every result is
computed once per module and shared by the tests.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

# k_brent: 1024 threads, two pixels per trip (2048); with H3D_BRENT_LDS_KB=16
# the LDS head holds 1024 pixels at M = 2 (at M = 4 its 512 pixels are less
# than a block: no head, everything streamed)
LEN_BRENT = (1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 4097)
# k_brent_gang: 256 threads, trip 512, slices of 1024 pixels
LEN_GANG = (255, 256, 257, 511, 512, 513, 1025)
DESIGNS = ((2, 2), (4, 4), (1, 2), (3, 4))
FULL = {(2, 2): True, (4, 4): False, (1, 2): False, (3, 4): False}

_cache = {}


def _data(design, lengths):
    """Synthetic NB counts, one distance per segment: means 20-200,
    dispersion 0.02, f uniform in [0.7, 1.4]."""
    key = ('data', design, lengths)
    if key not in _cache:
        rng = np.random.RandomState(1234 + 17 * sum(design) + len(lengths))
        n, R = sum(lengths), sum(design)
        mu = rng.uniform(20., 200., size=(n, 1))
        f = rng.uniform(0.7, 1.4, size=(n, R))
        size = 1. / 0.02
        mean = mu * f
        raw = rng.negative_binomial(size, size / (size + mean)).astype(np.int64)
        dist = np.repeat(np.arange(len(lengths), dtype=np.int32), lengths)
        cond = np.repeat(np.arange(len(design), dtype=np.int32), design)
        _cache[key] = (raw, f, dist, cond)
    return _cache[key]


def _run(design, lengths, **switches):
    """(disp_per_dist, segment flags, qcml iterations, evaluations) of one
    call on a context opened with ``switches`` in the environment."""
    key = ('run', design, lengths, tuple(sorted(switches.items())))
    if key in _cache:
        return _cache[key]
    from hic3defdr_amd import _native
    raw, f, dist, cond = _data(design, lengths)
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
        D, C = len(lengths), len(design)
        out = np.empty((D, C), dtype=np.float64)
        flags = np.zeros((D, C), dtype=np.int32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        rc = ctx.lib.h3d_disp_per_dist(
            ctx.handle, p(raw), p(f), p(dist), n, R, C, p(cond), D,
            _native.H3D_EST['qcml'], p(out), p(flags))
        # (-3: a segment's search failed -- its flag says so, the other
        # segments' results stand)
        if rc != -3:
            _native._check(rc, 'h3d_disp_per_dist')
        qi, ev = ctx.disp_seg_stats(D, C)
    finally:
        ctx.close()
    _cache[key] = (out, flags, qi, ev)
    return _cache[key]


def _brent(design, **extra):
    sw = dict(H3D_BRENT=0, H3D_BRENT_LDS_KB=16)
    sw.update(extra)
    return _run(design, LEN_BRENT, **sw)


def _gang(design, **extra):
    return _run(design, LEN_GANG, H3D_BRENT=2, **extra)


def _oracle(design, lengths):
    key = ('oracle', design, lengths)
    if key not in _cache:
        import oracle
        raw, f, dist, cond = _data(design, lengths)
        want = np.empty((len(lengths), len(design)))
        for d in range(len(lengths)):
            for c in range(len(design)):
                m, r = dist == d, cond == c
                if design[c] == 1:
                    # no reference value: the NLL of a one-replicate
                    # condition does not depend on the dispersion (with n = 1
                    # and z = d its four terms cancel), so the reference's
                    # cml minimises rounding noise and its qcml ends where
                    # that noise happens to repeat, or never (3 of these 12
                    # segments ran into the oracle's 1000-iteration guard)
                    want[d, c] = np.nan
                    continue
                want[d, c] = oracle.qcml(raw[m][:, r].astype(float),
                                         f=f[m][:, r])
        _cache[key] = want
    return _cache[key]


def _check_oracle(design, lengths, got, flags):
    """each segment against the oracle's qcml at test_gpu_operators.py's
    tolerance; where the oracle has no value (see _oracle) there is nothing
    to compare the segment with"""
    want = _oracle(design, lengths)
    for d, ln in enumerate(lengths):
        for c in range(len(design)):
            print(design, ln, c, got[d, c], want[d, c], flags[d, c],
                  rel_err(got[d, c], want[d, c]))
    for d, ln in enumerate(lengths):
        for c in range(len(design)):
            if np.isnan(want[d, c]):
                continue
            assert flags[d, c] == 0, (ln, c)
            assert rel_err(got[d, c], want[d, c]) < 1e-6, (ln, c)


def _same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize('design', DESIGNS, ids=lambda d: '%d+%d' % d)
def test_brent_full_equals_general(design):
    """k_brent, H3D_NLL_FULL=1 against =0: disp_per_dist, the segment flags
    and the qcml iteration / evaluation counts bit for bit (1+2 and 3+4 are
    not full: both runs take the general instantiation)."""
    full = _brent(design, H3D_NLL_FULL=1)
    gen = _brent(design, H3D_NLL_FULL=0)
    print(design, 'full' if FULL[design] else 'general both',
          'evals', full[3].sum(), 'iters', full[2].sum())
    _same(full, gen)
    assert np.all(full[3] > 0)


@pytest.mark.parametrize('design', DESIGNS, ids=lambda d: '%d+%d' % d)
def test_gang_full_equals_general(design):
    """k_brent_gang (H3D_BRENT=2), H3D_NLL_FULL=1 against =0, as above."""
    full = _gang(design, H3D_NLL_FULL=1)
    gen = _gang(design, H3D_NLL_FULL=0)
    print(design, 'evals', full[3].sum(), 'iters', full[2].sum())
    _same(full, gen)
    assert np.all(full[3] > 0)


@pytest.mark.parametrize('design', DESIGNS, ids=lambda d: '%d+%d' % d)
def test_brent_matches_oracle(design):
    """every segment against the oracle's qcml (test_gpu_operators.py's call
    and tolerance)"""
    got = _brent(design, H3D_NLL_FULL=1)
    _check_oracle(design, LEN_BRENT, got[0], got[1])


@pytest.mark.parametrize('design', DESIGNS, ids=lambda d: '%d+%d' % d)
def test_gang_matches_oracle(design):
    got = _gang(design, H3D_NLL_FULL=1)
    _check_oracle(design, LEN_GANG, got[0], got[1])


@pytest.mark.parametrize('design', DESIGNS, ids=lambda d: '%d+%d' % d)
def test_brent_head_size_does_not_matter(design):
    """the default LDS head (every segment here fits it: no streamed tail)
    against the 16 KB head, and a 32 KB one: head and tail read the same
    values in the same order. (The head is whole blocks of 1024 pixels: 16
    KB is 1024 pixels at M = 2 and none at M = 4, where 32 KB is 1024. With
    a 512-pixel head -- 16 KB at M = 4 before the head was rounded --
    threads 512.. took other pixels and 16 of the 24 values of 4+4 and of
    3+4 differed from the default head's by up to 2.4e-10 relative.)"""
    small = _brent(design, H3D_NLL_FULL=1)
    sw = dict(H3D_BRENT=0, H3D_NLL_FULL=1)
    default = _run(design, LEN_BRENT, **sw)
    np.testing.assert_array_equal(small[0], default[0])
    mid = _brent(design, H3D_NLL_FULL=1, H3D_BRENT_LDS_KB=32)
    np.testing.assert_array_equal(mid[0], default[0])
