"""The NLL term's r >= 5 and n r >= 5 forms (GPU): same bits as the general
form.

``nll_pixel_r5`` (mode 3: r >= 5 and n r >= 10) and ``nll_pixel_nr5`` (mode
4: n r >= 5) compute only what ``nll_pixel``'s per-lane selects pick in their
ranges (csrc/h3d_model.h), so every value must be bit-identical:

- the per-pixel terms through the gfx950 self-test library
  (``h3dt_nll_terms``), forms 3 and 4 against form 0 at the edges of their
  ranges, with pseudodata that puts the lgamma arguments d + r and z + n r on
  the shift thresholds 5 and 10 and one ulp to either side;
- whole searches with ``H3D_NLL_RANGES=1`` against ``=0`` under ``k_brent``
  and the gang kernel: ``disp_per_dist``, the segment flags and the
  iteration / evaluation counts. Every bounded search opens at r = 1.64,
  0.63, 3.28, 5.92 (tools/brent_points.py), so each search of a condition of
  two or more replicates runs the new dispatch. 1+3 has a single-replicate
  condition (general form whatever the switch says) and takes the general
  (M = 4) instantiations; 2+2 takes the full ones.
"""
import ctypes

import numpy as np
import pytest

from unit_abi import load_gfx950
from test_gpu_nll_paths import _run, _same

pytestmark = pytest.mark.gpu

D = ctypes.POINTER(ctypes.c_double)

# k_brent: 1024 threads, two pixels per trip; with H3D_BRENT_LDS_KB=16 the
# LDS head is 1024 pixels at M = 2, so 1025.. cross it into the streamed tail
LENGTHS = (1, 1023, 1024, 1025, 2047, 2048, 2049)
DESIGNS = ((2, 2), (1, 3))

_cache = {}


def _lib():
    if 'lib' not in _cache:
        _cache['lib'] = load_gfx950()
    return _cache['lib']


def _delta_for(r):
    """a delta whose r = 1 / delta - 1 (nll_const's arithmetic) is >= r,
    by as little as the rounding allows"""
    delta = 1. / (1. + r)
    while 1. / delta - 1 < r:
        delta = np.nextafter(delta, 0.)
    return delta


def _near(v):
    """v and its neighbours up to three ulps either side, >= 0"""
    out = [v]
    lo = hi = v
    for _ in range(3):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return [x for x in out if x >= 0.]


def _pseudo(r, n):
    """(pixels, n) pseudodata: 0, 1e-300, a spread up to 200, and the values
    that put d + r and z + n r at 5 and 10 +- a few ulps"""
    nr = n * r
    rng = np.random.RandomState(int(r * 100) + n)
    rows = [np.zeros(n), np.full(n, 1e-300), np.full(n, 200.),
            np.r_[200., np.zeros(n - 1)], np.r_[1e-300, np.full(n - 1, 200.)]]
    for t in (5., 10.):
        for d in _near(max(t - r, 0.)):
            # d + r on the threshold in one replicate, in all of them
            rows.append(np.r_[d, rng.uniform(0, 20, n - 1)])
            rows.append(np.full(n, d))
        for z in _near(max(t - nr, 0.)):
            # z = the first replicate alone: z + n r on the threshold
            rows.append(np.r_[z, np.zeros(n - 1)])
            rows.append(np.r_[np.zeros(n - 1), z])
    rows += list(rng.uniform(0, 12, (300, n)))
    rows += list(rng.uniform(0, 200, (300, n)))
    rows += list(np.floor(rng.uniform(0, 12, (100, n))))
    ps = np.ascontiguousarray(np.array(rows, dtype=np.float64))
    assert np.all(ps >= 0)
    return ps


def _terms(ps, delta, mode):
    lib = _lib()
    out = np.empty(len(ps))
    rc = lib.h3dt_nll_terms(ctypes.c_int64(len(ps)), ps.shape[1],
                            ps.ctypes.data_as(D), ctypes.c_double(delta),
                            mode, out.ctypes.data_as(D))
    assert rc == 0
    return out


@pytest.mark.parametrize('n', (2, 4))
@pytest.mark.parametrize('mode,r', [(3, 5.0), (3, 5.92), (3, 9.99),
                                    (4, 2.5), (4, 3.28), (4, 4.99)])
def test_form_equals_general(mode, r, n):
    delta = _delta_for(r)
    ra = 1. / delta - 1
    assert ra >= r and (ra >= 5. if mode == 3 else n * ra >= 5.)
    ps = _pseudo(ra, n)
    got, want = _terms(ps, delta, mode), _terms(ps, delta, 0)
    arg = ps + ra
    print('mode', mode, 'r', ra, 'n', n, 'pixels', len(ps),
          'd + r in [%.17g, %.17g]' % (arg.min(), arg.max()),
          'on 5:', int((arg == 5.).sum()), 'on 10:', int((arg == 10.).sum()),
          'differing', int((got.view(np.int64) != want.view(np.int64)).sum()))
    assert np.all(np.isfinite(want))
    np.testing.assert_array_equal(got.view(np.int64), want.view(np.int64))


def _brent(design, ranges):
    return _run(design, LENGTHS, H3D_BRENT=0, H3D_BRENT_LDS_KB=16,
                H3D_NLL_RANGES=ranges)


def _gang(design, ranges):
    return _run(design, LENGTHS, H3D_BRENT=2, H3D_NLL_RANGES=ranges)


@pytest.mark.parametrize('design', DESIGNS, ids=lambda d: '%d+%d' % d)
def test_brent_ranges_equal_general(design):
    on, off = _brent(design, 1), _brent(design, 0)
    print(design, 'evals', on[3].sum(), 'iters', on[2].sum())
    _same(on, off)
    assert np.all(on[3] > 0)


@pytest.mark.parametrize('design', DESIGNS, ids=lambda d: '%d+%d' % d)
def test_gang_ranges_equal_general(design):
    on, off = _gang(design, 1), _gang(design, 0)
    print(design, 'evals', on[3].sum(), 'iters', on[2].sum())
    _same(on, off)
    assert np.all(on[3] > 0)
