"""log_fast's table bucket from the mantissa's bits (csrc/h3d_special.h,
log_fast_index) against the FP64 expression it replaced (log_fast_index_fp),
through the two builds of the test ABI (host: libh3d_hosttest.so; gfx950:
libh3d_selftest.so, marked gpu).

The bucket is an integer, so the comparison is exact everywhere: bit index ==
FP index, device == host, and log_fast returns the same 64 bits with either
index. Inputs: every half-step boundary m = 1/2 + (2j + 1)/2048 (where the
rounding of 1024 (m - 1/2) flips) with its two neighbours, every power of two
of the double range (subnormals included), DBL_MIN / DBL_MAX and the
subnormals next to them, and 10^5 seeded random doubles."""
import ctypes

import numpy as np
import pytest

from unit_abi import load_gfx950, load_host

D = ctypes.POINTER(ctypes.c_double)
I = ctypes.POINTER(ctypes.c_int32)

_cache = {}


def _inputs():
    if 'x' in _cache:
        return _cache['x']
    j = np.arange(512, dtype=np.float64)
    edge = 0.5 + (2 * j + 1) / 2048.  # exact: 11 fraction bits
    parts = [edge, np.nextafter(edge, 0.), np.nextafter(edge, 1.)]
    # the same boundaries at other exponents (frexp strips them)
    parts += [edge * 2. ** 40, np.nextafter(edge, 0.) * 2. ** -900]
    parts.append(2. ** np.arange(-1074, 1024, dtype=np.float64))
    tiny, huge = np.finfo(np.float64).tiny, np.finfo(np.float64).max
    parts.append(np.array([
        tiny, np.nextafter(tiny, 0.), np.nextafter(tiny, 1.),
        huge, np.nextafter(huge, 0.),
        5e-324, 1e-323, np.nextafter(tiny, 0.) / 2, 1.0,
        np.nextafter(1.0, 0.), np.nextafter(1.0, 2.), np.nextafter(0.5, 0.)]))
    rng = np.random.RandomState(20261)
    # random bit patterns of positive finite doubles: every exponent, every
    # fraction equally likely
    bits = rng.randint(0, 2 ** 52, size=100000, dtype=np.int64) | (
        rng.randint(0, 2047, size=100000, dtype=np.int64) << 52)
    rnd = bits.view(np.float64)
    rnd = rnd[rnd > 0]
    parts.append(rnd)
    # and random mantissas near 1 and over the NLL's argument range
    parts.append(rng.uniform(0.5, 1., 20000))
    parts.append(10. ** rng.uniform(-3, 5, 20000))
    x = np.ascontiguousarray(np.concatenate(parts))
    assert np.all(x > 0) and np.all(np.isfinite(x))
    _cache['x'] = x
    return x


def _index(lib, x):
    bits = np.full(x.size, -7, dtype=np.int32)
    fp = np.full(x.size, -9, dtype=np.int32)
    lib.h3dt_log_index(ctypes.c_int64(x.size), x.ctypes.data_as(D),
                       bits.ctypes.data_as(I), fp.ctypes.data_as(I))
    return bits, fp


def _unary(lib, name, x):
    out = np.empty_like(x)
    getattr(lib, 'h3dt_' + name)(ctypes.c_int64(x.size), x.ctypes.data_as(D),
                                 out.ctypes.data_as(D))
    return out


def _host():
    if 'host' not in _cache:
        _cache['host'] = load_host()
    return _cache['host']


def _device():
    if 'dev' not in _cache:
        _cache['dev'] = load_gfx950()
    return _cache['dev']


def _expected_index(x):
    """round-half-up of 1024 (m - 1/2) in exact integer arithmetic"""
    m, _ = np.frexp(x)
    frac = m.view(np.int64) & ((1 << 52) - 1)  # m = (1 + frac 2^-52) / 2
    return ((frac + (1 << 42)) >> 43).astype(np.int32)  # 512 frac 2^-52 + 1/2


def _check(lib):
    x = _inputs()
    bits, fp = _index(lib, x)
    print('inputs', x.size, 'buckets hit', np.unique(bits).size,
          'range', bits.min(), bits.max())
    np.testing.assert_array_equal(bits, fp)
    np.testing.assert_array_equal(bits, _expected_index(x))
    assert bits.min() == 0 and bits.max() == 512
    assert np.unique(bits).size == 513
    a = _unary(lib, 'log_fast', x)
    b = _unary(lib, 'log_fast_fp_index', x)
    np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))
    return bits, a


def test_bit_index_equals_fp_index_host():
    _check(_host())


@pytest.mark.gpu
def test_bit_index_equals_fp_index_gfx950():
    bits, _ = _check(_device())
    host_bits, _ = _index(_host(), _inputs())
    np.testing.assert_array_equal(bits, host_bits)
