"""The random stream of simulate(gpu=True) (csrc/h3d_philox.h): Philox4x32-10
against the published Random123 known answers and a pure-Python restatement,
and the map from two words to a uniform, through the host build and the
gfx950 build of the same source (h3dt_philox).

The uniform is ((hi << 32 | lo) >> 12) + 1/2, scaled by 2^-52: 52 bits and
the half fill a double's 53 significant bits exactly, so the smallest and
largest values are 2^-53 and 1 - 2^-53 and 1 - u is exact. (With 53 bits the
half would be a 54th: the largest value, 1 - 2^-54, is not a double and
rounds to 1, outside the open interval the sampler needs.)"""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

from unit_abi import load_gfx950, load_host

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

KNOWN = [
    ((0, 0, 0, 0), (0, 0),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2,
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
     (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.fixture(scope='module',
                params=['host', pytest.param('gfx950', marks=pytest.mark.gpu)])
def lib(request):
    return load_host() if request.param == 'host' else load_gfx950()


def philox_py(ctr, key):
    """Philox4x32-10 in Python integers."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0, p1 & MASK,
                          (p0 >> 32) ^ c3 ^ k1, p0 & MASK)
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox(lib, ctr, key):
    ctr = np.ascontiguousarray(ctr, dtype=np.uint32).reshape(-1, 4)
    key = np.ascontiguousarray(key, dtype=np.uint32).reshape(-1, 2)
    out = np.empty_like(ctr)
    u = np.empty((len(ctr), 2))
    vp = ctypes.c_void_p
    lib.h3dt_philox(ctypes.c_int64(len(ctr)), ctr.ctypes.data_as(vp),
                    key.ctypes.data_as(vp), out.ctypes.data_as(vp),
                    u.ctypes.data_as(vp))
    return out, u


def test_restatement_meets_the_known_answers():
    for ctr, key, want in KNOWN:
        assert philox_py(ctr, key) == want


def test_known_answers(lib):
    out, _ = philox(lib, [k[0] for k in KNOWN], [k[1] for k in KNOWN])
    for got, (_, _, want) in zip(out, KNOWN):
        assert tuple(int(w) for w in got) == want


def test_random_counters_and_keys(lib):
    rng = np.random.default_rng(2021)
    ctr = rng.integers(0, 2 ** 32, (10000, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, (10000, 2), dtype=np.uint64)
    # the stream's own counters too: small pixel indices, replicates, streams
    ctr[:2000, 1] = 0
    ctr[:2000, 2] = rng.integers(0, 32, 2000)
    ctr[:2000, 3] = rng.integers(0, 24, 2000)
    out, u = philox(lib, ctr, key)
    want = np.array([philox_py([int(v) for v in c], [int(v) for v in k])
                     for c, k in zip(ctr, key)], dtype=np.uint32)
    np.testing.assert_array_equal(out, want)
    # the uniforms of the same outputs, exactly
    w = want.astype(np.uint64)
    for col, (lo, hi) in enumerate(((0, 1), (2, 3))):
        m = ((w[:, hi] << np.uint64(32)) | w[:, lo]) >> np.uint64(12)
        for i in range(0, len(m), 97):
            assert Fraction(float(u[i, col])) == \
                (Fraction(int(m[i])) + Fraction(1, 2)) / 2 ** 52
        np.testing.assert_array_equal(
            u[:, col], (m.astype(np.float64) + 0.5) * 2.0 ** -52)


def test_uniform_map_extremes():
    """The smallest and largest uniforms, 2^-53 and 1 - 2^-53, lie strictly
    inside (0, 1), and 1 - u is exact for every u of the stream's form
    (checked in rationals at both ends and at random words)."""
    rng = np.random.default_rng(3)
    ms = [0, 1, 2 ** 52 - 2, 2 ** 52 - 1] + \
        [int(v) for v in rng.integers(0, 2 ** 52, 2000)]
    for m in ms:
        exact = (Fraction(m) + Fraction(1, 2)) / 2 ** 52
        u = (float(m) + 0.5) * 2.0 ** -52
        assert Fraction(u) == exact and 0 < u < 1
        assert Fraction(1.0 - u) == 1 - exact
    assert (0.0 + 0.5) * 2.0 ** -52 == 2.0 ** -53
    assert (float(2 ** 52 - 1) + 0.5) * 2.0 ** -52 == 1 - 2.0 ** -53


def test_uniform_map_extremes_in_the_library(lib):
    """h3dt_philox_uniform on the extreme words and around the 12 dropped
    bits; then 10,000 draws inside the closed range of the map."""
    lo = np.array([0, 0xFFF, 0x1000, MASK, MASK - 0xFFF, 0, MASK],
                  dtype=np.uint32)
    hi = np.array([0, 0, 0, MASK, MASK, 0x80000000, 0x7FFFFFFF],
                  dtype=np.uint32)
    u = np.empty(len(lo))
    vp = ctypes.c_void_p
    lib.h3dt_philox_uniform(ctypes.c_int64(len(lo)), lo.ctypes.data_as(vp),
                            hi.ctypes.data_as(vp), u.ctypes.data_as(vp))
    np.testing.assert_array_equal(
        u, [2.0 ** -53, 2.0 ** -53, 3 * 2.0 ** -53, 1 - 2.0 ** -53,
            1 - 2.0 ** -53, 0.5 + 2.0 ** -53, 0.5 - 2.0 ** -53])
    np.testing.assert_array_equal(1 - u[[3, 5, 6]],
                                  [2.0 ** -53, 0.5 - 2.0 ** -53,
                                   0.5 + 2.0 ** -53])
    rng = np.random.default_rng(4)
    ctr = rng.integers(0, 2 ** 32, (10000, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, (10000, 2), dtype=np.uint64)
    _, u = philox(lib, ctr, key)
    assert u.min() >= 2.0 ** -53 and u.max() <= 1 - 2.0 ** -53
    # roughly uniform: the mean of 20,000 uniforms within 5 standard errors
    assert abs(u.mean() - 0.5) < 5 * np.sqrt(1 / 12 / u.size)
