"""The unit-test ABI h3dt_* itself (csrc/h3d_unit_abi.h): that its two builds
export what tests/unit_abi.py lists, and that the gfx950 build's runner
(for_each / k_each in csrc/h3d_selftest.hip) visits every index once, ORs the
flags and honours the argument checks exactly as the host's serial loop does.
The numerics behind the entries are the other modules' business; here only
integer-exact entries are used, so the two builds must agree bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest

from hic3defdr_amd import build as h3dbuild
from unit_abi import GFX950_ONLY, HOST_ONLY, SHARED, load_gfx950, load_host

M = 32                # h3d::kMaxReps
H3D_FLAG_BADIN = 16
GRID_MAX, BLOCK = 4096, 256
VP = ctypes.c_void_p


def _p(a):
    return a.ctypes.data_as(VP)


# ---- the exported names (no device) ---------------------------------------

def test_exported_names():
    host = ctypes.CDLL(h3dbuild.build_hosttest())
    # a hipcc-built shared object loads through ctypes without a device
    dev = ctypes.CDLL(h3dbuild.build_selftest())
    assert not set(SHARED) & set(HOST_ONLY) and not set(SHARED) & set(GFX950_ONLY)
    for name in SHARED:
        assert hasattr(host, name) and hasattr(dev, name), name
    for name in HOST_ONLY:
        assert hasattr(host, name) and not hasattr(dev, name), name
    for name in GFX950_ONLY:
        assert hasattr(dev, name) and not hasattr(host, name), name


def test_lists_match_the_sources():
    found = set()
    for src in ('h3d_unit_abi.h', 'h3d_hosttest.cpp', 'h3d_selftest.hip'):
        with open(os.path.join(h3dbuild.CSRC, src)) as fh:
            text = fh.read()
        found |= {m[:-1] for m in re.findall(r'h3dt_[a-z0-9_]+\(', text)}
        # the one-line entries: H3DT_UNARY(name, fn) defines h3dt_<name>
        found |= {'h3dt_' + m for m in
                  re.findall(r'^H3DT_(?:UNARY|BINARY)\(([a-z0-9_]+),', text, re.M)}
    assert found == set(SHARED) | set(HOST_ONLY) | set(GFX950_ONLY)
    assert len(set(SHARED)) == len(SHARED)


# ---- the runner (gfx950 against the host) ---------------------------------

@pytest.fixture(scope='module')
def libs():
    return load_host(), load_gfx950()


def philox(lib, ctr, key):
    n = len(ctr)
    # preset: an element the runner skipped would keep the 0x5A pattern
    out = np.full((n, 4), 0x5A5A5A5A, dtype=np.uint32)
    u = np.full((n, 2), -7.0)
    lib.h3dt_philox(ctypes.c_int64(n), _p(ctr), _p(key), _p(out), _p(u))
    return out, u


@pytest.mark.gpu
def test_runner_visits_every_index_once(libs):
    """n = 0, one element, either side of one block, and the smallest n at
    which a thread takes a second grid-stride trip"""
    host, dev = libs
    rng = np.random.default_rng(7)
    n_max = GRID_MAX * BLOCK + 3
    ctr = rng.integers(0, 2 ** 32, (n_max, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 2 ** 32, (n_max, 2), dtype=np.uint64).astype(np.uint32)
    want, want_u = philox(host, ctr, key)
    for n in (0, 1, 255, 257, n_max):
        got, got_u = philox(dev, ctr[:n], key[:n])
        np.testing.assert_array_equal(got, want[:n])
        assert got_u.tobytes() == want_u[:n].tobytes()


def nb_draw(lib, bm, disp, u1, u2, with_path):
    n = bm.size
    lam = np.empty(n)
    k = np.full(n, -9, dtype=np.int32)
    path = np.full(n, -9, dtype=np.int32)
    lib.h3dt_nb_draw.restype = ctypes.c_int
    fl = lib.h3dt_nb_draw(ctypes.c_int64(n), _p(bm), _p(disp), _p(u1), _p(u2),
                          _p(lam), _p(k), _p(path) if with_path else None)
    return fl, k, path


@pytest.mark.gpu
def test_runner_ors_the_flags_and_skips_null_outputs(libs):
    """1,000 valid draws and one bad element (disp = NaN) in the last
    position alone; lambda is not compared (the two libms differ)"""
    host, dev = libs
    rng = np.random.default_rng(8)
    n = 1001
    bm = 10. ** rng.uniform(-1, 3, n)
    disp = 10. ** rng.uniform(-3, 0, n)
    u1, u2 = ((rng.integers(0, 2 ** 52, n).astype(np.float64) + 0.5) * 2. ** -52
              for _ in range(2))
    disp[-1] = np.nan
    res = {}
    for name, lib in (('host', host), ('gfx950', dev)):
        fl, k, path = nb_draw(lib, bm, disp, u1, u2, True)
        assert fl == H3D_FLAG_BADIN and k[-1] == -1, name
        assert np.all(k[:-1] >= 0), name
        fl0, k0, path0 = nb_draw(lib, bm[:-1], disp[:-1], u1[:-1], u2[:-1], True)
        assert fl0 == 0, name
        np.testing.assert_array_equal(k0, k[:-1])
        np.testing.assert_array_equal(path0, path[:-1])
        fl_n, k_n, path_n = nb_draw(lib, bm, disp, u1, u2, False)
        assert fl_n == fl and np.all(path_n == -9), name
        np.testing.assert_array_equal(k_n, k)
        res[name] = path
    np.testing.assert_array_equal(res['gfx950'], res['host'])


@pytest.mark.gpu
@pytest.mark.parametrize('r', (0, M + 1))
def test_bad_replicate_count_is_refused_before_any_staging(libs, r):
    n = 5
    x = np.ones((n, M + 1), dtype=np.int32)
    f = np.ones((n, M + 1))
    for lib in libs:
        for entry, extra in ((lib.h3dt_equalize, (ctypes.c_double(0.05),)),
                             (lib.h3dt_fit_mu, (_p(f),))):
            entry.restype = ctypes.c_int
            out = np.full((n, M + 1), -7.0)
            assert entry(ctypes.c_int64(n), r, _p(x), _p(f), *extra, _p(out)) == -1
            assert np.all(out == -7.0)
