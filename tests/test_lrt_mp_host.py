"""lrt_pixel (csrc/h3d_model.h) against the exact LRT fixture
tests/golden/unit_lrt_mp.npz, through the two builds behind the h3dt_* test
ABI (test_special_host.py's ``lib``: g++ on the CPU, hipcc for gfx950 in the
self-test kernel on the GPU), with the bounds of lrt_mp_cases.py -- the same
ones test_gpu_lrt_edges.py holds the production kernels to."""
import ctypes

import numpy as np
import pytest

import lrt_mp_cases as cases
from test_special_host import I, _p, lib  # noqa: F401  (lib: the fixture)


def host_lrt(lib, d, refit):  # noqa: F811
    raw32 = np.ascontiguousarray(d.raw, dtype=np.int32)
    n = d.n
    p, llr, m0 = np.empty(n), np.empty(n), np.empty(n)
    m1 = np.empty((n, d.C))
    st = lib.h3dt_lrt(ctypes.c_int64(n), d.R, d.C, _p(raw32, I), _p(d.f),
                      _p(d.disp_wide), _p(d.cond, I), int(refit), _p(p),
                      _p(llr), _p(m0), _p(m1))
    assert st == 0
    return p, llr, m0, m1


@pytest.mark.parametrize('R,C', cases.DESIGNS)
@pytest.mark.parametrize('refit', [True, False])
def test_lrt_pixel_vs_mp(lib, R, C, refit):  # noqa: F811
    d = cases.design(R, C)
    cases.check(d, host_lrt(lib, d, refit), refit, 'lrt_pixel')


def test_fixture_is_complete():
    """Every cell has its 32 pixels, at most 2 % of any cell were redrawn
    (no finite root of a score), the raw counts fit int32, no condition is
    empty of counts, and the underflow edge is present."""
    under = 0
    for R, C in cases.DESIGNS:
        d = cases.design(R, C)
        assert d.n == len(cases.FAMILIES) * cases.NPIX
        assert d.raw.shape == (d.n, R) and d.disp.shape == (d.n, C)
        assert np.all(d.redraws <= 0.02 * cases.NPIX)
        assert d.raw.min() >= 0 and d.raw.max() < 2 ** 31
        sizes = np.bincount(d.cond, minlength=C)
        assert sizes.min() >= 1 and (C == R or len(set(sizes)) > 1)
        for c in range(C):
            assert np.all(d.raw[:, d.cond == c].sum(axis=1) > 0)
        under += int((d.ref[True]['lnp'] < cases.LN_MIN_SUBNORMAL).sum())
    assert under > 0


def test_fixture_subsample_recomputed():
    """60 pixels of the fixture recomputed with mpmath (where installed):
    the file is what its generator writes."""
    pytest.importorskip('mpmath')
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                        'make_golden_lrt_mp.py')
    spec = importlib.util.spec_from_file_location('make_golden_lrt_mp', path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    rng = np.random.default_rng(4)
    for j in range(60):
        R, C = cases.DESIGNS[j % len(cases.DESIGNS)]
        d = cases.design(R, C)
        i = int(rng.integers(0, d.n))
        r = gen.lrt_exact(d.raw[i], d.f[i], d.disp[i], d.cond, C)
        for refit, tag in ((True, ''), (False, '_nr')):
            ref = d.ref[refit]
            assert r['mu0' + tag] == ref['mu0'][i]
            np.testing.assert_array_equal(r['mu1' + tag], ref['mu1'][i])
            assert r['llr' + tag] == ref['llr'][i]
            assert r['p' + tag] == ref['p'][i]
            assert r['p_lo' + tag] == ref['p_lo'][i]
            assert r['p_hi' + tag] == ref['p_hi'][i]
            assert np.float32(r['lnp' + tag]) == np.float32(ref['lnp'][i])
            assert np.float32(r['S' + tag]) == np.float32(ref['S'][i])
