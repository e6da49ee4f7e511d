"""The per-pixel NLL term (csrc/h3d_model.h nll_pixel*, csrc/h3d_special.h
lgam_nll*) against the exact terms of tests/golden/unit_cml_mp.npz, through
``h3dt_nll_terms`` of the two builds test_special_host.py loads: ``host``
(g++, runs on the CPU) and ``gfx950`` (the self-test library: the device code
in a kernel on the MI355X, marked gpu).

Every form on every term case inside its domain (cml_mp_cases.in_domain):
replicate counts 1 .. 32 -- the fold of the shift products after 8 factors,
np_sum's pairwise branch from 8 on, 1, 3, 5, 9 or 17 replicates in a wider
slot -- seven pseudodata families from all-zero to 1e7, at both ends of the
search interval, either side of the form switches at r = 5, 10, 20, and four
interior deltas. The bound is |got - want| <= 32 eps S (cml_mp_cases'
docstring); a test prints the worst error per family in units of it.

Worst ratio per (form, family) over every replicate count and delta, host
build / gfx950:

    form  zeros      tiny       sparse     frac       benign     large      mixed
    0     0.28/0.22  0.27/0.27  0.33/0.28  0.23/0.22  0.05/0.05  0.04/0.04  0.06/0.06
    1     0.02/0.02  0.04/0.03  0.03/0.03  0.03/0.03  0.04/0.05  0.04/0.04  0.04/0.03
    2     0.02/0.02  0.04/0.03  0.02/0.03  0.03/0.03  0.04/0.05  0.04/0.04  0.03/0.03
    3     0.02/0.02  0.05/0.03  0.04/0.03  0.04/0.04  0.05/0.05  0.04/0.04  0.04/0.03
    4     0.28/0.22  0.26/0.17  0.33/0.25  0.13/0.13  0.05/0.05  0.04/0.04  0.04/0.04

(Forms 0 and 4 come nearest at r < 5, where every argument is shifted twice;
the host's worst is 0.33 at n = 31, delta = 0.6.) What the bound resolves,
tried once on scratch copies of the host build: stirling_nll's 1/1260 made
1/1261 (6e-12 at y = 10) fails forms 0, 1, 3 and 4 at every n >= 2 (not form
2, which has its own series, nor n = 1, whose term cancels identically);
nll_pixel's fold without its ``prod = 1`` fails form 0 at all 13 replicate
counts and nothing else; 1/1188 made 1/1189 (7e-14 at y = 10) stays inside
the bound, which is 32 eps of |lgamma(10)| = 9e-14 per log-gamma there.
"""
import ctypes

import numpy as np
import pytest

import cml_mp_cases as cc

from unit_abi import load_gfx950, load_host

D = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope='module',
                params=['host', pytest.param('gfx950', marks=pytest.mark.gpu)])
def lib(request):
    return load_host() if request.param == 'host' else load_gfx950()


def terms(lib, ps, delta, mode):
    ps = np.ascontiguousarray(ps, dtype=np.float64)
    out = np.full(len(ps), np.nan)
    rc = lib.h3dt_nll_terms(ctypes.c_int64(len(ps)), ps.shape[1],
                            ps.ctypes.data_as(D), ctypes.c_double(delta),
                            mode, out.ctypes.data_as(D))
    assert rc == 0
    return out


def worst_units(lib, mode, n):
    """{family: (worst error in units of the bound, its delta)} over the
    deltas inside the form's domain; None where there is none"""
    data, want, S = cc.term_cases(n)
    deltas = cc.term_deltas()
    out = {}
    for fi, fam in enumerate(cc.TERM_FAMILIES):
        worst = None
        for di, delta in enumerate(deltas):
            if not cc.in_domain(mode, delta, n):
                continue
            got = terms(lib, data[fi], delta, mode)
            with np.errstate(invalid='ignore'):
                u = cc.term_units(got, want[fi, di], S[fi, di])
            u = float(np.max(np.where(np.isfinite(got), u, np.inf)))
            if worst is None or u > worst[0]:
                worst = (u, float(delta))
        out[fam] = worst
    return out


@pytest.mark.parametrize('n', cc.TERM_N)
@pytest.mark.parametrize('mode', cc.MODES)
def test_term_vs_mp(lib, mode, n):
    if mode >= 3 and n < 2:
        # forms 3 and 4 are for conditions of two or more replicates: no case
        # of n = 1 lies in their domain
        assert not any(cc.in_domain(mode, d, n) for d in cc.term_deltas())
        return
    figs = worst_units(lib, mode, n)
    for fam, w in figs.items():
        assert w is not None, (mode, n, fam)
        print('term form=%d n=%-2d %-7s worst=%.4f of the bound (delta=%.17g)'
              % (mode, n, fam, w[0], w[1]))
    bad = {fam: w for fam, w in figs.items() if not w[0] <= 1}
    assert not bad, (mode, n, bad)


@pytest.mark.parametrize('n', cc.SEG_N)
def test_qcml_f1_state_machine(lib, n):
    """``h3dt_qcml`` -- equalize_pixel, nll_pixel (general form) and seg_step,
    the state machine the kernels run -- with f = 1 on the integer families:
    the equalize pass returns the counts, so the dispersion the loop ends on
    is held to the segment bound of the exact minimiser (cml_mp_cases). Worst
    fraction of the bound, host and gfx950 alike: 0.88 (``under``, on the
    lower bound, where the search's last point is 5.9e-6 inside the interval
    by construction), 0.26 elsewhere."""
    lib.h3dt_qcml.restype = ctypes.c_double
    I = ctypes.POINTER(ctypes.c_int32)
    bad = []
    for fam in cc.QCML_FAMILIES:
        seg = cc.segment(fam, n)
        x = np.ascontiguousarray(seg.data, dtype=np.int32)
        f = np.ones(x.shape)
        st = ctypes.c_int(0)
        disp = lib.h3dt_qcml(ctypes.c_int64(len(x)), n, x.ctypes.data_as(I),
                             f.ctypes.data_as(D), ctypes.byref(st))
        try:
            cc.check_segment(seg, disp, st.value, 'h3dt_qcml')
        except AssertionError as e:
            bad.append(e.args[0])
    assert not bad, bad


def test_fixture_covers_the_issue():
    """the deltas reach both ends of the interval and both sides of every
    form switch; the zero terms are stored as exact zeros"""
    deltas = cc.term_deltas()
    g = cc.fixture()
    np.testing.assert_array_equal(g['term_deltas'], deltas)
    r = cc.r_of(deltas)
    assert r[0] == 9999.0 and deltas[1] == cc.BRENT_B
    for k, r0 in ((2, 5.), (5, 10.), (8, 20.)):
        assert r[k] < r0 <= r[k + 1] < r[k + 2]
    for n in cc.TERM_N:
        data, want, S = cc.term_cases(n)
        assert data.shape == (len(cc.TERM_FAMILIES), cc.NPIX, n)
        assert np.all(want[0] == 0) and np.all(S >= 2 * n + 2)
        if n == 1:
            assert np.all(want == 0)


def test_fixture_segments_recomputed():
    """five segment cases' stored minimisers hold up in plain float64
    (scipy's gammaln): the objective at delta_star is below its value 1e-4
    to either side (a side outside the interval is skipped: ``under`` and
    ``ceiling`` sit on the bounds), and the flat region fits tol2."""
    from scipy.special import gammaln

    def f(data, delta):
        n = data.shape[1]
        r = 1. / delta - 1
        z = data.sum(1)
        return -np.sum(gammaln(data + r).sum(1) + gammaln(n * r)
                       - gammaln(z + n * r) - n * gammaln(r))
    for fam, n in (('benign', 2), ('over', 9), ('under', 4), ('ceiling', 5),
                   ('frac', 3)):
        s = cc.segment(fam, n)
        assert cc.BRENT_A <= s.lo <= s.delta_star <= s.hi <= cc.BRENT_B
        assert s.hi - s.lo <= cc.tol2(s.delta_star)
        f0 = f(s.data, s.delta_star)
        for x in (s.delta_star - 1e-4, s.delta_star + 1e-4):
            if cc.BRENT_A <= x <= cc.BRENT_B:
                assert f(s.data, x) > f0, (fam, n, x)
