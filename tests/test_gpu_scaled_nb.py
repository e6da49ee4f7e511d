"""hic3defdr_amd.util.scaled_nb (kernels of csrc/h3d_nb.hip) on the GPU vs the
reference's own values: tests/golden/unit_nb.npz and the per-R fixture
tests/golden/unit_scaled_nb.npz (make_golden_scaled_nb.py: R in {1, 2, 3, 4,
5, 8, 9, 16, 17, 32}, 257 pixels each, 95-130 of which carry the mu_out
clamp from replicate 0 into the later replicates for every R >= 2).

Bars are those of tests/test_special_host.py for the same functions. The
fixture was first run through the host build of the same headers
(libh3d_hosttest.so, M = 32): worst fit_mu_hat distance 6.0e-13 relative
(bar 1e-9), worst equalize distance 8.8e-4 of its tolerance rtol 1e-9 + atol
1e-12, worst q2qnbinom distance 4.9e-4 of rtol 1e-10 + atol 1e-12 (its 161
infinite values equal) -- no stored mean is limited by the reference's
secant exit, so seed 21 stands.
"""
import ctypes

import numpy as np
import pytest
from scipy.special import gammaln

from conftest import golden, rel_err

pytestmark = pytest.mark.gpu

R_LIST = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)
NO_ROOT = 'bracketing interval not found within 100 doublings'


@pytest.fixture(scope='module')
def nb():
    from hic3defdr_amd.util import scaled_nb
    return scaled_nb


@pytest.fixture(scope='module')
def ctx():
    from hic3defdr_amd import _native
    return _native.context()


@pytest.fixture(scope='module')
def unit():
    return golden('unit_nb.npz')


@pytest.fixture(scope='module')
def fix():
    g = golden('unit_scaled_nb.npz')
    assert tuple(int(r) for r in g['R_list']) == R_LIST
    return {k: g[k] for k in g.files}


def inputs(fix, R):
    p = 'r%d_' % R
    return (fix[p + 'x'].astype(np.int64), fix[p + 'b'].astype(np.float64),
            fix[p + 'alpha'].astype(np.float64))


def test_fit_mu_hat_vs_unit_nb(nb, unit):
    x, b = unit['fmh_x'], unit['fmh_b']
    assert rel_err(nb.fit_mu_hat(x, b, unit['fmh_alpha']),
                   unit['fmh_mu']) < 1e-9
    assert rel_err(nb.fit_mu_hat(x, b, 0.05),
                   unit['fmh_mu_scalar_alpha']) < 1e-9


@pytest.mark.parametrize('R', R_LIST)
def test_fit_mu_hat_every_r_and_alpha_form(nb, fix, R):
    x, b, alpha = inputs(fix, R)
    forms = dict(full=alpha, scalar=0.05, row=alpha[0], col=alpha[:, :1])
    for name, a in forms.items():
        mu = nb.fit_mu_hat(x, b, a, verbose=False)
        assert mu.shape == (len(x),)
        err = rel_err(mu, fix['r%d_fmh_%s' % (R, name)])
        print('R=%d %s: rel_err %.2e' % (R, name, err))
        assert err < 1e-9, (R, name)


def test_fit_mu_hat_doctest_calls(nb):
    """The six calls of scaled_nb.py:97-137, to the printed digits."""
    x = np.array([[1, 2], [3, 4], [5, 6]])
    b = np.array([[0.9, 1.1], [0.8, 1.2], [0.7, 1.3]])
    alpha = np.array([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]])
    calls = [
        ((x, b, alpha), [1.47251127, 3.53879843, 5.86853465]),
        ((x, b, np.array([0.1, 0.2])), [1.47251127, 3.53749833, 5.85554075]),
        ((x, b, np.array([0.1, 0.2, 0.3])[:, None]),
         [1.49544092, 3.51679438, 5.73129492]),
        ((np.array([1, 2]), np.array([0.9, 1.1]), np.array([0.1, 0.2])),
         [1.47251127]),
        ((np.array([1, 2]), np.array([0.9, 1.1]), 0.1), [1.49544092]),
        ((np.array([[2, 3, 4, 2], [6, 9, 3, 1]]),
          np.array([[0.45, 0.53, 0.088, 0.091], [0.70, 0.83, 0.14, 0.15]]),
          np.array([[0.0071, 0.0071, 0.0073, 0.0073],
                    [0.0070, 0.0070, 0.0072, 0.0072]])),
         [9.5900971, 10.45962955]),
    ]
    for args, want in calls:
        got = nb.fit_mu_hat(*args)
        assert got.shape == (len(want),)
        np.testing.assert_allclose(got, want, rtol=1e-8)


def test_equalize_vs_unit_nb(nb, unit):
    for s in range(int(unit['n_segs'])):
        out = nb.equalize(unit['seg%d_data' % s], unit['seg%d_f' % s], 0.02)
        np.testing.assert_allclose(out, unit['seg%d_equalize' % s],
                                   rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize('R', R_LIST)
def test_equalize_every_r_scalar_and_per_pixel_alpha(nb, fix, R):
    x, b, alpha = inputs(fix, R)
    np.testing.assert_allclose(nb.equalize(x, b, 0.02),
                               fix['r%d_eq_scalar' % R], rtol=1e-9,
                               atol=1e-12)
    np.testing.assert_allclose(nb.equalize(x, b, alpha[:, 0]),
                               fix['r%d_eq_px' % R], rtol=1e-9, atol=1e-12)


def test_q2qnbinom_vs_unit_nb(nb, unit):
    out = nb.q2qnbinom(unit['q2q_x'], unit['q2q_mu_in'].copy(),
                       unit['q2q_mu_out'].copy(), unit['q2q_alpha'])
    np.testing.assert_allclose(out, unit['q2q'], rtol=1e-10, atol=1e-12)


def test_q2qnbinom_mutates_its_means_like_the_reference(nb, fix):
    mu_in, mu_out = fix['q2q_mu_in'].copy(), fix['q2q_mu_out'].copy()
    out = nb.q2qnbinom(fix['q2q_x'], mu_in, mu_out, fix['q2q_alpha'])
    np.testing.assert_allclose(out, fix['q2q'], rtol=1e-10, atol=1e-12)
    np.testing.assert_array_equal(mu_in, fix['q2q_mu_in_after'])
    np.testing.assert_array_equal(mu_out, fix['q2q_mu_out_after'])
    assert np.any(mu_in != fix['q2q_mu_in'])
    # a scalar alpha and means that are no arrays: nothing to write back
    one = nb.q2qnbinom(3.0, 0.1, 2.0, 0.05)
    assert one == nb.q2qnbinom(np.array([3.0]), np.array([0.25]),
                               np.array([0.25]), 0.05)[0]


def test_logpmf_within_16_eps_of_the_term_sum(nb, fix, unit):
    """|logpmf - reference| <= 16 eps S per element, S = the sum of the
    absolute values of the seven terms of scaled_nb.py:32-33 (each at most
    ~2 ulp off from lgam / log; the value itself cancels, so a bar relative
    to it would be wrong). Measured on an MI355X: worst ratio 0.036 of
    the bar on the broadcast grid, 0.040 on unit_nb.npz's."""
    eps = np.finfo(float).eps
    for k, m, phi, ref in ((fix['lp_k'], fix['lp_m'], fix['lp_phi'],
                            fix['logpmf']),
                           (unit['lp_k'], unit['lp_m'], unit['lp_phi'],
                            unit['logpmf'])):
        got = nb.logpmf(k, m, phi)
        assert got.shape == ref.shape
        kk, mm, pp = np.broadcast_arrays(k.astype(float), m, phi)
        r = 1. / pp
        terms = [gammaln(r + kk), gammaln(kk + 1), gammaln(r), r * np.log(r),
                 r * np.log(r + mm), kk * np.log(mm), kk * np.log(r + mm)]
        S = sum(np.abs(t) for t in terms)
        ratio = np.abs(got - ref) / (16 * eps * S)
        print('logpmf: worst |delta| / (16 eps S) = %.3f' % ratio.max())
        assert np.all(ratio <= 1.0)


@pytest.mark.parametrize('R', (4, 9))
def test_launch_tails_give_the_same_bits(nb, fix, R):
    x, b, alpha = inputs(fix, R)
    mu = nb.fit_mu_hat(x, b, alpha)
    eq = nb.equalize(x, b, 0.02)
    for n in (1, 63, 64, 65, 257):
        np.testing.assert_array_equal(nb.fit_mu_hat(x[:n], b[:n], alpha[:n]),
                                      mu[:n])
        np.testing.assert_array_equal(nb.equalize(x[:n], b[:n], 0.02), eq[:n])
    assert nb.fit_mu_hat(x[:0], b[:0], alpha[:0]).shape == (0,)
    assert nb.equalize(x[:0], b[:0], 0.02).shape == (0, R)


@pytest.fixture(scope='module')
def selftest():
    from unit_abi import load_gfx950
    return load_gfx950()


@pytest.mark.parametrize('R', R_LIST)
def test_production_kernels_vs_selftest_m32(ctx, selftest, fix, R):
    """k_nb_fit_mu<M> / k_nb_equalize<M> at the dispatched M against the
    self-test library's M = 32 kernels over the same device functions."""
    D = ctypes.POINTER(ctypes.c_double)
    I = ctypes.POINTER(ctypes.c_int32)
    x, b, alpha = inputs(fix, R)
    n = len(x)
    x32 = np.ascontiguousarray(x, dtype=np.int32)
    b = np.ascontiguousarray(b)
    alpha = np.ascontiguousarray(alpha)
    mu, fl = ctx.nb_fit_mu(x, b, alpha)
    ref = np.empty(n)
    assert selftest.h3dt_fit_mu(ctypes.c_int64(n), R, x32.ctypes.data_as(I),
                                b.ctypes.data_as(D), alpha.ctypes.data_as(D),
                                ref.ctypes.data_as(D)) == 0
    assert fl == 0
    e_mu = rel_err(mu, ref)
    eq, _, fl = ctx.nb_equalize(x, b, 0.02)
    ref_eq = np.empty((n, R))
    assert selftest.h3dt_equalize(ctypes.c_int64(n), R, x32.ctypes.data_as(I),
                                  b.ctypes.data_as(D), ctypes.c_double(0.02),
                                  ref_eq.ctypes.data_as(D)) == 0
    assert fl == 0
    e_eq = rel_err(eq, ref_eq)
    print('R=%d: fit_mu bit-equal %s (%.1e), equalize bit-equal %s (%.1e)' % (
        R, np.array_equal(mu, ref), e_mu, np.array_equal(eq, ref_eq), e_eq))
    assert e_mu < 1e-14
    assert e_eq < 1e-14


def test_qcml_loop_from_equalize_reaches_the_reference(nb, unit):
    """dispersion.py:33-43 written out with the new equalize and the
    existing cml: start at 0.01, iterate while |delta| >= 1e-4."""
    from hic3defdr_amd.util import dispersion
    for s in range(int(unit['n_segs'])):
        data, f = unit['seg%d_data' % s], unit['seg%d_f' % s]
        disp, delta, it = 0.01, np.inf, 0
        while delta >= 1e-4:
            new = dispersion.cml(nb.equalize(data, f, disp))
            delta, disp, it = abs(disp - new), new, it + 1
            assert it < 50
        assert rel_err(disp, unit['seg%d_qcml' % s]) < 1e-6, s


def test_all_zero_row_raises_the_reference_error(nb, fix):
    x, b, alpha = inputs(fix, 4)
    x = x.copy()
    x[100] = 0
    with pytest.raises(ValueError, match=NO_ROOT):
        nb.fit_mu_hat(x, b, alpha)
    with pytest.raises(ValueError, match=NO_ROOT):
        nb.equalize(x, b, 0.02)
    with pytest.raises(ValueError, match=NO_ROOT):
        nb.fit_mu_hat(np.array([0, 0]), np.array([0.9, 1.1]), 0.1)


def test_equalize_dev_on_torch_tensors_equals_host_call(ctx, fix):
    import torch
    dev = torch.device('cuda', 0)
    for R in (3, 4, 16):
        x, b, alpha = inputs(fix, R)
        n = len(x)
        want, want_mu, _ = ctx.nb_equalize(x, b, 0.02, want_mu=True)
        want_px, _, _ = ctx.nb_equalize(x, b, alpha[:, 0])
        tx = torch.from_numpy(x.astype(np.int32)).to(dev)
        tb = torch.from_numpy(b).to(dev)
        ta = torch.from_numpy(np.ascontiguousarray(alpha[:, 0])).to(dev)
        out = torch.full((n, R), -1., dtype=torch.float64, device=dev)
        mu = torch.full((n,), -1., dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)   # (the ctx has its own stream)
        assert ctx.nb_equalize_dev(tx.data_ptr(), tb.data_ptr(), 0.02, n, R,
                                   out.data_ptr(),
                                   d_mu_hat=mu.data_ptr()) == 0
        np.testing.assert_array_equal(out.cpu().numpy(), want)
        np.testing.assert_array_equal(mu.cpu().numpy(), want_mu)
        assert ctx.nb_equalize_dev(tx.data_ptr(), tb.data_ptr(), 0.0, n, R,
                                   out.data_ptr(),
                                   d_alpha_px=ta.data_ptr()) == 0
        np.testing.assert_array_equal(out.cpu().numpy(), want_px)
        mu2 = torch.full((n,), -1., dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        a02 = torch.full((1,), 0.02, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        assert ctx.nb_fit_mu_dev(tx.data_ptr(), tb.data_ptr(), a02.data_ptr(),
                                 (0, 0), n, R, mu2.data_ptr()) == 0
        np.testing.assert_array_equal(mu2.cpu().numpy(),
                                      ctx.nb_fit_mu(x, b, 0.02)[0])
        assert rel_err(mu2.cpu().numpy(), want_mu) < 1e-14
