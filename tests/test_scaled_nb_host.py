"""hic3defdr_amd.util.scaled_nb without a GPU: the reference's names and
signatures (hic3defdr/util/scaled_nb.py), the two host formulas, and every
rejection that has to happen before a device is touched."""
import inspect

import numpy as np
import pytest

from hic3defdr_amd.util import scaled_nb

X = np.array([[1, 2], [3, 4], [5, 6]])
B = np.array([[0.9, 1.1], [0.8, 1.2], [0.7, 1.3]])
A = np.array([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]])


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    """Any attempt to open a context fails the test: these inputs must be
    turned away by the Python layer."""
    def boom(*a, **k):
        raise RuntimeError('a device context was requested')
    monkeypatch.setattr(scaled_nb._native, 'context', boom)


def test_names_and_signatures():
    want = {
        'logpmf': ['k', 'm', 'phi'],
        'mvr': ['mean', 'disp'],
        'inverse_mvr': ['mean', 'var'],
        'fit_mu_hat': ['x', 'b', 'alpha', 'verbose'],
        'equalize': ['data', 'f', 'alpha'],
        'q2qnbinom': ['x', 'mu_in', 'mu_out', 'alpha'],
    }
    for name, params in want.items():
        fn = getattr(scaled_nb, name)
        assert list(inspect.signature(fn).parameters) == params, name
    assert inspect.signature(scaled_nb.fit_mu_hat).parameters[
        'verbose'].default is True


def test_mvr_round_trip_bit_exact():
    rng = np.random.default_rng(3)
    mean = 10 ** rng.uniform(-2, 4, 1000)
    disp = 10 ** rng.uniform(-4, 1, 1000)
    var = scaled_nb.mvr(mean, disp)
    np.testing.assert_array_equal(var, mean + mean**2 * disp)
    back = scaled_nb.inverse_mvr(mean, var)
    np.testing.assert_array_equal(back, (var - mean) / mean**2)
    np.testing.assert_allclose(back, disp, rtol=1e-6)
    assert scaled_nb.mvr(2.0, 0.5) == 4.0
    assert scaled_nb.inverse_mvr(2.0, 4.0) == 0.5


@pytest.mark.parametrize('x, b, a', [
    (np.array([[1, -2], [3, 4], [5, 6]]), B, A),
    (np.array([[1, np.inf], [3, 4], [5, 6]]), B, A),
    (np.array([[1, np.nan], [3, 4], [5, 6]]), B, A),
    (X, np.array([[0.9, 0.0], [0.8, 1.2], [0.7, 1.3]]), A),
    (X, -B, A),
    (X, np.array([[0.9, np.inf], [0.8, 1.2], [0.7, 1.3]]), A),
    (X, B, np.array([[0.0, 0.2], [0.3, 0.4], [0.5, 0.6]])),
    (X, B, -0.1),
    (X, B, np.array([0.1, np.nan])),
    (X, B, np.inf),
])
def test_reference_asserts(x, b, a):
    with pytest.raises(AssertionError):
        scaled_nb.fit_mu_hat(x, b, a)
    if np.ndim(a) != 1:     # (R,) is no equalize form
        with pytest.raises(AssertionError):
            scaled_nb.equalize(x, b, a[:, 0] if np.ndim(a) == 2 else a)


def test_counts_must_be_integers_below_2_31():
    for fn in (scaled_nb.fit_mu_hat, scaled_nb.equalize):
        with pytest.raises(ValueError):
            fn(np.array([[1.5, 2], [3, 4], [5, 6]]), B, 0.1)
        with pytest.raises(ValueError):
            fn(np.array([[2.0 ** 31, 2], [3, 4], [5, 6]]), B, 0.1)
    with pytest.raises(ValueError):
        scaled_nb.fit_mu_hat(np.array([1.5, 2]), np.array([0.9, 1.1]), 0.1)


def test_more_than_32_replicates():
    x = np.ones((5, 33), dtype=int)
    b = np.ones((5, 33))
    with pytest.raises(ValueError):
        scaled_nb.fit_mu_hat(x, b, 0.1)
    with pytest.raises(ValueError):
        scaled_nb.equalize(x, b, 0.1)


def test_shapes_that_do_not_broadcast():
    with pytest.raises(ValueError):
        scaled_nb.equalize(X, B, np.array([0.1, 0.2]))   # (R,), not (n,)
    with pytest.raises(ValueError):
        scaled_nb.equalize(X[0], B[0], 0.1)


def test_empty_inputs_launch_nothing():
    assert scaled_nb.fit_mu_hat(np.zeros((0, 4), int), np.ones((0, 4)),
                                0.1).shape == (0,)
    assert scaled_nb.equalize(np.zeros((0, 4), int), np.ones((0, 4)),
                              0.1).shape == (0, 4)
    e = np.empty(0)
    assert scaled_nb.q2qnbinom(e, e.copy(), e.copy(), 0.1).shape == (0,)
    assert scaled_nb.logpmf(np.zeros((0, 3)), 1.0, np.ones(3)).shape == (0, 3)
