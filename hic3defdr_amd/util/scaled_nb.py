"""Operator-level drop-ins for the reference's scaled negative-binomial
numerics (hic3defdr/util/scaled_nb.py): same names and signatures; computed
on the GPU by the kernels of csrc/h3d_nb.hip, which call the device functions
the fused estimate_disp / lrt kernels are built from (h3d_model.h: fit_mu,
equalize_pixel, q2q, logpmf).

- ``fit_mu_hat(x, b, alpha)``: the MLE of the mean under fixed dispersion,
  every broadcast form of the reference's doctest;
- ``equalize(data, f, alpha)``: common-scale pseudodata, alpha a scalar or
  one value per pixel;
- ``q2qnbinom(x, mu_in, mu_out, alpha)``: the quantile map, clamping
  ``mu_in`` / ``mu_out`` in place as the reference does;
- ``logpmf(k, m, phi)``: the NB log-likelihood;
- ``mvr`` / ``inverse_mvr``: two flops each, plain numpy on the host.

Pixels keep the caller's order. There is no CPU fallback: without libh3d.so
or a gfx950 device the GPU functions raise ``H3DError``. Input that the
reference rejects is rejected before anything is uploaded.
"""
import numpy as np

from hic3defdr_amd import _native

_MAX_REPS = 32
_NO_ROOT = 'bracketing interval not found within 100 doublings'


def logpmf(k, m, phi):
    """scaled_nb.py:12-33. numpy broadcasting of ``k``, ``m``, ``phi``; the
    result has the broadcast shape."""
    k, m, phi = np.broadcast_arrays(np.asarray(k, dtype=np.float64),
                                    np.asarray(m, dtype=np.float64),
                                    np.asarray(phi, dtype=np.float64))
    if k.size == 0:
        return np.empty(k.shape)
    out = _native.context().nb_logpmf(k, m, phi)
    return out if out.ndim else out[()]


def mvr(mean, disp):
    """scaled_nb.py:36-50."""
    return mean + mean**2 * disp


def inverse_mvr(mean, var):
    """scaled_nb.py:53-68."""
    return (var-mean) / mean**2


def _check_model(x, b, alpha):
    """The reference's three input asserts (scaled_nb.py:139-141)."""
    if not np.all((alpha > 0) & np.isfinite(alpha)):
        raise AssertionError('alpha must be positive and finite')
    if not np.all((x >= 0) & np.isfinite(x)):
        raise AssertionError('x must be non-negative and finite')
    if not np.all((b > 0) & np.isfinite(b)):
        raise AssertionError('b must be positive and finite')


def _counts(x):
    """Counts as the kernels read them: integers in [0, 2^31) (float arrays
    holding integers are fine, as util/dispersion.qcml takes them)."""
    if x.dtype.kind not in 'iuf' and x.dtype.kind != 'b':
        raise ValueError('counts must be numbers')
    if x.size and not np.all(x == np.floor(x)):
        raise ValueError('counts must be integers')
    if x.size and x.max() >= 2 ** 31:
        raise ValueError('counts must be below 2^31')
    if x.shape[-1] > _MAX_REPS:
        raise ValueError('at most %d replicates per pixel' % _MAX_REPS)
    if x.shape[-1] < 1:
        raise ValueError('at least one replicate per pixel')
    return x.astype(np.int64)


def fit_mu_hat(x, b, alpha, verbose=True):
    """scaled_nb.py:71-183: ``x``, ``b`` (pixels, replicates) or one pixel's
    vectors (the result then has shape (1,)); ``alpha`` a scalar, (R,),
    (n, 1) or (n, R). A pixel without a root (an all-zero row) raises the
    reference's ValueError. ``verbose`` is accepted; nothing is printed."""
    x, b, alpha = np.asarray(x), np.asarray(b), np.asarray(alpha)
    _check_model(x, b, alpha)
    if x.ndim not in (1, 2):
        raise ValueError('x must be (pixels, replicates) or one pixel')
    if x.ndim == 1:
        if alpha.ndim > 1:
            raise ValueError('alpha of one pixel must be a scalar or (R,)')
        x = x[None, :]
    xi = _counts(x)
    n, R = xi.shape
    b = np.broadcast_to(b, (n, R))
    if n == 0:
        return np.empty(0)
    mu, fl = _native.context().nb_fit_mu(xi, b, alpha)
    if fl & 16:
        raise AssertionError('alpha and b must be positive and finite')
    if fl or not np.all(np.isfinite(mu)):
        raise ValueError(_NO_ROOT)
    return mu


def equalize(data, f, alpha):
    """scaled_nb.py:186-214. ``alpha``: a scalar, or one dispersion per
    pixel (n,)."""
    data, f, alpha = np.asarray(data), np.asarray(f), np.asarray(alpha)
    _check_model(data, f, alpha)
    if data.ndim != 2:
        raise ValueError('data must be (pixels, replicates)')
    xi = _counts(data)
    n, R = xi.shape
    f = np.broadcast_to(f, (n, R))
    if alpha.ndim and alpha.shape != (n,):
        raise ValueError('alpha must be a scalar or (n,)')
    if n == 0:
        return np.empty((0, R))
    out, _, fl = _native.context().nb_equalize(xi, f, alpha)
    if fl & 16:
        raise AssertionError('alpha and f must be positive and finite')
    if fl:
        raise ValueError(_NO_ROOT)
    return out


def q2qnbinom(x, mu_in, mu_out, alpha):
    """scaled_nb.py:217-275. ``x`` is any real array (the map is continuous
    in x); ``alpha`` a scalar or one per value. Where ``mu_in`` / ``mu_out``
    are writable float64 arrays of the result's shape, the clamp at 0.25 is
    written back into them, as the reference does (:240-242)."""
    bx, bi, bo = np.broadcast_arrays(np.asarray(x, dtype=np.float64),
                                     np.asarray(mu_in, dtype=np.float64),
                                     np.asarray(mu_out, dtype=np.float64))
    shape = bx.shape
    alpha = np.asarray(alpha, dtype=np.float64)
    if alpha.ndim:
        alpha = np.ascontiguousarray(np.broadcast_to(alpha, shape))
    if bx.size == 0:
        return np.empty(shape)
    mi = np.array(bi, dtype=np.float64, order='C')
    mo = np.array(bo, dtype=np.float64, order='C')
    out = _native.context().nb_quantile_map(
        np.ascontiguousarray(bx).reshape(-1), mi.reshape(-1), mo.reshape(-1),
        alpha.reshape(-1) if alpha.ndim else alpha).reshape(shape)
    for given, clamped in ((mu_in, mi), (mu_out, mo)):
        if isinstance(given, np.ndarray) and given.dtype == np.float64 and \
                given.flags.writeable and given.shape == shape:
            given[...] = clamped
    return out if out.ndim else out[()]
