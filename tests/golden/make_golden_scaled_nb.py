"""Generates tests/golden/unit_scaled_nb.npz by running the REFERENCE's
hic3defdr/util/scaled_nb.py (fit_mu_hat, equalize, q2qnbinom, logpmf).

Run where the reference is installed, with the interpreter and refshim that
make_golden.py documents:

    PYTHONPATH=tests/golden/refshim:<reference> PYTHONDONTWRITEBYTECODE=1 \
        MPLBACKEND=agg python3.9 tests/golden/make_golden_scaled_nb.py

The fixture holds inputs and recorded outputs only. For every replicate
count R in R_LIST (each M = 2 / 4 / 8 / 16 / 32 instantiation of the
k_nb_* kernels filled and partly filled), N = 257 pixels:

    mu = 10**U(-0.5, 2.5), b = exp(N(0, 0.5)) with b[:, 0] *= 0.02,
    alpha = 10**U(-3, 0) per entry, NB counts (a row that sums to 0 gets a 1
    in its last column)

b and alpha are rounded to float32 before anything is computed and stored as
float32 (exact, half the bytes). Stored per R (prefix ``r<R>_``):

    x, b, alpha
    fmh_full / fmh_scalar / fmh_row / fmh_col   fit_mu_hat with alpha (n, R),
                        0.05, alpha[0] (R,), alpha[:, :1] (n, 1)
    eq_scalar           equalize(x, b, 0.02)
    eq_px               equalize at the per-pixel alpha[:, 0]: the loop of
                        scaled_nb.py:207-213 over the reference's q2qnbinom,
                        with fit_mu_hat at alpha[:, :1]

The small first factor puts mu_hat * b[:, 0] below q2qnbinom's 0.25 floor
while mu_hat * gmean(b) is above it, so replicate 0 clamps the SHARED mu_out
and the clamp carries into the later replicates (scaled_nb.py:240-242 as
called from :213). The generator asserts that this happens in every set with
R >= 2 (with one replicate gmean(b) is b[:, 0], so it cannot), and that every
mean is finite.

Also: ``q2q_*`` one q2qnbinom call with a vector alpha including the
arguments as the reference left them (mu_in / mu_out mutated), and ``lp_*`` a
logpmf grid in the broadcast shapes (n, R) x (n, 1) x (R,).
"""
import os

import numpy as np

from hic3defdr.util import scaled_nb
from lib5c.util.mathematics import gmean

HERE = os.path.dirname(os.path.abspath(__file__))
R_LIST = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)
N = 257
SEED = 21


def draw(rng, R):
    mu = 10 ** rng.uniform(-0.5, 2.5, N)
    b = np.exp(rng.normal(0, 0.5, (N, R)))
    b[:, 0] *= 0.02
    alpha = 10 ** rng.uniform(-3, 0, (N, R))
    b = b.astype(np.float32).astype(np.float64)
    alpha = alpha.astype(np.float32).astype(np.float64)
    x = rng.negative_binomial(1 / alpha, 1 / (1 + alpha * mu[:, None] * b))
    x[x.sum(axis=1) == 0, -1] = 1
    return x, b, alpha


def equalize_px(x, b, alpha_px):
    """scaled_nb.py:207-213 with one dispersion per pixel."""
    f_mean = gmean(b, pseudocount=0, axis=1)
    mu_hat = scaled_nb.fit_mu_hat(x, b, alpha_px[:, None], verbose=False)
    mu_in = mu_hat[:, None] * b
    mu_out = mu_hat * f_mean
    out = np.zeros_like(x, dtype=float)
    for i in range(x.shape[1]):
        out[:, i] = scaled_nb.q2qnbinom(x[:, i], mu_in[:, i], mu_out, alpha_px)
    return out


def main():
    rng = np.random.default_rng(SEED)
    out = {'R_list': np.array(R_LIST), 'seed': np.array(SEED)}
    for R in R_LIST:
        x, b, alpha = draw(rng, R)
        p = 'r%d_' % R
        out[p + 'x'] = x.astype(np.int32)
        out[p + 'b'] = b.astype(np.float32)
        out[p + 'alpha'] = alpha.astype(np.float32)
        forms = dict(full=alpha, scalar=0.05, row=alpha[0], col=alpha[:, :1])
        for name, a in forms.items():
            mu = scaled_nb.fit_mu_hat(x, b, a, verbose=False)
            assert mu.shape == (N,) and np.all(np.isfinite(mu)), (R, name)
            out[p + 'fmh_' + name] = mu
        out[p + 'eq_scalar'] = scaled_nb.equalize(x, b, 0.02)
        out[p + 'eq_px'] = equalize_px(x, b, alpha[:, 0].copy())
        assert np.all(np.isfinite(out[p + 'eq_scalar']))
        assert np.all(np.isfinite(out[p + 'eq_px']))
        mu02 = scaled_nb.fit_mu_hat(x, b, 0.02, verbose=False)
        carry = int(np.sum((mu02 * b[:, 0] < 0.25) &
                           (mu02 * gmean(b, pseudocount=0, axis=1) >= 0.25)))
        out[p + 'n_carry'] = np.array(carry)
        print('R=%2d clamp-carry pixels: %d of %d' % (R, carry, N))
        assert R == 1 or carry > 0, R

    # q2qnbinom, vector alpha, means on both sides of the 0.25 floor
    m = 600
    xq = np.concatenate([rng.integers(0, 5, m // 2),
                         rng.integers(0, 3000, m // 2)]).astype(float)
    mu_in = np.concatenate([10 ** rng.uniform(-2, 1, m // 2),
                            10 ** rng.uniform(0, 3.3, m // 2)])
    mu_out = mu_in * np.exp(rng.normal(0, 0.4, m))
    al = 10 ** rng.uniform(-3, 1, m)
    out.update(q2q_x=xq, q2q_mu_in=mu_in.copy(), q2q_mu_out=mu_out.copy(),
               q2q_alpha=al)
    out['q2q'] = scaled_nb.q2qnbinom(xq, mu_in, mu_out, al)
    out['q2q_mu_in_after'] = mu_in
    out['q2q_mu_out_after'] = mu_out
    assert np.any(mu_in != out['q2q_mu_in']) and np.any(mu_out != out['q2q_mu_out'])

    # logpmf in broadcast shapes (n, R) x (n, 1) x (R,)
    n, R = 96, 8
    k = np.rint(10 ** rng.uniform(0, np.log10(5000), (n, R))).astype(np.int64)
    k[rng.random((n, R)) < 0.15] = 0
    k[0, 0], k[1, 1] = 0, 5000
    mm = 10 ** rng.uniform(-3, 4, (n, 1))
    ph = 10 ** rng.uniform(-7, 1, R)
    ph[0], ph[-1] = 1e-7, 10.0
    out.update(lp_k=k, lp_m=mm, lp_phi=ph,
               logpmf=scaled_nb.logpmf(k, mm, ph))
    assert out['logpmf'].shape == (n, R)
    np.savez_compressed(os.path.join(HERE, 'unit_scaled_nb.npz'), **out)


if __name__ == '__main__':
    main()
