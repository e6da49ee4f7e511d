"""Matrices and host-side reference runs shared by test_balancing_host.py and
test_gpu_balancing.py."""
import numpy as np
import scipy.sparse as sparse

from conftest import golden

SIMREPS = ['A1', 'A2', 'B1', 'B2']
SIM_SIZES = {'chrA': 420, 'chrB': 300}
SIM_KEYS = [(rep, chrom) for chrom in ('chrA', 'chrB') for rep in SIMREPS]


def sim_matrix(rep, chrom):
    """One of the reference's 8 simulated matrices (sim_small2.npz)."""
    g = golden('sim_small2.npz')
    n = SIM_SIZES[chrom]
    return sparse.csr_matrix(
        (g['sim__%s__%s__data' % (rep, chrom)],
         g['sim__%s__%s__indices' % (rep, chrom)],
         g['sim__%s__%s__indptr' % (rep, chrom)]), shape=(n, n))


def clamp_matrix(seed, n=96):
    """A banded Poisson matrix scaled by 10^U(-3, 3) per bin: its first CG
    steps leave the box [0.1, 3] (seed 0: the high clamp once; seed 2: the
    low clamp once)."""
    rng = np.random.default_rng(seed)
    a = np.triu(rng.poisson(6.0, (n, n)).astype(float))
    i, j = np.indices((n, n))
    a *= abs(i - j) <= 12
    d = 10 ** rng.uniform(-3, 3, n)
    return sparse.csr_matrix(a * d[:, None] * d[None, :])


def host_run(matrix, tol=1e-6, x0=None, delta=0.1, ddelta=3, max_iter=3000):
    """The host KR class on `matrix`, its clamps counted: dict(x, rows,
    outer, inner (per outer step), norms, low, high, res_sq)."""
    from hic3defdr_amd.util import balancing as hb

    class Counting(hb._KR):
        low = high = 0
        inners = ()

        def _hit_box(self, y, step, y_try):
            out = hb._KR._hit_box(self, y, step, y_try)
            if out is not None:
                if np.min(y_try) <= self.lo:
                    self.low += 1
                else:
                    self.high += 1
            return out

        def inner(self, rho, tol_in):
            out = hb._KR.inner(self, rho, tol_in)
            self.inners = self.inners + (out[1],)
            return out

        def _scaled_rowsums(self):
            out = hb._KR._scaled_rowsums(self)
            self.norms = getattr(self, 'norms', ()) + (np.sqrt(out),)
            return out

    full = hb._symmetrised(matrix)
    rows = full.getnnz(1) > 0
    kr = Counting(full[rows, :][:, rows], x0, tol, delta, ddelta, False)
    x = kr.solve(max_iter)
    # (the first residual is the start vector's, before any step)
    return dict(x=x, rows=rows, outer=len(kr.inners), inner=list(kr.inners),
                norms=list(kr.norms[1:]), low=kr.low, high=kr.high,
                res_sq=kr._scaled_rowsums())
