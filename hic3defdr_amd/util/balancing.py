"""Knight-Ruiz matrix balancing for the simulated replicates (reference
hic3defdr/util/balancing.py:5-208; algorithm: Knight & Ruiz, IMA J. Numer.
Anal. 2013, with Juicer's "sum factor" rescale), used before a simulated
data set is analysed (README.md:586-614).

`kr_balance` is host code (scipy.sparse): some ten Newton steps and twenty
sparse mat-vecs per matrix. That is off the hot path at fixture size (a few
hundred bins, milliseconds); at the size of one mm10 chromosome replicate
(about 19,500 bins, 2.4 M stored entries) the filter and the balancing take
seconds per matrix on the host, and over the 80 replicate matrices of the
simulated genome they outweigh the GPU analysis they feed.
For that size `kr_balance_gpu`, `kr_bias` and `balance_files` run the same
arithmetic on the GPU (`h3d_kr_balance`, csrc/h3d_balance.hip) and have no
CPU fallback.

The host code is organised as a Newton outer iteration (`_KR.solve`) around
a box-constrained conjugate-gradient inner solve (`_KR.inner`); the
arithmetic (the (n, 1) column shapes, the order of the products and the
clamps) is the published one the reference transcribes, so the bias vectors
agree with the reference's to rounding (tests/test_simulation.py pins them at
1e-9)."""
import numpy as np
import scipy.sparse as sparse

from hic3defdr_amd.util.printing import eprint


def _symmetrised(array):
    """The symmetric matrix of the upper triangle of `array` (CSR)."""
    up = sparse.triu(sparse.csr_matrix(array))
    return (up + up.transpose() - sparse.diags([up.diagonal()], [0])).tocsr()


def _col_dot(a, b):
    # inner product of two (n, 1) columns as a (1, 1) matrix product
    return np.dot(a.T, b)


class _KR(object):
    """State of one balancing run on the non-empty rows `A` of the matrix."""

    def __init__(self, A, x0, tol, lo, hi, verbose):
        self.A = A
        self.lo, self.hi = lo, hi
        self.verbose = verbose
        self.target = tol ** 2           # stop once |1 - x (A x)|^2 <= target
        self.floor_eta = 0.5 * tol
        self.x = np.ones((A.shape[0], 1)) if x0 is None else x0
        self.history = []

    def _scaled_rowsums(self):
        self.v = self.x * self.A.dot(self.x)
        self.r = 1 - self.v
        return float(_col_dot(self.r, self.r)[0, 0])

    def _hit_box(self, y, step, y_try):
        """CG left the box [lo, hi]: the largest multiple of `step` that
        keeps y inside (None: stay inside, continue)."""
        if np.min(y_try) <= self.lo:
            if self.lo == 0:
                return y
            down = np.where(step < 0)
            return y + np.min((self.lo - y[down]) / step[down]) * step
        if np.max(y_try) >= self.hi:
            up = np.where(y_try > self.hi)
            # the builtin min, as the transcription (the values are 1-D here)
            return y + min((self.hi - y[up]) / step[up]) * step
        return None

    def inner(self, rho, tol_in):
        """Preconditioned CG on (diag(x) A diag(x) + diag(v)) y = 1 from
        y = 1; returns (y, the inner iterations, the last rho)."""
        x, v, A = self.x, self.v, self.A
        y = np.ones_like(x)
        k, rho_prev, p = 0, None, None
        z = None
        while rho > tol_in:
            k += 1
            if k == 1:
                z = self.r / v
                p = z.copy()
                rho = _col_dot(self.r, z)
            else:
                p = z + (rho / rho_prev) * p
            w = x * A.dot(x * p) + v * p
            alpha = rho / _col_dot(p, w)
            step = alpha * p
            y_try = y + step
            clamped = self._hit_box(y, step, y_try)
            if clamped is not None:
                return clamped, k, rho
            y = y_try
            self.r = self.r - alpha * w
            rho_prev = rho
            z = self.r / v
            rho = _col_dot(self.r, z)
        return y, k, rho

    def solve(self, max_iter):
        g, eta_cap = 0.9, 0.1
        eta = eta_cap
        rho = self._scaled_rowsums()
        res_sq = res_prev = rho
        if self.verbose:
            print('it in. it res')
        outer = 0
        while res_sq > self.target:
            if max_iter is not None and outer > max_iter:
                break
            outer += 1
            y, k, rho = self.inner(rho, max(eta ** 2 * res_sq, self.target))
            self.x = self.x * y
            rho = self._scaled_rowsums()
            res_sq = rho
            ratio, res_prev = res_sq / res_prev, res_sq
            norm = np.sqrt(res_sq)
            # forcing term of the inexact Newton step (Eisenstat-Walker)
            eta_last, eta = eta, g * ratio
            if g * eta_last ** 2 > 0.1:
                eta = max(eta, g * eta_last ** 2)
            eta = max(min(eta, eta_cap), self.floor_eta / norm)
            if self.verbose:
                print('{} {} {:.3e}'.format(outer, k, norm))
                self.history.append(norm)
        return self.x


def kr_balance(array, tol=1e-6, x0=None, delta=0.1, ddelta=3, fl=1,
               max_iter=3000):
    """Returns (balanced CSR, bias, residual norms) as the reference
    (balancing.py:5-208): `array` is symmetrised from its upper triangle,
    empty rows sit out the iteration and get bias 0, the scaling vector is
    rescaled so the balanced matrix keeps the original total, and bias is
    its inverse. The balanced matrix is upper triangular when the input
    was; fl == 1 prints the convergence table."""
    upper_input = sparse.tril(array, k=-1).nnz == 0
    full = _symmetrised(array)
    rows = full.getnnz(1) > 0
    kr = _KR(full[rows, :][:, rows], x0, tol, delta, ddelta, fl == 1)
    x = kr.solve(max_iter)
    scale = np.zeros(rows.shape, dtype=float)
    scale[rows] = np.squeeze(x)

    def apply(s):
        d = sparse.diags([s], [0])
        return d.dot(full).dot(d)
    scale *= np.sqrt(full.sum() / apply(scale).sum())
    balanced = apply(scale)
    nz = scale != 0
    scale[nz] = 1 / scale[nz]
    if upper_input:
        balanced = sparse.triu(balanced).tocsr()
    return balanced, scale, np.array(kr.history)


# ---- the same on the GPU ---------------------------------------------------

def _upper_canonical(array):
    """(the upper triangle of `array` as canonical CSR, whether `array` had
    nothing stored below the diagonal); ValueError unless it is square."""
    if hasattr(array, 'indptr') and not sparse.issparse(array):
        # the native NPZ reader's CSR (canonical already)
        array = sparse.csr_matrix((array.data, array.indices, array.indptr),
                                  shape=array.shape)
    m = sparse.csr_matrix(array)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError('the matrix must be square, got %r' % (m.shape,))
    row = np.repeat(np.arange(m.shape[0], dtype=m.indices.dtype),
                    np.diff(m.indptr))
    upper_input = bool(np.all(m.indices >= row))
    if not (upper_input and m.has_canonical_format):
        m = sparse.triu(m, format='csr')
        m.sum_duplicates()
        m.sort_indices()
    return m, upper_input


def _check_kr_args(tol, max_iter):
    if not tol >= 0:
        raise ValueError('tol must not be negative, got %r' % (tol,))
    if max_iter is not None and max_iter != int(max_iter):
        raise ValueError('max_iter must be an integer or None')


def _x0_by_bin(up, x0, min_nnz, k):
    """`x0` (one value per row of the iteration, as `kr_balance` takes it)
    spread over the bins, or None; ValueError on a wrong length. The rows of
    the iteration are the bins that keep an entry after the filter."""
    if x0 is None:
        return None
    from hic3defdr_amd.util.filtering import wiped_bins
    coo = up.tocoo()
    keep = coo.data != 0
    if min_nnz != 0 and k != 0:
        wipe = wiped_bins(up, min_nnz, k)
        keep &= ~wipe[coo.row] & ~wipe[coo.col]
    rows = np.zeros(up.shape[0], dtype=bool)
    rows[coo.row[keep]] = True
    rows[coo.col[keep]] = True
    x0 = np.asarray(x0, dtype=float)
    if x0.size != rows.sum():
        raise ValueError('x0 must have one value per non-empty row (%d), got '
                         '%d' % (rows.sum(), x0.size))
    by_bin = np.ones(up.shape[0])
    by_bin[rows] = x0.ravel()
    return by_bin


def _print_table(res):
    print('it in. it res')
    for i, (k, norm) in enumerate(zip(res['inner'], res['norms'])):
        print('{} {} {:.3e}'.format(i + 1, k, norm))


def kr_balance_gpu(array, tol=1e-6, x0=None, delta=0.1, ddelta=3, fl=1,
                   max_iter=3000, stats=None):
    """`kr_balance` on the GPU (`h3d_kr_balance`): the same arguments, the
    same (balanced CSR, bias, residual norms). The iteration is symmetrised
    from the upper triangle of `array`; the balanced matrix is upper
    triangular when the input was; fl == 1 prints the convergence table
    (after the run) and returns its norms, as the host code does. `stats`: a
    dict that receives the run's counters (`_native.Context.KR_STATS`).
    Raises ValueError for a non-square matrix, a negative tol or an x0 of the
    wrong length before any device call, H3DError without a device."""
    from hic3defdr_amd import _native
    up, upper_input = _upper_canonical(array)
    _check_kr_args(tol, max_iter)
    x0 = _x0_by_bin(up, x0, 0, 0)
    res = _native.context().kr_balance(
        up.indptr, up.indices, up.data, up.shape[0], tol=tol, lo=delta,
        hi=ddelta, max_iter=max_iter, x0=x0, balanced=True)
    if stats is not None:
        stats.update(res['stats'])
    balanced = sparse.csr_matrix((res['balanced'], up.indices, up.indptr),
                                 shape=up.shape)
    balanced.eliminate_zeros()
    if not upper_input:
        balanced = (balanced + balanced.transpose() - sparse.diags(
            [balanced.diagonal()], [0])).tocsr()
    if fl == 1:
        _print_table(res)
    return balanced, res['bias'], res['norms'] if fl == 1 else np.array([])


def kr_bias(matrix, min_nnz=25, k=300, tol=1e-6, x0=None, delta=0.1,
            ddelta=3, fl=0, max_iter=3000, stats=None):
    """The bias vector of `kr_balance(filter_sparse_rows_count(matrix,
    min_nnz, k), ...)` in one device pass (`h3d_kr_balance`): the matrix is
    uploaded once, filtered, symmetrised and balanced on the GPU, and only
    the bias comes back. `matrix`: a scipy sparse matrix or the native NPZ
    reader's CSR; the keywords after `k` are `kr_balance`'s (fl defaults to
    0 here: no table). Errors as `kr_balance_gpu`."""
    from hic3defdr_amd import _native
    up, _ = _upper_canonical(matrix)
    _check_kr_args(tol, max_iter)
    if min_nnz < 0 or k < 0:
        raise ValueError('min_nnz and k must not be negative')
    x0 = _x0_by_bin(up, x0, min_nnz, k)
    res = _native.context().kr_balance(
        up.indptr, up.indices, up.data, up.shape[0], min_nnz=min_nnz, k=k,
        tol=tol, lo=delta, hi=ddelta, max_iter=max_iter, x0=x0)
    if stats is not None:
        stats.update(res['stats'])
    if fl == 1:
        _print_table(res)
    return res['bias']


def balance_files(infile_pattern, repnames, chroms, suffix='_kr.bias', **kw):
    """The README's balancing loop over the simulated replicates
    (README.md:602-614) on the GPU: for every replicate and chromosome, reads
    `infile_pattern` (with `<rep>` and `<chrom>` replaced; the name ends in
    `_raw.npz`) with the native NPZ reader, runs `kr_bias(matrix, **kw)` and
    writes the bias with np.savetxt next to it, `_raw.npz` replaced by
    `suffix`. Returns the files written."""
    from hic3defdr_amd import _native
    written = []
    for repname in repnames:
        for chrom in chroms:
            eprint('balancing rep %s chrom %s' % (repname, chrom))
            infile = infile_pattern.replace('<rep>', repname) \
                .replace('<chrom>', chrom)
            if not infile.endswith('_raw.npz'):
                raise ValueError('infile_pattern must end in _raw.npz')
            outfile = infile[:-len('_raw.npz')] + suffix
            np.savetxt(outfile, kr_bias(_native.load_npz_csr(infile), **kw))
            written.append(outfile)
    return written
