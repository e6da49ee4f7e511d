"""Sparse-bin filtering before balancing (reference
hic3defdr/util/filtering.py:7-72, used by the README's simulation workflow
ahead of kr_balance).

``filter_sparse_rows_count`` is the host code (scipy.sparse);
``filter_sparse_rows_count_gpu`` runs the same filter on the GPU
(``h3d_filter_sparse_rows``, csrc/h3d_balance.hip) and has no CPU fallback.
``util.balancing.kr_bias`` runs filter and balancing in one device pass."""
import numpy as np
import scipy.sparse as sparse


def wiped_bins(matrix, min_nnz=25, k=300):
    """The (n,) bool mask of the bins ``filter_sparse_rows_count`` wipes."""
    m = sparse.coo_matrix(matrix)
    m.sum_duplicates()
    n = m.shape[0]
    off = m.col - m.row
    band = (off >= 1) & (off <= min(n, k)) & (m.data > 0)
    # bin j: contacts (j, j+1..j+k) downstream, (j-k..j-1, j) upstream
    down = np.bincount(m.row[band], minlength=n)
    up = np.bincount(m.col[band], minlength=n)
    return (up < min_nnz) & (down < min_nnz)


def filter_sparse_rows_count(matrix, min_nnz=25, k=300):
    """Zeroes (rows and columns of) every bin that has fewer than
    ``min_nnz`` nonzero contacts with its ``k`` nearest upstream bins AND
    fewer than ``min_nnz`` with its ``k`` nearest downstream bins, counted on
    the upper triangle (the reference symmetrises its upper band,
    filtering.py:52-55). CSR input comes back CSR without the wiped entries;
    a dense array is wiped in place of a copy."""
    dense = isinstance(matrix, np.ndarray)
    if min_nnz == 0 or k == 0:
        return matrix.copy()
    wipe = wiped_bins(matrix, min_nnz, k)
    if dense:
        out = matrix.copy()
        out[:, wipe] = 0
        out[wipe, :] = 0
        return out
    keep = sparse.diags([~wipe], [0], dtype=int)
    return keep.dot(sparse.csr_matrix(matrix)).dot(keep)


def filter_sparse_rows_count_gpu(matrix, min_nnz=25, k=300):
    """``filter_sparse_rows_count`` of a square scipy sparse matrix on the
    GPU: the CSR matrix without the entries of the wiped bins, in the
    input's dtype. A dense array raises ``ValueError`` (the dense form stays
    host code); without a device the call raises ``H3DError``."""
    from hic3defdr_amd import _native
    if not sparse.issparse(matrix):
        raise ValueError('filter_sparse_rows_count_gpu takes a scipy sparse '
                         'matrix; dense arrays go through '
                         'filter_sparse_rows_count')
    if matrix.shape[0] != matrix.shape[1]:
        raise ValueError('the matrix must be square, got %r'
                         % (matrix.shape,))
    if min_nnz < 0 or k < 0:
        raise ValueError('min_nnz and k must not be negative')
    if min_nnz == 0 or k == 0:
        return matrix.copy()
    m = matrix.tocsr()
    if m is matrix:
        m = m.copy()
    m.sum_duplicates()
    m.sort_indices()
    n = m.shape[0]
    indptr, indices, data, _ = _native.context().filter_sparse_rows(
        m.indptr, m.indices, m.data, n, min_nnz, k)
    return sparse.csr_matrix((data.astype(m.dtype), indices, indptr),
                             shape=m.shape)
