"""Seeded inputs for every entry point of h3d.h that takes host buffers, and
the fixed order they are replayed in (tests/test_gpu_host_staging.py; recorded
by tools/record_host_entries.py into tests/golden/host_entries_parent.npz).

The sizes n = 0, 1, 257, 1 run in that order on ONE context: an empty call, a
single lane, one element past a 256-lane block, and a small call into slots
an earlier call grew. R = 3 takes the scalar loads of the row kernels, R = 4
the vector ones; C = 2. Where an argument is optional both forms run.

Nothing here is a yardstick of correctness -- the other suites hold the
numbers to the reference. These cases pin what the library returns, bit for
bit, so that a change to its host plumbing shows."""
import contextlib
import hashlib
import os
import zlib

import numpy as np

SIZES = (0, 1, 257, 1)
REPS = (3, 4)
C = 2
COND = {3: np.array([0, 1, 0], dtype=np.int32),
        4: np.array([0, 0, 1, 1], dtype=np.int32)}
D = 3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, 'tests', 'golden', 'host_entries_parent.npz')
SENTINEL = 0xA5


def source_sha():
    """sha256 over the sorted contents of csrc/* and include/h3d.h."""
    csrc = os.path.join(REPO, 'hic3defdr_amd', 'csrc')
    paths = sorted(os.path.join(csrc, f) for f in os.listdir(csrc))
    paths.append(os.path.join(REPO, 'include', 'h3d.h'))
    h = hashlib.sha256()
    for p in paths:
        h.update(os.path.basename(p).encode())
        with open(p, 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def counts(key, n, R):
    return _rng('counts', key, n, R).poisson(6.0, (n, R)).astype(np.int64)


def factors(key, n, R):
    return _rng('f', key, n, R).uniform(0.5, 2.0, (n, R))


def dists(key, n):
    return _rng('dist', key, n).integers(0, D, n).astype(np.int32)


def values(key, *shape):
    """Doubles with ties, zeros of both signs and a spread of magnitudes."""
    r = _rng('values', key, shape)
    v = np.round(r.normal(0.0, 3.0, shape), 1)
    v[r.random(shape) < 0.05] = -0.0
    return v


def csr(n_bins, seed):
    """An upper-triangular banded CSR matrix (indptr, indices, data) with a
    full diagonal: what the KR balancing and the window gather take."""
    r = _rng('csr', n_bins, seed)
    indptr, indices, data = [0], [], []
    for i in range(n_bins):
        cols = [j for j in range(i, min(i + 5, n_bins))
                if j == i or r.random() < 0.7]
        indices += cols
        data += list(r.integers(1, 50, len(cols)).astype(float))
        indptr.append(len(indices))
    return (np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int32),
            np.array(data, dtype=np.float64))


def native_csr(parts, n_bins):
    from hic3defdr_amd import _native
    return _native.CSR(parts[0], parts[1], parts[2], (n_bins, n_bins))


# bins of the CSR cases per size of the sequence (6 - 40 bins)
CSR_BINS = {0: 0, 1: 6, 257: 40}


class _SentinelNumpy(object):
    """numpy, except that ``empty`` fills its result with SENTINEL bytes: an
    output the library leaves untouched is then recorded as such, not as
    whatever the allocator held."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def empty(shape, dtype=float):
        a = np.empty(shape, dtype=dtype)
        a.reshape(-1).view(np.uint8)[...] = SENTINEL
        return a

    @staticmethod
    def empty_like(a):
        return _SentinelNumpy.empty(a.shape, a.dtype)


@contextlib.contextmanager
def sentinel_outputs(native):
    """The wrappers of ``native`` (hic3defdr_amd._native) allocate their
    outputs filled with SENTINEL while this is active."""
    saved = native.np
    native.np = _SentinelNumpy()
    try:
        yield
    finally:
        native.np = saved


def _flat(res):
    """The arrays of a wrapper's result, in order (None: an absent output)."""
    if isinstance(res, dict):
        res = [res[k] for k in sorted(res)]
    elif not isinstance(res, (tuple, list)):
        res = [res]
    out = []
    for r in res:
        if isinstance(r, dict):
            out += _flat(r)
        elif r is None:
            out.append(np.zeros(0, dtype=np.uint8))
        else:
            out.append(np.ascontiguousarray(r))
    return out


def cases_of(n):
    """[(name, call(ctx))] of one size of the sequence, in replay order."""
    out = []

    def add(name, fn):
        out.append(('%s n=%d' % (name, n), fn))

    for R in REPS:
        cond = COND[R]
        x, f, dist = counts('x', n, R), factors('f', n, R), dists('d', n)
        bal = _rng('bal', n, R).gamma(2.0, 3.0, (n, R))
        tab = _rng('tab', R).uniform(0.01, 0.2, (D, C))
        disp_px = _rng('disp_px', n, R).uniform(0.01, 0.2, (n, C))
        alpha_px = _rng('alpha_px', n, R).uniform(0.01, 0.2, n)
        alpha_rep = _rng('alpha_rep', R).uniform(0.01, 0.2, R)
        t = 'R=%d' % R
        # prepare_data
        add('size_factors_cmor ' + t,
            lambda c, bal=bal, dist=dist: c.size_factors_cmor(bal, dist, 0))
        add('size_factors conditional_scaling bins ' + t,
            lambda c, bal=bal, dist=dist:
            c.size_factors(bal, dist, 'conditional_scaling', 2))
        add('size_factors median_of_ratios ' + t,
            lambda c, bal=bal, dist=dist:
            c.size_factors(bal, dist, 'median_of_ratios'))
        add('size_factors simple_scaling ' + t,
            lambda c, bal=bal, dist=dist:
            c.size_factors(bal, dist, 'simple_scaling'))
        # estimate_disp, lrt
        add('disp_per_dist ' + t,
            lambda c, x=x, f=f, dist=dist, cond=cond:
            c.disp_per_dist(x, f, dist, cond, C, D))
        add('lrt ' + t,
            lambda c, x=x, f=f, dist=dist, tab=tab, cond=cond:
            c.lrt(x, f, dist, tab, cond))
        add('lrt per-pixel disp, no disp_out ' + t,
            lambda c, x=x, f=f, d=disp_px, cond=cond:
            c.lrt(x, f, None, d, cond, want_disp=False))
        add('lrt_wide ' + t,
            lambda c, x=x, f=f, cond=cond, R=R:
            c.lrt_wide(x, f, np.full((len(x), R), 0.05), cond, C))
        add('lrt_poisson ' + t,
            lambda c, x=x, f=f, cond=cond: c.lrt_poisson(x, f, cond, C))
        add('mme_per_pixel f ' + t,
            lambda c, x=x, f=f, cond=cond:
            c.mme_per_pixel(x.astype(float), f, cond, C, 1e-4))
        add('mme_per_pixel no f ' + t,
            lambda c, x=x, cond=cond:
            c.mme_per_pixel(x.astype(float), None, cond, C))
        if n >= 1:
            add('cml ' + t,
                lambda c, x=x, f=f: np.float64(c.cml(np.tile(x / f, (8, 1)))))
        # scaled NB operators
        add('nb_fit_mu scalar alpha ' + t,
            lambda c, x=x, f=f: c.nb_fit_mu(x, f, 0.05))
        add('nb_fit_mu alpha (R,) ' + t,
            lambda c, x=x, f=f, a=alpha_rep: c.nb_fit_mu(x, f, a))
        add('nb_fit_mu alpha (n, R) ' + t,
            lambda c, x=x, f=f, a=alpha_px, ar=alpha_rep:
            c.nb_fit_mu(x, f, np.outer(a, ar / ar[0])))
        add('nb_equalize scalar alpha ' + t,
            lambda c, x=x, f=f: c.nb_equalize(x, f, 0.05))
        add('nb_equalize alpha_px, mu_hat ' + t,
            lambda c, x=x, f=f, a=alpha_px: c.nb_equalize(x, f, a, True))
        # diagnostics with a replicate axis
        sc = values('scaled', n, R) ** 2 + 0.5
        keys = _rng('keys', n, R).integers(-1, 5, n).astype(np.int32)
        add('group_sums ' + t,
            lambda c, keys=keys, sc=sc: c.group_sums(keys, sc, 5))
        q = _rng('q', n, R).uniform(0, 0.2, n)
        loop = _rng('loop', n, R).random(n) < 0.5
        add('ma_stats ' + t,
            lambda c, sc=sc, cond=cond, q=q:
            c.ma_stats(sc, cond, C, 0, 1, q, 0.1))
        add('ma_stats loop_idx ' + t,
            lambda c, sc=sc, cond=cond, q=q, loop=loop:
            c.ma_stats(sc, cond, C, 1, 0, q[:int(loop.sum())], 0.1, loop))
        cols = values('cols', R, n)
        add('rank_average ' + t, lambda c, v=cols: c.rank_average(v))
        add('corr_matrix ' + t, lambda c, v=cols: c.corr_matrix(v))
        add('corr_matrix ranked ' + t,
            lambda c, v=cols: c.corr_matrix(v, ranked=True))
        add('pixel_moments ' + t,
            lambda c, sc=sc, R=R:
            c.pixel_moments(sc, np.array([0, R - 1], dtype=np.int32)))
        bias = _rng('bias', R).uniform(0.5, 2.0, (12, R))
        row = _rng('row', n, R).integers(0, 12, n).astype(np.int32)
        col = _rng('col', n, R).integers(0, 13, n).astype(np.int32)
        add('balance_pixels ' + t,
            lambda c, row=row, col=col, x=x, bias=bias:
            c.balance_pixels(row, col, x, bias))

    # entry points without a replicate axis
    v = values('flat', n)
    pos = np.abs(v) + 0.25
    add('nb_quantile_map scalar alpha',
        lambda c: c.nb_quantile_map(np.floor(pos * 3), pos.copy(),
                                    pos[::-1].copy(), 0.05))
    a_el = _rng('a_el', n).uniform(0.01, 0.2, n)

    def q2q_el(c):
        mi, mo = pos.copy(), pos[::-1].copy()
        return c.nb_quantile_map(np.floor(pos * 3), mi, mo, a_el), mi, mo
    add('nb_quantile_map alpha per element', q2q_el)
    add('nb_logpmf', lambda c: c.nb_logpmf(np.floor(pos * 3), pos, a_el))
    edges = np.array([-6.0, -1.0, 0.0, 0.5, 6.0])
    add('histogram', lambda c: c.histogram(v, edges))
    label = _rng('label', n).integers(-1, 3, n).astype(np.int8)
    add('density_grid',
        lambda c: c.density_grid(v, v[::-1], label, 3, edges, edges[1:]))
    add('bh', lambda c: c.bh(_rng('p', n).uniform(0, 1, n)))
    # evaluation
    prow = np.arange(7, dtype=np.int64)
    qrow = _rng('qrow', n).integers(0, 9, n)
    qcol = qrow + _rng('qcol', n).integers(0, 2, n)
    add('pixel_membership',
        lambda c: c.pixel_membership(qrow, qcol, prow, prow + 1))
    add('pixel_membership empty set',
        lambda c: c.pixel_membership(qrow, qcol, prow[:0], prow[:0]))
    if n >= 1:
        lab = _rng('lab', n).random(n) < 0.3
        add('roc_curve', lambda c: c.roc_curve(lab, np.abs(v), 5))
        add('roc_curve complement, keep intermediate',
            lambda c: c.roc_curve(lab, np.abs(v) / 10, 5, False, True))
    ranks = np.array([0, n // 2, max(n - 1, 0)], dtype=np.int64)[:3 if n else 0]
    add('order_stats', lambda c: c.order_stats(v, ranks))
    lo = np.array([0, 2, 5], dtype=np.int64)
    add('bin_fractions',
        lambda c: c.bin_fractions(_rng('pv', n).uniform(0, 1, n),
                                  _rng('pd', n).integers(0, 9, n), lo, lo + 2,
                                  0.3))
    # dense views: n windows over a CSR matrix of a few bins
    nb = CSR_BINS[257]
    ip, ix, dt = csr(nb, 1)
    org = _rng('org', n).integers(-2, nb, (n, 2)).astype(np.int32)
    add('window_gather indptr',
        lambda c: c.window_gather(ix, dt, org, 3, 4, (nb, nb), indptr=ip,
                                  symmetrize=True))
    rows = np.repeat(np.arange(nb, dtype=np.int32), np.diff(ip))
    dt2 = np.stack([dt, dt * 0.5], axis=1)
    add('window_gather row, two columns, mean',
        lambda c: c.window_gather(ix, dt2, org, 3, 4, (nb, nb), row=rows,
                                  mean=True, fill=0.0))
    stack = values('stack', n, 3, 4)
    stack[_rng('stack_nan', n).random(stack.shape) < 0.2] = np.nan
    add('stack_aggregate', lambda c: c.stack_aggregate(stack))
    # the sparse-bin filter and KR balancing: the CSR's bins follow the size
    kb = CSR_BINS[n]
    kip, kix, kdt = csr(kb, 2)
    ub = kb or 6
    mats = [native_csr(csr(ub, 3 + r), ub) for r in range(2)]
    ubias = _rng('ubias', ub).uniform(0.5, 2.0, (ub, 2))
    add('sparse_union', lambda c: c.sparse_union(mats, ubias, 3))
    add('filter_sparse_rows',
        lambda c: c.filter_sparse_rows(kip, kix, kdt, kb, min_nnz=3, k=4))
    add('kr_balance',
        lambda c: c.kr_balance(kip, kix, kdt, kb))
    add('kr_balance filter, x0, balanced',
        lambda c: c.kr_balance(kip, kix, kdt, kb, min_nnz=2, k=4,
                               x0=np.linspace(0.5, 1.5, kb), balanced=True))
    return out


def sequence():
    """[(name, call)] of the whole replay: the sizes of SIZES in order (the
    second n = 1 pass is named apart)."""
    seq = []
    for step, n in enumerate(SIZES):
        for name, fn in cases_of(n):
            seq.append(('%d: %s' % (step, name), fn))
    return seq


def run_case(native, ctx, fn):
    """(rc, [arrays]) of one call: a libh3d error gives its code and no
    arrays."""
    with sentinel_outputs(native):
        try:
            res = fn(ctx)
        except native.H3DError as e:
            if e.code is None:
                raise
            return e.code, []
    return 0, _flat(res)


def replay(native, ctx, before=None):
    """{key: array} of the whole sequence on ``ctx``: '<name>/rc' and
    '<name>/<i>' per output. ``before(name)`` runs ahead of every case."""
    got = {}
    for name, fn in sequence():
        if before is not None:
            before(name)
        rc, arrays = run_case(native, ctx, fn)
        got[name + '/rc'] = np.array(rc, dtype=np.int64)
        for i, a in enumerate(arrays):
            got['%s/%d' % (name, i)] = a
    return got


def same_bytes(a, b):
    """Equal dtype, shape and bytes (a NaN by its bit pattern)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and \
        np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))
