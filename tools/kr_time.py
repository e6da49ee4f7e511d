"""Times the sparse-bin filter and KR balancing of one chromosome-sized
simulated replicate on the host and on the GPU.

    python tools/kr_time.py [--bins 19500 --band 200 --reps 20 --out FILE]

The matrix is generated here (no files): upper triangular, band-limited to
``--band`` bins, Poisson counts around a distance decay times a per-bin
coverage factor, a few bins nearly empty so that the filter has work; at the
defaults about 19,500 bins and 2.4 M stored entries, the shape of one mm10
chr1 replicate of the simulated genome.

Figures, one JSON line:

- ``host_filter_s`` / ``host_kr_s``: ``filter_sparse_rows_count`` and
  ``kr_balance`` (scipy.sparse host code), host clock, one run each;
- ``gpu_kr_bias_s``: ``kr_bias`` from the host CSR -- the checks, the upload,
  filter, symmetrise, iteration, rescale and the bias download -- host clock,
  median of ``--reps`` after one warm-up call (``gpu_kr_bias_first_s``: that
  first call, which also allocates the ctx's buffers);
- ``gpu_iter_ms``: the iteration alone (first residual to convergence, the
  per-step record reads included), device events around it on the ctx
  stream, median of ``--reps``; ``gpu_filter_ms`` / ``gpu_symmetrise_ms`` /
  ``gpu_rescale_ms`` the other device stages the same way;
- ``outer`` / ``inner``: the Newton and CG step counts of the GPU run
  (``host_outer`` / ``host_inner``: the host's).

The GPU bias is compared with the host's before anything is printed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sparse

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_replicate(n, band, seed=0):
    """The synthetic replicate: int64 CSR, upper triangular."""
    rng = np.random.default_rng(seed)
    cover = rng.lognormal(0.0, 0.35, n)
    cover[rng.random(n) < 0.02] *= 0.002      # bins the filter should wipe
    rows, cols, vals = [], [], []
    for d in range(band + 1):
        i = np.arange(n - d)
        mean = 30.0 / (1.0 + d) ** 0.75 * cover[i] * cover[i + d]
        v = rng.poisson(mean)
        keep = v > 0
        rows.append(i[keep])
        cols.append(i[keep] + d)
        vals.append(v[keep])
    m = sparse.coo_matrix((np.concatenate(vals), (np.concatenate(rows),
                                                  np.concatenate(cols))),
                          shape=(n, n)).tocsr()
    m.sort_indices()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bins', type=int, default=19500)
    ap.add_argument('--band', type=int, default=200)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    from hic3defdr_amd import _native
    from hic3defdr_amd.util.balancing import _KR, _symmetrised, kr_balance, \
        kr_bias
    from hic3defdr_amd.util.filtering import filter_sparse_rows_count

    m = make_replicate(args.bins, args.band)
    res = {'bins': args.bins, 'band': args.band, 'nnz': int(m.nnz),
           'reps': args.reps}

    t0 = time.perf_counter()
    filt = filter_sparse_rows_count(m)
    t1 = time.perf_counter()
    _, host_bias, _ = kr_balance(filt, fl=0)
    t2 = time.perf_counter()
    res['host_filter_s'] = t1 - t0
    res['host_kr_s'] = t2 - t1
    res['wiped'] = int((host_bias == 0).sum())

    # the host's step counts (the class again, its inner solve counted)
    inner = []

    class Counting(_KR):
        def inner(self, rho, tol_in):
            out = _KR.inner(self, rho, tol_in)
            inner.append(out[1])
            return out
    full = _symmetrised(filt)
    rows = full.getnnz(1) > 0
    Counting(full[rows, :][:, rows], None, 1e-6, 0.1, 3, False).solve(3000)
    res['host_outer'], res['host_inner'] = len(inner), int(sum(inner))

    ctx = _native.context()
    stats = {}
    t0 = time.perf_counter()
    bias = kr_bias(m, stats=stats)
    res['gpu_kr_bias_first_s'] = time.perf_counter() - t0
    assert np.array_equal(bias == 0, host_bias == 0)
    nz = host_bias != 0
    res['bias_rel_err_vs_host'] = float(np.max(
        np.abs(bias[nz] - host_bias[nz]) / np.abs(host_bias[nz])))
    assert res['bias_rel_err_vs_host'] < 1e-9
    res['outer'], res['inner'] = stats['outer'], stats['inner']
    res['rows'] = stats['rows']

    wall = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        again = kr_bias(m)
        wall.append(time.perf_counter() - t0)
        assert np.array_equal(again, bias), 'a rerun changed the bias'
    # the device stages, in runs of their own (the events cost host time)
    scopes = {'kr_filter': [], 'kr_symmetrise': [], 'kr_iter': [],
              'kr_rescale': []}
    ctx.profile(True)
    for _ in range(args.reps):
        ctx.profile_reset()
        kr_bias(m)
        for name, vals in scopes.items():
            vals.append(ctx.profile_read(name)[0])
    ctx.profile(False)
    res['gpu_kr_bias_s'] = float(np.median(wall))
    res['gpu_kr_bias_min_s'] = float(np.min(wall))
    for name, vals in scopes.items():
        res['gpu_%s_ms' % name[3:]] = float(np.median(vals))
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
