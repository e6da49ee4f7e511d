"""Times the per-cluster statistics on the GPU (kernels of csrc/h3d_cstat.hip)
on the pixels and the calls of one cfg2-sized chromosome.

    python tools/cstat_time.py [--bins 20000 --dmax 200 --reps 20 --size 1
                                --out FILE]

Input: tools/calls_time.py's table -- the pixels of
``synthetic.draw_band(bins, (2, 2), dmax, keys=True)`` in (row, col) order
with uniform q-values -- and, as clusters, what ``threshold_clusters_gpu``
returns at fdr 0.01 and ``--size`` (1: every cluster): the small sig clusters,
then the insig ones, which are one giant component and specks. Data: K = 1
(the q-values) and K = 4 (the q-values and three random columns).

Figures per K, one JSON line:

- ``k<K>_dev_ms``: h3d_cluster_stats_dev (scope ``cstat``: every kernel of
  the call and its two status reads) on device tensors, mean / max / min
  wanted, ``sorted`` set, HIP events on the ctx stream, median of ``--reps``
  after 3 warm-up calls; ``k<K>_dev_unsorted_ms`` the same with the table
  shuffled and the sort run;
- ``k<K>_host_s``: the whole host-array call ``Context.cluster_stats``
  (checks, upload, kernels, downloads), host clock, median of ``--reps``
  after a warm-up call; ``k<K>_check_s`` the share of it spent in the host
  checks (``check_cluster_stats`` alone);
- ``k<K>_ref_loop_s``: the reference's scheme -- a scipy CSR per column, a
  Python lambda per cluster indexing it -- on this machine's CPU, one run,
  over the clusters below ``--ref-max`` pixels only (the giant component is
  left out of this leg: its fancy index alone is millions of tuples);
  ``ref_loop_clusters`` / ``ref_loop_pixels`` say how much that is. Its means
  are checked against the GPU's under the summation bound.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bins', type=int, default=20000)
    ap.add_argument('--dmax', type=int, default=200)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--fdr', type=float, default=0.01)
    ap.add_argument('--size', type=int, default=1)
    ap.add_argument('--ref-max', type=int, default=100000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import scipy.sparse as sparse
    import torch
    from hic3defdr_amd import _native, synthetic
    from hic3defdr_amd.util.thresholding import threshold_clusters_gpu

    _, _, dist, row, _ = synthetic.draw_band(args.bins, (2, 2), args.dmax,
                                             seed=0, keys=True)
    row = row.astype(np.int64)
    col = row + dist.astype(np.int64)
    order = np.lexsort((col, row))          # the outdir layout: (row, col)
    row, col = row[order], col[order]
    n = len(row)
    rng = np.random.default_rng(0)
    q = rng.random(n)
    sig, insig = threshold_clusters_gpu(q, row, col, args.fdr, args.size)
    pix = [cl.pixels() for cl in (sig, insig)]
    prow = np.concatenate([p[0] for p in pix])
    pcol = np.concatenate([p[1] for p in pix])
    sizes = np.concatenate([sig.sizes(), insig.sizes()])
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n_rows, n_cols = int(row.max()) + 1, int(col.max()) + 1
    ctx = _native.context(0)
    dev = torch.device('cuda', ctx.device)
    reducers = ('mean', 'max', 'min')
    out = {'bins': args.bins, 'dmax': args.dmax, 'pixels': int(n),
           'fdr': args.fdr, 'size': args.size, 'reps': args.reps,
           'clusters': int(len(sizes)),
           'cluster_pixels': int(starts[-1]), 'largest': int(sizes.max())}

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t_prow, t_pcol, t_starts = up(prow), up(pcol), up(starts)
    shuffle = rng.permutation(n)
    for K in (1, 4):
        data = np.column_stack([q] + [rng.normal(size=n)
                                      for _ in range(K - 1)])
        for name, perm, is_sorted in (('dev_ms', None, True),
                                      ('dev_unsorted_ms', shuffle, False)):
            t = [up(a if perm is None else a[perm]) for a in (row, col, data)]

            def fn():
                return ctx.cluster_stats_dev(t[0], t[1], t[2], n_rows, n_cols,
                                             t_prow, t_pcol, t_starts,
                                             reducers=reducers,
                                             sorted=is_sorted)
            for _ in range(3):
                got_dev = fn()
            ctx.profile(True, level=2)
            ms = []
            for _ in range(args.reps):
                ctx.profile_reset()
                fn()
                ms.append(ctx.profile_read('cstat')[0])
            ctx.profile(False)
            out['k%d_%s' % (K, name)] = round(float(np.median(ms)), 4)

        def host():
            return ctx.cluster_stats(row, col, data, prow, pcol, starts,
                                     reducers=reducers, sorted=True)
        got = host()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            host()
            ts.append(time.perf_counter() - t0)
        out['k%d_host_s' % K] = round(float(np.median(ts)), 5)
        t0 = time.perf_counter()
        _native.check_cluster_stats(row, col, data, prow, pcol, starts)
        out['k%d_check_s' % K] = round(time.perf_counter() - t0, 5)
        for f in reducers:      # the shuffled table gives the same bits
            assert got_dev[f].cpu().numpy().tobytes() == got[f].tobytes(), f

        # the reference's scheme on the small clusters
        small = np.flatnonzero(sizes <= args.ref_max)
        t0 = time.perf_counter()
        csrs = [sparse.coo_matrix((data[:, i], (row, col))).tocsr()
                for i in range(K)]
        ref = np.empty((len(small), K))
        for i in range(K):
            for j, k in enumerate(small):
                a, b = starts[k], starts[k + 1]
                ref[j, i] = np.mean(csrs[i][prow[a:b], pcol[a:b]])
        out['k%d_ref_loop_s' % K] = round(time.perf_counter() - t0, 4)
        out['ref_loop_clusters'] = int(len(small))
        out['ref_loop_pixels'] = int(sizes[small].sum())
        bound = (2 * sizes[small, None] + 2) * 2.0 ** -53 * np.abs(data).max()
        assert np.all(np.abs(got['mean'][small] - ref) <= bound)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
