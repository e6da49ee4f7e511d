"""Times the calls on the GPU (kernels of csrc/h3d_clusters.hip) on the pixels
of one cfg2-sized chromosome, and collect() with and without gpu=True on cfg1
at full size.

    python tools/calls_time.py [--bins 20000 --dmax 200 --reps 20 --out FILE]
                               [--no-cfg1]

Input: the pixels of ``synthetic.draw_band(bins, (2, 2), dmax, keys=True)``
-- cfg2's pixel count -- with uniform q-values, thresholded at fdr 0.01:
about 1 % of the pixels are sig (tens of thousands of small clusters) and
the 99 % insig pixels are one giant component and a few specks. Three class
vectors are labelled: ``both`` (the one pass threshold(gpu=True) makes),
``sig`` (the insig pixels absent) and ``insig`` (the sig pixels absent).

Figures, one JSON line:

- ``<input>_label_ms`` / ``<input>_lists_ms``: the labelling kernels
  (h3d_label_components_dev, scope ``ccl_label``) and the list kernels
  (h3d_cluster_lists_dev, min_size 3, scope ``ccl_lists``) alone, HIP events
  on the ctx stream, median of ``--reps`` after 3 warm-up calls; the events
  span the call's one or two status reads as well;
- ``threshold_gpu_host_s``: the whole host-array call
  ``threshold_clusters_gpu`` (checks, upload, kernels, downloads, the two
  ClusterLists), host clock, median of ``--reps`` after a warm-up call;
- ``threshold_cpu_s``: ``threshold_clusters`` (the default path) on the same
  arrays, this machine's CPU, one run, its partition checked equal;
- ``cfg1``: ``collect(fdr=[0.01, 0.05], cluster_size=[3, 4])`` default and
  ``gpu=True`` on cfg1 at full size (each from q-values alone), host clock,
  with the seconds spent in text formatting and file reads / writes
  (``text_io_s``: save_clusters, ClusterList.texts, the TSV writer and
  reader) -- ``collect_timed`` below, which tools/run_e2e.py uses for cfg3.
"""
import argparse
import glob
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG1 = {'chr18': 9070, 'chr19': 6143}


def canonical(cl, n):
    """A ClusterList over n pixels -> labels numbered by first member."""
    raw = np.full(n, -1, dtype=np.int64)
    raw[cl.members] = np.repeat(np.arange(len(cl)), cl.sizes())
    present = np.flatnonzero(raw >= 0)
    uniq, first = np.unique(raw[present], return_index=True)
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[np.argsort(first, kind='stable')] = np.arange(len(uniq))
    raw[present] = rank[np.searchsorted(uniq, raw[present])]
    return raw


def collect_timed(h, gpu, fdr=(0.01, 0.05), cluster_size=(3, 4)):
    """Removes the call files of h's outdir, runs collect() and returns
    {'collect_s', 'text_io_s'}: the whole step and the part of it inside the
    text formatting and the file reads / writes."""
    from hic3defdr_amd.analysis import analysis
    from hic3defdr_amd.util import clusters
    from hic3defdr_amd.util.cluster_table import ClusterTable
    for pat in ('*.json', '*.tsv'):
        for f in glob.glob(os.path.join(h.outdir, pat)):
            os.remove(f)
    spent = [0.0, 0]

    def timed(fn):
        def wrapper(*a, **k):
            spent[1] += 1
            t = time.perf_counter() if spent[1] == 1 else None
            try:
                return fn(*a, **k)
            finally:
                spent[1] -= 1
                if t is not None:
                    spent[0] += time.perf_counter() - t
        return wrapper
    saved = [(analysis, 'save_clusters', analysis.save_clusters),
             (analysis, 'load_cluster_list', analysis.load_cluster_list),
             (clusters.ClusterList, 'texts', clusters.ClusterList.texts),
             (ClusterTable, 'to_tsv', ClusterTable.to_tsv),
             (ClusterTable, 'read_tsv', ClusterTable.__dict__['read_tsv'])]
    try:
        for obj, name, fn in saved:
            if isinstance(fn, classmethod):
                setattr(obj, name, classmethod(timed(fn.__func__)))
            else:
                setattr(obj, name, timed(fn))
        t0 = time.perf_counter()
        h.collect(fdr=list(fdr), cluster_size=list(cluster_size), gpu=gpu)
        h.flush()
        total = time.perf_counter() - t0
    finally:
        for obj, name, fn in saved:
            setattr(obj, name, fn)
    return {'collect_s': round(total, 4), 'text_io_s': round(spent[0], 4)}


def cfg1_collect():
    import pandas as pd
    from hic3defdr_amd import HiC3DeFDR, synthetic
    tmp = tempfile.mkdtemp(prefix='h3d_calls_time_')
    try:
        kw = synthetic.write_dataset(tmp, CFG1, dist_thresh_max=200, seed=0)
        design = pd.DataFrame(kw['design'], index=kw['reps'],
                              columns=kw['conds'])
        h = HiC3DeFDR(raw_npz_patterns=kw['raw_npz_patterns'],
                      bias_patterns=kw['bias_patterns'], chroms=kw['chroms'],
                      design=design, outdir=os.path.join(tmp, 'out'),
                      dist_thresh_max=200, loop_patterns=kw['loop_patterns'],
                      res=10000)
        h.run_to_qvalues(verbose=False)
        collect_timed(h, True)                      # grows the ctx's buffers
        out = {'default': collect_timed(h, False), 'gpu': collect_timed(h, True)}
        with open(os.path.join(h.outdir, 'results_0.05_3.tsv')) as fh:
            out['results_0.05_3_rows'] = len(fh.read().split('\n')) - 2
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bins', type=int, default=20000)
    ap.add_argument('--dmax', type=int, default=200)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--fdr', type=float, default=0.01)
    ap.add_argument('--no-cfg1', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    from hic3defdr_amd import _native, synthetic
    from hic3defdr_amd.util.thresholding import (threshold_clusters,
                                                 threshold_clusters_gpu)

    _, _, dist, row, _ = synthetic.draw_band(args.bins, (2, 2), args.dmax,
                                             seed=0, keys=True)
    row = row.astype(np.int64)
    col = row + dist.astype(np.int64)
    order = np.lexsort((col, row))          # the outdir layout: (row, col)
    row, col = row[order], col[order]
    n = len(row)
    q = np.random.default_rng(0).random(n)
    ctx = _native.context(0)
    dev = torch.device('cuda', ctx.device)
    t_row, t_col = torch.from_numpy(row).to(dev), torch.from_numpy(col).to(dev)
    both = ctx.threshold_classes_dev(torch.from_numpy(q).to(dev), args.fdr)
    absent = torch.full_like(both, 255)
    inputs = {'both': both, 'sig': torch.where(both == 0, both, absent),
              'insig': torch.where(both == 1, both, absent)}

    out = {'bins': args.bins, 'dmax': args.dmax, 'pixels': int(n),
           'fdr': args.fdr, 'reps': args.reps,
           'sig_pixels': int((both == 0).sum())}
    for name, t_cls in inputs.items():
        def fn():
            label, nc = ctx.label_components_dev(t_row, t_col, t_cls, 1)
            return nc, ctx.cluster_lists_dev(label, t_cls, t_row, t_col, nc, 3)
        for _ in range(3):
            nc, lists = fn()
        ctx.profile(True, level=2)
        ms = {'ccl_label': [], 'ccl_lists': []}
        for _ in range(args.reps):
            ctx.profile_reset()
            fn()
            for s in ms:
                ms[s].append(ctx.profile_read(s)[0])
        ctx.profile(False)
        out[name + '_label_ms'] = round(float(np.median(ms['ccl_label'])), 4)
        out[name + '_lists_ms'] = round(float(np.median(ms['ccl_lists'])), 4)
        out[name + '_clusters'] = int(nc)
        out[name + '_largest'] = int(lists['size'].max()) if nc else 0

    def host():
        return threshold_clusters_gpu(q, row, col, args.fdr, 3)
    host()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        got = host()
        ts.append(time.perf_counter() - t0)
    out['threshold_gpu_host_s'] = round(float(np.median(ts)), 5)
    t0 = time.perf_counter()
    want = threshold_clusters(q, row, col, args.fdr)
    out['threshold_cpu_s'] = round(time.perf_counter() - t0, 5)
    for g, w, idx in ((got[0], want[0], np.flatnonzero(q < args.fdr)),
                      (got[1], want[1], np.flatnonzero(q >= args.fdr))):
        w = w.size_filter(3)
        full = np.full(n, -1, dtype=np.int64)
        full[idx] = canonical(w, len(idx))          # w indexes the subset
        np.testing.assert_array_equal(canonical(g, n), full)
    if not args.no_cfg1:
        out['cfg1'] = cfg1_collect()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
