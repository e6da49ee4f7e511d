"""Times the APA stack on cfg1 at full size: a width-21 window over every
cluster collect() called, for every replicate of ``scaled``.

    python tools/apa_time.py [--width 21 --reps 20 --out FILE]

Three figures, one JSON line:

- ``gather_ms``: the device time of the gather itself (h3d_window_gather_dev
  on resident tables, all replicates of a chromosome in one launch), device
  events around it on the ctx stream, warmed up, median of ``--reps``;
- ``class_s``: ``HiC3DeFDR.apa_stack`` per chromosome and replicate from the
  outdir (loads, checks, upload, gather, download), host clock;
- ``scipy_wall_s`` / ``scipy_cpu_s``: the reference's way -- a Python loop
  slicing a scipy CSR matrix once per cluster (written here) -- one task per
  (chromosome, replicate) on up to 16 fresh worker processes: the slowest
  task and the tasks' sum.

The dataset is tests/test_gpu_cfg1.py's (synthetic, regenerated from its
seed). The GPU and scipy stacks are compared before anything is printed.
"""
import argparse
import concurrent.futures
import json
import multiprocessing
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import scipy.sparse as sparse

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG1 = {'chr18': 9070, 'chr19': 6143}


def scipy_stack(task):
    """The reference's loop (a worker process; never touches the GPU):
    (seconds of the loop alone, the stack)."""
    row, col, data, n_bins, points, starts, width, min_dist = task
    m = sparse.coo_matrix((data, (row, col)), shape=(n_bins, n_bins)).tocsr()
    r = width // 2
    t0 = time.perf_counter()
    stack = np.zeros((len(starts) - 1, width, width))
    for k in range(len(starts) - 1):
        com = points[starts[k]:starts[k + 1]].mean(axis=0)
        i, j = int(com[0]), int(com[1])
        if abs(com[1] - com[0]) < min_dist or com.min() < r or \
                n_bins - com.max() < r or max(i, j) + r + 1 > n_bins:
            stack[k] = np.nan
        else:
            stack[k] = m[i - r:i + r + 1, j - r:j + r + 1].toarray()
    return time.perf_counter() - t0, stack


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--width', type=int, default=21)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import pandas as pd
    import torch
    from hic3defdr_amd import HiC3DeFDR, _native, synthetic
    from hic3defdr_amd.util.apa import apa_windows
    from hic3defdr_amd.util.clusters import ClusterList, load_cluster_list
    from hic3defdr_amd.util.matrices import check_table

    g = np.load(os.path.join(REPO, 'tests', 'golden', 'full_cfg1.npz'),
                allow_pickle=False)
    dmax, width = int(g['meta_dmax']), args.width
    tmp = tempfile.mkdtemp(prefix='h3d_apa_')
    try:
        kw = synthetic.write_dataset(tmp, CFG1, dist_thresh_max=dmax,
                                     seed=int(g['meta_seed']))
        design = pd.DataFrame(kw['design'], index=kw['reps'],
                              columns=kw['conds'])
        h = HiC3DeFDR(raw_npz_patterns=kw['raw_npz_patterns'],
                      bias_patterns=kw['bias_patterns'], chroms=kw['chroms'],
                      design=design, outdir=os.path.join(tmp, 'out'),
                      dist_thresh_max=dmax, loop_patterns=kw['loop_patterns'],
                      res=10000)
        h.run_to_qvalues(verbose=False)
        h.collect(fdr=0.05, cluster_size=3)
        h.flush()
        R = len(kw['reps'])
        dev = torch.device('cuda', 0)
        ctx = _native.context(0)
        stream = torch.cuda.Stream(dev)
        torch.cuda.set_stream(stream)
        ctx.set_stream(stream.cuda_stream)

        per_chrom, tasks, n_clusters = {}, [], 0
        for chrom in kw['chroms']:
            pts, starts = [], [0]
            for kind in ['insig'] + list(kw['conds']):
                cl = load_cluster_list('%s/%s_0.05_3_%s.json'
                                       % (h.outdir, kind, chrom))
                r, c = cl.pixels()
                pts.append(np.stack([r, c], axis=1))
                starts += (starts[-1] + cl.starts[1:]).tolist()
            pts = np.concatenate(pts)
            starts = np.array(starts, dtype=np.int64)
            n_clusters += len(starts) - 1
            n_bins = h.load_bias(chrom).shape[0]
            row, col, scaled = h.load_data('scaled', chrom, coo=True)
            per_chrom[chrom] = (row, col, scaled, n_bins, pts, starts)
            for k in range(R):
                tasks.append((row, col, np.ascontiguousarray(scaled[:, k]),
                              n_bins, pts, starts, width, width + 1))

        # -- the gather alone, on resident tables ---------------------------
        gather_ms, stacks = 0.0, {}
        for chrom, (row, col, scaled, n_bins, pts, starts) in \
                per_chrom.items():
            cl = ClusterList(pts[:, 0], pts[:, 1], np.arange(len(pts)),
                             starts)
            origins, _ = apa_windows(cl, width, n_bins)
            r32, c32 = check_table(row, col)
            W = len(origins)
            t_row = torch.from_numpy(r32).to(dev)
            t_col = torch.from_numpy(c32).to(dev)
            t_data = torch.from_numpy(np.ascontiguousarray(scaled)).to(dev)
            t_org = torch.from_numpy(origins).to(dev)
            t_out = torch.empty((R, W, width, width), dtype=torch.float64,
                                device=dev)

            def gather():
                ctx.window_gather_dev(
                    t_col.data_ptr(), t_data.data_ptr(), len(r32), R,
                    (n_bins, n_bins), np.arange(R), t_org.data_ptr(), W,
                    width, width, t_out.data_ptr(), d_row=t_row.data_ptr(),
                    symmetrize=False, fill=0.0)
            for _ in range(3):
                gather()
            ms = []
            for _ in range(args.reps):
                a = torch.cuda.Event(enable_timing=True)
                b = torch.cuda.Event(enable_timing=True)
                a.record(stream)
                gather()
                b.record(stream)
                b.synchronize()
                ms.append(a.elapsed_time(b))
            gather_ms += float(np.median(ms))
            stacks[chrom] = t_out.cpu().numpy()

        # -- through the class, from the outdir -----------------------------
        for chrom in kw['chroms']:         # warm-up (scratch growth)
            h.apa_stack('scaled', chrom, [[(5, 40)]], width,
                        rep=kw['reps'][0])
        t0 = time.perf_counter()
        for chrom, (_, _, _, _, pts, starts) in per_chrom.items():
            cl = ClusterList(pts[:, 0], pts[:, 1], np.arange(len(pts)),
                             starts)
            for k, rep in enumerate(kw['reps']):
                st = h.apa_stack('scaled', chrom, cl, width, rep=rep)
                assert np.array_equal(st, stacks[chrom][k], equal_nan=True)
        class_s = time.perf_counter() - t0
        ctx.set_stream(None)
        torch.cuda.set_stream(torch.cuda.default_stream(dev))

        # -- the scipy loop, on fresh processes -----------------------------
        n_proc = min(16, len(tasks))
        with concurrent.futures.ProcessPoolExecutor(
                n_proc, mp_context=multiprocessing.get_context('spawn')) as ex:
            res = list(ex.map(scipy_stack, tasks))
        for t, (chrom, k) in zip(res, [(c, k) for c in kw['chroms']
                                       for k in range(R)]):
            assert np.array_equal(t[1], stacks[chrom][k], equal_nan=True), \
                (chrom, k)
        line = json.dumps({
            'config': 'cfg1', 'width': width, 'clusters': n_clusters,
            'replicates': R, 'windows': n_clusters * R,
            'gather_ms': round(gather_ms, 4), 'gather_reps': args.reps,
            'class_s': round(class_s, 4),
            'scipy_wall_s': round(max(t[0] for t in res), 4),
            'scipy_cpu_s': round(sum(t[0] for t in res), 4),
            'scipy_processes': n_proc,
            'stacks_equal': True})
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                        exist_ok=True)
            with open(args.out, 'w') as fh:
                fh.write(line + '\n')
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
