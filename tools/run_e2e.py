"""BASELINE configs[2] (cfg3, the mouse genome at 10 kb: 20 chromosomes,
~263k bins, R = 4 as 2 + 2, dist_thresh_max 200) END TO END through the
product class, files included: the synthetic genome is written in the
reference's input layout (per-replicate NPZ + bias files, loop-cluster
JSON; synthetic.py's generator, each chromosome from its own seed, written
by a process pool), then ``HiC3DeFDR.run_to_qvalues()`` (prepare_data ->
estimate_disp -> lrt -> bh, analysis.py:305-364 of the reference) and
``collect()`` run on it, each stage timed; the outdir writes land behind the
stages (write-behind) and the wait for the last of them is reported.

    python tools/run_e2e.py [--chroms 20] [--workers 16] [--keep DIR]
                            [--collect-gpu]

``--collect-gpu`` (single rank): afterwards collect() is run again from the
q-values alone, default and with gpu=True, each with the seconds it spends in
text formatting and file reads / writes (tools/calls_time.py collect_timed).

Prints one JSON line. Under torchrun it runs the sharded path (each rank
its LPT chromosomes, the distance re-shard, the sample-sort BH).
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

DMAX = 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chroms', type=int, default=20)
    ap.add_argument('--workers', type=int, default=16)
    ap.add_argument('--seed', type=int, default=3)
    ap.add_argument('--keep', default=None,
                    help='write the dataset and outdir here and keep them')
    ap.add_argument('--collect-gpu', action='store_true',
                    help='time collect() default and gpu=True side by side')
    ap.add_argument('--profile', type=int, default=0,
                    help='cProfile the stages, print the top N to stderr')
    args = ap.parse_args()
    import pandas as pd
    from hic3defdr_amd import HiC3DeFDR
    from hic3defdr_amd.synthetic import MM10_BINS, write_genome
    bins = list(MM10_BINS[:args.chroms])
    base = args.keep or tempfile.mkdtemp(prefix='h3d_e2e_')
    os.makedirs(base, exist_ok=True)
    try:
        t0 = time.perf_counter()
        kw = write_genome(base, bins, args.seed, args.workers, dmax=DMAX)
        write_s = time.perf_counter() - t0
        print('genome written: %d chromosomes, %d bins, %.1f s' % (
            len(bins), sum(bins), write_s), file=sys.stderr, flush=True)
        design = pd.DataFrame(kw['design'], index=kw['reps'],
                              columns=kw['conds'])
        h = HiC3DeFDR(raw_npz_patterns=kw['raw_npz_patterns'],
                      bias_patterns=kw['bias_patterns'], chroms=kw['chroms'],
                      design=design, outdir=os.path.join(base, 'out'),
                      dist_thresh_max=DMAX, loop_patterns=kw['loop_patterns'],
                      res=10000)
        # process start costs, reported apart: torch's import (the device
        # allocator; the first _shards() pulls it in) and the HIP context
        t = time.perf_counter()
        h._shards()
        h._ctx()
        init_s = time.perf_counter() - t
        print('  init (torch import, HIP context) %.3f s' % init_s,
              file=sys.stderr, flush=True)
        stages = {}
        if args.profile:
            import cProfile
            prof = cProfile.Profile()
            prof.enable()
        t = time.perf_counter()
        for name, fn in (('prepare_data', lambda: h.prepare_data(verbose=False)),
                         ('estimate_disp', h.estimate_disp),
                         ('lrt', lambda: h.lrt(verbose=False)),
                         ('bh', h.bh),
                         ('outdir_flush', h.flush)):
            fn()
            now = time.perf_counter()
            stages[name + '_s'] = now - t
            t = now
            print('  %s %.3f s' % (name, stages[name + '_s']), file=sys.stderr,
                  flush=True)
        total = sum(stages.values())
        if args.profile:
            import pstats
            prof.disable()
            for key in ('cumulative', 'tottime'):
                pstats.Stats(prof, stream=sys.stderr).sort_stats(key) \
                    .print_stats(args.profile)
        t = time.perf_counter()
        h.collect(fdr=[0.01, 0.05], cluster_size=[3, 4])
        h.flush()
        collect_s = time.perf_counter() - t
        sh = h._shards()
        n_disp = sum(int(h.load_data('disp_idx', c).sum()) for c in sh.mine)
        q = np.concatenate([h.load_data('qvalues', c) for c in sh.mine]) \
            if sh.mine else np.zeros(0)
        out = {
            'config': 'cfg3 end to end (files)', 'chroms': len(bins),
            'bins': int(sum(bins)), 'reps': 4, 'conds': 2,
            'dist_thresh_max': DMAX, 'rank': sh.rank, 'world': sh.world,
            'disp_pixels_this_rank': n_disp,
            'init_s': init_s, 'run_to_qvalues_s': total, 'stages': stages,
            'pixels_per_s_run_to_qvalues': n_disp / total,
            'estimate_disp_plus_lrt_s': stages['estimate_disp_s'] +
            stages['lrt_s'],
            'collect_s': collect_s, 'write_dataset_s': write_s,
            'loop_pixels_q_lt_0.05': int(np.sum(q < 0.05)),
        }
        if args.collect_gpu and sh.world == 1:
            sys.path.insert(0, os.path.join(REPO, 'tools'))
            from calls_time import collect_timed
            collect_timed(h, True)                  # grows the ctx's buffers
            out['collect_default'] = collect_timed(h, False)
            out['collect_gpu'] = collect_timed(h, True)
        if sh.rank == 0:
            print(json.dumps(out), flush=True)
    finally:
        if not args.keep:
            shutil.rmtree(base, ignore_errors=True)


if __name__ == '__main__':
    main()
