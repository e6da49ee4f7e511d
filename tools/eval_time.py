"""Times the evaluation operators (kernels of csrc/h3d_eval.hip) on the disp
pixels of one cfg2-sized chromosome.

    python tools/eval_time.py [--bins 20000 --dmax 250 --reps 20 --out FILE]

Input: the pixels of ``synthetic.draw_band(bins, (2, 2), dmax, keys=True)``
-- cfg2's pixel count -- with uniform p- and q-values; about 1 % of the
pixels form the cluster set, so about 1 % of the labels are positive.

Figures, one JSON line, per operator ``membership``
(``pixel_membership_gpu``), ``evaluate`` (``evaluate_gpu``) and
``distance_bias`` (8 ranges):

- ``<op>_kernel_ms``: the operator's kernels alone, HIP events on the ctx
  stream around the launches between the upload and the download (the
  library's profile scopes ``eval_*``, summed), median of ``--reps`` after 3
  warm-up calls;
- ``<op>_host_s``: the whole host-array call (checks, upload, kernels,
  download), host clock, median of ``--reps`` after a warm-up call that grows
  the ctx's buffers;
- ``<op>_cpu_s``: the host function it stands beside (``pixel_membership``,
  ``evaluate`` with scikit-learn, the numpy expressions of
  plotting/distance_bias.py) on the same arrays, this machine's CPU, one
  run, with the GPU result checked equal to it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCOPES = {
    'membership': ('eval_membership',),
    'evaluate': ('eval_roc',),
    'distance_bias': ('eval_order_stats', 'eval_bin_fractions'),
}
BINS = [(None, 15), (16, 30), (31, 60), (61, 120), (121, None), (None, None),
        (10, 100), (200, None)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bins', type=int, default=20000)
    ap.add_argument('--dmax', type=int, default=250)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import warnings
    from hic3defdr_amd import _native, synthetic
    from hic3defdr_amd.util import clusters, diagnostics, evaluation

    _, _, dist, row, _ = synthetic.draw_band(args.bins, (2, 2), args.dmax,
                                             seed=0, keys=True)
    n = len(row)
    rng = np.random.default_rng(0)
    row = row.astype(np.int64)
    dist = dist.astype(np.int64)
    col = row + dist
    pvalues = rng.random(n)
    qvalues = rng.random(n)
    member = rng.random(n) < 0.01
    pix = np.stack([row[member], col[member]], axis=1)
    pix = pix[rng.permutation(len(pix))]
    ctx = _native.context(0)
    y_true = clusters.pixel_membership_gpu(row, col, [pix])

    ops = {
        'membership': lambda: clusters.pixel_membership_gpu(row, col, [pix]),
        'evaluate': lambda: evaluation.evaluate_gpu(y_true, qvalues),
        'distance_bias': lambda: diagnostics.distance_bias(pvalues, dist,
                                                           BINS),
    }

    def kernel_ms(fn, scopes):
        for _ in range(3):
            fn()
        ctx.profile(True, level=2)
        ms = []
        for _ in range(args.reps):
            ctx.profile_reset()
            fn()
            ms.append(sum(ctx.profile_read(s)[0] for s in scopes))
        ctx.profile(False)
        return float(np.median(ms))

    def host_s(fn):
        fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    def cpu_bias():
        p_star = np.percentile(pvalues, 100 * 0.05)
        out = []
        for lo, hi in BINS:
            idx = np.ones(n, dtype=bool)
            if lo is not None:
                idx[dist < lo] = False
            if hi is not None:
                idx[dist > hi] = False
            out.append(np.mean(pvalues[idx] < p_star))
        return p_star, np.array(out)

    def cpu_evaluate():
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            return evaluation.evaluate(y_true, qvalues)

    cpu = {
        'membership': lambda: (clusters.pixel_membership(row, col, [pix]),),
        'evaluate': cpu_evaluate,
        'distance_bias': cpu_bias,
    }

    out = {'bins': args.bins, 'dmax': args.dmax, 'pixels': int(n),
           'set_pixels': int(len(pix)), 'positives': int(y_true.sum()),
           'reps': args.reps}
    for name, fn in ops.items():
        out[name + '_kernel_ms'] = round(kernel_ms(fn, SCOPES[name]), 4)
        out[name + '_host_s'] = round(host_s(fn), 5)
        t0 = time.perf_counter()
        want = cpu[name]()
        out[name + '_cpu_s'] = round(time.perf_counter() - t0, 5)
        got = fn()
        got = got if isinstance(got, tuple) else (got,)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b, name)
    out['curve_points'] = int(len(ops['evaluate']()[3]))
    out['upload_mb'] = {
        'membership': round((n + len(pix)) * 16 / 1e6, 1),
        'evaluate': round(n * 9 / 1e6, 1),
        'distance_bias': round(n * (8 + 16) / 1e6, 1)}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
