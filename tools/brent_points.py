"""Census of the bounded-Brent searches' trial points on the bench's cfg2
inputs (CPU only).

The Brent kernels pick the form of the NLL term per evaluation from r =
1 / delta - 1 (csrc/h3d_model.h nll_mode: large r >= 20, mid r >= 10, r >= 5,
n r >= 5, general), so what a form is worth depends on where the searches
put their trial points. This runs the oracle's qcml (oracle/restatement.py,
untouched: its minimize_scalar_bounded is wrapped for the run) on every k-th
distance of the cfg2 chromosome (bench.py's CPU inputs, seed 0), both
conditions, records every trial point and prints

- the histogram of qcml iterations per segment,
- the evaluations per search,
- the searches' opening points,
- the evaluations split by r range, per search.

    python tools/brent_points.py [--every 6] [--bins 20000 --dmax 250]
"""
import argparse
import collections
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--every', type=int, default=6,
                    help='take every k-th distance')
    ap.add_argument('--bins', type=int, default=20000)
    ap.add_argument('--dmax', type=int, default=250)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()

    import oracle
    from oracle import restatement
    from bench import _cpu_inputs

    inp = _cpu_inputs(args.bins, args.dmax, args.seed)
    raw, f, dist, design = inp['raw'], inp['f'], inp['dist'], inp['design']
    cond = design.argmax(axis=1)

    searches = []  # per search: the trial points, in order
    inner = restatement.minimize_scalar_bounded

    def recording(func, x1, x2, **kw):
        pts = []

        def wrapped(x):
            pts.append(float(x))
            return func(x)
        out = inner(wrapped, x1, x2, **kw)
        searches.append(pts)
        return out

    iters = collections.Counter()
    n_of_search = []
    restatement.minimize_scalar_bounded = recording
    try:
        present = np.unique(dist)
        for d in present[::args.every]:
            m = dist == d
            for c in range(design.shape[1]):
                rsel = cond == c
                before = len(searches)
                oracle.qcml(raw[m][:, rsel].astype(float), f=f[m][:, rsel])
                iters[len(searches) - before] += 1
                n_of_search += [int(rsel.sum())] * (len(searches) - before)
    finally:
        restatement.minimize_scalar_bounded = inner

    segs = sum(iters.values())
    print('segments %d (every %d-th of %d distances x %d conditions), '
          'searches %d' % (segs, args.every, len(present), design.shape[1],
                           len(searches)))
    print('qcml iterations per segment:',
          ', '.join('%d: %d (%.0f %%)' % (k, v, 100. * v / segs)
                    for k, v in sorted(iters.items())))
    ev = np.array([len(p) for p in searches])
    print('evaluations per search: mean %.1f, min %d, max %d'
          % (ev.mean(), ev.min(), ev.max()))
    to_r = lambda x: 1. / x - 1  # noqa: E731
    opening = collections.Counter(
        tuple(round(to_r(x), 2) for x in p[:6]) for p in searches)
    print('opening points (r of the first six evaluations): searches')
    for k, v in opening.most_common(5):
        print('  %s: %d' % (' '.join('%.2f' % r for r in k), v))
    last = np.array([to_r(p[-1]) for p in searches])
    print('r at the last evaluation: %.1f .. %.1f (delta %.4f .. %.4f)'
          % (last.min(), last.max(), 1 / (1 + last.max()),
             1 / (1 + last.min())))
    split = collections.Counter()
    for p, n in zip(searches, n_of_search):
        for x in p:
            r = to_r(x)
            if r >= 20:
                split['large (r >= 20)'] += 1
            elif r >= 10:
                split['mid (10 <= r < 20)'] += 1
            elif n >= 2 and r >= 5:
                split['general: r >= 5'] += 1
            elif n >= 2 and n * r >= 5:
                split['general: n r >= 5, r < 5'] += 1
            else:
                split['general: n r < 5'] += 1
    print('evaluations per search by r range:')
    for k in ('general: n r < 5', 'general: n r >= 5, r < 5',
              'general: r >= 5', 'mid (10 <= r < 20)', 'large (r >= 20)'):
        print('  %-26s %.2f' % (k, split[k] / float(len(searches))))


if __name__ == '__main__':
    main()
