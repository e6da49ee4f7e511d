"""Times the diagnostics operators (hic3defdr_amd.util.diagnostics, kernels of
csrc/h3d_diag.hip) on the disp pixels of one cfg2-sized chromosome.

    python tools/diag_time.py [--bins 20000 --dmax 250 --reps 20 --out FILE]

Input: ``synthetic.draw_band(bins, (2, 2), dmax, keys=True)`` -- the cfg2
shape, R = 4: ``scaled = raw / f``, uniform p-values, q-values for half of
the pixels (the "loop" pixels), a fitted dispersion per pixel.

Figures, one JSON line, per operator ``dd_curves``, ``value_histogram``,
``ma_stats``, ``density_grid``, ``spearman``, ``pearson``, ``mvr_data``:

- ``<op>_kernel_ms``: the operator's kernels alone, HIP events on the ctx
  stream around the launches between the upload and the download (the
  library's profile scopes ``diag_*``, summed), median of ``--reps`` after 3
  warm-up calls;
- ``<op>_host_s``: the whole host-array call (checks, upload, kernels,
  download), host clock, median of ``--reps`` after a warm-up call that grows
  the ctx's buffers;
- ``<op>_numpy_s``: the numpy / scipy expression the reference evaluates, on
  the first ``--cpu-pixels`` pixels, this machine's CPU, one run, with the
  GPU result on that prefix checked against it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCOPES = {
    'dd_curves': ('diag_group_sums',),
    'value_histogram': ('diag_histogram',),
    'ma_stats': ('diag_ma_scan', 'diag_ma_stats'),
    'density_grid': ('diag_density_grid',),
    'spearman': ('diag_rank_average', 'diag_corr_matrix'),
    'pearson': ('diag_corr_matrix',),
    'mvr_data': ('diag_pixel_moments', 'diag_group_sums'),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bins', type=int, default=20000)
    ap.add_argument('--dmax', type=int, default=250)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--cpu-pixels', type=int, default=50000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import scipy.stats as st
    from hic3defdr_amd import _native, synthetic
    from hic3defdr_amd.util import diagnostics as diag

    raw, f, dist, row, _ = synthetic.draw_band(args.bins, (2, 2), args.dmax,
                                               seed=0, keys=True)
    n, R = raw.shape
    rng = np.random.default_rng(0)
    row = row.astype(np.int64)
    col = row + dist
    scaled = raw / f
    before = raw.astype(np.float64)
    design = np.array([[1, 0], [1, 0], [0, 1], [0, 1]], dtype=bool)
    loop_idx = rng.random(n) < 0.5
    pvalues = rng.random(n)
    qvalues = rng.random(int(loop_idx.sum()))
    disp_fit = 0.01 + 0.001 * dist
    xe, ye = np.linspace(-2, 12, 73), np.linspace(-6, 6, 73)
    cols = np.ascontiguousarray(scaled.T)
    ctx = _native.context(0)
    ma = diag.ma_stats(scaled, design, (0, 1), qvalues, 0.05, loop_idx)

    ops = {
        'dd_curves': lambda: diag.dd_curves(row, col, before, scaled),
        'value_histogram': lambda: diag.value_histogram(pvalues),
        'ma_stats': lambda: diag.ma_stats(scaled, design, (0, 1), qvalues,
                                          0.05, loop_idx),
        'density_grid': lambda: diag.density_grid(ma['a'], ma['m'],
                                                  ma['label'], 4, xe, ye),
        'spearman': lambda: diag.correlation_matrix(cols, 'spearman'),
        'pearson': lambda: diag.correlation_matrix(cols, 'pearson'),
        'mvr_data': lambda: diag.mvr_data(scaled[:, :2], dist, disp_fit),
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

    m = min(args.cpu_pixels, n)
    e = np.linspace(0, 1, 21)
    nl = int(loop_idx[:m].sum())

    def np_dd():
        d = col[:m] - row[:m]
        nn = max(row[:m].max(), col[:m].max()) + 1
        b = np.digitize(d, np.linspace(0, 1000, 101), right=True)
        bs = np.arange(1, b.max() + 1)
        return [np.array([np.sum(x[b == k, :], axis=0) / float(nn - k)
                          for k in bs]) for x in (before[:m], scaled[:m])]

    def np_ma():
        mean = np.dot(scaled[:m], design.astype(float)) / design.sum(axis=0)
        with np.errstate(all='ignore'):
            return (np.log2(mean[:, 0]) - np.log2(mean[:, 1]),
                    0.5 * (np.log2(mean[:, 0]) + np.log2(mean[:, 1])),
                    qvalues[:nl] < 0.05)

    def np_density():
        fin = np.isfinite(ma['a'][:m]) & np.isfinite(ma['m'][:m])
        return [np.histogram2d(ma['a'][:m][fin & (ma['label'][:m] == l)],
                               ma['m'][:m][fin & (ma['label'][:m] == l)],
                               bins=[xe, ye])[0] for l in range(4)]

    def np_corr(fn):
        out = np.eye(R)
        for i in range(R):
            for j in range(i + 1, R):
                out[i, j] = out[j, i] = fn(cols[i, :m], cols[j, :m])[0]
        return out

    def np_mvr():
        x = scaled[:m, :2]
        mean, var = np.mean(x, axis=1), np.var(x, ddof=1, axis=1)
        with np.errstate(all='ignore'):
            return mean, var, [np.mean(mean[dist[:m] == d])
                               for d in range(dist[:m].max() + 1)]

    cpu = {
        'dd_curves': np_dd,
        'value_histogram': lambda: np.histogram(pvalues[:m], bins=e)[0],
        'ma_stats': np_ma,
        'density_grid': np_density,
        'spearman': lambda: np_corr(st.spearmanr),
        'pearson': lambda: np_corr(st.pearsonr),
        'mvr_data': np_mvr,
    }

    out = {'bins': args.bins, 'dmax': args.dmax, 'pixels': int(n),
           'R': int(R), 'reps': args.reps, 'cpu_pixels': int(m)}
    for name, fn in ops.items():
        out[name + '_kernel_ms'] = round(kernel_ms(fn, SCOPES[name]), 4)
        out[name + '_host_s'] = round(host_s(fn), 5)
        t0 = time.perf_counter()
        want = cpu[name]()
        out[name + '_numpy_s'] = round(time.perf_counter() - t0, 5)
        # the GPU operator on the same prefix against the numpy result
        if name == 'value_histogram':
            np.testing.assert_array_equal(
                diag.value_histogram(pvalues[:m])[0], want)
        elif name in ('spearman', 'pearson'):
            got = diag.correlation_matrix(cols[:, :m], name)
            assert np.abs(got - want).max() <= 4 * m * 2.0 ** -53
        elif name == 'dd_curves':
            got = diag.dd_curves(row[:m], col[:m], before[:m], scaled[:m])
            np.testing.assert_allclose(got[1], want[0], rtol=1e-11)
            np.testing.assert_allclose(got[2], want[1], rtol=1e-11)
        elif name == 'mvr_data':
            got = diag.mvr_data(scaled[:m, :2], dist[:m], disp_fit[:m])
            np.testing.assert_allclose(got['pixel_mean'], want[0],
                                       rtol=1e-15)
            np.testing.assert_allclose(got['pixel_var'], want[1], rtol=1e-14,
                                       atol=1e-300)
    out['upload_mb'] = {
        'dd_curves': round(n * (4 + 16 * R) / 1e6, 1),
        'value_histogram': round(n * 8 / 1e6, 1),
        'ma_stats': round(n * (8 * R + 5) / 1e6, 1),
        'density_grid': round(n * 17 / 1e6, 1),
        'spearman': round(n * 8 * R / 1e6, 1),
        'mvr_data': round(n * (16 + 20) / 1e6, 1)}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
