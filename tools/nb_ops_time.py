"""Times the scaled-NB operators (hic3defdr_amd.util.scaled_nb: equalize and
fit_mu_hat, kernels of csrc/h3d_nb.hip) on the disp pixels of one cfg2-sized
chromosome in the CALLER's pixel order.

    python tools/nb_ops_time.py [--bins 20000 --dmax 250 --reps 20 --out FILE]

Input: ``synthetic.draw_band(bins, (2, 2), dmax)`` -- the cfg2 shape, R = 4,
pixels in the band's own order (distance-major as drawn; no coherence sort).
equalize runs at the dispersion 0.02 over all four replicates, fit_mu_hat at
the scalar dispersion 0.05.

Figures, one JSON line:

- ``equalize_kernel_ms`` / ``fit_mu_kernel_ms``: the kernel alone on resident
  device buffers (``Context.nb_equalize_dev`` / ``nb_fit_mu_dev``), HIP
  events around the launch on the ctx stream (the library's profile scopes
  ``nb_equalize`` / ``nb_fit_mu``), median of ``--reps`` after 3 warm-up
  calls;
- ``equalize_host_s`` / ``fit_mu_host_s``: the whole host-array call
  (checks, int64 -> int32 conversion, upload, kernel, download), host clock,
  median of ``--reps`` after one warm-up call that grows the ctx's buffers;
- ``upload_mb`` / ``download_mb``: what the host-array equalize call moves;
- ``oracle_equalize_s`` / ``oracle_fit_mu_s``: the oracle's numpy / scipy
  restatement of the reference on the first ``--cpu-pixels`` pixels, this
  machine's CPU, one run each, with the GPU results checked against them.
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
    ap.add_argument('--dmax', type=int, default=250)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--cpu-pixels', type=int, default=50000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    import oracle
    from hic3defdr_amd import _native, synthetic
    from hic3defdr_amd.util import scaled_nb

    raw, f, _ = synthetic.draw_band(args.bins, (2, 2), args.dmax, seed=0)
    keep = raw.sum(axis=1) > 0          # (an all-zero row has no MLE)
    raw = np.ascontiguousarray(raw[keep])
    f = np.ascontiguousarray(f[keep])
    n, R = raw.shape
    dev = torch.device('cuda', 0)
    ctx = _native.context(0)
    t_x = torch.from_numpy(raw.astype(np.int32)).to(dev)
    t_f = torch.from_numpy(f).to(dev)
    t_a = torch.full((1,), 0.05, dtype=torch.float64, device=dev)
    t_pd = torch.empty((n, R), dtype=torch.float64, device=dev)
    t_mu = torch.empty((n,), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)

    def k_equalize():
        assert ctx.nb_equalize_dev(t_x.data_ptr(), t_f.data_ptr(), 0.02, n, R,
                                   t_pd.data_ptr()) == 0

    def k_fit():
        assert ctx.nb_fit_mu_dev(t_x.data_ptr(), t_f.data_ptr(),
                                 t_a.data_ptr(), (0, 0), n, R,
                                 t_mu.data_ptr()) == 0

    def kernel_ms(fn, scope):
        for _ in range(3):
            fn()
        ctx.profile(True, level=2)
        ms = []
        for _ in range(args.reps):
            ctx.profile_reset()
            fn()
            ms.append(ctx.profile_read(scope)[0])
        ctx.profile(False)
        return float(np.median(ms))

    def host_s(fn):
        fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), out

    eq_ms = kernel_ms(k_equalize, 'nb_equalize')
    fit_ms = kernel_ms(k_fit, 'nb_fit_mu')
    eq_s, pd = host_s(lambda: scaled_nb.equalize(raw, f, 0.02))
    fit_s, mu = host_s(lambda: scaled_nb.fit_mu_hat(raw, f, 0.05))
    np.testing.assert_array_equal(pd, t_pd.cpu().numpy())
    np.testing.assert_array_equal(mu, t_mu.cpu().numpy())

    m = min(args.cpu_pixels, n)
    t0 = time.perf_counter()
    o_mu = oracle.fit_mu_hat(raw[:m].astype(np.int64), f[:m], 0.05)
    t1 = time.perf_counter()
    o_pd = oracle.equalize(raw[:m].astype(np.int64), f[:m], 0.02)
    t2 = time.perf_counter()
    np.testing.assert_allclose(mu[:m], o_mu, rtol=1e-9)
    np.testing.assert_allclose(pd[:m], o_pd, rtol=1e-9, atol=1e-12)

    line = json.dumps({
        'bins': args.bins, 'dmax': args.dmax, 'pixels': int(n), 'R': int(R),
        'reps': args.reps,
        'equalize_kernel_ms': round(eq_ms, 4),
        'fit_mu_kernel_ms': round(fit_ms, 4),
        'equalize_host_s': round(eq_s, 5),
        'fit_mu_host_s': round(fit_s, 5),
        'upload_mb': round(n * R * 16 / 1e6, 1),
        'download_mb': round(n * R * 8 / 1e6, 1),
        'cpu_pixels': int(m),
        'oracle_fit_mu_s': round(t1 - t0, 4),
        'oracle_equalize_s': round(t2 - t1, 4),
        'matches_oracle': True})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
