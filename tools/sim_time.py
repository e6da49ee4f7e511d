"""Times simulate on the GPU (kernel k_nb_sample of csrc/h3d_sim.hip) against
the host simulate on the pixels of one cfg2-sized chromosome.

    python tools/sim_time.py [--bins 20000 --dmax 250 --reps 20 --out FILE]

Input: the pixels of ``synthetic.draw_band(bins, (4, 4), dmax, keys=True)``
put in (row, col) order; the first condition's four replicates give the mean
and the biases, tiled to J = 8 simulated replicates as
``SimulatingHiC3DeFDR.simulate`` does; 1000 small clusters; the dispersion
0.05 (1 + d / dmax).

Figures, one JSON line:

- ``kernel_ms``: k_nb_sample alone (the library's profile scope
  ``nb_sample`` around the launch of h3d_simulate_dev on resident tensors),
  median of ``--reps`` after 3 warm-up calls;
- ``simulate_gpu_s``: the whole ``simulate_gpu`` call with its generator
  drained (checks, classes, perturbation, upload, kernel, download, the CSR
  replicates), host clock, median of 5 after a warm-up call;
- ``simulate_host_s``: the host ``simulate`` on the same arguments with its
  generator drained, this machine's CPU, one run;
- ``path_share``: the share of draws decided by each Poisson path of
  csrc/h3d_sample.h (``sum``, ``sum_verify``, ``walk``, ``walk_verify``,
  ``bisect``), counted on the host (libh3d_hosttest.so) over the kernel's own
  uniforms for every 16th pixel of all replicates -- no counters in the
  kernel.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = ('sum', 'sum_verify', 'walk', 'walk_verify', 'bisect')


def host_paths(lib, bm, disp, seed, stream, rep, pixels):
    """Path and count of the draws (seed, stream, rep, pixels) on the host."""
    vp = ctypes.c_void_p
    n = len(pixels)
    ctr = np.zeros((n, 4), dtype=np.uint32)
    ctr[:, 0] = pixels & 0xFFFFFFFF
    ctr[:, 1] = pixels >> 32
    ctr[:, 2] = rep
    ctr[:, 3] = stream
    key = np.empty((n, 2), dtype=np.uint32)
    key[:, 0], key[:, 1] = seed & 0xFFFFFFFF, seed >> 32
    words = np.empty((n, 4), dtype=np.uint32)
    u = np.empty((n, 2))
    lib.h3dt_philox(ctypes.c_int64(n), ctr.ctypes.data_as(vp),
                    key.ctypes.data_as(vp), words.ctypes.data_as(vp),
                    u.ctypes.data_as(vp))
    u1, u2 = np.ascontiguousarray(u[:, 0]), np.ascontiguousarray(u[:, 1])
    bm, disp = np.ascontiguousarray(bm), np.ascontiguousarray(disp)
    lam = np.empty(n)
    k = np.empty(n, dtype=np.int32)
    path = np.empty(n, dtype=np.int32)
    lib.h3dt_nb_draw(ctypes.c_int64(n), bm.ctypes.data_as(vp),
                     disp.ctypes.data_as(vp), u1.ctypes.data_as(vp),
                     u2.ctypes.data_as(vp), lam.ctypes.data_as(vp),
                     k.ctypes.data_as(vp), path.ctypes.data_as(vp))
    return path, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bins', type=int, default=20000)
    ap.add_argument('--dmax', type=int, default=250)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--no-host', action='store_true',
                    help='skip the host simulate')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    from hic3defdr_amd import _native, synthetic
    from hic3defdr_amd import build as h3dbuild
    from hic3defdr_amd.util import simulation

    raw, f, dist, row, bias = synthetic.draw_band(args.bins, (4, 4),
                                                  args.dmax, seed=0, keys=True)
    col = row + dist
    order = np.lexsort((col, row))
    row, col = row[order].astype(np.int64), col[order].astype(np.int64)
    mean = np.mean(raw[order, :4] / f[order, :4], axis=1)
    bias = np.tile(bias[:, :4], 2)
    sf = np.tile(0.8 + 0.1 * np.arange(4), 2)
    n, J = len(row), bias.shape[1]
    dmax = args.dmax

    def disp_fn(d):
        return 0.05 * (1 + np.asarray(d, dtype=np.float64) / dmax)

    rng = np.random.default_rng(0)
    picks = rng.choice(n, 1000, replace=False)
    clusters = [[(int(row[i]), int(col[i]))] for i in picks]
    kw = dict(beta=0.5, p_diff=0.4, trend='dist', verbose=False)

    ctx = _native.context(0)

    def gpu_call():
        classes, mats = simulation.simulate_gpu(
            row, col, mean, disp_fn, bias, sf, clusters, seed=args.seed,
            stream=0, ctx=ctx, **kw)
        return classes, list(mats)

    gpu_call()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        classes, mats = gpu_call()
        ts.append(time.perf_counter() - t0)
    out = {'bins': args.bins, 'dmax': args.dmax, 'pixels': int(n), 'J': J,
           'reps': args.reps, 'simulate_gpu_s': round(float(np.median(ts)), 4),
           'mean_count': round(float(np.mean([m.data.mean() for m in mats])),
                               3)}

    # the kernel alone, on resident tensors (unperturbed means: the same work)
    dev = torch.device('cuda', ctx.device)
    pos = mean > 0
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (
        row[pos].astype(np.int32), col[pos].astype(np.int32), mean[pos],
        mean[pos], bias, sf, disp_fn(np.arange(int((col - row).max()) + 1)))]
    for _ in range(3):
        ctx.simulate_dev(*t, seed=args.seed)
    ctx.profile(True, level=2)
    ms = []
    for _ in range(args.reps):
        ctx.profile_reset()
        ctx.simulate_dev(*t, seed=args.seed)
        ms.append(ctx.profile_read('nb_sample')[0])
    ctx.profile(False)
    out['kernel_ms'] = round(float(np.median(ms)), 3)
    out['draws_per_us'] = round(int(pos.sum()) * J / (out['kernel_ms'] * 1e3),
                                1)

    if not args.no_host:
        np.random.seed(args.seed)
        t0 = time.perf_counter()
        _, host_mats = simulation.simulate(row, col, mean, disp_fn, bias, sf,
                                           clusters, **kw)
        host_mats = list(host_mats)
        out['simulate_host_s'] = round(time.perf_counter() - t0, 3)
        out['host_mean_count'] = round(
            float(np.mean([m.data.mean() for m in host_mats])), 3)

    # Poisson path shares, on the host over the kernel's own uniforms
    lib = ctypes.CDLL(h3dbuild.build_hosttest())
    r_, c_, m_ = row[pos], col[pos], mean[pos]
    px = np.arange(0, len(r_), 16, dtype=np.uint64)
    table = disp_fn(np.arange(int((c_ - r_).max()) + 1))
    counts = np.zeros(len(PATHS), dtype=np.int64)
    for j in range(J):
        bm = m_[px] * (bias[r_[px], j] * bias[c_[px], j] * sf[j])
        path, _ = host_paths(lib, bm, table[(c_ - r_)[px]], args.seed, 0, j,
                             px)
        counts += np.bincount(path, minlength=len(PATHS))[:len(PATHS)]
    out['path_share'] = {k: round(float(v) / counts.sum(), 5)
                         for k, v in zip(PATHS, counts)}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
