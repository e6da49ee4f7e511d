"""bench.py's command line on one GPU, at a small cfg2 shape: a plain run
prints the headline line alone (nothing of --full's legs), --steps sets the
timed steps, ms_per_step and value describe the same time, and
--dump-outputs writes the last timed step's arrays as float64 .npy files
whose per-pixel rows follow sample_idx and which hold no NaN (disp_per_dist
is written at the distances the inputs hold pixels at)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS, DMAX = 2000, 100
FULL_ONLY = ('roofline', 'kernel_rooflines', 'kernels_ms_per_step',
             'measured_peaks', 'cpu_baseline', 'parity_sample',
             'parity_vs_reference', 'result_sha16', 'e2e_run_to_qvalues',
             'e2e_cfg3_run_to_qvalues', 'other_configs')


def test_plain_run_and_dump(tmp_path):
    out = str(tmp_path / 'dump')
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1',
         '--steps', '2', '--warmup', '1', '--bins', str(BINS), '--dmax',
         str(DMAX), '--dump-outputs', out],
        cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
        timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert (d['steps'], d['warmup'], d['n_gpus']) == (2, 1, 1)
    assert d['unit'] == 'pixels/s' and d['higher_is_better'] is True
    assert d['dtype'] == 'f64' and d['metric'].startswith('pixels/sec')
    n = d['config']['disp_pixels_total']
    assert n > 0 and d['ms_per_step'] > 0
    assert abs(d['value'] - n / (d['ms_per_step'] * 1e-3)) <= 1e-9 * d['value']
    assert not [k for k in FULL_ONLY if k in d]

    got = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert sorted(got) == ['disp', 'disp_per_dist', 'disp_per_dist_distances',
                           'llr', 'mu0', 'mu1', 'p', 'sample_idx']
    assert all(a.dtype == np.float64 for a in got.values())
    assert all(np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    # the band of this generator holds every distance but the first few
    ds = got['disp_per_dist_distances']
    assert np.array_equal(ds, np.arange(ds[0], DMAX + 1)) and ds[0] <= 8
    assert got['disp_per_dist'].shape == (len(ds), 2)
    assert np.all(got['disp_per_dist'] > 0)
    idx = got['sample_idx']
    assert np.array_equal(idx, np.arange(n))      # below the sample size
    for k in ('p', 'llr', 'mu0'):
        assert got[k].shape == (n,)
    for k in ('mu1', 'disp'):
        assert got[k].shape == (n, 2)
    assert np.all((got['p'] >= 0) & (got['p'] <= 1))
    assert np.all(np.isfinite(got['mu0']) & (got['mu0'] > 0))
    assert np.all(np.isfinite(got['disp']) & (got['disp'] > 0))
