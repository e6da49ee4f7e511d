"""Multi-rank product on the GPU: HiC3DeFDR.run_to_qvalues() under torchrun
with 2 ranks on cuda:0 (gloo on device tensors), launched as fresh child
processes. Every chromosome is prepared and tested by the rank LPT assigns
it; estimate_disp runs either the distance re-shard (default: one
all_to_all of the disp pixels, the single-GPU driver per rank, one table
all-reduce; parallel.disp_per_dist_by_distance) or the device driver's
multi-rank branch (H3D_DISP_SHARD=pass: per-pass all-reduce of the NLL sums
through parallel.make_allreduce on torch's stream); BH is the sample sort
over the ranks (parallel.bh_sharded: all_gathers of splitters and bucket
counts, two all_to_alls). The outdir must match the reference goldens like
the single-rank run does (tests/test_gpu_e2e.py). The same product run
under RCCL ('nccl'): one rank (RCCL takes one GPU per rank) with the
sharded paths forced, so the distance re-shard's uneven all_to_all_single,
the table all-reduce and bh_sharded's all_gathers / all_to_alls execute on
RCCL and the stream hand-off between libh3d and the collectives is
exercised.

The ranks start from the pytest process after the other GPU tests have run
in it (the file sorts among them; the parent holds a torch CUDA context and
a libh3d context with the cfg3 scratch). Round 2 kept this file first after
a stall of this launch; the cause was the stream race fixed in the same
commit (22afc53: each rank's libh3d kernels ran on the ctx's own stream
while the collective ran on torch's, so the ranks' Brent state machines
read each other's sums before they were reduced, diverged and deadlocked in
the all-reduce), not the parent's GPU state: round 3 runs this file after
test_alternatives, test_gpu_cfg3 and test_gpu_e2e in the same pytest
process (profiles/r03/gpu_tests_r03c.log), both modes green. The ranks'
output (H3D_DEBUG lines: qcml rounds, live segments, gang aborts) goes to a
log file, not a pipe, and is printed when the launch fails or times out."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import REPO, e2e_inputs, rel_err

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('shard,backend', [('distance', 'gloo'),
                                           ('pass', 'gloo'),
                                           ('distance', 'nccl')])
@pytest.mark.parametrize('name', ['small2'])
def test_two_ranks_run_to_qvalues_matches_reference(name, shard, backend):
    g, kw = e2e_inputs(name)
    assert len(kw['chroms']) == 2   # one chromosome per rank
    ranks = 2 if backend == 'gloo' else 1
    outdir = tempfile.mkdtemp(prefix='h3d_dist_')
    try:
        env = dict(os.environ, H3D_DEVICE='0', MASTER_ADDR='127.0.0.1',
                   OMP_NUM_THREADS='1', H3D_DEBUG='1')
        env.pop('H3D_DISP_SHARD', None)
        env.pop('H3D_FORCE_SHARDED', None)
        if shard == 'pass':
            env['H3D_DISP_SHARD'] = 'pass'
        if backend == 'nccl':
            env['H3D_FORCE_SHARDED'] = '1'
        port = 29600 + os.getpid() % 1000 + (7 if shard == 'pass' else 0) + \
            (13 if backend == 'nccl' else 0)
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
               '--nproc-per-node', str(ranks), '--master-addr', '127.0.0.1',
               '--master-port', str(port),
               os.path.join(REPO, 'tests', 'dist_product_main.py'), name,
               outdir, backend]
        log = os.path.join(outdir, 'ranks.log')
        with open(log, 'w') as fh:
            try:
                rc = subprocess.run(cmd, env=env, stdout=fh,
                                    stderr=subprocess.STDOUT,
                                    timeout=150).returncode
            except subprocess.TimeoutExpired:
                rc = 'timeout'
        text = open(log).read()
        assert rc == 0, text[-4000:]
        # the two ranks share one log: their lines may interleave
        owned = sorted(re.findall(r"rank \d of %d owns \[[^\]]*\]" % ranks,
                                  text))
        assert len(owned) == ranks and "'chrA'" in ' '.join(owned) and \
            "'chrB'" in ' '.join(owned), owned
        assert 'sharded paths True' in text, text[-2000:]
        if backend == 'nccl':
            assert 'backend nccl' in text, text[-2000:]
        # every rank read every chromosome's files right after the pipeline
        # returned: the same bytes as the files on disk now
        import hashlib
        for c in kw['chroms']:
            for st in ('qvalues', 'mu_hat_alt', 'disp'):
                a = np.load(os.path.join(outdir, '%s_%s.npy' % (st, c)))
                sha = hashlib.sha256(a.tobytes()).hexdigest()
                seen = []
                for r in range(ranks):
                    with open(os.path.join(outdir, 'read_rank%d.txt' % r)) \
                            as fh:
                        seen += [ln.split()[1] for ln in fh
                                 if ln.split()[0] == '%s_%s' % (st, c)]
                assert seen == [sha] * ranks, (st, c, seen, sha)
        assert 'rank 0 threshold/classify done' in text, text[-2000:]
        dpd = np.load(os.path.join(outdir, 'disp_per_dist.npy'))
        np.testing.assert_allclose(dpd, g['disp_per_dist'], rtol=1e-6,
                                   atol=1e-12)
        for c in kw['chroms']:
            def ld(st):
                return np.load(os.path.join(outdir, '%s_%s.npy' % (st, c)))
            for st in ('row', 'col', 'raw', 'disp_idx', 'loop_idx'):
                np.testing.assert_array_equal(ld(st), g['%s__%s' % (st, c)])
            for st, tol in (('disp', 1e-6), ('pvalues', 1e-6),
                            ('qvalues', 1e-6), ('mu_hat_null', 1e-8),
                            ('mu_hat_alt', 1e-8)):
                assert rel_err(ld(st), g['%s__%s' % (st, c)]) < tol, st
            for fdr in (0.01, 0.05, 0.1):
                np.testing.assert_array_equal(ld('qvalues') < fdr,
                                              g['qvalues__%s' % c] < fdr)
    finally:
        shutil.rmtree(outdir, ignore_errors=True)


def test_two_ranks_compact_reshard_equals_full_record():
    """The distance re-shard's compact exchange on the GPU, 2 ranks on
    cuda:0 over gloo (tests/dist_keys_main.py): Resident.disp_keys' keys and
    tables, PixelKeys.device_tables across the ranks and h3d_pixel_f_dev
    deliver raw, f and dist as the full record does, in dtype, shape and
    every bit -- per-pixel and per-replicate size factors, R = 4 and 9, a
    chromosome without disp pixels, the exchange in 1 and 3 parts."""
    env = dict(os.environ, H3D_DEVICE='0', MASTER_ADDR='127.0.0.1',
               OMP_NUM_THREADS='1')
    port = 29680 + os.getpid() % 1000
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
           '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port),
           os.path.join(REPO, 'tests', 'dist_keys_main.py')]
    with tempfile.TemporaryDirectory() as tmp:
        log = os.path.join(tmp, 'ranks.log')
        with open(log, 'w') as fh:
            try:
                rc = subprocess.run(cmd, env=env, stdout=fh,
                                    stderr=subprocess.STDOUT,
                                    timeout=150).returncode
            except subprocess.TimeoutExpired:
                rc = 'timeout'
        text = open(log).read()
    assert rc == 0, text[-4000:]
    for rank in range(2):
        assert re.search(r'rank %d of 2: \d+ variants, \d+ pixels received, '
                         r'bit-identical=True' % rank, text), text[-4000:]


def test_bh_sharded_gpu():
    """parallel.bh_sharded on the GPU (DeviceBhOps) with 3 ranks on cuda:0
    over gloo, 3 M p-values with ties, NaN and a heavy tie at 1: every q
    equals h3d_bh_dev's on the whole vector bit for bit."""
    env = dict(os.environ, H3D_DEVICE='0', MASTER_ADDR='127.0.0.1',
               OMP_NUM_THREADS='1')
    port = 29650 + os.getpid() % 1000
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
           '--nproc-per-node', '3', '--master-addr', '127.0.0.1',
           '--master-port', str(port),
           os.path.join(REPO, 'tests', 'dist_bh_main.py'), '3000000']
    with tempfile.TemporaryDirectory() as tmp:
        log = os.path.join(tmp, 'ranks.log')
        with open(log, 'w') as fh:
            try:
                rc = subprocess.run(cmd, env=env, stdout=fh,
                                    stderr=subprocess.STDOUT,
                                    timeout=150).returncode
            except subprocess.TimeoutExpired:
                rc = 'timeout'
        text = open(log).read()
    assert rc == 0, text[-4000:]
    assert 'bit-identical=True' in text, text[-4000:]
