"""simulate(gpu=True) through the class on the small2 dataset, set up as
tests/test_gpu_simulation.py does: the same files as the host path with the
same structure, data that is the documented function of (seed, chromosome,
replicate, pixel) alone, numpy's global stream untouched -- and a simulated
set the pipeline and evaluate(gpu=True) run through."""
import filecmp
import os
import shutil
import tempfile

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sparse

from conftest import e2e_inputs, golden

pytestmark = pytest.mark.gpu
SIMREPS = ['A1', 'A2', 'B1', 'B2']
SEED = 7


@pytest.fixture(scope='module')
def sims():
    """The analysis of small2, then simulate('ES') on the host (numpy
    seeded), on the GPU, on the GPU one chromosome at a time (last
    chromosome first) and on the GPU with another seed."""
    from hic3defdr_amd import HiC3DeFDR
    g = golden('sim_small2.npz')
    _, kw = e2e_inputs('small2')
    tmp = tempfile.mkdtemp(prefix='h3d_gpusim_')
    try:
        design = pd.DataFrame(kw['design'], index=kw['reps'],
                              columns=kw['conds'])
        h = HiC3DeFDR(raw_npz_patterns=kw['raw_npz_patterns'],
                      bias_patterns=kw['bias_patterns'], chroms=kw['chroms'],
                      design=design, outdir=os.path.join(tmp, 'out'),
                      dist_thresh_max=kw['dist_thresh_max'],
                      loop_patterns=kw['loop_patterns'])
        h.run_to_qvalues(verbose=False)
        d = {k: os.path.join(tmp, k) for k in ('host', 'gpu', 'single',
                                               'other')}
        np.random.seed(int(g['meta_seed']))
        h.simulate('ES', outdir=d['host'], verbose=False)
        np.random.seed(12345)
        state = np.random.get_state()
        h.simulate('ES', outdir=d['gpu'], verbose=False, gpu=True, seed=SEED)
        for c in reversed(kw['chroms']):
            h.simulate('ES', chrom=c, outdir=d['single'], verbose=False,
                       gpu=True, seed=SEED)
        h.simulate('ES', outdir=d['other'], verbose=False, gpu=True,
                   seed=SEED + 1)
        now = np.random.get_state()
        untouched = now[0] == state[0] and \
            np.array_equal(now[1], state[1]) and now[2:] == state[2:]
        yield dict(h=h, kw=kw, tmp=tmp, untouched=untouched, **d)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def load(d, rep, chrom):
    return sparse.load_npz(os.path.join(d, '%s_%s_raw.npz' % (rep, chrom)))


def test_same_files_and_structure_as_the_host_path(sims):
    assert sorted(os.listdir(sims['gpu'])) == sorted(os.listdir(sims['host']))
    assert filecmp.cmp(os.path.join(sims['gpu'], 'design.csv'),
                       os.path.join(sims['host'], 'design.csv'),
                       shallow=False)
    for c in sims['kw']['chroms']:
        lab_h = np.loadtxt(os.path.join(sims['host'], 'labels_%s.txt' % c),
                           dtype='U7')
        lab_g = np.loadtxt(os.path.join(sims['gpu'], 'labels_%s.txt' % c),
                           dtype='U7')
        assert lab_g.shape == lab_h.shape
        assert set(np.atleast_1d(lab_g)) <= {'constit', 'A', 'B'}
        for rep in SIMREPS:
            a, b = load(sims['host'], rep, c), load(sims['gpu'], rep, c)
            assert a.format == b.format == 'csr' and a.shape == b.shape
            for k in ('indptr', 'indices', 'data'):
                assert getattr(a, k).dtype == getattr(b, k).dtype, k
            np.testing.assert_array_equal(a.indptr, b.indptr)
            np.testing.assert_array_equal(a.indices, b.indices)
            assert b.data.min() >= 0 and b.data.max() > 0


def test_numpy_global_stream_is_untouched(sims):
    assert sims['untouched']


def test_data_is_simulate_gpu_of_the_outdir_arrays(sims):
    from hic3defdr_amd.util.clusters import load_clusters
    from hic3defdr_amd.util.simulation import simulate_gpu
    h, kw = sims['h'], sims['kw']
    reps = np.asarray(h.design['ES'], dtype=bool)
    for s, c in enumerate(kw['chroms']):
        bias = h.load_bias(c)[:, reps]
        sf = h.load_data('size_factors', c)
        sf = sf[:, reps] if sf.ndim == 2 else sf[reps]
        row, col = h.load_data('row', c), h.load_data('col', c)
        if sf.ndim == 2:
            dist = col - row
            sf = sf[[np.argmax(dist == d) for d in range(dist.max() + 1)], :]
        mean = np.mean(h.load_data('scaled', c)[:, reps], axis=1)
        clusters = load_clusters(
            kw['loop_patterns']['ES'].replace('<chrom>', c))
        classes, mats = simulate_gpu(
            row, col, mean, h.load_disp_fn('ES'), np.tile(bias, 2),
            np.tile(sf, 2), clusters, beta=0.5, p_diff=0.4, seed=SEED,
            stream=s, verbose=False)
        np.testing.assert_array_equal(
            np.atleast_1d(np.loadtxt(
                os.path.join(sims['gpu'], 'labels_%s.txt' % c), dtype='U7')),
            classes)
        mats = list(mats)
        assert len(mats) == len(SIMREPS)
        for rep, m in zip(SIMREPS, mats):
            f = load(sims['gpu'], rep, c)
            np.testing.assert_array_equal(f.data, m.data)
            np.testing.assert_array_equal(f.indices, m.indices)
            np.testing.assert_array_equal(f.indptr, m.indptr)


def test_a_chromosome_alone_gets_the_whole_calls_files(sims):
    names = sorted(os.listdir(sims['gpu']))
    assert sorted(os.listdir(sims['single'])) == names
    for n in names:
        if n.endswith('.npz'):
            a = sparse.load_npz(os.path.join(sims['gpu'], n))
            b = sparse.load_npz(os.path.join(sims['single'], n))
            np.testing.assert_array_equal(a.data, b.data)
            np.testing.assert_array_equal(a.indices, b.indices)
            np.testing.assert_array_equal(a.indptr, b.indptr)
        else:
            assert filecmp.cmp(os.path.join(sims['gpu'], n),
                               os.path.join(sims['single'], n), shallow=False)


def test_another_seed_changes_every_replicate(sims):
    for c in sims['kw']['chroms']:
        for rep in SIMREPS:
            a, b = load(sims['gpu'], rep, c), load(sims['other'], rep, c)
            np.testing.assert_array_equal(a.indices, b.indices)
            assert np.mean(a.data != b.data) > 0.05, (rep, c)
    # replicates of one call differ from each other too
    c = sims['kw']['chroms'][0]
    assert np.mean(load(sims['gpu'], 'A1', c).data !=
                   load(sims['gpu'], 'A2', c).data) > 0.05


def test_gpu_without_a_seed_is_refused_before_a_device_is_touched(
        sims, monkeypatch):
    from hic3defdr_amd import _native
    h = sims['h']

    def touched(*a, **k):
        raise AssertionError('a device was touched')
    monkeypatch.setattr(_native, 'context', touched)
    monkeypatch.setattr(type(h), '_ctx', touched)
    monkeypatch.setattr(type(h), 'load_data', touched)
    out = os.path.join(sims['tmp'], 'never')
    for seed in (None, 1.5, -3, 2 ** 63):
        with pytest.raises(ValueError, match='seed'):
            h.simulate('ES', outdir=out, verbose=False, gpu=True, seed=seed)
    assert not os.path.exists(out)


def test_simulated_set_runs_through_the_pipeline_and_evaluate(sims):
    """A smoke check, not a bar: balance, analyse, evaluate(gpu=True)."""
    from hic3defdr_amd import HiC3DeFDR
    from hic3defdr_amd.util.balancing import kr_balance
    from hic3defdr_amd.util.filtering import filter_sparse_rows_count
    kw, sim = sims['kw'], os.path.join(sims['tmp'], 'balanced')
    shutil.copytree(sims['gpu'], sim)   # the bias files go beside a copy
    for c in kw['chroms']:
        for rep in SIMREPS:
            fn = os.path.join(sim, '%s_%s_raw.npz' % (rep, c))
            m = sparse.load_npz(fn).tocsr()
            _, bias, _ = kr_balance(filter_sparse_rows_count(m), fl=0)
            np.savetxt(fn.replace('_raw.npz', '_kr.bias'), bias)
    out = os.path.join(sims['tmp'], 'simout')
    hs = HiC3DeFDR(
        raw_npz_patterns=[os.path.join(sim, '%s_<chrom>_raw.npz' % r)
                          for r in SIMREPS],
        bias_patterns=[os.path.join(sim, '%s_<chrom>_kr.bias' % r)
                       for r in SIMREPS],
        chroms=kw['chroms'], design=os.path.join(sim, 'design.csv'),
        outdir=out, dist_thresh_max=kw['dist_thresh_max'],
        loop_patterns={'ES': kw['loop_patterns']['ES']})
    hs.run_to_qvalues(verbose=False)
    hs.evaluate('ES', os.path.join(sim, 'labels_<chrom>.txt'), gpu=True)
    e = np.load(os.path.join(out, 'eval.npz'))
    assert e['fpr'][-1] == 1 and e['tpr'][-1] == 1
    assert np.all(np.diff(e['fpr']) >= 0) and np.all(np.diff(e['tpr']) >= 0)
