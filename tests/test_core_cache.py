"""The outdir write-behind cache of save_data / load_data (CPU only): a
stage reading its own output back gets the saved values, fresh arrays every
time, queued writes land in order (flush(), interpreter exit), and once a
write has landed any change of the file on disk wins over the cache."""
import os
import tempfile
import time

import numpy as np
import pandas as pd

from hic3defdr_amd import HiC3DeFDR


def _h():
    out = tempfile.mkdtemp(prefix='h3d_cache_')
    design = pd.DataFrame([[True, False], [True, False], [False, True]],
                          index=['a1', 'a2', 'b1'], columns=['A', 'B'])
    return HiC3DeFDR(['x_<chrom>.npz'] * 3, ['x_<chrom>.bias'] * 3,
                     ['chr1', 'chr2'], design, out)


def test_roundtrip_and_fresh_arrays():
    h = _h()
    a = np.arange(12.0).reshape(6, 2)
    h.save_data(a, 'scaled', 'chr1')
    a[0, 0] = -1.0                       # the cache holds its own copy
    b = h.load_data('scaled', 'chr1')
    assert b[0, 0] == 0.0
    b[1, 1] = 99.0                       # callers may mutate what they get
    np.testing.assert_array_equal(h.load_data('scaled', 'chr1'),
                                  np.arange(12.0).reshape(6, 2))
    idx = np.array([True, False, True, False, False, True])
    np.testing.assert_array_equal(h.load_data('scaled', 'chr1', idx=idx),
                                  np.arange(12.0).reshape(6, 2)[idx])
    np.testing.assert_array_equal(h.load_data('scaled', 'chr1', cond='B'),
                                  np.arange(12.0).reshape(6, 2)[:, 1])


def test_file_changed_on_disk_wins():
    h = _h()
    h.save_data(np.zeros(5), 'disp_idx', 'chr1')
    fname = os.path.join(h.outdir, 'disp_idx_chr1.npy')
    h.flush()                            # the queued write has landed
    assert h.is_current(fname)
    time.sleep(0.01)
    np.save(fname, np.ones(7))           # replaced behind the object's back
    assert not h.is_current(fname)
    np.testing.assert_array_equal(h.load_data('disp_idx', 'chr1'), np.ones(7))
    h.save_data(np.zeros(5), 'disp_idx', 'chr1')   # cached again
    h.flush()
    os.remove(fname)
    np.save(fname, np.full(5, 2.0))      # new inode, same size
    np.testing.assert_array_equal(h.load_data('disp_idx', 'chr1'),
                                  np.full(5, 2.0))


def test_same_size_rewrite_in_place_with_mtime_restored():
    h = _h()
    h.save_data(np.zeros(5), 'disp_idx', 'chr1')
    fname = os.path.join(h.outdir, 'disp_idx_chr1.npy')
    h.flush()
    st = os.stat(fname)
    time.sleep(0.02)                     # past the clock tick of the ctime
    with open(fname, 'r+b') as fh:       # same inode, same size
        np.save(fh, np.full(5, 3.0))
    os.utime(fname, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert os.stat(fname).st_mtime_ns == st.st_mtime_ns
    assert os.stat(fname).st_ino == st.st_ino
    np.testing.assert_array_equal(h.load_data('disp_idx', 'chr1'),
                                  np.full(5, 3.0))


def test_cache_is_bounded_lru(monkeypatch):
    from hic3defdr_amd.analysis.outdir import OutdirStore
    monkeypatch.setattr(OutdirStore, 'CACHE_BYTES', 3 * 800)
    h = _h()
    for i in range(10):                  # 10 chromosomes' worth of stages
        h.save_data(np.full(100, float(i)), 'pvalues', 'chr%d' % i)
        h.flush()
        assert h.cache_nbytes() <= 3 * 800
    assert h.cache_nbytes() == 3 * 800
    for i in range(10):                  # evicted ones come from disk
        np.testing.assert_array_equal(h.load_data('pvalues', 'chr%d' % i),
                                      np.full(100, float(i)))
    monkeypatch.setattr(OutdirStore, 'CACHE_BYTES', 0)
    h2 = _h()
    h2.save_data(np.zeros(10), 'pvalues', 'chr1')
    h2.flush()
    assert h2.cache_nbytes() == 0


def test_all_chroms_with_offsets_and_idx():
    h = _h()
    x = np.arange(10.0)
    off = np.array([0, 4, 10])
    h.save_data(x, 'pvalues', off)
    got, offsets = h.load_data('pvalues', 'all')
    np.testing.assert_array_equal(got, x)
    np.testing.assert_array_equal(offsets, off)
    idx = x % 3 == 0
    got, offsets = h.load_data('pvalues', 'all', idx=idx)
    np.testing.assert_array_equal(got, x[idx])


def test_write_behind_queue(monkeypatch):
    """A queued array is served before its write lands, a reader of the file
    waits for it, writes of one file land in order, and the queued array
    cannot be changed under the writer."""
    import threading
    from hic3defdr_amd.analysis import outdir
    gate = threading.Event()
    real = outdir._write_npy

    def slow(fname, data, ready=None):
        gate.wait(10)
        return real(fname, data, ready)
    monkeypatch.setattr(outdir, '_write_npy', slow)
    h = _h()
    fname = os.path.join(h.outdir, 'pvalues_chr1.npy')
    h.save_data(np.zeros(4), 'pvalues', 'chr1')
    h.save_data(np.ones(4), 'pvalues', 'chr1')     # the later write wins
    assert not os.path.exists(fname)
    assert h.is_current(fname)
    np.testing.assert_array_equal(h.load_data('pvalues', 'chr1'), np.ones(4))
    gate.set()
    np.testing.assert_array_equal(h.load_npy_file(fname), np.ones(4))
    h.flush()
    np.testing.assert_array_equal(np.load(fname), np.ones(4))
    mine = np.arange(3.0)
    h._save_npy(os.path.join(h.outdir, 'llr_chr1.npy'), mine, owned=True)
    assert not mine.flags.writeable
    h.flush()


def test_pending_writes_are_bounded_without_flush(monkeypatch):
    """Saving many chromosomes' stages without flush(): landed writes move
    into the size-limited cache on the next save, and the queued bytes stay
    under PENDING_BYTES even while the writer is slow (the save waits)."""
    import threading
    from hic3defdr_amd.analysis import outdir
    from hic3defdr_amd.analysis.outdir import OutdirStore
    monkeypatch.setattr(OutdirStore, 'CACHE_BYTES', 4 * 800)
    monkeypatch.setattr(OutdirStore, 'PENDING_BYTES', 3 * 800)
    real = outdir._write_npy
    started = threading.Semaphore(0)

    def slow(fname, data, ready=None):
        started.release()
        time.sleep(0.002)
        return real(fname, data, ready)
    monkeypatch.setattr(outdir, '_write_npy', slow)
    h = _h()
    peak = 0
    for i in range(40):
        for stage in ('pvalues', 'llr', 'mu_hat_null'):
            h.save_data(np.full(100, float(i)), stage, 'chr%d' % i)
            peak = max(peak, h.pending_nbytes())
            assert h.cache_nbytes() <= 4 * 800
    assert peak <= 3 * 800
    h.flush()
    assert h.pending_nbytes() == 0
    for i in (0, 17, 39):
        np.testing.assert_array_equal(h.load_data('llr', 'chr%d' % i),
                                      np.full(100, float(i)))


def test_landed_writes_leave_the_queue_on_the_next_save():
    h = _h()
    h.save_data(np.zeros(1000), 'pvalues', 'chr1')
    deadline = time.time() + 10
    pending = h._store.pending
    while pending[os.path.join(h.outdir, 'pvalues_chr1.npy')].future.done() \
            is False and time.time() < deadline:
        time.sleep(0.001)
    h.save_data(np.zeros(10), 'llr', 'chr1')
    assert os.path.join(h.outdir, 'pvalues_chr1.npy') not in pending
    assert h.cache_nbytes() >= 8000
    h.flush()


def test_ready_callable_runs_before_write_and_read():
    """An array still being filled by an async device -> host copy
    (analysis/d2h.py) is queued with its ``ready`` callable: the writer and
    any reader of the queued array call it before touching the values."""
    h = _h()
    buf = np.zeros(6)
    calls = []

    def ready():
        if not calls:
            buf[:] = np.arange(6.0)      # the copy "lands"
        calls.append(1)
    h._save_npy(os.path.join(h.outdir, 'pvalues_chr1.npy'), buf[:4],
                owned=True, ready=ready)
    h._save_npy(os.path.join(h.outdir, 'pvalues_chr2.npy'), buf[4:],
                owned=True, ready=ready)
    np.testing.assert_array_equal(h.load_data('pvalues', 'chr2'),
                                  [4.0, 5.0])
    h.flush()
    np.testing.assert_array_equal(
        np.load(os.path.join(h.outdir, 'pvalues_chr1.npy')), np.arange(4.0))
    assert calls


def test_evicted_large_arrays_are_released_off_the_main_thread(monkeypatch):
    """The cache's evictions hand large arrays to the background reaper
    (outdir._Reaper): each is released once the reaper has run, and the
    files and later reads are unaffected."""
    import gc
    import weakref
    from hic3defdr_amd.analysis import outdir
    monkeypatch.setattr(outdir.OutdirStore, 'CACHE_BYTES', 40 << 20)
    monkeypatch.setattr(outdir._Reaper, '_MIN_BYTES', 1 << 20)
    h = _h()
    refs = []
    for k in range(4):
        a = np.full(2_000_000, float(k))          # 16 MB each
        refs.append(weakref.ref(a))
        h._save_npy(h._npy('scaled', 'chr%d' % k), a, owned=True)
        del a
        h.flush()
        h._store.settle_landed()
    # two of the four fit the 40 MB cache: the older ones were evicted
    deadline = time.time() + 10
    while time.time() < deadline and (refs[0]() is not None or
                                      refs[1]() is not None):
        gc.collect()
        time.sleep(0.01)
    assert refs[0]() is None and refs[1]() is None
    for k in range(4):
        np.testing.assert_array_equal(
            np.load(h._npy('scaled', 'chr%d' % k)), np.full(2_000_000, float(k)))
