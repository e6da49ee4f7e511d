"""The outdir's files below the stage semantics of core.py: the write-behind
threads, the bounded cache of what an object saved, and the tokens that say
whether a file is still the version somebody mirrored (resident.py)."""
import atexit
import collections
import concurrent.futures
import ctypes
import os
import sys
import threading
import zlib

import numpy as np


def file_stamp(fname):
    """What identifies a version of ``fname`` on disk (a rewrite that
    restores the mtime still moves the ctime), or None when it cannot be
    stat'ed."""
    try:
        st = os.stat(fname)
    except OSError:
        return None
    return (st.st_ino, st.st_size, st.st_mtime_ns, st.st_ctime_ns)


def disk_token(fname):
    """The token of a file no OutdirStore writes (the bias files)."""
    return ('disk', file_stamp(fname))


def _write_npy(fname, data, ready=None):
    if ready is not None:
        ready()      # an async device -> host copy still landing in `data`
    np.save(fname, data)
    return file_stamp(fname)


def _write_bytes(fname, blob):
    with open(fname, 'wb') as fh:
        fh.write(blob)


class _NpyWriter(object):
    """The outdir's write-behind threads: queued .npy writes land on
    background threads (the product's stages hand their results over and go
    on; reference core.py:198-218 writes them inline). A file's writes go to
    one lane (a single thread chosen by the file name), so they land in
    order; different files land in parallel on H3D_NPY_WRITERS lanes
    (default 4: prepare_data's ~0.5 GB of cfg2 arrays is page-cache copying
    that scales with threads). Worker threads of concurrent.futures are
    joined at interpreter exit, so every queued write lands; an error of one
    is reported on stderr there if nobody read it."""

    def __init__(self):
        self._lock = threading.Lock()
        self._ex = None
        self._futs = []

    def submit(self, fname, data, ready=None, fn=None):
        """Queues np.save of ``data`` (or ``fn(fname, data)``) on the lane
        of ``fname``."""
        with self._lock:
            if self._ex is None:
                n = max(1, int(os.environ.get('H3D_NPY_WRITERS', '4')))
                self._ex = [concurrent.futures.ThreadPoolExecutor(
                    1, thread_name_prefix='h3d-npy%d' % i) for i in range(n)]
                atexit.register(self._report)
            self._futs = [f for f in self._futs if not f.done()]
            lane = zlib.crc32(os.fsencode(os.path.abspath(fname))) % \
                len(self._ex)
            fut = self._ex[lane].submit(_write_npy, fname, data, ready) \
                if fn is None else self._ex[lane].submit(fn, fname, data)
            self._futs.append(fut)
            return fut

    def _report(self):
        for f in list(self._futs):
            try:
                f.result()
            except Exception as e:   # noqa: BLE001 -- exit-time report
                sys.stderr.write('hic3defdr_amd: outdir write failed: %r\n'
                                 % (e,))


_WRITER = _NpyWriter()


class _Reaper(object):
    """Drops the outdir's large host arrays on a background thread. Freeing
    a large numpy buffer unmaps its pages: ~36 ms per GB on the GPU box's
    host (7 ms for a 200 MB array, measured r05), paid by whichever thread
    drops the last reference -- the cache's evictions put ~0.35 s of it on
    the main thread of a whole-genome prepare_data. Handed here, the frees
    run while the main thread waits in libh3d / HIP calls (which release the
    GIL). The arrays are immutable once queued (OutdirStore.save), so
    dropping them elsewhere changes nothing but where the unmapping runs."""

    _MIN_BYTES = 8 << 20

    def __init__(self):
        self._lock = threading.Lock()
        self._q = None

    @staticmethod
    def _release_pages(a):
        """Returns the pages of numpy array ``a`` to the kernel with
        madvise(MADV_DONTNEED) through ctypes -- which drops the GIL -- when
        this thread holds the only reference to it and it owns its buffer:
        the free() that follows then unmaps mostly released pages. numpy
        frees a buffer while holding the GIL, so a large free on this thread
        used to stall every Python thread (~36 ms per GB on the GPU box; the
        main thread's GIL waits showed up in every call of prepare_data).
        H3D_REAP_MADVISE=0 turns it off."""
        if not _MADVISE or not isinstance(a, np.ndarray) or \
                not a.flags.owndata or a.nbytes < _Reaper._MIN_BYTES:
            return
        # nobody else holds it: the references are _run's local, this
        # frame's ``a`` and getrefcount's argument (a view's base or any
        # other holder makes it more, and the pages stay)
        if sys.getrefcount(a) > 3:
            return
        libc = _libc()
        if libc is None:
            return
        page = 4096
        addr = a.ctypes.data
        lo = (addr + page - 1) // page * page
        hi = (addr + a.nbytes) // page * page
        if hi > lo:
            libc.madvise(ctypes.c_void_p(lo), ctypes.c_size_t(hi - lo), 4)

    def _run(self):
        q = self._q
        while True:
            obj = q.get()
            arrs = list(obj) if isinstance(obj, tuple) else [obj]
            obj = None
            while arrs:
                a = arrs.pop()
                self._release_pages(a)
                a = None

    def drop(self, obj, nbytes):
        if nbytes < self._MIN_BYTES:
            return
        with self._lock:
            if self._q is None:
                import queue
                self._q = queue.SimpleQueue()
                threading.Thread(target=self._run, name='h3d-reap',
                                 daemon=True).start()
        self._q.put(obj)


_MADVISE = os.environ.get('H3D_REAP_MADVISE', '1') != '0' and \
    sys.platform.startswith('linux')
_LIBC = []


def _libc():
    if not _LIBC:
        try:
            lib = ctypes.CDLL(None, use_errno=True)
            lib.madvise.argtypes = [ctypes.c_void_p, ctypes.c_size_t,
                                    ctypes.c_int]
            lib.madvise.restype = ctypes.c_int
            _LIBC.append(lib)
        except (OSError, AttributeError):
            _LIBC.append(None)
    return _LIBC[0]


_REAPER = _Reaper()


class _Queued(object):
    """A write on its way to the outdir: its ``future``, the ``array`` being
    written (None for a bytes write) and the array's ``ready`` callable."""
    __slots__ = ('future', 'array', 'ready')

    def __init__(self, future, array=None, ready=None):
        self.future, self.array, self.ready = future, array, ready

    @property
    def nbytes(self):
        return 0 if self.array is None else self.array.nbytes


class OutdirStore(object):
    """One analysis object's view of its outdir files: a write-through cache
    of the arrays it saved, behind a write-behind queue.

    A later stage reading its own output back skips the disk read -- but
    only while the file on disk is still the one written (file_stamp), so
    edits or replacements of the outdir files are always seen. The cache is
    an LRU over the arrays' bytes, at most CACHE_BYTES (H3D_NPY_CACHE_BYTES,
    default 1 GiB; 0 turns it off), so a whole-genome run does not keep a
    second copy of every stage of every chromosome on the host.

    Writes are behind (_WRITER: H3D_NPY_WRITERS lanes, the writes of one
    file name in order on one lane): save() returns once the array is
    queued. The invariant every method here keeps: until its write has
    landed the queued array IS the file's content for every reader in this
    process (cached() serves it, wait() is for readers of the file itself);
    once it has landed the file's stamp decides. flush() and interpreter
    exit wait for every queued write; a write's error is raised by flush()
    or by the next read of that file.

    Used from the analysis object's own thread only: the writer and reaper
    threads get arrays and file names, never this object."""

    CACHE_BYTES = int(os.environ.get('H3D_NPY_CACHE_BYTES', 1 << 30))
    # Bytes the queued (not yet landed) writes may hold: a save beyond it
    # waits for the oldest queued writes first, so a whole-genome run's
    # stages do not pile up on the host faster than the disk takes them.
    PENDING_BYTES = int(os.environ.get('H3D_NPY_PENDING_BYTES', 4 << 30))

    def __init__(self):
        self.cache = collections.OrderedDict()   # fname -> (stamp, array)
        self.cache_bytes = 0
        self.pending = {}       # fname -> _Queued, in this object's order
        self.written = {}       # fname -> stamp of the landed array write
        self.generations = {}   # fname -> number of saves

    # -- the cache ---------------------------------------------------------
    def _cache_drop(self, fname):
        hit = self.cache.pop(fname, None)
        if hit is not None:
            self.cache_bytes -= hit[1].nbytes
            _REAPER.drop(hit, hit[1].nbytes)

    def _cache_put(self, fname, data, stamp):
        self._cache_drop(fname)
        cap = self.CACHE_BYTES
        if data.nbytes > cap:
            _REAPER.drop(data, data.nbytes)
            return
        while self.cache and self.cache_bytes + data.nbytes > cap:
            self._cache_drop(next(iter(self.cache)))    # least recently used
        self.cache[fname] = (stamp, data)
        self.cache_bytes += data.nbytes

    def cache_nbytes(self):
        """Bytes held by the cache."""
        return self.cache_bytes

    # -- the queue ---------------------------------------------------------
    def _settle(self, fname):
        """The queued write of ``fname`` if it has landed: an array goes to
        the cache under its file's stamp (it stays cached as long as the
        file is the one written). Returns the still-queued entry, or None."""
        q = self.pending.get(fname)
        if q is None or not q.future.done():
            return q
        del self.pending[fname]
        stamp = q.future.result()   # raises the write's error
        if q.array is not None:
            self.written[fname] = stamp
            self._cache_put(fname, q.array, stamp)
        return None

    def settle_landed(self):
        """Moves every landed write from the queue into the size-limited
        cache (and its stamp into the written files)."""
        for fname in [f for f, q in self.pending.items()
                      if q.future.done()]:
            self._settle(fname)

    def pending_nbytes(self):
        """Bytes held by the queued (not yet landed) writes."""
        return sum(q.nbytes for q in self.pending.values())

    def _bound_pending(self, incoming):
        """Waits for queued array writes, oldest first in this object's queue
        order (the writer keeps that order per file name only: across its
        lanes an older write is likelier to have landed, not certain to),
        until the queue plus ``incoming`` bytes fit PENDING_BYTES (a single
        larger array is still queued, alone)."""
        self.settle_landed()
        held = self.pending_nbytes()
        for fname, q in list(self.pending.items()):
            if held + incoming <= self.PENDING_BYTES:
                break
            if q.array is not None:
                self.wait(fname)
                held -= q.nbytes

    def wait(self, fname):
        """Returns once this object's queued write of ``fname`` has landed
        (raises its error)."""
        q = self.pending.get(fname)
        if q is not None:
            q.future.result()
            self._settle(fname)

    def flush(self):
        """Waits for every queued write (raises the first write error)."""
        for fname in list(self.pending):
            self.wait(fname)

    def _begin(self, fname):
        """The start of every save: the generation goes up, what is cached
        or queued for ``fname`` is dropped. Returns the earlier queued entry
        (its write still lands first: same file name, same lane)."""
        self.generations[fname] = self.generations.get(fname, 0) + 1
        self._cache_drop(fname)
        return self.pending.pop(fname, None)

    def save(self, fname, data, owned=False, ready=None):
        """Queues ``data`` for ``fname``. ``owned``: the caller hands the
        array over (a fresh result nobody else holds), so it is queued and
        cached without a copy. ``ready``: a callable that returns once
        ``data`` holds its values (an async device -> host copy into it is
        in flight, analysis/d2h.py); the writer and every reader of the
        queued array call it first."""
        data = np.asanyarray(data)
        prev = self._begin(fname)
        if type(data) is not np.ndarray:
            # a subclass np.save may write differently: saved here, after
            # the earlier queued write, and not cached
            if prev is not None:
                prev.future.result()
            np.save(fname, data)
            self.written[fname] = file_stamp(fname)
            return
        self._bound_pending(data.nbytes)
        if not owned:
            if ready is not None:
                ready()
                ready = None
            data = data.copy()
        data.setflags(write=False)   # the queued content must not change
        self.pending[fname] = _Queued(_WRITER.submit(fname, data, ready),
                                      data, ready)

    def save_bytes(self, fname, blob):
        """Queues the bytes ``blob`` for ``fname``: waited for like an array
        write (wait(), flush()), never cached, 0 bytes of the queue."""
        self._begin(fname)
        self.pending[fname] = _Queued(
            _WRITER.submit(fname, blob, fn=_write_bytes))

    # -- reading -----------------------------------------------------------
    def cached(self, fname):
        """The array ``fname`` holds, without reading the file: the queued
        one, or the cached one while the file is the one written; else
        None. Not a copy."""
        q = self._settle(fname)
        if q is not None and q.array is not None:
            if q.ready is not None:
                q.ready()    # the queued array's async copy has landed
            return q.array
        hit = self.cache.get(fname)
        if hit is None:
            return None
        if file_stamp(fname) == hit[0]:
            self.cache.move_to_end(fname)
            return hit[1]
        self._cache_drop(fname)
        return None

    def read(self, fname, idx, col):
        """One .npy, optionally subset by a row mask and/or one column."""
        a = self.cached(fname)
        if a is not None:
            # copies, as np.load hands out fresh arrays
            if idx is None:
                return a.copy() if col is None else a[:, col].copy()
            return a[idx] if col is None else a[idx, col]
        if idx is None:
            a = np.load(fname)
            return a if col is None else a[:, col]
        a = np.load(fname, mmap_mode='r')
        return np.asarray(a[idx] if col is None else a[idx, col])

    def n_rows(self, fname):
        """Rows of the array in ``fname`` (from the file's header when it is
        not cached)."""
        a = self.cached(fname)
        return (a if a is not None else np.load(fname, mmap_mode='r')).shape[0]

    # -- which version of a file -------------------------------------------
    def is_current(self, fname):
        """True when ``fname`` holds what this object last wrote there (its
        write queued, or landed and not modified since)."""
        if self._settle(fname) is not None:
            return True
        stamp = self.written.get(fname)
        return stamp is not None and file_stamp(fname) == stamp

    def generation(self, fname):
        """How many times this object has saved ``fname`` (0: never)."""
        return self.generations.get(fname, 0)

    def token(self, fname):
        """What a mirror of ``fname``'s content keeps to ask later whether
        the file still holds it (token_valid): ('ours', generation) for a
        file this object wrote that is still that write, else ('disk', file
        stamp)."""
        if self.is_current(fname):
            return ('ours', self.generation(fname))
        return disk_token(fname)

    def token_valid(self, fname, token):
        """Whether ``fname`` is still the version ``token`` was taken of."""
        kind, tok = token
        if kind == 'ours':
            return self.generation(fname) == tok and self.is_current(fname)
        return file_stamp(fname) == tok
