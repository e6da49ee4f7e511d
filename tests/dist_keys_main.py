"""torchrun worker for tests/test_gpu_multirank.py::
test_two_ranks_compact_reshard_equals_full_record: the distance re-shard's
two pixel exchanges on the GPU, side by side. Every rank builds the resident
entries of its chromosomes of one seeded synthetic genome (three chromosomes
of 2-5 thousand union pixels; genome index g belongs to rank g % world, so
two ranks hold 0 and 2 / 1 and PixelKeys.device_tables interleaves their
rows), takes its disp pixels from Resident.disp_pixels and their keys from
Resident.disp_keys, and ships them to the owners of their distances twice:
the full record (parallel.exchange_by_owner) and the keys of f
(parallel.exchange_compact, f rebuilt by h3d_pixel_f_dev), on a side stream
shared by libh3d and torch as analysis._disp_per_dist_sharded sets it up.
A rank prints ``bit-identical=True`` only if raw, f and dist of the two
agree in dtype, shape and every bit, for every variant -- per-pixel size
factors by distance bin (a conditional norm's) and per-replicate ones, R = 4
and 9, genome index 2 with and without disp pixels -- cut into 1 and 3 parts.
Backend gloo, every rank on the GPU H3D_DEVICE names.

    torchrun --nproc-per-node 2 tests/dist_keys_main.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

# union pixels, bias rows, size-factor rows of genome index 0, 1, 2
GENOME = ((4001, 150, 12), (2503, 80, 5), (3102, 111, 3))
DMAX = 24
# (R, per-replicate size factors, index 2 without disp pixels)
VARIANTS = ((4, False, False), (4, True, False), (9, False, False),
            (9, True, True), (4, False, True))


def _entry(g, R, per_rep, no_disp, dev, seed):
    """The ChromDev of genome index g (files={}: always current)."""
    import numpy as np
    import torch
    from hic3defdr_amd.analysis.resident import ChromDev
    n, nb, ns = GENOME[g]
    rng = np.random.default_rng([seed, g])
    row = np.sort(rng.integers(0, nb - DMAX, n)).astype(np.int32)
    col = (row + rng.integers(0, DMAX, n)).astype(np.int32)
    raw = rng.poisson(5, (n, R)).astype(np.int32)
    bias = np.exp(rng.normal(0, 0.2, (nb, R)))
    bias[rng.random(bias.shape) < 0.05] = 0.0
    if per_rep:
        sf = rng.uniform(0.5, 2.0, R)
    else:   # one row per distance bin, two bins with equal rows
        tab = rng.uniform(0.5, 2.0, (ns, R))
        tab[ns - 1] = tab[0]
        sf = tab[(col - row) * ns // DMAX]
    di = rng.random(n) < (0.0 if no_disp else 0.4)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return ChromDev(up(row), up(col), up(raw), up(sf), per_rep,
                    up(di.astype(np.uint8)), int(di.sum()), bias, {})


def _same(a, b):
    import torch
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == torch.float64:
        a = a.contiguous().view(torch.int64)
        b = b.contiguous().view(torch.int64)
    return bool(torch.equal(a, b))


def main():
    import torch
    import torch.distributed as dist
    from hic3defdr_amd import _native, parallel
    from hic3defdr_amd.analysis.resident import Resident
    dist.init_process_group('gloo')
    rank, world = dist.get_rank(), dist.get_world_size()
    dev = torch.device('cuda', int(os.environ.get('H3D_DEVICE', '0')))
    torch.cuda.set_device(dev)
    ctx = _native.context(dev.index)

    class _H(object):
        _store = None       # no entry mirrors an outdir file

        def _ctx(self):
            return ctx
    names = ['c%d' % g for g in range(len(GENOME))]
    index = {c: g for g, c in enumerate(names)}
    mine = [c for c in names if index[c] % world == rank]
    ok, moved = True, 0
    for v, (R, per_rep, empty2) in enumerate(VARIANTS):
        res = Resident(_H())
        for c in mine:
            g = index[c]
            res.chroms[c] = _entry(g, R, per_rep, empty2 and g == 2, dev,
                                   50 + v)
        t_raw, t_f, t_dist, _ = res.disp_pixels(mine, R)
        owner = t_dist.long() * 7 % world
        torch.cuda.current_stream(dev).synchronize()
        stream = torch.cuda.Stream(dev)
        ctx.set_stream(stream.cuda_stream)
        try:
            with torch.cuda.stream(stream):
                keys = res.disp_keys(mine, index)
                for chunks in (1, 3):
                    full = parallel.exchange_by_owner(t_raw, t_f, t_dist,
                                                      owner, chunks=chunks)
                    comp = parallel.exchange_compact(ctx, t_raw, t_dist, keys,
                                                     owner, chunks=chunks)
                    stream.synchronize()
                    same = all(_same(a, b) for a, b in zip(full, comp))
                    print('rank %d R=%d per_rep=%s empty2=%s chunks=%d: sent '
                          '%d received %d same=%s'
                          % (rank, R, per_rep, empty2, chunks,
                             t_raw.shape[0], full[0].shape[0], same),
                          flush=True)
                    ok = ok and same and len(full) == len(comp) == 3
                    moved += int(full[0].shape[0])
        finally:
            stream.synchronize()
            ctx.set_stream(None)
    ok = ok and moved > 0
    print('rank %d of %d: %d variants, %d pixels received, bit-identical=%s'
          % (rank, world, len(VARIANTS), moved, ok), flush=True)
    # every rank leaves with the same status
    t_ok = torch.tensor([int(ok)], dtype=torch.int64)
    dist.all_reduce(t_ok, op=dist.ReduceOp.MIN)
    dist.destroy_process_group()
    if not int(t_ok.item()):
        sys.exit(1)


if __name__ == '__main__':
    main()
