"""The dispersion search against the exact CML minimiser (GPU): every NLL
form and every kernel that runs the bounded search, on the segment cases of
tests/golden/unit_cml_mp.npz (mpmath; cml_mp_cases.py derives the bound).

- ``ctx.cml(data)`` on every segment case: ``k_brent<4 | 8 | 16 | 32>`` on
  given pseudodata (general form only; ``frac`` is not integer). The cases
  of 1025 and 2049 pixels again with ``H3D_BRENT_LDS_KB=16``, where they
  cross the LDS head into the streamed tail.
- The whole qcml driver, ``h3d_disp_per_dist`` with f = 1, on the integer
  families of cml_mp_cases.QCML_FAMILIES (which says why ``over``, ``huge``
  and ``ceiling`` are left out: the first has no result in the reference
  either, and at delta near 0.97 a tol2 move in delta is more than qcml's
  1e-4 in disp, so the loop may not settle). One case per distance, each
  condition's columns a case of that condition's width: with f = 1 the
  equalize pass returns the counts, every qcml iteration is a CML search on
  the same data, and whichever iteration ends the loop must meet the segment
  bound. Designs 2+2 (M = 2, the full form), 4+4, 3+5 (mixed widths in one
  slot), 8+8 and 16+16, each three ways: ``H3D_BRENT=0`` (k_brent, 16 KB
  head), ``H3D_BRENT=2`` (k_brent_gang) and the multi-rank driver
  (k_disp_work + k_seg_reduce + k_seg_update) with the identity reduce of
  test_gpu_disp_paths._noop_call. The optima lie at r ~ 50 (benign, large),
  r ~ 2000 (poisson), r = 9999 (under: the lower bound) and r ~ 0.5 (sparse),
  and every search opens at r = 1.64, 0.63, 3.28, 5.92: the large and the
  general form each hold an optimum, and the mid and r >= 5 forms are
  evaluated on the way to one.
- An all-zero segment (65 x 4): the objective is rounding noise, there is
  no minimiser to compare with; the result is finite, inside the bounds,
  unflagged, and the same bits on a second call.

Every case prints its distance to delta_star as a fraction of the bound
(``-rP``). Worst fraction per entry point, measured on an MI355X:

    ctx.cml (default head)            0.96  (ceiling; under 0.88; 0.26 elsewhere)
    ctx.cml (16 KB head, long cases)  0.23
    disp_per_dist, H3D_BRENT=0        0.88  (under; 0.26 elsewhere)
    disp_per_dist, H3D_BRENT=2        0.88  (under; 0.26 elsewhere)
    multi-rank driver                 0.88  (under; 0.26 elsewhere)

(``under`` and ``ceiling`` sit on the bounds, which a bounded search never
evaluates: its last point is 5.9e-6 inside at 1e-4 and 3.4e-6 to 6.4e-6 inside
at 100/101, by construction and as oracle.cml's is. The all-zero segment ends
at delta = 0.377.)
"""
import numpy as np
import pytest

import cml_mp_cases as cc
from test_gpu_disp_paths import _host_call, _noop_call, _ok, _open

pytestmark = pytest.mark.gpu

DESIGNS = ((2, 2), (4, 4), (3, 5), (8, 8), (16, 16))
WAYS = (('brent', dict(H3D_BRENT=0, H3D_BRENT_LDS_KB=16)),
        ('gang', dict(H3D_BRENT=2)),
        ('multirank', {}))

_cache = {}


@pytest.fixture(scope='module')
def ctx():
    with _open() as c:
        yield c


@pytest.fixture(scope='module')
def ctx_small_head():
    with _open(H3D_BRENT=0, H3D_BRENT_LDS_KB=16) as c:
        yield c


def _id(case):
    return '%s-n%d-L%d' % case


@pytest.mark.parametrize('case', cc.seg_cases(), ids=_id)
def test_cml_segment(ctx, case):
    seg = cc.segment(*case)
    # (a failed search raises: h3d_cml returns H3D_ENOCONV on kFlagBrentFail)
    disp = ctx.cml(seg.data)
    cc.check_segment(seg, disp, 0, 'cml')


@pytest.mark.parametrize('case', cc.SEG_LONG, ids=_id)
def test_cml_segment_streamed_tail(ctx_small_head, case):
    seg = cc.segment(*case)
    disp = ctx_small_head.cml(seg.data)
    cc.check_segment(seg, disp, 0, 'cml-16KB')


def _plan(design):
    """[(segment of condition 0, segment of condition 1)] per distance: the
    five families at 65 pixels, the second condition one family on; where
    both widths have them, the cases of 1025 and 2049 pixels."""
    a, b = design
    fams = cc.QCML_FAMILIES
    plan = [(cc.segment(fam, a), cc.segment(fams[(k + 1) % len(fams)], b))
            for k, fam in enumerate(fams)]
    long_ = {(fam, n, ln) for fam, n, ln in cc.SEG_LONG}
    for fam, other in (('benign', 'sparse'), ('sparse', 'benign')):
        for ln in (1025, 2049):
            if (fam, a, ln) in long_ and (other, b, ln) in long_:
                plan.append((cc.segment(fam, a, ln), cc.segment(other, b, ln)))
    return plan


def _inputs(design):
    key = ('inputs', design)
    if key not in _cache:
        plan = _plan(design)
        raw = np.concatenate([np.hstack([s0.data, s1.data])
                              for s0, s1 in plan]).astype(np.int64)
        lengths = [s0.length for s0, _ in plan]
        dist = np.repeat(np.arange(len(plan), dtype=np.int32), lengths)
        # (the driver sorts: hand it the pixels in no particular order)
        perm = np.random.RandomState(sum(design)).permutation(len(raw))
        cond = np.repeat(np.arange(2, dtype=np.int32), design)
        _cache[key] = (plan, (np.ascontiguousarray(raw[perm]),
                              np.ones(raw.shape), dist[perm], cond,
                              len(plan)))
    return _cache[key]


@pytest.mark.parametrize('way', WAYS, ids=[w for w, _ in WAYS])
@pytest.mark.parametrize('design', DESIGNS, ids=lambda d: '%d+%d' % d)
def test_qcml_f1(design, way):
    name, switches = way
    plan, data = _inputs(design)
    with _open(**switches) as c:
        if name == 'multirank':
            rc, out, flags, ncalls = _noop_call(c, data)
            assert ncalls > 10
        else:
            rc, out, flags = _host_call(c, data)
    _ok(rc, 'h3d_disp_per_dist')
    what = '%s %d+%d' % ((name,) + design)
    bad = []
    for d, segs in enumerate(plan):
        for k, seg in enumerate(segs):
            try:
                cc.check_segment(seg, out[d, k], int(flags[d, k]), what)
            except AssertionError as e:
                bad.append(e.args[0])
    assert not bad, bad
    assert not flags.any()


def test_all_zero_segment(ctx):
    data = np.zeros((65, 4))
    first = ctx.cml(data)
    second = ctx.cml(data)
    delta = first / (1. + first)
    print('all-zero 65 x 4: disp', first, 'delta', delta)
    assert np.isfinite(first)
    assert cc.BRENT_A <= delta <= cc.BRENT_B
    assert np.float64(first).tobytes() == np.float64(second).tobytes()
