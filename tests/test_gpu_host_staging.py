"""The host-buffer entry points of libh3d against what the library returned
before their staging was gathered into one helper (csrc/h3d_ctx.h,
``HostCall``): tests/golden/host_entries_parent.npz, recorded by
tools/record_host_entries.py from the parent's sources.

The same kernels run over the same inputs, so every output is compared bit
for bit (a NaN by its bit pattern) and every return code exactly. The cases
and their order are tests/host_entry_cases.py's."""
import ctypes

import numpy as np
import pytest

import host_entry_cases as hec

pytestmark = pytest.mark.gpu

EARG, EINPUT = -1, -5
# the entry points that reject a count beyond int32 after their uploads
REJECTING = ('lrt', 'lrt_poisson', 'disp_per_dist', 'nb_fit_mu',
             'nb_equalize')


@pytest.fixture(scope='module')
def fixture():
    return np.load(hec.FIXTURE, allow_pickle=False)


def _assert_replay(got, fixture, what):
    keys = [k for k in fixture.files if k not in ('source_sha', 'commit')]
    assert sorted(got) == sorted(keys), what
    for k in keys:
        assert hec.same_bytes(got[k], fixture[k]), '%s: %s' % (what, k)


# csrc/* + include/h3d.h of the commit the fixture was recorded at
PARENT_SHA = '7b4ca941a44a03693cef7de4e9b0c2cee89da17c0f15c4d0d3ec388914db13eb'
PARENT_COMMIT = '6e9a0ba7a2e9d5367c36950ac95725f7be86dcd2'


def test_fixture_was_recorded_from_the_parent_sources(fixture):
    stored = str(fixture['source_sha'])
    assert stored == PARENT_SHA and str(fixture['commit']) == PARENT_COMMIT
    assert stored != hec.source_sha(), (
        'host_entries_parent.npz was recorded from the sources under test '
        '(csrc/* + include/h3d.h sha256 %s): it must be the recording of '
        'the parent of the change that introduced HostCall' % stored)


def test_replay_gives_the_recorded_bits(fixture):
    from hic3defdr_amd import _native
    ctx = _native.Context(0)
    try:
        got = hec.replay(_native, ctx)
    finally:
        ctx.close()
    _assert_replay(got, fixture, 'replay')


def _count_inputs():
    rng = np.random.default_rng(5)
    n, R = 300, 4
    raw = rng.poisson(20, (n, R)).astype(np.int64)
    raw[n // 2, 1] = 2 ** 31
    f = np.exp(rng.normal(0, 0.1, (n, R)))
    dist = rng.integers(0, hec.D, n).astype(np.int32)
    return raw, f, dist, hec.COND[R]


def _reject_after_upload(_native, ctx, entry):
    """A count beyond int32: H3D_EINPUT, known once the counts are on the
    device."""
    raw, f, dist, cond = _count_inputs()
    call = {
        'lrt': lambda: ctx.lrt(raw, f, dist, np.full((hec.D, hec.C), 0.1),
                               cond),
        'lrt_poisson': lambda: ctx.lrt_poisson(raw, f, cond, hec.C),
        'disp_per_dist': lambda: ctx.disp_per_dist(raw, f, dist, cond, hec.C,
                                                   hec.D),
        'nb_fit_mu': lambda: ctx.nb_fit_mu(raw, f, 0.05),
        'nb_equalize': lambda: ctx.nb_equalize(raw, f, 0.05, want_mu=True),
    }[entry]
    with pytest.raises(_native.H3DError) as e:
        call()
    assert e.value.code == EINPUT, entry


def _reject_before_upload(ctx, entry):
    """NULL buffers with n = 5: H3D_EARG ahead of any upload."""
    lib, h, N = ctx.lib, ctx.handle, None
    cond = hec.COND[4]
    cp = cond.ctypes.data_as(ctypes.c_void_p)
    rc = {
        'lrt': lambda: lib.h3d_lrt(h, N, N, N, N, 5, 4, 2, cp, hec.D, 1, N, N,
                                   N, N, N),
        'lrt_poisson': lambda: lib.h3d_lrt_poisson(h, N, N, 5, 4, 2, cp, N, N,
                                                   N, N),
        'disp_per_dist': lambda: lib.h3d_disp_per_dist(h, N, N, N, 5, 4, 2,
                                                       cp, hec.D, 0, N, N),
        'nb_fit_mu': lambda: lib.h3d_nb_fit_mu(h, N, N, N, 0, 0, 5, 4, N, N),
        'nb_equalize': lambda: lib.h3d_nb_equalize(h, N, N, 0.05, N, 5, 4, N,
                                                   N, N),
    }[entry]()
    assert rc == EARG, entry


def test_a_rejected_call_leaves_the_ctx_as_it_was(fixture):
    """The sequence again, each good call of a rejecting entry point right
    after one of its rejections (after its uploads at R = 3, ahead of them
    at R = 4): the good call still gives the recorded bits."""
    from hic3defdr_amd import _native
    ctx = _native.Context(0)
    rejected = []

    def before(name):
        entry = name.split(': ', 1)[1].split(' ')[0]
        if entry not in REJECTING:
            return
        if 'R=3' in name:
            _reject_after_upload(_native, ctx, entry)
        else:
            _reject_before_upload(ctx, entry)
        rejected.append(name)

    try:
        got = hec.replay(_native, ctx, before)
    finally:
        ctx.close()
    # each entry point, each size of the sequence, both kinds
    assert len(set(n.split(': ', 1)[1].split(' ')[0] for n in rejected)) == 5
    assert len(rejected) >= 5 * 2 * len(hec.SIZES)
    _assert_replay(got, fixture, 'replay with rejections')
