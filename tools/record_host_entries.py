"""Records what the host-buffer entry points of libh3d return for the cases
of tests/host_entry_cases.py, into tests/golden/host_entries_parent.npz.

    python tools/record_host_entries.py [--commit HASH] [--out FILE]

The fixture is the yardstick of tests/test_gpu_host_staging.py: it is
recorded ONCE from a tree whose csrc/ is the one a change to the host
plumbing starts from, never from the changed code. Next to every output
array and return code it stores the sha256 of csrc/* and include/h3d.h at
recording time (``source_sha``) and the commit (``commit``), so a fixture
recorded from the code under test shows in review and fails the test."""
import argparse
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import host_entry_cases as hec
    from hic3defdr_amd import _native
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default=None)
    ap.add_argument('--out', default=hec.FIXTURE)
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(
        ['git', '-C', REPO, 'rev-parse', 'HEAD']).decode().strip()
    ctx = _native.Context(0)
    got = hec.replay(_native, ctx)
    ctx.close()
    codes = sorted(set(int(v) for k, v in got.items() if k.endswith('/rc')))
    got['source_sha'] = np.array(hec.source_sha())
    got['commit'] = np.array(commit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **got)
    print('%d calls, %d arrays, return codes %s, %d bytes, sources %s' % (
        len(hec.sequence()), len(got), codes, os.path.getsize(args.out),
        hec.source_sha()[:16]), flush=True)
    for k in sorted(got):
        if k.endswith('/rc') and int(got[k]) != 0:
            print('  rc %d: %s' % (int(got[k]), k[:-3]), flush=True)


if __name__ == '__main__':
    main()
