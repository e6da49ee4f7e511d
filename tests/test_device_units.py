"""One kernel, one home: every device kernel of libh3d.so is compiled into
one object, and hipcub / rocprim are included by the h3d_cub_*.hip units
alone (csrc/h3d_cub.h).

libh3d.so is linked without relocatable device code, so each .hip unit
carries its own code object and nothing removes a kernel that two units both
compile. The test reads the built objects as bytes: a kernel's descriptor is
the symbol <mangled name>.kd in the object's device code.
"""
import collections
import glob
import os
import re

import pytest

from hic3defdr_amd import build as h3dbuild

KD = re.compile(rb'\x00([A-Za-z_][\w$.]*)\.kd\x00')
INCLUDE = re.compile(r'^\s*#\s*include\s*[<"](hipcub|rocprim)/', re.M)


def is_cub_unit(name):
    return name.startswith('h3d_cub_')


@pytest.fixture(scope='module')
def kernels():
    """object file name -> the mangled names of the kernels in it"""
    h3dbuild.build_native()
    objs = sorted(glob.glob(os.path.join(h3dbuild.LIBDIR, 'obj', '*.hip.o')))
    wanted = {src + '.o' for src, cc in h3dbuild.NATIVE_SRCS if cc == 'hipcc'}
    # (an object left by an earlier source list is not part of the library)
    out = {}
    for path in objs:
        if os.path.basename(path) in wanted:
            with open(path, 'rb') as fh:
                out[os.path.basename(path)] = {
                    m.group(1).decode() for m in KD.finditer(fh.read())}
    assert set(out) == wanted
    return out


def test_scan_reads_the_objects(kernels):
    # an object format the scan cannot read must not pass as "no duplicates"
    assert any('k_brent' in n for n in kernels['h3d_api.hip.o'])
    cub = [o for o in kernels if is_cub_unit(o)]
    assert cub
    for o in cub:
        assert any('rocprim' in n for n in kernels[o]), o


def test_kernel_outside_the_cub_units_has_one_home(kernels):
    homes = collections.defaultdict(list)
    for obj, names in kernels.items():
        for n in names:
            homes[n].append(obj)
    twice = {n: sorted(o) for n, o in homes.items()
             if len(o) > 1 and not all(is_cub_unit(x) for x in o)}
    assert not twice, '%d kernels compiled into more than one object: %s' % (
        len(twice), sorted(twice.items())[:5])


def test_only_the_cub_units_include_hipcub():
    found = []
    for pat in ('*.hip', '*.cpp', '*.h'):
        for path in sorted(glob.glob(os.path.join(h3dbuild.CSRC, pat))):
            name = os.path.basename(path)
            with open(path, errors='replace') as fh:
                if INCLUDE.search(fh.read()):
                    found.append(name)
    assert found, 'no unit includes hipcub: the pattern no longer matches'
    assert all(is_cub_unit(n) and n.endswith('.hip') for n in found), found
