"""The two builds of the unit-test ABI h3dt_* (csrc/h3d_unit_abi.h) as ctypes
libraries, and the names each of them exports."""
import ctypes
import os

from hic3defdr_amd import build as h3dbuild

# defined once in csrc/h3d_unit_abi.h, compiled into both libraries
SHARED = ['h3dt_' + n for n in (
    'lgam', 'lgam_nll', 'log_fast', 'log_fast_fp_index', 'ndtr', 'ndtri',
    'log1pmx', 'lgam1p', 'igam', 'igamc', 'igami', 'igamci', 'chi2_sf',
    'exp_fast', 'log_fast_checked', 'recip_fast', 'div_fast', 'philox',
    'philox_uniform', 'nb_draw', 'sim_bm', 'poisson_quantile', 'igam_pq',
    'igam_inv', 'igam_step_taylor', 'log_index', 'q2q', 'fit_mu',
    'equalize_alpha', 'equalize', 'nll_terms', 'lrt', 'qcml')]
# csrc/h3d_hosttest.cpp alone
HOST_ONLY = ['h3dt_' + n for n in (
    'exp_fast_straight', 'disp_rounds', 'ccl_labels', 'q_class',
    'argmax_class')]
# csrc/h3d_selftest.hip alone
GFX950_ONLY = ['h3dt_device_ok']


def load_host():
    """libh3d_hosttest.so (g++; built here when stale)."""
    return ctypes.CDLL(h3dbuild.build_hosttest())


def load_gfx950():
    """libh3d_selftest.so (hipcc, gfx950) on a machine with a device."""
    # one HIP runtime per process: torch's first, as _native.load_library
    # does (the selftest library loaded first leaves torch without devices
    # for the GPU tests that run after this module)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    # prebuilt in-tree by build() (the GPU box does not compile)
    path = os.path.join(h3dbuild.LIBDIR, 'libh3d_selftest.so')
    if not os.path.exists(path):
        raise RuntimeError('libh3d_selftest.so missing: run build()')
    lib = ctypes.CDLL(path)
    assert lib.h3dt_device_ok() == 1, 'no HIP device for the gfx950 self-test'
    return lib
