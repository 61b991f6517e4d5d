"""The GNR kernels of xrnerf_amd/csrc/xr_gnr.hip -- the SAME source the GPU library is built from -- compiled for the host and run lane
by lane by the HIP-on-CPU shim (tests/hip_emu): the bodies of tests/test_gpu_gnr.py through the emulated ops, against the reference's own
kernels (tests/golden/ref_gnr.npz).  On this tier the bitwise bars are absolute."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
G = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(G, 'ref_gnr.npz'))


def emulated_gnr():
    """context manager: emulib.emulated_ops with the host build of xr_gnr added and bound (GNR_SIGNATURES)"""
    import contextlib
    import emulib as E
    from xrnerf_amd import _lib

    @contextlib.contextmanager
    def cm():
        with E.emulated_ops() as dev:
            ml = E.MultiLib(E.ALL_SOURCES + ('xr_gnr',))
            for name, (res, args) in list(_lib.SIGNATURES.items()) + list(_lib.GNR_SIGNATURES.items()):
                try:
                    fn = getattr(ml, name)
                except AttributeError:
                    continue
                fn.restype, fn.argtypes = res, args
            _lib._lib = ml

            def check(rc, what=''):
                if rc != 0:
                    raise _lib.XrError('%s failed (%d): %s' % (what, rc, ml.last_errors()))
            _lib.check = check
            yield dev
    return cm()


@pytest.fixture(scope='module')
def edev():
    with emulated_gnr() as dev:
        yield dev


def _T():
    import test_gpu_gnr as T
    return T


@pytest.mark.parametrize('name', _T().STRUCT_CASES)
def test_structure_is_exact_and_repeats(edev, gold, name):
    _T().check_structure(edev, gold, name)


@pytest.mark.parametrize('N', _T().QUERY_N)
def test_nearest_and_inside_against_the_reference_kernels(edev, gold, N):
    _T().check_queries(edev, gold, 'm3', N)


def test_nearest_and_inside_on_the_icosahedron(edev, gold):
    _T().check_queries(edev, gold, 'm0', 64)


def test_all_fixture_queries_vertices_and_centroids_included(edev, gold):
    _T().check_queries(edev, gold, 'm3', 4000)


@pytest.mark.parametrize('key,N', (('m0', None), ('m3', 1000)))
def test_embedding_against_the_reference_lines(edev, gold, key, N):
    _T().check_embedding(edev, gold, key, N)


def test_flat_mesh_no_points_and_bad_grids_launch_nothing(edev, gold):
    _T().check_launch_nothing(edev, gold)


def test_non_finite_queries_touch_no_table(edev, gold):
    _T().check_non_finite_queries(edev, gold)
