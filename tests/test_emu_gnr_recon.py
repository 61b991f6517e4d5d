"""The reconstruction kernels of xrnerf_amd/csrc/xr_gnr_recon.hip -- the SAME source the GPU library is built from -- compiled for the
host and run lane by lane by the HIP-on-CPU shim (tests/hip_emu): the bodies of tests/test_gpu_gnr_recon.py through the emulated ops (the whole
reconstruction, whose network runs for minutes on the shim, stays with the tensor-op tier and the MI355X)."""
import contextlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def emulated_gnr_recon():
    """test_emu_gnr_render.emulated_gnr_render with the host build of xr_gnr_recon added to its MultiLib tuple"""
    import emulib as E
    from xrnerf_amd import _lib

    @contextlib.contextmanager
    def cm():
        with E.emulated_ops() as dev:
            ml = E.MultiLib(E.ALL_SOURCES + ('xr_gnr', 'xr_gnr_render', 'xr_gnr_recon'))
            for name, (res, args) in list(_lib.SIGNATURES.items()) + list(_lib.GNR_SIGNATURES.items()) + list(_lib.GNR_RENDER_SIGNATURES.items()) + \
                    list(_lib.GNR_RECON_SIGNATURES.items()):
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
            from xrnerf_amd import ops
            assert ops.gnr_recon_kernels_available(), 'the host build has no xr_gnr_recon entry points'
            yield dev
    return cm()


@pytest.fixture(scope='module')
def edev():
    with emulated_gnr_recon() as dev:
        yield dev


def _T():
    import test_gpu_gnr_recon as T
    return T


@pytest.mark.parametrize('N', _T().HULL_SIZES)
def test_grid_points_bit_for_bit_and_hull_flags(edev, N):
    _T().check_grid_hull(edev, N)


@pytest.mark.parametrize('N,reso0,kind', _T().OCTREE_CASES)
def test_octree_bookkeeping_equals_the_restatement(edev, N, reso0, kind):
    _T().check_octree(edev, N, reso0, kind)


def test_surface_of_all_256_corner_patterns_is_closed(edev):
    _T().check_surface_patterns(edev)


def test_surface_of_random_volumes_is_closed(edev):
    _T().check_surface_random(edev)


def test_surface_sphere_and_torus(edev):
    _T().check_surface_solids(edev)


def test_surface_degenerate_volumes(edev):
    _T().check_surface_degenerate(edev)


def test_world_transform_point_rows_and_sigmoid_scatter(edev):
    _T().check_small_stages(edev)


def test_laplacian_smoothing(edev):
    _T().check_smooth(edev)


def test_bad_arguments_launch_nothing(edev):
    """XR_EINVAL and untouched outputs: a grid of one point, too many views, a level that is no level, a fold at reso 1"""
    import ctypes as C
    import torch
    from xrnerf_amd import _lib
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    lin = (C.c_double * 9)(0, 1, 1, 0, 1, 1, 0, 1, 1)
    center, w2c, cams, masks = torch.zeros(3), torch.eye(4).repeat(9, 1, 1), torch.ones((9, 4)), torch.ones((9, 4, 4))
    state, vol, ws, total = torch.full((27,), 7, dtype=torch.uint8), torch.full((27,), 7.0), torch.full((64,), 7, dtype=torch.int32), torch.full((2,), 7, dtype=torch.int32)
    hull = lambda N, V, sf: lib.xr_gnr_recon_hull(N, lin, sf, p(center), None, p(w2c), p(cams), 4, V, p(masks), 4, 4, 4.0, 4.0, p(state), None)
    assert hull(1, 1, 1.0) < 0 and hull(3, 9, 1.0) < 0 and hull(3, 0, 1.0) < 0 and hull(3, 1, 0.0) < 0 and hull(2000, 1, 1.0) < 0
    assert lib.xr_gnr_recon_select_count(3, 0, p(state), p(ws), 256, p(total), None) < 0
    assert lib.xr_gnr_recon_select_count(3, 3, p(state), p(ws), 256, p(total), None) < 0
    assert lib.xr_gnr_recon_select_count(3, 1, p(state), p(ws), 0, p(total), None) < 0
    assert lib.xr_gnr_recon_fold(3, 1, p(vol), p(state), p(ws), 256, None) < 0
    assert lib.xr_gnr_recon_fold(3, 2, p(vol), p(state), p(ws), 1, None) < 0
    assert lib.xr_gnr_recon_surface_count(p(vol), 1, 0.5, p(ws), 256, p(total), None) < 0
    assert lib.xr_gnr_recon_surface_count(p(vol), 3, 0.5, p(ws), 16, p(total), None) < 0
    for t in (state, vol, ws, total):
        assert bool((t == 7).all())
