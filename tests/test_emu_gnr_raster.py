"""The rasteriser kernels of xrnerf_amd/csrc/xr_gnr_raster.hip -- the SAME source the GPU library is built from -- compiled for the host
and run lane by lane by the HIP-on-CPU shim (tests/hip_emu): the bodies of tests/test_gpu_gnr_raster.py through the emulated ops."""
import contextlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def emulated_gnr_raster():
    """test_emu_gnr_render.emulated_gnr_render with the host build of xr_gnr_raster added to its MultiLib tuple"""
    import emulib as E
    from xrnerf_amd import _lib

    @contextlib.contextmanager
    def cm():
        with E.emulated_ops() as dev:
            ml = E.MultiLib(E.ALL_SOURCES + ('xr_gnr', 'xr_gnr_render', 'xr_gnr_raster'))
            for name, (res, args) in list(_lib.SIGNATURES.items()) + list(_lib.GNR_SIGNATURES.items()) + list(_lib.GNR_RENDER_SIGNATURES.items()) + \
                    list(_lib.GNR_RASTER_SIGNATURES.items()):
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
            assert ops.gnr_raster_kernels_available(), 'the host build has no xr_gnr_raster entry points'
            yield dev
    return cm()


@pytest.fixture(scope='module')
def edev():
    with emulated_gnr_raster() as dev:
        yield dev


def _T():
    import test_gpu_gnr_raster as T
    return T


@pytest.mark.parametrize('name', _T().CASE_NAMES)
def test_fixture_cases_bit_for_bit(edev, name):
    _T().check_fixture(edev, name)


def test_one_pixel_no_face_one_vertex_one_face(edev):
    _T().check_small_shapes(edev)


@pytest.mark.parametrize('persp', (True, False))
def test_random_meshes_equal_the_restatement(edev, persp):
    _T().check_random_meshes(edev, persp)


def test_more_than_a_wave_of_vertices_in_one_pixel(edev):
    _T().check_crowded_pixel(edev)


def test_views_in_one_call_output_slices_and_repeatability(edev):
    _T().check_views_slices_and_repeat(edev)


def test_depth_maps_of_the_generated_scene(edev):
    _T().check_depth_maps(edev)


def test_prepare_data_builds_or_keeps_the_depth_maps(edev):
    _T().check_prepare_data(edev)


def test_render_rays_on_rasterised_depth_and_scan_depth_maps(edev):
    _T().check_render_rays_on_raster_depth(edev)


def test_header_table_and_host_build_agree(edev):
    _T().check_symbols()


def test_refusals_launch_nothing(edev):
    _T().check_refusals(edev)
