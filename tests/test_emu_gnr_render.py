"""The GNR renderer kernels of xrnerf_amd/csrc/xr_gnr_render.hip -- the SAME source the GPU library is built from -- compiled for the
host and run lane by lane by the HIP-on-CPU shim (tests/hip_emu): the bodies of tests/test_gpu_gnr_render.py through the emulated ops,
against the reference's own renderer (tests/golden/ref_gnr_render.npz) and the float64 restatement."""
import contextlib
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
    return np.load(os.path.join(G, 'ref_gnr_render.npz'))


def emulated_gnr_render():
    """test_emu_gnr.emulated_gnr with the host build of xr_gnr_render added to its MultiLib tuple"""
    import emulib as E
    from xrnerf_amd import _lib

    @contextlib.contextmanager
    def cm():
        with E.emulated_ops() as dev:
            ml = E.MultiLib(E.ALL_SOURCES + ('xr_gnr', 'xr_gnr_render'))
            for name, (res, args) in list(_lib.SIGNATURES.items()) + list(_lib.GNR_SIGNATURES.items()) + list(_lib.GNR_RENDER_SIGNATURES.items()):
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
            assert ops.gnr_render_kernels_available(), 'the host build has no xr_gnr_render entry points'
            yield dev
    return cm()


@pytest.fixture(scope='module')
def edev():
    with emulated_gnr_render() as dev:
        yield dev
    _T().write_ratios('kernels\' host build')


def _T():
    import test_gpu_gnr_render as T
    return T


@pytest.mark.parametrize('R,V', _T().HULL_CASES)
def test_hull_flags_order_and_rows(edev, gold, R, V):
    from xrnerf_amd import ops
    assert ops.gnr_render_kernels_available()
    _T().check_hull(edev, gold, R, V)


def test_hull_with_the_training_draws(edev, gold):
    _T().check_hull(edev, gold, 48, 4, 'trn')


def test_hull_of_288_rays_scans_the_counts_in_two_sweeps(edev, gold):
    _T().check_hull(edev, gold, 48, 2, tile=6)


def test_hull_nan_ray_camera_behind_and_nothing_to_do(edev, gold):
    _T().check_hull_edges(edev, gold)


@pytest.mark.parametrize('N,C', _T().GATHER_CASES)
def test_gather_against_float64_grid_sample(edev, gold, N, C):
    _T().check_gather(edev, gold, N, C)


@pytest.mark.parametrize('mode', _T().MODES)
def test_gather_holds_the_fixture(edev, gold, mode):
    _T().check_gather_fixture(edev, gold, mode)


@pytest.mark.parametrize('N,C', _T().GATHER_BWD_CASES)
def test_gather_backward_to_the_feature_maps(edev, gold, N, C):
    _T().check_gather_backward(edev, gold, N, C)


@pytest.mark.parametrize('mode', _T().MODES)
def test_compositor_holds_the_fixture_forward_and_backward(edev, gold, mode):
    _T().check_composite_fixture(edev, gold, mode)


@pytest.mark.parametrize('V,white,S', _T().COMPOSITE_CASES)
def test_compositor_empty_full_and_opaque_rays(edev, gold, V, white, S):
    _T().check_composite_cases(edev, gold, V, white, S)


@pytest.mark.parametrize('mode', _T().MODES)
def test_stages_chained_on_the_fixture(edev, gold, mode):
    _T().check_end_to_end_stages(edev, gold, mode)


def test_bad_arguments_launch_nothing(edev, gold):
    """XR_EINVAL and untouched outputs: too many views, a camera row of 7 entries, a row stride below the row, C not a multiple of 4"""
    import ctypes as C
    import torch
    from xrnerf_amd import _lib, ops
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    T = _T()
    inp = T.hull_inputs(edev, gold, 'inf', 3, 4)
    rank, table, total = (torch.full((n,), 7, dtype=torch.int32) for n in (48, 6, 1))
    head = lambda V, cols: (p(inp['rays']), p(inp['t_vals']), 3, 16, p(inp['calibs']), p(inp['persps']), cols, V, p(inp['masks']), 64, 64, 64.0, 64.0)
    for V, cols in ((9, 11), (0, 11), (4, 7), (4, 3)):
        assert lib.xr_gnr_hull_count(*head(V, cols), p(rank), p(table), p(total), None) < 0
    assert lib.xr_gnr_hull_count(*head(4, 11)[:9], 64, 64, 0.0, 64.0, p(rank), p(table), p(total), None) < 0
    xy, feats, img = torch.zeros((2, 4, 2)), torch.zeros((4, 3, 3, 8)), torch.zeros((4, 3, 5, 5))
    out, rgb = torch.full((2, 4, 12), 7.0), torch.full((2, 4, 3), 7.0)
    assert lib.xr_gnr_gather(p(xy), 2, 4, p(feats), 3, 3, 8, p(img), 5, 5, 0, p(out), 10, 0, p(rgb), None) < 0           # ld < C + 3
    assert lib.xr_gnr_gather(p(xy), 2, 4, p(feats), 3, 3, 6, p(img), 5, 5, 0, p(out), 12, 0, p(rgb), None) < 0           # C % 4
    assert lib.xr_gnr_gather(p(xy), 2, 4, p(feats), 3, 3, 8, p(img), 5, 5, 0, p(out), 12, 2, p(rgb), None) < 0           # col0 + C + 3 > ld
    net = torch.zeros((2, 8))
    o = [torch.full((n,), 7.0) for n in (18, 3, 3, 48, 2)]
    assert lib.xr_gnr_composite_forward(p(net), 8, p(rgb), p(rank), p(table), p(inp['t_vals']), None, 3, 16, 4, 2, 0, 0.0, 0.0, 0,
                                        *[p(t) for t in o], None) < 0                                               # ld < 4 + V + 1
    for t in [rank, table, total, out, rgb] + o:
        assert bool((t == 7).all())


@pytest.fixture(scope='module')
def params():
    return _T().load_params()


def test_gnrmlp_strict_load_output_alpha_only_and_parameter_gradients(edev, gold, params):
    _T().check_mlp(edev, gold, params)


def test_gnrmlp_with_two_views_against_the_restatement(edev, gold, params):
    _T().check_mlp_two_views(edev, gold, params)


@pytest.mark.parametrize('mode', _T().MODES)
def test_render_rays_on_the_fixture(edev, gold, params, mode):
    _T().check_render_rays(edev, gold, params, mode)


def test_config_builds_refusals_and_empty_hull(edev, gold, params):
    _T().check_renderer_contract(edev, gold, params)
