"""tests/test_gpu_compositor_f64.py's bodies on the host build of the kernels (tests/hip_emu): the compositor's own sources, every
element of every written row against the float64 reference within 2 u e.  Cases A (edges), C (short, ragged last workgroups) and
D (staged and direct workgroups of k_composite_train in one launch, rays above 128 samples) -- what the emulation finishes in
seconds; B and E run on the GPU.  The host build takes expf from libm where the GPU has v_exp_f32: the bar is the same."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

COMBOS = [('A', 2, 3), ('A', 3, 3), ('A', 1, 1), ('A', 0, 2), ('C', 2, 3), ('D', 2, 3), ('D', 0, 2)]


@pytest.fixture(scope='module')
def edev():
    import emulib
    ctx = emulib.emulated_ops()
    dev = ctx.__enter__()
    yield dev
    ctx.__exit__(None, None, None)


@pytest.mark.parametrize('case,ra,da', COMBOS)
def test_forward_backward_inference_against_float64_on_the_host(edev, case, ra, da):
    import test_gpu_compositor_f64 as G
    G.separate_kernels(edev, case, ra, da)


@pytest.mark.parametrize('case,ra,da', COMBOS)
def test_fused_16_lane_form_against_float64_on_the_host(edev, case, ra, da):
    import test_gpu_compositor_f64 as G
    G.fused(edev, case, ra, da, wave=False)


@pytest.mark.parametrize('case,ra,da', COMBOS)
def test_fused_wave_per_ray_form_against_float64_on_the_host(edev, case, ra, da):
    import test_gpu_compositor_f64 as G
    G.fused(edev, case, ra, da, wave=True)


def test_depth_slices_equal_the_full_composite_on_the_host(edev):
    import test_gpu_compositor_f64 as G
    G.slices(edev, 'A', 2, 3)
    G.slices(edev, 'A', 0, 2)
