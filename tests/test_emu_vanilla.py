"""The vanilla-NeRF kernels of xrnerf_amd/csrc/xr_vanilla.hip -- the SAME source the GPU library is built from -- compiled for the host
and run lane by lane by the HIP-on-CPU shim (tests/hip_emu): the bodies of tests/test_gpu_vanilla.py through the emulated ops, against
the float64 restatement (tests/vanilla_restatement.py) and the reference's training step (tests/golden/ref_vanilla_train.npz).  Ray
counts stay at or below 66 so that the file runs in seconds; the 200-step convergence run is left to the GPU."""
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
    return np.load(os.path.join(G, 'ref_vanilla_train.npz'))


@pytest.fixture(scope='module')
def edev():
    """emulib.emulated_ops with xr_vanilla's host build added to the library handle"""
    import emulib as E
    from xrnerf_amd import _lib
    ctx = E.emulated_ops()
    dev = ctx.__enter__()
    ml = E.MultiLib(E.ALL_SOURCES + ('xr_vanilla',))
    for name, (res, args) in list(_lib.SIGNATURES.items()) + list(_lib.VANILLA_SIGNATURES.items()):
        try:
            fn = getattr(ml, name)
        except AttributeError:
            continue
        fn.restype, fn.argtypes = res, args
    _lib._lib = ml

    def check(rc, what=''):                     # error messages come from this handle's objects (emulated_ops restores the original)
        if rc != 0:
            raise _lib.XrError('%s failed (%d): %s' % (what, rc, ml.last_errors()))
    _lib.check = check
    yield dev
    ctx.__exit__(None, None, None)


@pytest.mark.parametrize('R,S', [(1, 3), (5, 7), (3, 64), (9, 100), (66, 16)])
def test_encode_and_render_against_float64(edev, R, S):
    import test_gpu_vanilla as T
    T.check_encode(edev, R, S)
    T.check_render(edev, R, S)


@pytest.mark.parametrize('S,N', [(3, 1), (5, 7), (16, 24), (64, 128), (100, 200)])
def test_resampling_inverts_the_cdf_and_merges_exactly(edev, S, N):
    import test_gpu_vanilla as T
    T.check_resample(edev, S, N)


def test_resampling_size_limits(edev):
    import test_gpu_vanilla as T
    T.check_resample_size_limits(edev)


def test_one_training_step_against_the_reference_fixture(edev, gold):
    import test_gpu_vanilla as T
    T.check_fixture_step(edev, gold, repeat=True)          # with the repeatability check: a second identical step gives the same bits


def test_training_step_issues_the_vanilla_kernels(edev, gold):
    import test_gpu_vanilla as T
    T.check_path_taken(edev, gold)


def test_config1_mlp_is_one_node_and_equals_the_layer_by_layer_graph(edev):
    import test_gpu_vanilla as T
    T.check_full_config(edev, 11)
