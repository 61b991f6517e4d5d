"""The Animatable-NeRF kernels of xrnerf_amd/csrc/xr_aninerf.hip -- the SAME source the GPU library is built from -- compiled for the
host and run lane by lane by the HIP-on-CPU shim (tests/hip_emu): the bodies of tests/test_gpu_aninerf.py through the emulated ops,
against the restatements (tests/aninerf_restatement.py) and the reference's steps (tests/golden/ref_aninerf.npz).  Closest-vertex
cases stay at N V <= 10^6; the repeated step, val_step and the 100-step convergence run are left to the GPU."""
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
    return np.load(os.path.join(G, 'ref_aninerf.npz'))


@pytest.fixture(scope='module')
def edev():
    """emulib.emulated_ops with the host builds of xr_aninerf (and xr_vanilla, whose encoder the modules use) added to the handle"""
    import emulib as E
    from xrnerf_amd import _lib
    ctx = E.emulated_ops()
    dev = ctx.__enter__()
    ml = E.MultiLib(E.ALL_SOURCES + ('xr_vanilla', 'xr_aninerf'))
    for name, (res, args) in list(_lib.SIGNATURES.items()) + list(_lib.VANILLA_SIGNATURES.items()) + list(_lib.ANINERF_SIGNATURES.items()):
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


def _cases():
    import test_gpu_aninerf as T
    return [(n, v) for n in T.N_SHAPES for v in T.V_SHAPES if n * v <= 10 ** 6]


@pytest.mark.parametrize('N,V', _cases())
def test_closest_vertex_matches_the_fp32_restatement_bit_for_bit(edev, N, V):
    import test_gpu_aninerf as T
    T.check_closest(edev, N, V)


def test_closest_vertex_duplicate_and_on_vertex(edev):
    import test_gpu_aninerf as T
    T.check_closest_edges(edev)


def test_selection_is_nonzero_of_the_restated_mask(edev):
    import test_gpu_aninerf as T
    T.check_select(edev)


@pytest.mark.parametrize('N', [1, 63, 65, 130, 300])
def test_blend_head_forward_and_backward(edev, N):
    import test_gpu_aninerf as T
    T.check_blend(edev, N)


@pytest.mark.parametrize('M', [1, 63, 65, 130])
def test_skinning_forward_and_backward_against_float64_autograd(edev, M):
    import test_gpu_aninerf as T
    T.check_skin(edev, M)


def test_skinning_inverts_a_one_hot_rotation(edev):
    import test_gpu_aninerf as T
    T.check_skin_one_hot(edev)


@pytest.mark.parametrize('padded', [0, 1])
@pytest.mark.parametrize('L', [0, 6, 10])
def test_encode_backward_against_float64_autograd(edev, L, padded):
    import test_gpu_aninerf as T
    T.check_encode_backward(edev, L, padded)


def test_train_pose_step_against_the_reference_fixture(edev, gold):
    import test_gpu_aninerf as T
    T.check_train_pose_step(edev, gold)


def test_novel_pose_step_against_the_reference_fixture(edev, gold):
    import test_gpu_aninerf as T
    T.check_novel_pose_step(edev, gold)


def test_training_step_issues_the_aninerf_kernels(edev, gold):
    import test_gpu_aninerf as T
    T.check_path_taken(edev, gold)


def test_state_dict_registry_and_frozen_parameters(gold):
    import test_gpu_aninerf as T
    T.check_state_dict_and_registry(gold)
