"""The NeuralBody kernels of xrnerf_amd/csrc/xr_neuralbody.hip -- the SAME source the GPU library is built from -- compiled for the host
and run lane by lane by the HIP-on-CPU shim (tests/hip_emu): the bodies of tests/test_gpu_neuralbody.py through the emulated ops,
against the float64 dense restatement (tests/neuralbody_restatement.py) and the reference's step (tests/golden/ref_neuralbody.npz).
The repeated fixture step is left to the GPU (the emulated MFMA is a rendezvous of 64 fibers per instruction)."""
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
    return np.load(os.path.join(G, 'ref_neuralbody.npz'))


@pytest.fixture(scope='module')
def edev():
    """emulib.emulated_ops with the host builds of xr_neuralbody (and xr_vanilla / xr_aninerf, whose encoder the MLP uses) added"""
    import emulib as E
    from xrnerf_amd import _lib
    ctx = E.emulated_ops()
    dev = ctx.__enter__()
    ml = E.MultiLib(E.ALL_SOURCES + ('xr_vanilla', 'xr_aninerf', 'xr_neuralbody'))
    for name, (res, args) in list(_lib.SIGNATURES.items()) + list(_lib.VANILLA_SIGNATURES.items()) + \
            list(_lib.ANINERF_SIGNATURES.items()) + list(_lib.NEURALBODY_SIGNATURES.items()):
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
    ctx.__exit__(None, None, None)


def _T():
    import test_gpu_neuralbody as T
    return T


@pytest.mark.parametrize('out_sh', _T().STRUCT_SH)
@pytest.mark.parametrize('V', _T().STRUCT_V)
def test_structure_matches_the_restatement_exactly(edev, V, out_sh):
    _T().check_structure(edev, V, out_sh)


def test_structure_with_two_scan_sweeps_matches_the_restatement_exactly(edev):
    _T().check_structure(edev, *_T().STRUCT_TWO_SWEEPS)


def test_bad_out_sh_and_volume_over_the_cap_launch_nothing(edev):
    _T().check_structure_errors(edev)


def test_no_vertices_give_empty_levels(edev):
    _T().check_no_vertices(edev)


@pytest.mark.parametrize('N', _T().CONV_N)
@pytest.mark.parametrize('cin,cout,strided', _T().CONV_LAYERS)
def test_convolution_forward_and_gradients_against_float64(edev, cin, cout, strided, N):
    _T().check_conv(edev, cin, cout, strided, N)


@pytest.mark.parametrize('strided_out', [False, True])
@pytest.mark.parametrize('N', _T().SAMPLE_N)
def test_sampling_forward_and_row_gradients_against_float64(edev, N, strided_out):
    _T().check_sampling(edev, N, strided_out)


def test_sampling_edges_and_exact_zeros(edev):
    _T().check_sampling_edges(edev)


def test_fixture_step_against_the_reference_and_its_launch_counts(edev, gold):
    """one emulated step serves both checks (40 s of emulated MFMA each otherwise)"""
    net, out, fwd, bwd = _T().counted_step(edev, gold)
    _T().assert_launch_counts(fwd, bwd)
    _T().check_fixture_step(edev, gold, repeat=False, first=(net, out))


def test_render_frame_runs_the_sparse_network_once(edev, gold):
    _T().check_render_frame(edev, gold)
