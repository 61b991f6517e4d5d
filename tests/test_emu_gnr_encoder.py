"""The encoder kernels of xrnerf_amd/csrc/xr_gnr_encoder.hip -- the SAME source the GPU library is built from -- compiled for the host
and run lane by lane by the HIP-on-CPU shim (tests/hip_emu): the stage checks of tests/test_gpu_gnr_encoder.py at their smallest
shapes, and HGFilter with one stack on [1, 3, 16, 16] against the restatement.  Fibers are slow: the shapes stay small."""
import contextlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def emulated_gnr_encoder():
    """emulib.emulated_ops with the host build of xr_gnr_encoder added to its MultiLib tuple and bound (GNR_ENCODER_SIGNATURES)"""
    import emulib as E
    from xrnerf_amd import _lib

    @contextlib.contextmanager
    def cm():
        with E.emulated_ops() as dev:
            ml = E.MultiLib(E.ALL_SOURCES + ('xr_gnr_encoder',))
            for name, (res, args) in list(_lib.SIGNATURES.items()) + list(_lib.GNR_ENCODER_SIGNATURES.items()):
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
            assert ops.gnr_encoder_kernels_available(), 'the host build has no xr_gnr_encoder entry points'
            yield dev
    return cm()


@pytest.fixture(scope='module')
def edev():
    with emulated_gnr_encoder() as dev:
        yield dev
    _T().write_ratios('kernels\' host build')


def _T():
    import test_gpu_gnr_encoder as T
    return T


# one row, one ragged tile, two images with a ragged second row tile; the stem; the strided layer; a 1x1 layer
EMU_CONV_CASES = [(1, 1, 1, 32, 32, 3, 1), (1, 3, 2, 64, 128, 3, 1), (2, 5, 7, 32, 32, 3, 1), (2, 12, 10, 3, 64, 7, 2), (2, 6, 8, 128, 128, 3, 2),
                  (2, 5, 7, 64, 128, 1, 1)]


@pytest.mark.parametrize('case', EMU_CONV_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_conv_against_float64_conv2d(edev, case):
    _T().check_conv(edev, case)


def test_conv_reads_and_writes_slices_of_wider_buffers(edev):
    _T().check_conv_slices(edev)


def test_conv_pads_with_zeros_after_the_norm(edev):
    _T().check_conv_padding_after_norm(edev)


def test_conv_refuses_unsupported_shapes(edev):
    _T().check_conv_refusals(edev)


@pytest.mark.parametrize('case', _T().STATS_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_group_statistics_and_apply(edev, case):
    _T().check_stats(edev, case)


@pytest.mark.parametrize('case', _T().POOL_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_avg_pool(edev, case):
    _T().check_pool(edev, case)


@pytest.mark.parametrize('case', _T().BICUBIC_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_bicubic_upsampling_with_and_without_addend(edev, case):
    _T().check_bicubic(edev, case)


def test_conv_block_against_the_restatement(edev):
    _T().check_module(edev, 'block 64->128')


def test_filter_with_one_stack(edev):
    _T().check_filter_small(edev)
