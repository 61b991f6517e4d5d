"""The evaluation kernels of xrnerf_amd/csrc/xr_eval.hip -- the SAME source the GPU library is built from -- compiled for the host and
run lane by lane by the HIP-on-CPU shim (tests/hip_emu): the bodies of tests/eval_cases.py through the emulated ops.  Both builds use
-ffp-contract=off, so the bits seen here are the bits the MI355X produces."""
import contextlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import eval_cases as K  # noqa: E402
from xrnerf_amd import evaluate  # noqa: E402,F401  (every check here is about this module)


def emulated_eval():
    """emulib.emulated_ops with the host build of xr_eval and its table on top"""
    import emulib as E
    from xrnerf_amd import _lib

    @contextlib.contextmanager
    def cm():
        with E.emulated_ops() as dev:
            ml = E.MultiLib(E.ALL_SOURCES + ('xr_eval',))
            for name, (res, args) in list(_lib.SIGNATURES.items()) + list(_lib.EVAL_SIGNATURES.items()):
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
            assert ops.eval_kernels_available(), 'the host build has no xr_eval entry points'
            yield dev
    return cm()


@pytest.fixture(scope='module')
def edev():
    with emulated_eval() as dev:
        yield dev


@pytest.mark.parametrize('name', K.CASE_NAMES)
def test_fixture_cases_under_their_bars(edev, name):
    K.check_fixture(edev, name)


def test_channel_first_views_and_slices_of_wider_buffers(edev):
    K.check_views_and_slices(edev)


def test_identical_images_and_odd_values(edev):
    K.check_degenerate(edev)


def test_refusals_launch_nothing(edev):
    K.check_refusals(edev)
    K.check_kernel_refusals(edev)


def test_header_table_and_host_build_agree(edev):
    K.check_symbols()


def test_validate_hook_on_kernel_frames(edev):
    K.check_validate_hook(edev, 'tensor')


def test_test_hook_on_kernel_frames(edev):
    K.check_test_hook(edev, 'tensor')


def test_evaluate_frames_reads_back_once(edev):
    K.check_evaluate_frames(edev, *K.fixture_renderer(edev))


def test_kernels_and_tensor_ops_give_the_same_map(edev):
    """the tensor-op path performs the kernels' operations in the kernels' order: the same S, bit for bit"""
    import torch
    for name in ('7x7', '11x11g', '37x70'):
        c = K.case(name)
        x, y = torch.from_numpy(c['rgb']), torch.from_numpy(c['gt'])
        taps, cov = evaluate.window(7, c['gauss'])
        C1, C2 = (0.01 * K.DATA_RANGE) ** 2, (0.03 * K.DATA_RANGE) ** 2
        _, smap = evaluate._ssim_tensor_ops(x, y, taps, cov, C1, C2)
        _, got = evaluate.calculate_ssim(x, y, data_range=K.DATA_RANGE, gaussian_weights=c['gauss'], full=True)
        K.same_bits(got, smap, '%s: kernels against tensor ops' % name)
