"""The ray sampler and the pyramid of xrnerf_amd/csrc/xr_multiscale.hip -- the SAME source the GPU library is built from -- compiled for the
host and run lane by lane by the HIP-on-CPU shim (tests/hip_emu): the bodies of tests/multiscale_cases.py through the emulated ops.  Both
builds use -ffp-contract=off, so the bits seen here are the bits the MI355X produces.  The end-to-end body trains and validates
MipNerfNetwork on the emulated Mip-NeRF kernels as well (xr_eval serves TestHook's frame metrics)."""
import contextlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import multiscale_cases as K  # noqa: E402
from xrnerf_amd import multiscale  # noqa: E402,F401  (every check here is about this module)


def emulated_multiscale():
    """emulib.emulated_ops with the host builds of xr_multiscale and xr_eval and their tables on top"""
    import emulib as E
    from xrnerf_amd import _lib

    @contextlib.contextmanager
    def cm():
        with E.emulated_ops() as dev:
            ml = E.MultiLib(E.ALL_SOURCES + ('xr_multiscale', 'xr_eval'))
            for name, (res, args) in list(_lib.SIGNATURES.items()) + list(_lib.MULTISCALE_SIGNATURES.items()) + list(_lib.EVAL_SIGNATURES.items()):
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
            assert ops.multiscale_kernels_available(), 'the host build has no xr_multiscale entry points'
            yield dev
    return cm()


@pytest.fixture(scope='module')
def edev():
    with emulated_multiscale() as dev:
        yield dev


def test_every_full_frame_whole_and_in_pieces(edev):
    K.check_frames(edev)


def test_training_draw_with_and_without_randomised_z(edev):
    K.check_draw(edev)


def test_out_of_range_index_is_a_nan_ray(edev):
    K.check_out_of_range(edev)


def test_fused_compose_is_one_launch_and_the_fixture(edev):
    K.check_compose(edev)


def test_sample_on_plain_tensors(edev):
    K.check_tensor_sample(edev)


def test_refusals_and_empty_launch_nothing(edev):
    K.check_refusals(edev)


def test_h2_raises(edev):
    K.check_h2_raises(edev)


def test_pyramid_bytes_and_pixels(edev):
    K.check_pyramid(edev)


def test_converter_and_round_trip(edev, tmp_path):
    K.check_converter(edev, str(tmp_path))


def test_dataset_items_are_the_fixture(edev, tmp_path):
    ds = K.check_dataset(edev, str(tmp_path))
    assert ds['train'].native and ds['train'].table is not None and ds['train'].rays is None      # served by the emulated kernels


def test_train_validate_and_test_hook_from_build_dataset(edev, tmp_path):
    K.check_end_to_end(edev, str(tmp_path))


def test_header_table_and_host_build_agree(edev):
    K.check_symbols()
