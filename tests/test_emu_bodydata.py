"""The human-data kernels of xrnerf_amd/csrc/xr_bodydata.hip -- the SAME source the GPU library is built from -- compiled for the host and
run lane by lane by the HIP-on-CPU shim (tests/hip_emu): the bodies of tests/bodydata_cases.py through the emulated ops.  Both builds use
-ffp-contract=off, so the bits seen here are the bits the MI355X produces.  The end-to-end body trains NeuralBodyNetwork and
AniNeRFNetwork on the emulated kernels from build_dataset / iterate."""
import contextlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import bodydata_cases as K  # noqa: E402
from xrnerf_amd import bodydata  # noqa: E402,F401  (every check here is about this module)


def emulated_bodydata():
    """emulib.emulated_ops with the host builds of xr_bodydata and of the two networks' families and their tables on top"""
    import emulib as E
    from xrnerf_amd import _lib

    @contextlib.contextmanager
    def cm():
        with E.emulated_ops() as dev:
            ml = E.MultiLib(E.ALL_SOURCES + ('xr_bodydata', 'xr_vanilla', 'xr_aninerf', 'xr_neuralbody'))
            for name, (res, args) in list(_lib.SIGNATURES.items()) + list(_lib.BODYDATA_SIGNATURES.items()) + list(_lib.VANILLA_SIGNATURES.items()) + \
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
            from xrnerf_amd import ops
            assert ops.bodydata_kernels_available(), 'the host build has no xr_body entry points'
            yield dev
    return cm()


@pytest.fixture(scope='module')
def edev():
    with emulated_bodydata() as dev:
        yield dev


def test_prepared_picture_against_the_specification(edev):
    K.check_prepare(edev)


def test_silhouette_lists_are_the_specification(edev):
    K.check_lists(edev)


def test_training_items_are_the_reference_bit_for_bit(edev):
    K.check_train(edev)


def test_item_that_exhausts_eight_rounds(edev):
    K.check_short(edev)


def test_empty_list_raises_and_launches_nothing(edev):
    K.check_empty(edev)


def test_frames_are_the_reference_bit_for_bit(edev):
    K.check_frames(edev)


def test_fused_compose_launches_and_the_fixture(edev):
    K.check_compose(edev)


def test_dataset_items_from_the_frame_store(edev, tmp_path):
    ds = K.check_dataset(edev, str(tmp_path))
    assert ds['train'].store.native and ds['train'].store.prepared == 3


def test_train_and_validate_from_build_dataset(edev, tmp_path):
    K.check_end_to_end(edev, str(tmp_path))


def test_header_table_and_host_build_agree(edev):
    K.check_symbols()
