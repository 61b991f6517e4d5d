"""xrnerf_amd/csrc/xr_bungeedata.hip and xr_bungee.hip -- the SAME sources the GPU library is built from -- compiled for the host and run
lane by lane by the HIP-on-CPU shim (tests/hip_emu): the bodies of tests/scenedata_cases.py through the emulated ops.  Both builds use
-ffp-contract=off and correctly rounded division and square root, so the bits seen here are the bits the MI355X produces (checked at
360 x 640 as well: tools/microbench_scenedata.py compares the device's frame with the same IEEE lines in numpy)."""
import contextlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import scenedata_cases as K  # noqa: E402
from xrnerf_amd import bungeedata, kilodata  # noqa: E402,F401  (every check here is about these modules)


def emulated_scenedata():
    """emulib.emulated_ops with the host builds of xr_bungee, xr_bungeedata and xr_pipeline and their tables on top"""
    import emulib as E
    from xrnerf_amd import _lib

    @contextlib.contextmanager
    def cm():
        with E.emulated_ops() as dev:
            ml = E.MultiLib(E.ALL_SOURCES + ('xr_bungee', 'xr_bungeedata', 'xr_pipeline'))
            for name, (res, args) in list(_lib.SIGNATURES.items()) + list(_lib.BUNGEE_SIGNATURES.items()) + list(_lib.BUNGEEDATA_SIGNATURES.items()) + \
                    list(_lib.PIPELINE_SIGNATURES.items()):
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
            assert ops.bungeedata_kernels_available(), 'the host build has no xr_bungeedata entry points'
            yield dev
    return cm()


@pytest.fixture(scope='module')
def edev():
    with emulated_scenedata() as dev:
        yield dev


def test_every_training_item_of_three_stages_is_the_fixture(edev, tmp_path):
    K.check_items(edev, str(tmp_path))


def test_fused_compose_is_one_launch(edev, tmp_path):
    K.check_compose(edev, str(tmp_path))


def test_validation_frame_is_pose_rays_and_bungee_zvals(edev, tmp_path):
    K.check_frame(edev, str(tmp_path))


def test_out_of_range_indices_and_short_batches(edev, tmp_path):
    K.check_out_of_range(edev, str(tmp_path))


def test_rows_the_sort_reorders(edev):
    K.check_sort(edev)


def test_instant_ngp_transforms(edev):
    K.check_hash_steps(edev)


def test_set_stage_is_a_fresh_dataset(edev, tmp_path):
    K.check_set_stage(edev, str(tmp_path))


def test_kilonerf_dataset_items(edev, tmp_path):
    K.check_kilo_dataset(edev, str(tmp_path))


def test_node_dataset_items(edev, tmp_path):
    K.check_node_dataset(edev, str(tmp_path))


def test_train_and_validate_from_build_dataset(edev, tmp_path):
    K.check_end_to_end(edev, str(tmp_path))


def test_header_table_and_host_build_agree(edev):
    K.check_symbols()
