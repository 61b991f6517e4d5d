"""The GeneBody kernels of xrnerf_amd/csrc/xr_genebody.hip -- the SAME source the GPU library is built from -- compiled for the host and
run lane by lane by the HIP-on-CPU shim (tests/hip_emu): the bodies of tests/genebody_cases.py through the emulated ops.  Both builds use
-ffp-contract=off and explicitly rounded single operations, so the bits seen here are the bits the MI355X produces."""
import contextlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import genebody_cases as K  # noqa: E402
from xrnerf_amd import genebody  # noqa: E402,F401  (every check here is about this module)


def emulated_genebody():
    """emulib.emulated_ops with the host build of xr_genebody and its table on top"""
    import emulib as E
    from xrnerf_amd import _lib

    @contextlib.contextmanager
    def cm():
        with E.emulated_ops() as dev:
            ml = E.MultiLib(E.ALL_SOURCES + ('xr_genebody',))
            for name, (res, args) in list(_lib.SIGNATURES.items()) + list(_lib.GENEBODY_SIGNATURES.items()):
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
            assert ops.genebody_kernels_available(), 'the host build has no xr_gb entry points'
            yield dev
    return cm()


@pytest.fixture(scope='module')
def edev():
    with emulated_genebody() as dev:
        yield dev


def test_crop_boxes_are_the_specification(edev):
    K.check_crop_box(edev)


def test_resized_planes_are_the_specification(edev):
    K.check_resize(edev)


def test_views_in_their_roles_and_camera_rows(edev):
    K.check_assemble_and_calib(edev)


def test_dataset_items_are_the_reference_items(edev, tmp_path):
    K.check_dataset(edev, str(tmp_path))


def test_store_prepares_more_views_than_one_launch_takes(edev):
    K.check_store_chunks(edev)


def test_prepare_data_takes_the_batch_as_it_is(edev, tmp_path):
    K.check_prepare_data(edev, str(tmp_path))


def test_refused_arguments_launch_nothing(edev):
    import torch
    from xrnerf_amd import _lib, ops
    with pytest.raises(_lib.XrError):
        ops.gb_crop_box([np.zeros((4, 4), np.uint8)] * (ops.GB_MAX_VIEWS + 1), edev)
    with pytest.raises(_lib.XrError):
        ops.gb_crop_box((torch.zeros(16, dtype=torch.uint8), [(8, 4, 4)]))             # the mask leaves its buffer
    z = torch.zeros((4, 4, 3), dtype=torch.uint8)
    with pytest.raises(_lib.XrError):
        ops.gb_assemble([z], [torch.zeros((4, 4), dtype=torch.uint8)], None, 2, 4, False)   # num_views above V


def test_header_table_and_host_build_agree(edev):
    K.check_symbols()
