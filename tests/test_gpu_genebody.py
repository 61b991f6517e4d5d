"""GeneBody data on the MI355X (xrnerf_amd/csrc/xr_genebody.hip behind xrnerf_amd/genebody.py): the fixture of
tests/golden/ref_genebody.npz through the four kernels and through build_dataset (tests/genebody_cases.py holds the bodies; every kernel is
run twice and its bytes compared), the view store's cache hit and eviction, and GnrNetwork.prepare_data fed by iterate(dataset)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import genebody_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from xrnerf_amd import ops
    assert ops.genebody_kernels_available(), 'the library has no xr_gb entry points'
    yield torch.device('cuda:0')


def test_build_dataset_knows_the_genebody_dataset(dev, tmp_path):
    """KeyError before xrnerf_amd/genebody.py existed: DATASETS held nothing for GNR"""
    from xrnerf_amd.pipelines import build_dataset
    opt = K.write_tree(str(tmp_path))
    for phase in ('train', 'val', 'test'):
        ds = build_dataset(dict(type='GeneBodyDataset', opt=opt, phase=phase, pipeline=[]))
        assert ds.device.type == 'cuda' and len(ds) > 0


def test_crop_boxes_are_the_specification(dev):
    K.check_crop_box(dev)


def test_resized_planes_are_the_specification(dev):
    K.check_resize(dev)


def test_views_in_their_roles_and_camera_rows(dev):
    K.check_assemble_and_calib(dev)


def test_dataset_items_are_the_reference_items(dev, tmp_path):
    """train and evaluation items equal to the recorded reference items; a second pass and a pass under a budget of one view repeat the bits"""
    K.check_dataset(dev, str(tmp_path))


def test_store_prepares_more_views_than_one_launch_takes(dev):
    K.check_store_chunks(dev)


def test_prepare_data_takes_the_batch_as_it_is(dev, tmp_path):
    K.check_prepare_data(dev, str(tmp_path))


def test_host_tensors_are_refused(dev):
    from xrnerf_amd import _lib, ops
    with pytest.raises(_lib.XrError):                               # host tensors handed to ops.*: there is no quiet CPU run
        ops.gb_crop_box([np.ones((8, 8), np.uint8)], 'cpu')
    with pytest.raises(_lib.XrError):
        ops.gb_assemble([torch.zeros((4, 4, 3), dtype=torch.uint8)], [torch.zeros((4, 4), dtype=torch.uint8)], None, 0, 4, False)


def test_header_table_and_library_export_the_declared_symbols(dev):
    K.check_symbols()
