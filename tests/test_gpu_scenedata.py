"""BungeeNeRF and KiloNeRF data on the MI355X (xrnerf_amd/bungeedata.py, xrnerf_amd/kilodata.py, xrnerf_amd/csrc/xr_bungeedata.hip): the
bodies of tests/scenedata_cases.py on the device.  Its header states the bars."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import scenedata_cases as K  # noqa: E402
from xrnerf_amd import bungeedata, kilodata  # noqa: E402,F401  (every check here is about these modules)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def test_every_training_item_of_three_stages_is_the_fixture(dev, tmp_path):
    K.check_items(dev, str(tmp_path))


def test_fused_compose_is_one_launch(dev, tmp_path):
    K.check_compose(dev, str(tmp_path))


def test_validation_frame_is_pose_rays_and_bungee_zvals(dev, tmp_path):
    K.check_frame(dev, str(tmp_path))


def test_out_of_range_indices_and_short_batches(dev, tmp_path):
    K.check_out_of_range(dev, str(tmp_path))


def test_rows_the_sort_reorders(dev):
    K.check_sort(dev)


def test_host_tensors_raise(dev):
    K.check_host_tensors_raise(dev)


def test_instant_ngp_transforms(dev):
    K.check_hash_steps(dev)


def test_set_stage_is_a_fresh_dataset(dev, tmp_path):
    K.check_set_stage(dev, str(tmp_path))


def test_kilonerf_dataset_items(dev, tmp_path):
    K.check_kilo_dataset(dev, str(tmp_path))


def test_node_dataset_items(dev, tmp_path):
    K.check_node_dataset(dev, str(tmp_path))


def test_train_and_validate_from_build_dataset(dev, tmp_path):
    K.check_end_to_end(dev, str(tmp_path))


def test_header_table_and_library_agree(dev):
    K.check_symbols()
