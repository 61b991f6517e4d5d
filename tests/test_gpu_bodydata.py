"""ZJU-MoCap / H36M human data on the MI355X (xrnerf_amd/csrc/xr_bodydata.hip behind xrnerf_amd/bodydata.py): the fixture of
tests/golden/ref_bodydata.npz through the kernels, the fused Compose and the datasets (tests/bodydata_cases.py holds the bodies; every
kernel is run twice and its bytes compared), and NeuralBodyNetwork / AniNeRFNetwork fed only by build_dataset / iterate."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import bodydata_cases as K  # noqa: E402
from xrnerf_amd import bodydata  # noqa: E402,F401  (every check here is about this module)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from xrnerf_amd import ops
    assert ops.bodydata_kernels_available(), 'the library has no xr_body entry points'
    yield torch.device('cuda')


def test_prepared_picture_against_the_specification(dev):
    K.check_prepare(dev)


def test_silhouette_lists_are_the_specification(dev):
    K.check_lists(dev)


def test_training_items_are_the_reference_bit_for_bit(dev):
    K.check_train(dev)


def test_item_that_exhausts_eight_rounds(dev):
    K.check_short(dev)


def test_empty_list_raises_and_launches_nothing(dev):
    K.check_empty(dev)
    from xrnerf_amd import _lib, ops
    s = K.scene('small')
    pic = K.picture(torch.device('cpu'), s)
    with pytest.raises(_lib.XrError):                               # host tensors handed to ops.*: there is no quiet CPU run
        ops.body_frame(pic.cam(s['bounds']), pic.H, pic.W, pic.img)
    with pytest.raises(_lib.XrError):
        ops.body_prepare(torch.zeros((4, 4, 3), dtype=torch.uint8), torch.zeros((4, 4), dtype=torch.uint8), s['K'], [0] * 5, 1, False)


def test_frames_are_the_reference_bit_for_bit(dev):
    K.check_frames(dev)


def test_fused_compose_launches_and_the_fixture(dev):
    K.check_compose(dev)


def test_dataset_items_from_the_frame_store(dev, tmp_path):
    ds = K.check_dataset(dev, str(tmp_path))
    assert ds['train'].store.native and ds['train'].store.prepared == 3


def test_train_and_validate_from_build_dataset(dev, tmp_path):
    K.check_end_to_end(dev, str(tmp_path))


def test_header_table_and_library_export_the_declared_symbols(dev):
    K.check_symbols()
