"""Mip-NeRF multiscale data on the MI355X (xrnerf_amd/csrc/xr_multiscale.hip behind xrnerf_amd/multiscale.py): the fixture of
tests/golden/ref_multiscale.npz through the kernels, the fused Compose, the converter and the dataset (tests/multiscale_cases.py holds the
bodies), and MipNerfNetwork trained, validated and tested on a tiny scene fed only by build_dataset / iterate."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import multiscale_cases as K  # noqa: E402
from xrnerf_amd import multiscale  # noqa: E402,F401  (every check here is about this module)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from xrnerf_amd import ops
    assert ops.multiscale_kernels_available(), 'the library has no xr_multiscale entry points'
    yield torch.device('cuda')


def test_every_full_frame_whole_and_in_pieces(dev):
    K.check_frames(dev)


def test_training_draw_with_and_without_randomised_z(dev):
    K.check_draw(dev)


def test_out_of_range_index_is_a_nan_ray(dev):
    K.check_out_of_range(dev)


def test_fused_compose_is_one_launch_and_the_fixture(dev):
    K.check_compose(dev)


def test_sample_on_plain_tensors(dev):
    K.check_tensor_sample(dev)


def test_refusals_and_empty_launch_nothing(dev):
    K.check_refusals(dev)
    from xrnerf_amd import _lib, ops
    t = K.table_of(torch.device('cpu'))
    with pytest.raises(_lib.XrError):                               # host tensors handed to ops.*: there is no quiet CPU run
        ops.ms_rays(t.cams, t.hw, t.prefix, t.sizes, idx=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(_lib.XrError):
        ops.ms_pyramid(torch.zeros((1, 4, 4, 4), dtype=torch.uint8), 2)


def test_h2_raises(dev):
    K.check_h2_raises(dev)


def test_pyramid_bytes_and_pixels(dev):
    K.check_pyramid(dev)


def test_converter_and_round_trip(dev, tmp_path):
    K.check_converter(dev, str(tmp_path))


def test_dataset_items_are_the_fixture(dev, tmp_path):
    ds = K.check_dataset(dev, str(tmp_path))
    assert ds['train'].native and ds['train'].table is not None and ds['train'].rays is None


def test_train_validate_and_test_hook_from_build_dataset(dev, tmp_path):
    K.check_end_to_end(dev, str(tmp_path))


def test_header_table_and_library_export_the_declared_symbols(dev):
    K.check_symbols()
