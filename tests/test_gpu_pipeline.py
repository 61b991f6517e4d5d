"""Scene data pipelines on the MI355X (xrnerf_amd/csrc/xr_pipeline.hip behind xrnerf_amd/pipelines.py): the fixture cases of
tests/golden/ref_pipeline.npz through the kernel and through Compose (tests/pipeline_cases.py holds the bodies), and NerfNetwork trained
and validated on a tiny scene fed only by build_dataset / iterate."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import pipeline_cases as K  # noqa: E402
import pipeline_scene as SC  # noqa: E402
from xrnerf_amd import pipelines  # noqa: E402,F401  (every check here is about this module)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from xrnerf_amd import ops
    assert ops.pipeline_kernels_available(), 'the library has no xr_pipeline entry points'
    yield torch.device('cuda')


@pytest.mark.parametrize('name', K.CASE_NAMES)
def test_fixture_cases_through_the_kernel(dev, name):
    K.check_fixture_kernel(dev, name)


@pytest.mark.parametrize('name', K.CASE_NAMES)
def test_fixture_cases_through_compose(dev, name):
    K.check_fixture_compose(dev, name)


@pytest.mark.parametrize('name', K.CASE_NAMES)
def test_fused_compose_equals_the_transforms_one_by_one(dev, name):
    K.check_fused_against_stepwise(dev, name)


def test_pieces_of_a_frame_concatenate_to_the_frame(dev):
    K.check_pieces(dev)


def test_nullable_outputs(dev):
    K.check_nullable_outputs(dev)


def test_refusals_and_empty_launch_nothing(dev):
    K.check_refusals_and_empty(dev)
    from xrnerf_amd import _lib, ops
    with pytest.raises(_lib.XrError):                               # host tensors handed to ops.*: there is no quiet CPU run
        ops.pipe_ray_front(6, 5, K.FX, K.FY, K.CX, K.CY, c2w=torch.eye(4)[:3])


def test_default_draws(dev):
    K.check_default_draws(dev)


def test_a_foreign_callable_inside_the_run_is_not_fused(dev):
    K.check_foreign_callable_is_not_fused(dev)


def test_header_table_and_library_export_the_declared_symbols(dev):
    K.check_symbols()


@pytest.mark.parametrize('kind', ['blender', 'blender_batching'])
def test_nerf_network_trains_and_validates_from_build_dataset(dev, tmp_path, kind):
    SC.check_train_and_validate(dev, str(tmp_path), kind)
