"""Test-set evaluation on the MI355X (xrnerf_amd/csrc/xr_eval.hip behind xrnerf_amd/evaluate.py): the SSIM map, its mean, the MSE and
the 8-bit images against tests/golden/ref_eval.npz under the bars of tests/eval_cases.py (where the bodies live), the hooks on device
frames, and evaluate_frames on a tiny HashNerfNetwork."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import eval_cases as K  # noqa: E402
from xrnerf_amd import evaluate  # noqa: E402,F401  (every check here is about this module)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from xrnerf_amd import ops
    assert ops.eval_kernels_available(), 'the library has no xr_eval entry points'
    yield torch.device('cuda')


@pytest.mark.parametrize('name', K.CASE_NAMES)
def test_fixture_cases_under_their_bars(dev, name):
    K.check_fixture(dev, name)


def test_channel_first_views_and_slices_of_wider_buffers(dev):
    K.check_views_and_slices(dev)


def test_identical_images_and_odd_values(dev):
    K.check_degenerate(dev)


def test_refusals(dev):
    K.check_refusals(dev)
    K.check_kernel_refusals(dev)
    from xrnerf_amd import _lib, ops
    x = torch.rand((1, 9, 9, 3))
    with pytest.raises(_lib.XrError):                               # host tensors handed to ops.*: there is no quiet CPU run
        ops.eval_ssim(x, x, [1.0 / 7] * 7, 49.0 / 48, 1e-4, 9e-4)
    with pytest.raises(_lib.XrError):
        ops.eval_to8b_pair(x[0], x[0])


def test_header_table_and_library_agree(dev):
    K.check_symbols()


def test_validate_hook_on_device_frames(dev):
    K.check_validate_hook(dev, 'tensor')


def test_test_hook_on_device_frames(dev):
    K.check_test_hook(dev, 'tensor')


def test_evaluate_frames_on_a_tiny_hashnerf_network(dev):
    """two 16 x 16 frames of an untrained-but-stepped HashNerfNetwork through train.render_frame, RGBA ground truths"""
    from xrnerf_amd.train import Trainer, render_frame
    tr = Trainer(dev, n_img=2, H=64, W=64)
    tr.step()
    focal = tr.data.focal * 16.0 / 64.0
    rng = np.random.default_rng(3)
    gts = [torch.from_numpy(np.concatenate([rng.uniform(0, 1, (16, 16, 3)), rng.choice([0.0, 0.5, 1.0], (16, 16, 1))], -1).astype(np.float32))
           for _ in range(2)]
    K.check_evaluate_frames(dev, lambda pose: render_frame(tr.net, pose, 16, 16, focal), [tr.data.poses[0], tr.data.poses[1]], gts)


def test_evaluate_frames_reads_back_once(dev):
    K.check_evaluate_frames(dev, *K.fixture_renderer(dev))
