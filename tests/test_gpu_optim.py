"""xr_adam_step_list and xr_log_window_add on the MI355X (xrnerf_amd/csrc/xr_optim.hip through train.FusedAdam.step, ops.adam_step_list and
runner.LogWindow): the list kernel against xr_adam_step_multi in every bit of p, m, v and ema after three steps, the log window against
numpy float64.  The bodies are tests/optim_cases.py's."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import optim_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda')


@pytest.mark.parametrize('grad_scale', (1.0, 0.125))
@pytest.mark.parametrize('with_ema', (False, True))
@pytest.mark.parametrize('count', range(6))
def test_list_kernel_against_adam_step_multi(dev, count, with_ema, grad_scale):
    """tensor counts 1, 4, 5, capacity, capacity + 1, 2 capacity + 3"""
    K.check_fused_adam(dev, K.counts()[count], with_ema, grad_scale)
    torch.cuda.synchronize()


@pytest.mark.parametrize('which', ('p', 'g', 'm', 'v', 'ema'))
def test_one_unaligned_buffer(dev, which):
    K.check_unaligned_each(dev, which)


def test_every_length_alone(dev):
    K.check_single_lengths(dev)


def test_refusals(dev):
    K.check_refusals(dev)


def test_log_window(dev):
    K.check_log_window(dev)


def test_a_nerf_network_is_one_launch(dev):
    """the 48 tensors of a coarse + fine NerfNetwork fit one work list"""
    from xrnerf_amd import ops
    assert ops.adam_list_capacity() >= 48
