"""The instant-ngp config end to end on the MI355X: apis.train_nerf / run_nerf on a HashNerfNetwork config through
runner.NgpIterRunner -- spans of the native loop with every iteration's loss and psnr added to the log window on the device -- against
train.Trainer driven by hand, bit for bit.  The bodies are tests/ngp_runner_cases.py's; the training runs are made once and shared."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ngp_runner_cases as NC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    return NC.Runs(torch.device('cuda:0'), str(tmp_path_factory.mktemp('ngp_runner')))


def test_the_runner_is_the_benchmarked_path(runs):
    NC.check_runner_is_the_benchmarked_path(runs)


def test_the_span_plan_does_not_matter(runs):
    NC.check_span_plan_does_not_matter(runs)


def test_the_logged_psnr_is_the_references(runs):
    NC.check_psnr_is_the_references(runs)


def test_end_to_end_with_validation_checkpoints_and_resume(runs):
    NC.check_end_to_end_with_validation(runs)


def test_the_test_pass_writes_the_spiral_and_frame_0_is_render_frame(runs):
    NC.check_test_pass(runs)


def test_logged_and_unlogged_entry_points_reach_the_same_bits(runs):
    NC.check_logged_against_unlogged_entry_point(runs)
