"""xrnerf_amd.runner / xrnerf_amd.apis on the MI355X: train_nerf / test_nerf / run_nerf end to end for vanilla NeRF and Mip-NeRF (FusedAdam
through the list kernel, the log window on the device), the Bungee stage loop against bungee.train_iteration on the reference fixture,
KiloNeRF fine-tuning through KiloNerfTrainRunner with val_step / test_step, BuildOccupancyTreeHook.  The bodies are tests/runner_cases.py's."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import runner_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda')


@pytest.mark.parametrize('kind', ['blender', 'mip'])
def test_train_test_and_run_nerf(dev, tmp_path, kind):
    RC.check_end_to_end(dev, str(tmp_path), kind)


def test_bungee_runner_iteration_equals_train_iteration(dev):
    """the fixture's first batch through BungeeNerfTrainRunner.train and through bungee.train_iteration, from the same weights and
    draws: every parameter bit for bit"""
    import test_gpu_bungee as T
    from xrnerf_amd import bungee, runner as R
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'ref_bungee.npz'))
    b = T.batch(gold, dev, 'it0_')
    b['z_vals'] = T._t(gold['it0_z_vals'], dev)
    n = int(b['scale_code'].max()) + 1
    rands = [T._t(r[:b['rays_o'].shape[0]], dev) for r in list(gold['loop_rand'])[:n]]
    nets = [T.build(dev, gold=gold) for _ in range(2)]
    opts = [torch.optim.Adam(net.parameters(), lr=5e-4, betas=(0.9, 0.999)) for net in nets]

    class Loader:
        def __iter__(self):
            return iter([T.loader(b)])

        def __len__(self):
            return 1
    runner = R.BungeeNerfTrainRunner(nets[0], optimizer=opts[0])
    runner.register_training_hooks(dict(policy='step', step=100, gamma=0.1, by_epoch=False), dict(grad_clip=None))
    runner.run([Loader()], [('train', 1)], 1, rands=rands)
    outs = bungee.train_iteration(nets[1], T.loader(b), opts[1], rands=rands)
    assert len(outs) == n and runner.iter == 1
    moved = False
    for (k, p), q in zip(nets[0].named_parameters(), nets[1].parameters()):
        assert torch.equal(p, q), k
        moved = moved or not np.array_equal(p.detach().cpu().numpy(), gold['init/' + k])
    assert moved


def test_kilonerf_runner_val_and_test_steps(dev, tmp_path):
    RC.check_kilo(dev, str(tmp_path))


def test_build_occupancy_tree_hook(dev, tmp_path):
    RC.check_occupancy_hook(dev, str(tmp_path))
