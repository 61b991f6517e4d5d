"""The NeuralBody modules on the host (xrnerf_amd/neuralbody.py's tensor-op path: rulebook from torch.unique / searchsorted,
index_select + matmul per tap, gather-based sampling) against the step of the reference's own modules in
tests/golden/ref_neuralbody.npz, with the bars of tests/test_gpu_neuralbody.py."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_gpu_neuralbody as T  # noqa: E402

CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'ref_neuralbody.npz'))


def test_tensor_op_step_against_the_reference_fixture(gold):
    T.check_fixture_step(CPU, gold, repeat=True, expect_kernels=False)


def test_state_dict_keys_shapes_and_registry(gold):
    T.check_state_dict_and_registry(gold)


def test_spconv_1x_checkpoint_loads_to_the_same_outputs(gold):
    net = T.network(CPU, gold)
    sd = {k: (v.permute(1, 2, 3, 4, 0).contiguous() if v.dim() == 5 else v.clone()) for k, v in net.state_dict().items()}
    assert any(v.dim() == 5 and v.shape[:3] == (3, 3, 3) for v in sd.values())
    old = T.network(CPU, gold)
    with torch.no_grad():
        for p in old.parameters():
            p.zero_()
    old.load_state_dict(sd, strict=True)
    with torch.no_grad():
        a = net.forward(T.batch(CPU, gold), True)
        b = old.forward(T.batch(CPU, gold), True)
    assert torch.equal(a['raw'], b['raw']) and torch.equal(a['rgb'], b['rgb'])


def test_render_frame_and_synthetic_frame(gold):
    from xrnerf_amd import neuralbody as NB
    T.check_render_frame(CPU, gold)
    d = NB.synthetic_frame(257, 5, n_rays=4, n_samples=3)
    assert d['latent_idx'].tolist() == [3] and d['pts'].shape == (4, 3, 3) and d['smpl_verts'].shape == (257, 3)


def test_train_step_moves_the_parameters(gold):
    from xrnerf_amd import neuralbody as NB
    net = T.network(CPU, gold)
    before = copy.deepcopy(net.state_dict())
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    out = NB.train_step(net, T.batch(CPU, gold, True), opt)
    assert np.isfinite(out['log_vars']['loss']) and abs(out['log_vars']['loss'] - float(gold['loss'])) < 1e-4
    after = net.state_dict()
    assert not torch.equal(before['smpl_conv.latent_codes.weight'], after['smpl_conv.latent_codes.weight'])
    assert not torch.equal(before['smpl_conv.xyzc_net.conv0.0.weight'], after['smpl_conv.xyzc_net.conv0.0.weight'])
    assert int(after['smpl_conv.xyzc_net.conv0.1.num_batches_tracked']) == 1
