"""BungeeNeRF behind the registry, without a GPU: the config's model dict builds, the module tree / seeded initialisation equal the
reference's (tests/golden/ref_bungee.npz), i_embed=-1 is refused, the google loader reads a directory, the host ray table equals
load_rays_bungee, and the stage loop skips the optimizer when the stage mask is empty."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
G = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(G, 'ref_bungee.npz'))


def test_config_model_dict_builds():
    import xrnerf_amd
    from xrnerf_amd import bungee
    cfg = json.load(open(os.path.join(G, 'bungee_model_cfg.json')))
    net = xrnerf_amd.build_network(cfg['model'])
    assert isinstance(net, bungee.BungeeNerfNetwork)
    assert isinstance(net.mlp, bungee.BungeeNerfMLP) and isinstance(net.render, bungee.BungeeNerfRender)
    assert net.mlp.embedder.get_embed_ch() == (63, 27) and net.N_importance == 65 and net.render.density_bias == -1


def test_keys_shapes_and_seeded_init_equal_the_reference(gold):
    import test_gpu_bungee as T
    torch.manual_seed(11)
    net = T.build('cpu', 64, 2)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold['keys']]
    for (k, v), shp in zip(sd.items(), gold['key_shapes']):
        assert list(v.shape) == [int(x) for x in shp[:v.dim()]], k
        assert np.array_equal(v.numpy(), gold['init/' + k]), k


def test_i_embed_minus_one_raises():
    from xrnerf_amd import bungee
    with pytest.raises(NotImplementedError):
        bungee.BungeeEmbedder(i_embed=-1)


def test_no_cpu_path():
    from xrnerf_amd import _lib
    import test_gpu_bungee as T
    net = T.build('cpu', 64, 0)
    with pytest.raises(_lib.XrError):
        net.mlp.run_mlp(torch.zeros(4, 90))


def test_ray_table_equals_load_rays_bungee(gold):
    from xrnerf_amd import bungee
    sc = bungee.synthetic_city(H=4, W=5, n_per_scale=2, seed=3)
    assert np.array_equal(sc['poses'], gold['poses']) and np.array_equal(sc['images'], gold['images'])
    t = bungee.BungeeRayTable(sc['H'], sc['W'], sc['focal'], sc['poses'], sc['images'], sc['scale_split'], 2,
                              perm=torch.tensor(gold['table_perm']), device='cpu')
    assert np.abs(t.rays_rgb.numpy() - gold['table_rays_rgb']).max() <= 1e-6
    assert np.abs(t.radii.numpy() - gold['table_radii']).max() <= 1e-8
    assert np.array_equal(t.scale_code.numpy(), gold['table_scale_code'])
    b = t.batch(0, 32)
    assert np.abs(b['viewdirs'].numpy() - gold['b_viewdirs']).max() <= 1e-6
    assert np.array_equal(b['scale_code'].numpy(), gold['b_scale_code'])


def test_google_loader_reads_a_directory(tmp_path):
    from PIL import Image
    from xrnerf_amd import bungee
    os.makedirs(tmp_path / 'images')
    rng = np.random.default_rng(0)
    ims = [rng.integers(0, 256, (6, 9, 3), dtype=np.uint8) for _ in range(3)]
    for i, im in enumerate(ims):
        Image.fromarray(im).save(tmp_path / 'images' / ('%03d.png' % i))
    poses = [list(np.eye(3, 5).ravel()) + [0.1, 5.0] for _ in range(3)]
    for p in poses:
        p[14] = 12.0                         # focal
    json.dump({'poses': poses, 'scene_scale': 0.01, 'scene_origin': [0, 0, -6371011], 'scale_split': [2, 1, 0]},
              open(tmp_path / 'poses_enu.json', 'w'))
    imgs, P, scale, origin, split = bungee.load_google_data(str(tmp_path), 3)
    assert imgs.shape == (3, 2, 3, 3) and P.shape == (3, 3, 5)
    assert np.allclose(imgs[1], ims[1].astype(np.float32).reshape(2, 3, 3, 3, 3).mean((1, 3)) / 255)
    assert P[0, 0, 4] == 2 and P[0, 1, 4] == 3 and P[0, 2, 4] == 4.0
    assert scale == 0.01 and split == [2, 1, 0] and origin[2] == -6371011


def test_empty_stage_mask_takes_no_optimizer_step():
    """the runner's `continue`: a stage whose loss is exactly 0 makes no backward and no step"""
    from xrnerf_amd import bungee

    class Net:
        def __init__(self):
            self.stages = []

        def train_step(self, data, optimizer, stage, rand=None):
            self.stages.append(stage)
            loss = torch.zeros((), requires_grad=True) * (0.0 if stage == 0 else 1.0) + (0.0 if stage == 0 else 2.0)
            return {'loss': loss, 'log_vars': {'loss': float(loss)}, 'num_samples': 4}

    class Opt:
        def __init__(self):
            self.calls = []

        def zero_grad(self):
            self.calls.append('zero')

        def step(self):
            self.calls.append('step')

    net, opt = Net(), Opt()
    outs = bungee.train_iteration(net, {'scale_code': torch.tensor([[[1], [2], [1]]])}, opt)
    assert net.stages == [0, 1, 2] and len(outs) == 3
    assert opt.calls == ['zero', 'step', 'zero', 'step']
