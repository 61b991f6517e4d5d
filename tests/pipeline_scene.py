"""A tiny Blender-format scene and the config-shaped `data` dicts over it: the shared bodies of the SceneBaseDataset tests
(tests/test_pipeline_host.py on host tensors, tests/test_gpu_pipeline.py on the MI355X)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

H, W, N_SPLIT, N_RAND, S = 8, 6, (3, 2, 4), 8, 8          # the precrop window of an 8 x 6 frame is 4 x 2: exactly N_RAND pixels


def write_scene(root):
    """transforms_{train,val,test}.json and RGBA PNGs, H x W, N_SPLIT frames"""
    from PIL import Image
    from xrnerf_amd.datasets import pose_spherical
    rng = np.random.default_rng(0)
    for s, k in zip(('train', 'val', 'test'), N_SPLIT):
        os.makedirs(os.path.join(root, s), exist_ok=True)
        frames = []
        for i in range(k):
            Image.fromarray(rng.integers(0, 256, (H, W, 4), dtype=np.uint8), 'RGBA').save(os.path.join(root, s, 'r_%d.png' % i))
            m = pose_spherical(float(rng.uniform(-180, 180)), float(rng.uniform(-60, -10)), 4.0).astype(np.float64)
            frames.append({'file_path': './%s/r_%d' % (s, i), 'transform_matrix': m.tolist()})
        json.dump({'camera_angle_x': 0.6911112070083618, 'frames': frames}, open(os.path.join(root, 'transforms_%s.json' % s), 'w'))


def write_llff_scene(root, n=6, h=6, w=8, factor=4):
    """a forward-facing rig in LLFF's layout: poses_bounds.npy, images/ and the down-scaled images_<factor>/"""
    from PIL import Image
    rng = np.random.default_rng(3)
    os.makedirs(os.path.join(root, 'images'), exist_ok=True)
    os.makedirs(os.path.join(root, 'images_%d' % factor), exist_ok=True)
    rows = []
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, (h * factor, w * factor, 3), dtype=np.uint8)).save(os.path.join(root, 'images', 'im_%02d.png' % i))
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, 'images_%d' % factor, 'im_%02d.png' % i))
        a = rng.normal(0, 0.08, 3)
        rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
        ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
        t = rng.normal(0, 0.4, 3) + [0, 0, 0.1 * i]
        pose = np.concatenate([rx @ ry, t[:, None], np.array([[h * factor], [w * factor], [300.0]])], 1)
        rows.append(np.concatenate([pose.reshape(-1), [1.2 + rng.uniform(0, 0.3), 9.0 + rng.uniform(0, 3)]]))
    np.save(os.path.join(root, 'poses_bounds.npy'), np.array(rows))


def llff_data_cfg(root, no_ndc):
    """the `data` dict of configs/nerf/nerf_llff_base01.py at this scene's sizes (no_ndc as given: the config ships True)"""
    base = dict(dataset_type='llff', datadir=root, half_res=False, testskip=8, N_rand_per_sampler=N_RAND, llffhold=3, no_ndc=no_ndc, white_bkgd=False,
                spherify=False, shape='greek', factor=4, is_batching=True, mode='train')
    tail = lambda train: [dict(type='GetViewdirs', enable=True), dict(type='ToNDC', enable=not no_ndc), dict(type='GetBounds', enable=True),
                          dict(type='GetZvals', enable=True, lindisp=False, N_samples=S), dict(type='PerturbZvals', enable=train), dict(type='GetPts', enable=True)]
    train = [dict(type='BatchSample', enable=True, N_rand=N_RAND), dict(type='DeleteUseless', keys=['rays_rgb', 'idx']),
             dict(type='ToTensor', enable=True, keys=['rays_o', 'rays_d', 'target_s'])] + tail(True) + [dict(type='DeleteUseless', enable=True, keys=['iter_n'])]
    test = [dict(type='ToTensor', enable=True, keys=['pose']), dict(type='GetRays', enable=True), dict(type='FlattenRays', enable=True)] + tail(False) + \
           [dict(type='DeleteUseless', enable=True, keys=['pose'])]
    return dict(train=dict(type='SceneBaseDataset', cfg=dict(base), pipeline=train), val=dict(type='SceneBaseDataset', cfg=dict(base, mode='val'), pipeline=test),
                test=dict(type='SceneBaseDataset', cfg=dict(base, mode='test', testskip=0), pipeline=test))


def data_cfg(root, kind):
    """the `data` dict of configs/nerf/nerf_blender_base01.py ('blender'), of configs/nerf/nerf_llff_base01.py's batching pipeline over
    the same scene ('blender_batching') or of configs/mipnerf/mipnerf_blender.py ('mip'), at this scene's sizes"""
    batching, mip = kind == 'blender_batching', kind == 'mip'
    base = dict(dataset_type='blender', datadir=root, half_res=False, testskip=1, white_bkgd=True, is_batching=batching, mode='train',
                N_rand_per_sampler=N_RAND)
    bounds = dict(type='GetBounds', enable=True, near_new=2., far_new=6.) if mip else dict(type='GetBounds', enable=True)
    tail = [dict(type='GetViewdirs', enable=True), dict(type='ToNDC', enable=False), bounds]
    zv = lambda train: [dict(type='GetZvals', enable=True, lindisp=False, N_samples=S, randomized=train and mip)] + \
        ([] if mip else [dict(type='PerturbZvals', enable=train), dict(type='GetPts', enable=True)])
    if batching:
        train = [dict(type='BatchSample', enable=True, N_rand=N_RAND), dict(type='DeleteUseless', keys=['rays_rgb', 'idx']),
                 dict(type='ToTensor', enable=True, keys=['rays_o', 'rays_d', 'target_s'])] + tail + zv(True) + \
                [dict(type='DeleteUseless', enable=True, keys=['iter_n'])]
    else:
        train = [dict(type='Sample'), dict(type='DeleteUseless', keys=['images', 'poses', 'i_data', 'idx']),
                 dict(type='ToTensor', enable=True, keys=['pose', 'target_s']), dict(type='GetRays', enable=True, include_radius=mip),
                 dict(type='SelectRays', enable=True, sel_n=N_RAND, precrop_iters=0 if mip else 1, precrop_frac=0.5, include_radius=mip)] + \
                tail + zv(True) + [dict(type='DeleteUseless', enable=True, keys=['pose', 'iter_n'])]
    test = [dict(type='ToTensor', enable=True, keys=['pose']), dict(type='GetRays', enable=True, include_radius=mip),
            dict(type='FlattenRays', enable=True, include_radius=mip)] + tail + zv(False) + [dict(type='DeleteUseless', enable=True, keys=['pose'])]
    return dict(train=dict(type='SceneBaseDataset', cfg=dict(base), pipeline=train),
                val=dict(type='SceneBaseDataset', cfg=dict(base, mode='val'), pipeline=test),
                test=dict(type='SceneBaseDataset', cfg=dict(base, mode='test', testskip=0), pipeline=test))


def model_cfg():
    """configs/nerf/nerf_blender_base01.py's `model` with a 2-layer, 32-wide MLP"""
    mlp = dict(type='NerfMLP', skips=[4], netdepth=2, netwidth=32, netchunk=1024 * 32, output_ch=5, use_viewdirs=True,
               embedder=dict(type='BaseEmbedder', i_embed=0, multires=4, multires_dirs=2))
    return dict(type='NerfNetwork', cfg=dict(phase='train', N_importance=8, is_perturb=True, chunk=1024 * 32, bs_data='rays_o'),
                mlp=mlp, mlp_fine=dict(mlp), render=dict(type='NerfRender', white_bkgd=True, raw_noise_std=0))


def datasets(dev, root, kind):
    from xrnerf_amd import pipelines
    if not os.path.exists(os.path.join(root, 'transforms_train.json')):
        write_scene(root)
    data = data_cfg(root, kind)
    return {k: pipelines.build_dataset(dict(data[k], device=dev)) for k in ('train', 'val', 'test')}


class Runner:
    def __init__(self, model, it=0):
        self.model, self.iter = model, it


def check_train_and_validate(dev, root, kind):
    """build_dataset(cfg.data.*) -> iterate -> NerfNetwork.train_step / val_step / test_step, nothing made by hand"""
    import xrnerf_amd
    from xrnerf_amd import pipelines
    ds = datasets(dev, root, kind)
    torch.manual_seed(0)
    net = xrnerf_amd.build_network(model_cfg()).to(dev)
    pipelines.SetValPipelineHook(valset=ds['val']).before_run(Runner(net))
    hook = pipelines.PassIterHook(dataset=ds['train'])
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    seen = 0
    for it, item in enumerate(pipelines.iterate(ds['train'])):
        assert all(isinstance(v, torch.Tensor) and v.shape[0] == 1 for v in item.values()), {k: type(v) for k, v in item.items()}
        assert tuple(item['pts'].shape) == (1, N_RAND, S, 3) and item['pts'].device.type == dev.type
        out = net.train_step(item, opt)
        opt.zero_grad()
        out['loss'].backward()
        opt.step()
        assert np.isfinite(out['log_vars']['loss']) and out['num_samples'] == N_RAND
        hook.after_train_iter(Runner(net, it + 1))
        seen += 1
        if seen == 2:
            break
    assert ds['train'].iter_n == 2 and any(p.grad is not None and float(p.grad.abs().sum()) > 0 for p in net.parameters())
    ds['val'].render_poses = ds['val'].render_poses[:2]           # two of the 40 spiral poses: the frames are what is checked, not their number
    val = net.val_step(next(iter(pipelines.iterate(ds['val']))))
    assert len(val['rgbs']) == N_SPLIT[2] and val['rgbs'][0].shape == (H, W, 3) and val['gt_imgs'][0].shape == (H, W, 3)
    assert len(val['spiral_rgbs']) == 2 and np.isfinite(val['rgbs'][0]).all()
    net.phase = 'test'
    pipelines.SetValPipelineHook(valset=ds['test']).before_run(Runner(net))
    items = list(pipelines.iterate(ds['test']))
    res = net.val_step(items[1])
    assert len(items) == len(ds['test']) and res['rgb'].shape == (H, W, 3) and res['idx'] == 1 and res['gt_img'].shape == (H, W, 3)
