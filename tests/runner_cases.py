"""The bodies of the runner / apis checks, shared by the host tier (tests/test_runner_host.py) and the GPU tier (tests/test_gpu_runner.py).

The end-to-end scene is the tiny Blender scene of tests/pipeline_scene.py, written by its own write_scene, with ONE change: frames are
8 x 7, not 8 x 6.  ValidateHook and TestHook measure SSIM with a 7 x 7 window, and a frame narrower than the window is refused
('win_size exceeds image extent.', as skimage refuses it for the reference's hooks): on 8 x 6 frames neither this project's hooks nor
the reference's can write anything (test_the_hooks_refuse_a_frame_narrower_than_the_ssim_window holds that).  7 is the smallest width
they take; the precrop window stays 4 x 2 = N_RAND pixels."""
import contextlib
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import pipeline_scene as SC  # noqa: E402

W_FRAME = 7
DATANAME = 'tiny'
MIP_LR = dict(lr_init=5e-4, lr_final=5e-6, max_steps=4, lr_delay_steps=2, lr_delay_mult=0.01)
MIP_LR_GOLD = os.path.join(G, 'ref_mip_lr.json')
MIP_LR_CASES = [dict(lr_init=5e-4, lr_final=5e-6, max_steps=1000000, lr_delay_steps=2500, lr_delay_mult=0.01),   # configs/mipnerf/*.py
                dict(lr_init=1e-3, lr_final=1e-5, max_steps=200, lr_delay_steps=0, lr_delay_mult=1)]
MIP_LR_ITERS = (0, 1, 1250, 2500, 500000, 2000000)

# the reference configs' hook lists, verbatim (configs/nerf/nerf_blender_base01.py:27-38, configs/mipnerf/mipnerf_blender.py:30-51)
NERF_TRAIN_HOOKS = [
    dict(type='SetValPipelineHook', params=dict(), variables=dict(valset='valset')),
    dict(type='ValidateHook', params=dict(save_folder='visualizations/validation')),
    dict(type='SaveSpiralHook', params=dict(save_folder='visualizations/spiral')),
    dict(type='PassIterHook', params=dict()),
    dict(type='OccupationHook', params=dict()),
]
MIP_TRAIN_HOOKS = [
    dict(type='SetValPipelineHook', params=dict(), variables=dict(valset='valset')),
    dict(type='ValidateHook', params=dict(save_folder='val_results/')),
    dict(type='SaveSpiralHook', params=dict(save_folder='spiral_results/')),
    dict(type='PassIterHook', params=dict()),
    dict(type='OccupationHook', params=dict()),
]
TEST_HOOKS = [
    dict(type='SetValPipelineHook', params=dict(), variables=dict(valset='testset')),
    dict(type='TestHook', params=dict(ndown=1, dump_json=True, save_img=True, save_folder='test_results/'), variables=dict()),
]


@contextlib.contextmanager
def scene_width(w=W_FRAME):
    """pipeline_scene's module, unedited, with its frame width set for the duration"""
    old = SC.W
    SC.W = w
    try:
        yield
    finally:
        SC.W = old


@contextlib.contextmanager
def two_spiral_poses():
    """apis.build_dataloader with the validation set's 40 spiral poses cut to two: the frames are what is checked, not their number"""
    from xrnerf_amd import apis
    orig = apis.build_dataloader

    def build(cfg, mode='train'):
        loader, ds = orig(cfg, mode)
        if mode == 'val':
            ds.render_poses = ds.render_poses[:2]
        return loader, ds
    apis.build_dataloader = build
    try:
        yield
    finally:
        apis.build_dataloader = orig


def mip_model_cfg():
    """configs/mipnerf/mipnerf_blender.py's `model` (tests/golden/mip_model_cfg.json, use_multiscale off) with a 3 x 32 MLP"""
    model = copy.deepcopy(json.load(open(os.path.join(G, 'mip_model_cfg.json')))['model'])
    model['mlp'].update(netdepth=3, netwidth=32, skips=[1])
    model['cfg'].update(use_multiscale=False, phase='train')
    return model


def config_dict(root, work_dir, kind, dev):
    """the names of configs/nerf/nerf_blender_base01.py ('blender') or configs/mipnerf/mipnerf_blender.py ('mip') at the scene's sizes:
    max_iters 4, workflow [('train', 2), ('val', 1)], checkpoints and log lines every 2 iterations"""
    mip = kind == 'mip'
    cfg = dict(
        method='mip_nerf' if mip else 'nerf',
        optimizer=dict(type='Adam', lr=5e-4) if mip else dict(type='Adam', lr=5e-4, betas=(0.9, 0.999)),
        optimizer_config=dict(grad_clip=None), max_iters=4,
        lr_config=dict(policy='Mip', by_epoch=False, **MIP_LR) if mip else dict(policy='step', step=500 * 1000, gamma=0.1, by_epoch=False),
        checkpoint_config=dict(interval=2, by_epoch=False), log_level='INFO',
        log_config=dict(interval=2, by_epoch=False, hooks=[dict(type='TextLoggerHook')]),
        workflow=[('train', 2), ('val', 1)], train_hooks=copy.deepcopy(MIP_TRAIN_HOOKS if mip else NERF_TRAIN_HOOKS),
        test_hooks=copy.deepcopy(TEST_HOOKS), train_runner=dict(type='NerfTrainRunner'), test_runner=dict(type='NerfTestRunner'),
        num_gpus=1, distributed=False, work_dir=work_dir, load_from=os.path.join(work_dir, 'latest.pth'),
        model=mip_model_cfg() if mip else SC.model_cfg(), device=str(dev))
    data = SC.data_cfg(root, kind)
    cfg['data'] = dict(data, train_loader=dict(batch_size=1, num_workers=0), val_loader=dict(batch_size=1, num_workers=0),
                       test_loader=dict(batch_size=1, num_workers=0))
    return cfg


def write_config_files(folder, cfg):
    """a config FILE as the reference writes them: the schedule in a base file named by `_base_`, the rest on top, with modules imported
    and a helper defined at module level (neither may reach the cfg)"""
    os.makedirs(folder, exist_ok=True)
    base_keys = ('optimizer', 'optimizer_config', 'lr_config', 'checkpoint_config', 'log_level', 'log_config')
    with open(os.path.join(folder, 'schedule.py'), 'w') as f:
        for k in base_keys:
            f.write('%s = %r\n' % (k, cfg[k]))
        f.write("log_config['interval'] = 1000\nmax_iters = 123\n")                 # overridden by the child
    path = os.path.join(folder, 'tiny_config.py')
    with open(path, 'w') as f:
        f.write("_base_ = ['./schedule.py']\nimport os\nfrom datetime import datetime\n\n\ndef helper():\n    return 1\n\n\n")
        for k, v in cfg.items():
            if k not in base_keys:
                f.write('%s = %r\n' % (k, v))
        f.write("log_config = dict(interval=%d)\n" % cfg['log_config']['interval'])
    return path


def prepare(tmp, kind, dev):
    """scene and cfg dict with '#DATANAME#' in the data and work directories -> (cfg dict, resolved work_dir)"""
    root = os.path.join(tmp, 'scene_' + DATANAME)
    with scene_width():
        SC.write_scene(root)
    cfg = config_dict(os.path.join(tmp, 'scene_#DATANAME#'), os.path.join(tmp, 'work_#DATANAME#'), kind, dev)
    return cfg, os.path.join(tmp, 'work_' + DATANAME)


def pngs(folder):
    return sorted(f for f in os.listdir(folder) if f.endswith('.png')) if os.path.isdir(folder) else []


def check_training_outputs(runner, work, kind, max_iters=4):
    from PIL import Image
    mip = kind == 'mip'
    assert runner.iter == max_iters
    assert os.path.isfile(os.path.join(work, 'iter_2.pth')) and os.path.isfile(os.path.join(work, 'iter_4.pth'))
    assert os.readlink(os.path.join(work, 'latest.pth')) == 'iter_4.pth'
    ckpt = torch.load(os.path.join(work, 'iter_4.pth'), map_location='cpu', weights_only=False)
    assert sorted(ckpt) == ['meta', 'optimizer', 'state_dict'] and ckpt['meta']['iter'] == 4
    assert list(ckpt['state_dict']) == list(runner.model.state_dict())
    val, spiral = ('val_results/', 'spiral_results/') if mip else ('visualizations/validation', 'visualizations/spiral')
    for it in (2, 4):
        frames = pngs(os.path.join(work, val, str(it)))
        assert frames == ['%03d.png' % i for i in range(SC.N_SPLIT[2])], frames
        assert Image.open(os.path.join(work, val, str(it), '000.png')).size == (2 * W_FRAME, SC.H)          # prediction beside ground truth
        for name in ('%d_rgb' % it, '%d_disp' % it):
            assert pngs(os.path.join(work, spiral, name)) == ['000.png', '001.png'], (name, os.listdir(os.path.join(work, spiral)))
        assert Image.open(os.path.join(work, spiral, '%d_rgb' % it, '001.png')).size == (W_FRAME, SC.H)
        from xrnerf_amd import evaluate
        assert os.path.isfile(os.path.join(work, spiral, '%d_rgb.mp4' % it)) == (evaluate.imageio_module() is not None)
    assert [h[0] for h in runner.log_history] == [2, 4]
    for _, lr, avg in runner.log_history:
        assert np.isfinite(avg['loss']) and avg['loss'] > 0 and np.isfinite(avg['psnr']), avg
    if mip:
        from xrnerf_amd.runner import MipLrUpdaterHook

        class At:
            def __init__(self, it):
                self.iter = it
        hook = MipLrUpdaterHook(by_epoch=False, **MIP_LR)
        assert [h[1] for h in runner.log_history] == [float(hook.get_lr(At(1), 5e-4)), float(hook.get_lr(At(3), 5e-4))]
        assert sorted(runner.log_history[0][2]) == ['loss', 'loss_coarse', 'loss_fine', 'psnr']
    else:
        assert [h[1] for h in runner.log_history] == [5e-4, 5e-4]
    assert runner.data_loader is not None and os.path.isdir(os.path.join(work, 'delete_me_to_stop'))


def check_test_outputs(runner, work):
    folder = os.path.join(work, 'test_results/')
    assert pngs(folder) == ['%03d.png' % i for i in range(SC.N_SPLIT[2])]
    res = json.load(open(os.path.join(folder, 'test_results.json')))
    assert sorted(res) == ['psnrs', 'results', 'ssims'] and len(res['psnrs']['0']) == SC.N_SPLIT[2] and np.isfinite(res['psnrs']['0']).all()
    assert runner.epoch == 1


def check_end_to_end(dev, tmp, kind, command_line=True):
    """train_nerf (checkpoints, validation PNGs, spiral frames, a finite logged loss), resume, test_nerf, and -- with `command_line` --
    the same through run_nerf(parse_args(...)) on a config file, and the refusals"""
    import pytest
    from xrnerf_amd import apis
    from xrnerf_amd.builder import ConfigDict
    cfg_dict, work = prepare(tmp, kind, dev)
    torch.manual_seed(0)
    with two_spiral_poses():
        cfg = apis.update_config(DATANAME, ConfigDict.wrap(copy.deepcopy(cfg_dict)))
        assert cfg.work_dir == work and cfg.data.train.cfg.datadir.endswith('scene_' + DATANAME)
        runner = apis.train_nerf(cfg)
        check_training_outputs(runner, work, kind)
        on_gpu = dev.type == 'cuda'
        assert type(runner.optimizer).__name__ == ('FusedAdam' if on_gpu else 'Adam')
        trained = {k: v.detach().cpu().clone() for k, v in runner.model.state_dict().items()}
        # resume from iter_2.pth: iteration, optimiser state and two more iterations
        cfg2 = apis.update_config(DATANAME, ConfigDict.wrap(copy.deepcopy(cfg_dict)))
        cfg2.resume_from = os.path.join(work, 'iter_2.pth')
        resumed = apis.train_nerf(cfg2)
        assert resumed.iter == 4 and [h[0] for h in resumed.log_history] == [4]
        steps = [int(st['step']) for st in resumed.optimizer.state.values()]
        assert steps and set(steps) == {4}, steps
        # test_nerf on the checkpoint train_nerf left
        cfg3 = apis.update_config(DATANAME, ConfigDict.wrap(copy.deepcopy(cfg_dict)))
        cfg3['model']['cfg']['phase'] = 'test'
        tested = apis.test_nerf(cfg3)
        check_test_outputs(tested, work)
        loaded = tested.model.state_dict()
        assert all(torch.equal(loaded[k].cpu(), torch.load(os.path.join(work, 'latest.pth'), map_location='cpu', weights_only=False)['state_dict'][k])
                   for k in list(trained)[:3])
        if not command_line:
            return
        # the same through the command line's path, on a config file
        cfg_dict['work_dir'] = os.path.join(tmp, 'cli_#DATANAME#')
        cfg_dict['load_from'] = os.path.join(cfg_dict['work_dir'], 'latest.pth')
        path = write_config_files(os.path.join(tmp, 'configs'), cfg_dict)
        loaded_cfg = apis.load_config(path)
        assert 'os' not in loaded_cfg and 'helper' not in loaded_cfg and 'datetime' not in loaded_cfg and '_base_' not in loaded_cfg
        assert loaded_cfg.max_iters == 4 and loaded_cfg.log_config == dict(cfg_dict['log_config']) and loaded_cfg.workflow == [('train', 2), ('val', 1)]
        cli_work = os.path.join(tmp, 'cli_' + DATANAME)
        runner = apis.run_nerf(apis.parse_args(['--config', path, '--dataname', DATANAME]))
        check_training_outputs(runner, cli_work, kind)
        tested = apis.run_nerf(apis.parse_args(['--config', path, '--dataname', DATANAME, '--test_only', '--load_from', 'iter_2.pth']))
        assert tested.model.phase == 'test'
        check_test_outputs(tested, cli_work)
        # refusals, each naming what it refuses
        bad = apis.update_config(DATANAME, ConfigDict.wrap(copy.deepcopy(cfg_dict)))
        bad.distributed = True
        with pytest.raises(NotImplementedError, match='distributed'):
            apis.train_nerf(bad)
        with pytest.raises(NotImplementedError, match='distributed'):
            apis.test_nerf(bad)
        bad = apis.update_config(DATANAME, ConfigDict.wrap(copy.deepcopy(cfg_dict)))
        bad.model = ConfigDict(type='HashNerfNetwork')
        with pytest.raises(NotImplementedError, match='instant-ngp'):
            apis.train_nerf(bad)
        bad = apis.update_config(DATANAME, ConfigDict.wrap(copy.deepcopy(cfg_dict)))
        bad.optimizer_config = ConfigDict(grad_clip=dict(max_norm=1.0))
        with pytest.raises(NotImplementedError, match='grad_clip'):
            apis.train_nerf(bad)
        bad = apis.update_config(DATANAME, ConfigDict.wrap(copy.deepcopy(cfg_dict)))
        bad.log_config = ConfigDict.wrap(dict(interval=2, hooks=[dict(type='TensorboardLoggerHook')]))
        with pytest.raises(NotImplementedError, match='TensorboardLoggerHook'):
            apis.train_nerf(bad)


# ------------------------------------------------------------------------------------------ the reference's MipLrUpdaterHook
def reference_mip_lr_class():
    """the reference's own MipLrUpdaterHook, its file imported unmodified on stubs of mmcv's hook base classes and imageio"""
    import importlib.util
    import types
    sys.path.insert(0, G)
    import ref_import
    ref_import._stub_mmcv()

    class Hook:
        pass

    class LrUpdaterHook(Hook):
        def __init__(self, by_epoch=True, **kwargs):
            self.by_epoch = by_epoch
    hooks = types.ModuleType('mmcv.runner.hooks')
    hooks.HOOKS, hooks.Hook = sys.modules['mmcv.utils'].Registry('hook'), Hook
    lr = types.ModuleType('mmcv.runner.hooks.lr_updater')
    lr.LrUpdaterHook = LrUpdaterHook
    saved = {k: sys.modules.get(k) for k in ('mmcv.runner.hooks', 'mmcv.runner.hooks.lr_updater', 'imageio')}
    sys.modules.update({'mmcv.runner.hooks': hooks, 'mmcv.runner.hooks.lr_updater': lr})
    if saved['imageio'] is None:
        sys.modules['imageio'] = types.ModuleType('imageio')
    try:
        spec = importlib.util.spec_from_file_location('ref_train_hooks', os.path.join(ref_import.REF, 'xrnerf', 'core', 'hooks', 'train_hooks.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod.MipLrUpdaterHook


class _At:
    def __init__(self, it):
        self.iter, self.epoch = it, 0


def mip_lr_values(cls):
    return [[float(cls(by_epoch=False, **case).get_lr(_At(it), 5e-4)) for it in MIP_LR_ITERS] for case in MIP_LR_CASES]


# ------------------------------------------------------------------------------------------ KiloNeRF
def kilo_scene(dev):
    """kilo.synthetic_scene at [16, 16, 16] -- one network, the smallest resolution -- and 8 x 8 poses around it"""
    from xrnerf_amd import kilo
    mlp, gmin, gmax = kilo.synthetic_scene(dev, resolution=[16, 16, 16], gmin=[-1., -1., -1.], gmax=[1., 1., 1.], seed=1, fill=0.3)
    return mlp, gmin.to(dev), gmax.to(dev), kilo.orbit_poses(3, radius=3.0).to(dev)


class KiloSet:
    """a KiloNerfDataset-shaped stand-in over camera rays: training items of N_RAND rays with z_vals, the val / test items of the reference"""
    H = W = 8
    FOCAL, NEAR, FAR, S, N_RAND = 10.0, 1.5, 4.5, 16, 32

    def __init__(self, dev, mode, gmin, gmax, poses):
        self.device, self.mode, self.gmin, self.gmax, self.poses, self.iter_n = dev, mode, gmin, gmax, poses, 0
        g = torch.Generator().manual_seed(3)
        self.images = torch.rand(poses.shape[0], self.H, self.W, 3, generator=g).to(dev)
        self.pipeline = self.frame

    def set_iter(self, it):
        self.iter_n = it

    def frame(self, data):
        from xrnerf_amd import kilo, ops
        o, d, v = kilo.camera_rays(data['pose'], self.H, self.W, self.FOCAL, self.device)
        R = o.shape[0]
        z = ops.mip_zvals(torch.full((R,), self.NEAR, device=self.device), torch.full((R,), self.FAR, device=self.device), self.S)
        return {'rays_o': o, 'rays_d': d, 'viewdirs': v, 'z_vals': z, 'src_shape': torch.tensor([self.H, self.W, 3])}

    def __len__(self):
        return {'train': 4, 'val': 1, 'test': self.poses.shape[0]}[self.mode]

    def __getitem__(self, idx):
        box = {'global_domain_min': self.gmin, 'global_domain_max': self.gmax}
        if self.mode == 'val':
            return dict(box, poses=self.poses[:1], images=self.images[:1], spiral_poses=self.poses[1:2])
        if self.mode == 'test':
            return dict(box, pose=self.poses[idx], image=self.images[idx], idx=idx)
        f = self.frame({'pose': self.poses[idx % self.poses.shape[0]]})
        pick = torch.arange(self.N_RAND, device=self.device) * 2
        item = {k: f[k][pick] for k in ('rays_o', 'rays_d', 'viewdirs', 'z_vals')}
        item['target_s'] = self.images[idx % self.poses.shape[0]].reshape(-1, 3)[pick]
        return dict(item, **box)


def check_kilo(dev, tmp):
    """two fine-tuning iterations through KiloNerfTrainRunner (FusedAdam on the GPU, the device log window), val_step and test_step of
    one 8 x 8 pose with the reference's keys"""
    import xrnerf_amd
    from xrnerf_amd import apis, kilo, runner as R
    from xrnerf_amd.builder import ConfigDict
    mlp, gmin, gmax, poses = kilo_scene(dev)
    for p in mlp.parameters():
        p.requires_grad_(True)
    net = xrnerf_amd.build_network(dict(type='KiloNerfNetwork', render=dict(type='NerfRender', white_bkgd=True, raw_noise_std=0),
                                        cfg=dict(phase='train', chunk=1024, bs_data='rays_o', is_perturb=False, N_importance=0,
                                                 l2_regularization_lambda=1e-6)))
    net.mlp = mlp                        # (the config's KiloNerfMLP reads its occupancy grid and weights from files)
    net = net.to(dev)
    cfg = ConfigDict.wrap(dict(method='kilo_nerf', optimizer=dict(type='Adam', lr=1e-3, betas=(0.9, 0.999))))
    optimizer = apis.get_optimizer(net, cfg)
    before = [p.detach().clone() for p in net.parameters()]
    trainset, valset, testset = (KiloSet(dev, m, gmin, gmax, poses) for m in ('train', 'val', 'test'))
    runner = apis.get_runner(dict(type='KiloNerfTrainRunner'))(net, optimizer=optimizer, work_dir=os.path.join(tmp, 'kilo'))
    assert type(runner) is R.KiloNerfTrainRunner
    runner.register_training_hooks(dict(policy='step', step=1000, gamma=0.1, by_epoch=False), dict(grad_clip=None),
                                   dict(interval=2, by_epoch=False), dict(interval=2, hooks=[dict(type='TextLoggerHook')]))
    apis.register_hooks([dict(type='SetValPipelineHook', params=dict(), variables=dict(valset='valset')),
                         dict(type='PassIterHook', params=dict())], runner=runner, valset=valset)
    runner.run([R.DataLoader(trainset), R.DataLoader(valset)], [('train', 2), ('val', 1)], 2)
    assert runner.iter == 2 and trainset.iter_n == 1 and os.path.isfile(os.path.join(tmp, 'kilo', 'iter_2.pth'))
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, net.parameters())), 'fine-tuning moved no parameter'
    (it, lr, avg), = runner.log_history
    assert it == 2 and lr == 1e-3 and sorted(avg) == ['L2 reg', 'loss', 'psnr'] and all(np.isfinite(v) for v in avg.values()), avg
    if dev.type == 'cuda':
        assert type(optimizer).__name__ == 'FusedAdam' and runner.log_buffer.names == ['loss', 'psnr', 'L2 reg']
    val = runner.outputs
    assert sorted(val) == ['disps', 'elapsed_time', 'gt_imgs', 'rgbs', 'spiral_disps', 'spiral_rgbs']
    assert len(val['rgbs']) == 1 and val['rgbs'][0].shape == (8, 8, 3) and val['disps'][0].shape == (8, 8) and val['spiral_rgbs'][0].shape == (8, 8, 3)
    assert np.isfinite(val['rgbs'][0]).all() and np.array_equal(val['gt_imgs'][0], valset.images[0].cpu().numpy())
    net.phase = 'test'
    item = next(iter(R.DataLoader(testset)))
    with torch.no_grad():
        res = net.val_step(item)
    assert sorted(res) == ['gt_img', 'idx', 'rgb'] and res['rgb'].shape == (8, 8, 3) and res['idx'] == 0
    assert np.isfinite(res['rgb']).all() and np.array_equal(res['gt_img'], testset.images[0].cpu().numpy())


def check_occupancy_hook(dev, tmp):
    """BuildOccupancyTreeHook.after_run on a 2-layer teacher at [4, 4, 4]: the file holds build_occupancy_grid's grid"""
    import xrnerf_amd
    from xrnerf_amd import kilo_distill
    from xrnerf_amd.builder import ConfigDict
    torch.manual_seed(4)
    teacher = xrnerf_amd.build_mlp(dict(type='NerfMLP', skips=[4], netdepth=2, netwidth=32, netchunk=1024 * 32, output_ch=4, use_viewdirs=True,
                                        embedder=dict(type='BaseEmbedder', i_embed=0, multires=4, multires_dirs=2))).to(dev)
    gmin, gmax = [-1.0, -1.2, -0.8], [1.0, 1.1, 0.9]
    # the threshold: the median over the voxels of the teacher's largest density on the lattice, so that the grid is mixed
    with torch.no_grad():
        pts = kilo_distill.occupancy_points(gmin, gmax, [4, 4, 4], (2, 2, 2), 0, 64, dev)
        sigma = teacher({'pts': pts, 'viewdirs': torch.zeros_like(pts)})['raw'][:, 3].reshape(64, 8).max(1).values
    threshold = float(sigma.median())
    occ = dict(resolution=[4, 4, 4], subsample_resolution=[2, 2, 2], threshold=threshold, voxel_batch_size=24, work_dir=os.path.join(tmp, 'occ'))
    cfg = ConfigDict.wrap(dict(global_domain_min=gmin, global_domain_max=gmax, build_occupancy_tree_config=occ))

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.mlp = teacher

    class Runner:
        import logging
        model, logger = Model(), logging.getLogger('xrnerf_amd.test')
    kilo_distill.BuildOccupancyTreeHook(cfg=cfg).after_run(Runner())
    saved = torch.load(os.path.join(tmp, 'occ', 'occupancy.pth'), map_location='cpu', weights_only=False)
    want = kilo_distill.build_occupancy_grid(teacher, cfg.global_domain_min, cfg.global_domain_max, [4, 4, 4], (2, 2, 2), threshold, 24)
    assert saved.dtype == torch.bool and tuple(saved.shape) == (4, 4, 4) and torch.equal(saved, want.cpu())
    assert 0 < int(saved.sum()) < 64, 'a grid that is all one value checks nothing: %d of 64' % int(saved.sum())
