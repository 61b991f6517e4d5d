"""xrnerf_amd.runner / xrnerf_amd.apis on the host: the runner's semantics on a recording model (no kernels), MipLrUpdaterHook against the
reference's own class, the Bungee stage loop against bungee.train_iteration, train_nerf / test_nerf / run_nerf end to end on host tensors
(vanilla NeRF; Mip-NeRF and KiloNeRF have no host-tensor path and run on the HIP-on-CPU shim, tests/hip_emu), BuildOccupancyTreeHook.

The expected sequences of the first test are written out from the reference's call sites (core/apis/train.py, core/runner/*.py,
core/hooks/train_hooks.py) and the restated mmcv rules: IterBasedRunner.run's workflow loop, hook priorities
(LR 10 < optimiser 40 < checkpoint 50 = train_hooks 50 in registration order < logger 90), every_n_iters on iter + 1, the 'step' policy."""
import contextlib
import json
import logging
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import runner_cases as RC  # noqa: E402

CPU = torch.device('cpu')


# ------------------------------------------------------------------------------------------ test 3: the recording model
class Items:
    def __init__(self, events, n=7):
        self.events, self.n = events, n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return {'k': i}

    def set_iter(self, it):
        self.events.append(('set_iter', it))


class Recorder(torch.nn.Module):
    def __init__(self, events):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(3))
        self.events = events

    def train_step(self, data, optimizer, **kwargs):
        assert self.training
        self.events.append(('train', int(data['k']), optimizer.param_groups[0]['lr']))
        loss = ((self.w - 1.0) ** 2).sum()
        return {'loss': loss, 'log_vars': {'loss': float(loss.detach())}, 'num_samples': 2}

    def val_step(self, data, **kwargs):
        assert not self.training and not torch.is_grad_enabled()
        self.events.append(('val', int(data['k'])))
        return {}


class LogLines(logging.Handler):
    def __init__(self, events):
        super().__init__()
        self.events = events

    def emit(self, record):
        msg = record.getMessage()
        if msg.startswith('Iter ['):
            self.events.append(('log', msg.split(']')[0] + ']'))


def recording_run(work_dir, resume_from=None):
    from xrnerf_amd import apis, runner as R
    events = []
    model = Recorder(events)
    optimizer = torch.optim.Adam(model.parameters(), lr=0.01)
    logger = logging.getLogger('xrnerf_amd.test_runner.%d' % id(events))
    logger.setLevel(logging.INFO)
    logger.propagate = False
    logger.addHandler(LogLines(events))
    runner = apis.get_runner(dict(type='NerfTrainRunner'))(model, optimizer=optimizer, work_dir=work_dir, logger=logger, meta=None)
    runner.register_training_hooks(dict(policy='step', step=4, gamma=0.1, by_epoch=False), dict(grad_clip=None),
                                   dict(interval=3, by_epoch=False), dict(interval=2, by_epoch=False, hooks=[dict(type='TextLoggerHook')]))
    apis.register_hooks([dict(type='PassIterHook', params=dict())], runner=runner)
    if resume_from:
        runner.resume(resume_from)
    trainset, valset = Items(events), Items([])
    runner.run([R.DataLoader(trainset), R.DataLoader(valset)], [('train', 3), ('val', 1)], 7)
    return runner, events, optimizer


def test_runner_semantics_on_a_recording_model(tmp_path):
    work = str(tmp_path / 'work')
    runner, events, optimizer = recording_run(work)
    lr = [0.01 * 0.1 ** (it // 4) for it in range(7)]
    assert lr[3] == 0.01 and lr[4] == 0.01 * 0.1 ** 1 and lr[6] < 0.0011

    def train(it):
        out = [('train', it, lr[it]), ('set_iter', it)]
        return out + ([('log', 'Iter [%d/7]' % (it + 1))] if (it + 1) % 2 == 0 else [])
    want = train(0) + train(1) + train(2) + [('val', 0)] + train(3) + train(4) + train(5) + [('val', 1)] + train(6) + [('val', 2)]
    assert events == want, events
    assert sum(e[0] == 'log' for e in events) == 3
    assert runner.iter == 7 and runner.epoch == 0 and [h[0] for h in runner.log_history] == [2, 4, 6]
    assert sorted(f for f in os.listdir(work) if f.endswith('.pth')) == ['iter_3.pth', 'iter_6.pth', 'latest.pth']
    assert os.path.islink(os.path.join(work, 'latest.pth')) and os.readlink(os.path.join(work, 'latest.pth')) == 'iter_6.pth'
    ckpt = torch.load(os.path.join(work, 'iter_3.pth'), weights_only=False)
    assert sorted(ckpt) == ['meta', 'optimizer', 'state_dict'] and ckpt['meta'] == {'iter': 3, 'epoch': 1}
    assert int(ckpt['optimizer']['state'][0]['step']) == 3 and ckpt['optimizer']['param_groups'][0]['initial_lr'] == 0.01
    # the logged loss is the window's average: iterations 0 and 1 of a model whose loss the optimiser lowers
    first = runner.log_history[0][2]['loss']
    assert 0 < first < 3.0 and runner.log_history[2][2]['loss'] < first
    hooks = [type(h).__name__ for h in runner.hooks]
    assert hooks == ['StepLrUpdaterHook', 'OptimizerHook', 'CheckpointHook', 'PassIterHook', 'TextLoggerHook'], hooks

    # resume from iter_3.pth: iteration 3 is next, the optimiser's step counters are back, the tail of the sequence is the same
    resumed, events2, optimizer2 = recording_run(str(tmp_path / 'work2'), resume_from=os.path.join(work, 'iter_3.pth'))
    strip = lambda ev: [e[:1] + e[2:] if e[0] == 'train' else (e[:1] if e[0] == 'val' else e) for e in ev]
    tail = strip(train(3) + train(4) + train(5) + [('val', 1)] + train(6) + [('val', 2)])
    assert strip(events2) == tail, events2
    assert resumed.iter == 7 and int(optimizer2.state[optimizer2.param_groups[0]['params'][0]]['step']) == 7
    assert torch.equal(resumed.model.w, runner.model.w), 'the resumed run did not end on the same parameters'
    assert sorted(f for f in os.listdir(str(tmp_path / 'work2')) if f.endswith('.pth')) == ['iter_6.pth', 'latest.pth']


def test_lr_policies_and_refusals():
    from xrnerf_amd import runner as R

    class At:
        def __init__(self, it):
            self.iter = it
    h = R.StepLrUpdaterHook(step=[2, 5], gamma=0.5, by_epoch=False)
    assert [h.get_lr(At(i), 1.0) for i in range(7)] == [1.0, 1.0, 0.5, 0.5, 0.5, 0.25, 0.25]
    assert R.StepLrUpdaterHook(step=2, gamma=0.1, min_lr=0.05).get_lr(At(9), 1.0) == 0.05
    r = R.IterRunner(torch.nn.Linear(1, 1))
    with pytest.raises(NotImplementedError, match='grad_clip'):
        r.register_training_hooks(None, dict(grad_clip=dict(max_norm=35)))
    with pytest.raises(NotImplementedError, match='poly'):
        r.register_training_hooks(dict(policy='poly', power=1.0))
    with pytest.raises(NotImplementedError, match='EMAHook'):
        r.register_training_hooks(None, custom_hooks_config=[dict(type='EMAHook', momentum=0.05)])
    with pytest.raises(KeyError, match='NoSuchRunner'):
        R.get_runner(dict(type='NoSuchRunner'))
    from xrnerf_amd.kilo_tree import KiloNerfDistillTrainRunner
    assert R.get_runner(dict(type='KiloNerfDistillTrainRunner')) is KiloNerfDistillTrainRunner
    assert issubclass(R.BungeeNerfTestRunner, R.EpochRunner) and issubclass(R.KiloNerfTestRunner, R.EpochRunner)


def test_mip_lr_against_the_reference_class():
    """6 iterations x 2 parameter sets: the reference's own class where its tree is present, the values it gave otherwise -- and both
    where both are there"""
    import ref_import
    from xrnerf_amd.runner import MipLrUpdaterHook
    got = RC.mip_lr_values(MipLrUpdaterHook)
    gold = json.load(open(RC.MIP_LR_GOLD))
    assert gold['cases'] == RC.MIP_LR_CASES and gold['iters'] == list(RC.MIP_LR_ITERS)
    assert got == gold['lr'], (got, gold['lr'])
    if ref_import.available():
        assert got == RC.mip_lr_values(RC.reference_mip_lr_class())


def test_config_helpers(tmp_path):
    from xrnerf_amd import apis
    from xrnerf_amd.builder import ConfigDict
    args = apis.parse_args([])
    assert (args.config, args.dataname, args.test_only, args.render_only, args.load_from) == ('configs/nerfs/nerf_base01.py', 'ficus', False, False, '')
    cfg = ConfigDict.wrap(dict(method='kilo_nerf', phase='finetune', work_dir='w/#DATANAME#/', resolution_table=dict(Lego=[16, 32, 16]),
                               model=dict(mlp=dict(type='KiloNerfMLP')), data=dict(train=dict(cfg=dict(datadir='d/#DATANAME#')))))
    cfg = apis.update_loadfrom('iter_5.pth', apis.update_config('Lego', cfg))
    assert cfg.work_dir == 'w/Lego/' and cfg.data.train.cfg.datadir == 'd/Lego' and cfg.model.mlp.resolution == [16, 32, 16]
    assert cfg.load_from == 'w/Lego/iter_5.pth' and apis.update_loadfrom('', cfg).load_from == 'w/Lego/iter_5.pth'
    pre = ConfigDict.wrap(dict(method='kilo_nerf', phase='pretrain', resolution_table=dict(Lego=[4, 4, 4]), build_occupancy_tree_config=dict(threshold=10)))
    assert apis.update_config('Lego', pre).build_occupancy_tree_config.resolution == [4, 4, 4]
    # _base_ lists merge recursively, _delete_ replaces
    (tmp_path / 'a.py').write_text("x = dict(p=1, q=dict(r=2, s=3))\ny = [1, 2]\nz = dict(keep=1)\n")
    (tmp_path / 'b.py').write_text("_base_ = ['a.py']\nw = 5\n")
    (tmp_path / 'c.py').write_text("_base_ = './b.py'\nx = dict(q=dict(r=7))\ny = [3]\nz = dict(_delete_=True, new=2)\n")
    c = apis.load_config(str(tmp_path / 'c.py'))
    assert c == dict(x=dict(p=1, q=dict(r=7, s=3)), y=[3], z=dict(new=2), w=5) and c.x.q.r == 7


def test_get_optimizer_animatable_branch_and_defaults():
    from xrnerf_amd import apis
    from xrnerf_amd.builder import ConfigDict

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)

        def get_params(self):
            return list(self.b.parameters())
    m = Model()
    opt = apis.get_optimizer(m, ConfigDict.wrap(dict(method='animatable_nerf', optimizer=dict(type='Adam', lr=3e-4, betas=(0.5, 0.6)))))
    assert [id(p) for p in opt.param_groups[0]['params']] == [id(p) for p in m.b.parameters()]
    assert opt.param_groups[0]['lr'] == 3e-4 and tuple(opt.param_groups[0]['betas']) == (0.9, 0.999)
    opt = apis.get_optimizer(m, ConfigDict.wrap(dict(method='nerf', optimizer=dict(type='Adam', lr=5e-4, betas=(0.9, 0.99)))))
    g = opt.param_groups[0]
    assert len(g['params']) == 4 and (g['lr'], tuple(g['betas']), g['eps'], g['weight_decay']) == (5e-4, (0.9, 0.99), 1e-8, 0)
    with pytest.raises(NotImplementedError, match='SGD'):
        apis.get_optimizer(m, ConfigDict.wrap(dict(method='nerf', optimizer=dict(type='SGD', lr=0.1))))


# ------------------------------------------------------------------------------------------ test 4: the Bungee stage loop
class TinyBungee(torch.nn.Module):
    """a differentiable stand-in with BungeeNerfNetwork.train_step's contract: the loss of stage s covers the rays of scale <= s and is
    exactly 0 where there are none"""

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.lin = torch.nn.Linear(3, 3)

    def train_step(self, data, optimizer, **kwargs):
        x, t, sc = data['x'][0], data['target_s'][0], data['scale_code'][0]
        mask = (sc <= kwargs['stage']).float()
        data['x'] = None                                   # (the reference's train_step mutates its batch: every stage gets a copy)
        loss = ((self.lin(x) * mask - t * mask) ** 2).mean()
        return {'loss': loss, 'log_vars': {'loss': loss.item(), 'psnr': 0.0}, 'num_samples': x.shape[0]}


def test_bungee_runner_iteration_equals_train_iteration():
    from xrnerf_amd import bungee, runner as R
    g = torch.Generator().manual_seed(0)
    batches = [{'x': torch.randn(1, 6, 3, generator=g), 'target_s': torch.randn(1, 6, 3, generator=g),
                'scale_code': torch.tensor([[[1], [2], [1], [2], [1], [2]]])} for _ in range(3)]        # no ray of scale 0: stage 0 is skipped

    class Loader:
        def __iter__(self):
            return iter([dict(b) for b in batches])

        def __len__(self):
            return len(batches)
    a, b = TinyBungee(), TinyBungee()
    opt_a, opt_b = (torch.optim.Adam(m.parameters(), lr=1e-2) for m in (a, b))
    runner = R.get_runner(dict(type='BungeeNerfTrainRunner'))(a, optimizer=opt_a)
    runner.register_training_hooks(dict(policy='step', step=100, gamma=0.1, by_epoch=False), dict(grad_clip=None), None,
                                   dict(interval=1, hooks=[dict(type='TextLoggerHook')]))
    runner.run([Loader()], [('train', 1)], 3)
    outs = [bungee.train_iteration(b, dict(batch), opt_b) for batch in batches]
    assert [len(o) for o in outs] == [3, 3, 3] and outs[0][0]['log_vars']['loss'] == 0.0 and outs[0][1]['log_vars']['loss'] > 0
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
    assert int(opt_a.state[a.lin.weight]['step']) == 6 == int(opt_b.state[b.lin.weight]['step'])          # two live stages x three batches
    assert runner.iter == 3 and [h[0] for h in runner.log_history] == [1, 1, 2, 2, 3, 3] and runner.log_history[-1][2]['stage'] == 2


# ------------------------------------------------------------------------------------------ test 5: end to end
def test_the_hooks_refuse_a_frame_narrower_than_the_ssim_window():
    """why the end-to-end scene is 8 x 7: the 8 x 6 frames of tests/pipeline_scene.py are narrower than the 7 x 7 SSIM window"""
    from xrnerf_amd import evaluate

    class Runner:
        outputs = {'rgbs': [np.zeros((8, 6, 3), np.float32)], 'gt_imgs': [np.ones((8, 6, 3), np.float32)]}
        work_dir, iter, logger = '/nonexistent', 0, logging.getLogger('xrnerf_amd.test')
    with pytest.raises(ValueError, match='win_size exceeds image extent'):
        evaluate.ValidateHook().after_val_iter(Runner())


def test_train_test_and_run_nerf_on_host_tensors(tmp_path):
    RC.check_end_to_end(CPU, str(tmp_path), 'blender')


@contextlib.contextmanager
def emulated(*extra):
    """emulib.emulated_ops with the host builds of `extra` sources and every family's table on top"""
    import emulib as E
    from xrnerf_amd import _lib
    with E.emulated_ops() as dev:
        ml = E.MultiLib(E.ALL_SOURCES + tuple(extra))
        tables = [v for k, v in vars(_lib).items() if k.endswith('SIGNATURES')]
        for table in tables:
            for name, (res, args) in table.items():
                try:
                    fn = getattr(ml, name)
                except AttributeError:
                    continue
                fn.restype, fn.argtypes = res, args
        _lib._lib = ml

        def check(rc, what=''):
            if rc != 0:
                raise _lib.XrError('%s failed (%d): %s' % (what, rc, ml.last_errors()))
        _lib.check = check
        yield dev


def test_train_and_test_mip_nerf_on_the_emulated_kernels(tmp_path):
    """(the command line's path is the vanilla test's above and the GPU tier's for both families: the emulator runs a lane at a time)"""
    with emulated('xr_optim', 'xr_eval', 'xr_pipeline', 'xr_vanilla') as dev:
        RC.check_end_to_end(dev, str(tmp_path), 'mip', command_line=False)


# ------------------------------------------------------------------------------------------ test 6: KiloNeRF
def test_kilonerf_runner_val_and_test_steps_on_the_emulated_kernels(tmp_path):
    with emulated('xr_optim', 'xr_vanilla') as dev:
        RC.check_kilo(dev, str(tmp_path))


def test_build_occupancy_tree_hook_on_the_emulated_kernels(tmp_path):
    with emulated('xr_vanilla') as dev:
        RC.check_occupancy_hook(dev, str(tmp_path))
