"""Host tier of the instant-ngp runner: runner.NgpIterRunner's span plan over a stub engine, ngp_hooks.EMAHook's buffers on
a host module, the refusals, and -- where the reference tree is present -- that its configs/instant_ngp/nerf_blender_local01.py loads and
every name it gives resolves.  No GPU, no library call."""
import logging
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xrnerf_amd import apis, ngp_hooks, pipelines, runner as R  # noqa: E402

REF_CFG = '/root/reference/configs/instant_ngp/nerf_blender_local01.py'


class Engine:
    """what NgpIterRunner asks of train.Trainer: run(k) -> the last iteration's outputs, and `iter`"""

    def __init__(self, log):
        self.iter, self.log = 0, log

    def run(self, k):
        self.log.append(k)
        self.iter += k
        return {'loss': torch.zeros(()), 'log_vars': {}, 'num_samples': 1, 'last': self.iter - 1}


class Model(torch.nn.Module):
    def __init__(self, log):
        super().__init__()
        self.log = log

    def val_step(self, data, **kwargs):
        self.log.append('val')
        return {}


class Opt:
    def __init__(self, lr=1e-2):
        self.param_groups = [{'lr': lr, 'params': []}]


class Items:
    """a dataset of `n` empty items that remembers what PassIterHook told it"""

    def __init__(self, n=3):
        self.n, self.iters = n, []

    def set_iter(self, it):
        self.iters.append(it)

    def __len__(self):
        return self.n

    def __getitem__(self, idx):
        return {}


class Ckpt(R.CheckpointHook):
    def __init__(self, seen, **kw):
        super().__init__(**kw)
        self.seen = seen

    def after_train_iter(self, runner):
        self.seen.append(('ckpt', runner.iter, runner.inner_iter, runner.outputs['last']))


class Text(R.TextLoggerHook):
    def __init__(self, seen, **kw):
        super().__init__(**kw)
        self.seen = seen

    def after_train_iter(self, runner):
        self.seen.append(('log', runner.iter, runner.inner_iter, runner.outputs['last']))
        super().after_train_iter(runner)


def make(max_iters, log_interval=8, ckpt_interval=20, lr_step=10):
    log, seen = [], []
    engine = Engine(log)
    runner = R.NgpIterRunner(Model(log), optimizer=Opt(), logger=logging.getLogger('xrnerf_amd.test'), engine=engine)
    runner.register_training_hooks(dict(policy='step', step=lr_step, gamma=0.2, by_epoch=False), dict(grad_clip=None), None, None)
    runner.register_hook(Ckpt(seen, interval=ckpt_interval), 'NORMAL')
    runner.register_hook(Text(seen, interval=log_interval), 'VERY_LOW')
    runner.register_hook(pipelines.PassIterHook(), 'NORMAL')
    train, val = Items(), Items(1)
    return runner, engine, log, seen, train, val, max_iters


def test_spans_end_where_a_hook_is_due_and_the_hooks_see_the_spans_last_iteration():
    runner, engine, log, seen, train, val, n = make(40)
    runner.run([R.DataLoader(train), R.DataLoader(val)], [('train', 20), ('val', 1)], n)
    assert log == [8, 8, 4, 'val', 4, 8, 8, 'val']
    assert runner.iter == 40 and engine.iter == 40
    # (hook, runner.iter, runner.inner_iter, the engine's last iteration): at 19 and 39 the checkpoint (NORMAL) runs before the logger
    assert seen == [('log', 7, 7, 7), ('log', 15, 15, 15), ('ckpt', 19, 19, 19), ('log', 23, 3, 23), ('log', 31, 11, 31),
                    ('ckpt', 39, 19, 39), ('log', 39, 19, 39)]
    assert train.iters == [7, 15, 19, 23, 31, 39]                     # PassIterHook: every span's last iteration
    # the schedule: the trainer's lr_at IS the hook's get_lr, across the milestones at 10, 20, 30; the group lr a logger prints is the
    # last iteration's
    hook = R.StepLrUpdaterHook(step=10, gamma=0.2)
    for i in range(40):
        assert runner.lr_at(i) == hook.get_lr(R._At(i), 1e-2)
    assert runner.lr_at(9) != runner.lr_at(10) != runner.lr_at(20)
    assert [(it, lr) for it, lr, _ in runner.log_history] == [(i + 1, hook.get_lr(R._At(i), 1e-2)) for i in (7, 15, 23, 31, 39)]


def test_an_unknown_per_iteration_hook_forces_spans_of_one():
    class Odd:
        def __init__(self):
            self.before, self.after = [], []

        def before_train_iter(self, runner):
            self.before.append(runner.iter)

        def after_iter(self, runner):                                   # the general name (mmcv's Hook base class routes it): val calls it too
            if runner.mode == 'train':
                self.after.append(runner.iter)
    runner, engine, log, seen, train, val, n = make(11)
    odd = Odd()
    runner.register_hook(odd)
    runner.run([R.DataLoader(train), R.DataLoader(val)], [('train', 6), ('val', 1)], n)
    assert log == [1] * 6 + ['val'] + [1] * 5 + ['val']
    assert odd.before == list(range(11)) and odd.after == list(range(11))
    assert [s[:2] for s in seen] == [('log', 7)]


def test_max_iters_that_is_no_multiple_of_anything_ends_on_the_exact_iteration():
    runner, engine, log, seen, train, val, n = make(37)
    runner.run([R.DataLoader(train), R.DataLoader(val)], [('train', 20), ('val', 1)], n)
    assert log == [8, 8, 4, 'val', 4, 8, 5, 'val'] and runner.iter == 37 and engine.iter == 37
    assert train.iters == [7, 15, 19, 23, 31, 36]
    # a run that resumes in the middle of a logging interval goes on from its iteration
    runner, engine, log, seen, train, val, n = make(30)
    runner._iter = 13
    runner.run([R.DataLoader(train), R.DataLoader(val)], [('train', 20), ('val', 1)], n)
    assert log == [3, 4, 4, 6, 'val'] and engine.iter == 30
    assert [s[:2] for s in seen] == [('log', 15), ('ckpt', 19), ('log', 23)]


# ------------------------------------------------------------------------------------------ EMAHook
class P(torch.nn.Module):
    def __init__(self, n):
        super().__init__()
        self.params = torch.nn.Parameter(torch.arange(n, dtype=torch.float32))


class Mlp(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.embedder_pos, self.embedder_dir, self.density_net, self.color_net = P(8), P(0), P(4), P(6)


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.mlp = Mlp()


class HookRunner:
    def __init__(self, model, optimizer):
        self.model, self.optimizer = model, optimizer


def test_ema_hook_registers_buffers_that_alias_the_optimisers_state():
    from xrnerf_amd.train import FusedAdam
    net = Net()
    params = [p for p in net.parameters() if p.numel() > 0]
    opt = FusedAdam(params, lr=1e-2)                        # (host tensors: only its state is used here, never its step)
    hook = ngp_hooks.EMAHook(momentum=0.05)
    run = HookRunner(net, opt)
    hook.before_run(run)
    assert opt.param_groups[0]['ema_momentum'] == 0.05 and opt.param_groups[0]['ema_warm_up'] == 100
    names = ['ema_mlp_embedder_pos_params', 'ema_mlp_density_net_params', 'ema_mlp_color_net_params']
    assert sorted(net.state_dict()) == sorted(['mlp.embedder_pos.params', 'mlp.embedder_dir.params', 'mlp.density_net.params', 'mlp.color_net.params',
                                               'ema_mlp_embedder_dir_params'] + names)
    for name, p in zip(names, params):
        buf, st = getattr(net, name), opt.state[p]
        assert buf is st['ema'] and buf.data_ptr() == st['ema'].data_ptr() and buf.data_ptr() != p.data_ptr()
        assert torch.equal(buf, p.detach())
        st['ema'].add_(1.0)                                 # what the optimiser writes is what state_dict() carries
        assert torch.equal(net.state_dict()[name], p.detach() + 1.0)
    assert net.ema_mlp_embedder_dir_params.numel() == 0
    # a resumed optimiser holds new state tensors: the buffers keep their storage and name the state again
    held = {name: getattr(net, name) for name in names}
    import copy
    saved = copy.deepcopy(opt.state_dict())                 # (what torch.load hands a resume: tensors of its own)
    for p in params:
        opt.state[p]['ema'].zero_()
    opt.load_state_dict(saved)
    assert all(opt.state[p]['ema'] is not held[name] for name, p in zip(names, params))
    hook.alias(run)
    for name, p in zip(names, params):
        assert getattr(net, name) is held[name] and opt.state[p]['ema'] is held[name] and torch.equal(held[name], p.detach() + 1.0)
    assert len(net.state_dict()) == 8
    # a parameter the optimiser does not hold would keep a stale average: refused by name
    net2 = Net()
    with pytest.raises(NotImplementedError, match='density_net'):
        ngp_hooks.EMAHook(momentum=0.05).before_run(HookRunner(net2, FusedAdam([net2.mlp.embedder_pos.params, net2.mlp.color_net.params])))
    with pytest.raises(NotImplementedError, match='FusedAdam'):
        ngp_hooks.EMAHook(momentum=0.05).before_run(HookRunner(net2, torch.optim.Adam([net2.mlp.embedder_pos.params])))


def test_refusals():
    from xrnerf_amd.builder import ConfigDict
    from xrnerf_amd.train import ngp_lego_model_cfg
    with pytest.raises(NotImplementedError, match='interval'):
        ngp_hooks.EMAHook(momentum=0.05, interval=2)
    runner = R.NgpIterRunner(Model([]), optimizer=Opt(), logger=logging.getLogger('xrnerf_amd.test'), engine=Engine([]))
    with pytest.raises(NotImplementedError, match='SyncBuffersHook'):
        runner.register_training_hooks(None, custom_hooks_config=[dict(type='EMAHook', momentum=0.05), dict(type='SyncBuffersHook')])
    plain = R.IterRunner(Model([]), optimizer=Opt(), logger=logging.getLogger('xrnerf_amd.test'))
    with pytest.raises(NotImplementedError, match='EMAHook'):
        plain.register_training_hooks(None, custom_hooks_config=[dict(type='EMAHook', momentum=0.05)])
    # the instant-ngp model on anything but the instant-ngp data, or without its parts: refused before anything is built (no file is read)
    cfg = ConfigDict.wrap(dict(method='nerf', distributed=False, model=ngp_lego_model_cfg(),
                               data=dict(train=dict(type='SceneBaseDataset', cfg=dict(datadir='/nonexistent'), pipeline=[]))))
    with pytest.raises(NotImplementedError, match='instant-ngp'):
        apis.train_nerf(cfg)
    with pytest.raises(NotImplementedError, match='instant-ngp'):
        apis.test_nerf(cfg)
    cfg.data.train.type = 'HashNerfDataset'
    del cfg.model['render']
    with pytest.raises(NotImplementedError, match='instant-ngp.*render'):
        apis.train_nerf(cfg)
    cfg.distributed = True
    with pytest.raises(NotImplementedError, match='distributed'):
        apis.train_nerf(cfg)


def _types(node, out):
    if isinstance(node, dict):
        if 'type' in node:
            out.append(node['type'])
        for v in node.values():
            _types(v, out)
    elif isinstance(node, (list, tuple)):
        for v in node:
            _types(v, out)
    return out


@pytest.mark.skipif(not os.path.exists(REF_CFG), reason='the reference tree is not present')
def test_the_reference_config_loads_and_every_name_it_gives_resolves():
    from xrnerf_amd import builder
    cfg = apis.update_config('lego', apis.load_config(REF_CFG))
    apis._refuse(cfg)                                               # the instant-ngp combination: accepted
    hooks = apis._hook_classes()
    for key in ('train_hooks', 'test_hooks', 'custom_hooks'):
        for h in cfg[key]:
            assert h['type'] in hooks, (key, h['type'])
    assert [h['type'] for h in cfg.custom_hooks] == ['EMAHook']
    for mode in ('train', 'val', 'test'):
        assert cfg.data[mode]['type'] in pipelines.DATASETS, mode
        for step in cfg.data[mode]['pipeline']:
            assert step['type'] in pipelines.PIPELINES, step['type']
    assert cfg.data.train.cfg.datadir == 'data/nerf_synthetic/lego'
    for t in _types(cfg.model, []):
        assert t in builder.MODELS or t in ('HashGrid', 'SphericalHarmonics', 'FullyFusedMLP'), t      # (the latter three: tcnn's otypes)
    assert cfg.model.type in builder.NETWORKS and cfg.lr_config.policy in R.LR_POLICIES
    assert R.get_runner(cfg.train_runner) is R.NerfTrainRunner and R.get_runner(cfg.test_runner) is R.NerfTestRunner
    net = builder.build_network(cfg.model)
    assert type(net).__name__ == 'HashNerfNetwork'
