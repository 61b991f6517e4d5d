"""train_nerf / test_nerf / run_nerf over a reference config file (core/apis/{api,train,test,helper}.py), single process.

    python -m xrnerf_amd.run_nerf --config configs/nerf/nerf_blender_base01.py --dataname lego [--test_only] [--load_from iter_5000.pth]

The config is the reference's Python file, loaded as it is (load_config: runpy + `_base_`); datasets, network, optimiser, runner and hooks
are built from the names it gives.  The loaders are in-process (runner.DataLoader over pipelines.iterate), the optimiser is train.FusedAdam
where the parameters live on the GPU, the runners and the lr / optimizer / checkpoint / log hooks are xrnerf_amd.runner's.
The instant-ngp config (a HashNerfNetwork on HashNerfDataset data) trains through runner.NgpIterRunner, which drives train.Trainer's native
loop in spans between the iterations at which a hook is due.
Out of scope, each refused by name: distributed runs, gradient clipping, logger hooks other than TextLoggerHook, custom_hooks other than the
instant-ngp config's EMAHook.
"""
import argparse
import logging
import os
import runpy
import types
from functools import reduce

import torch

from . import builder, pipelines, runner as _runner
from .builder import ConfigDict


# ------------------------------------------------------------------------------------------ config files
def _merge(base, child):
    """mmcv's Config._merge_a_into_b, child into base: dicts merge key by key unless the child's carries _delete_=True"""
    out = dict(base)
    for k, v in child.items():
        if isinstance(v, dict) and isinstance(out.get(k), dict) and not v.get('_delete_', False):
            out[k] = _merge(out[k], v)
        else:
            out[k] = {kk: vv for kk, vv in v.items() if kk != '_delete_'} if isinstance(v, dict) else v
    return out


def _load(path):
    ns = runpy.run_path(path)
    cfg = {k: v for k, v in ns.items() if not k.startswith('__') and not isinstance(v, (types.ModuleType, types.FunctionType, type))}
    bases = cfg.pop('_base_', [])
    bases = [bases] if isinstance(bases, str) else list(bases)
    merged = {}
    for b in bases:
        merged = _merge(merged, _load(os.path.join(os.path.dirname(os.path.abspath(path)), b)))
    return _merge(merged, cfg)


def load_config(path):
    """a reference config file -> builder.ConfigDict: the file's module-level names (modules, functions and classes left out), on top
    of the files its `_base_` lists, merged recursively"""
    return ConfigDict.wrap(_load(path))


def parse_args(argv=None):
    """core/apis/helper.py:20-38, the same flags"""
    parser = argparse.ArgumentParser(description='train a nerf')
    parser.add_argument('--config', help='train config file path', default='configs/nerfs/nerf_base01.py')
    parser.add_argument('--dataname', help='data name in dataset', default='ficus')
    parser.add_argument('--test_only', help='set to influence on testset once', action='store_true')
    parser.add_argument('--render_only', help='set to influence on testset once for visualization', action='store_true')
    parser.add_argument('--load_from', help='reset load_from', default='')
    return parser.parse_args(argv)


def replace_dataname(dataname, cfg):
    """every '#DATANAME#' in the cfg's strings, recursively (helper.py:41-49)"""
    if isinstance(cfg, str):
        cfg = cfg.replace('#DATANAME#', dataname)
    elif isinstance(cfg, dict):
        for k in cfg:
            cfg[k] = replace_dataname(dataname, cfg[k])
    elif isinstance(cfg, (list, tuple)):
        # (mmcv's Config hands lists through untouched; the strings the configs parametrise all sit under dicts.  Dicts inside
        # lists -- the hook lists -- are walked so that a save_folder may carry the name as well.)
        for v in cfg:
            if isinstance(v, dict):
                replace_dataname(dataname, v)
    return cfg


def kilo_replace(dataname, cfg):
    """helper.py:52-65: the scene's row of cfg.resolution_table into the places of the cfg its phase reads"""
    resolution = cfg.resolution_table[dataname]
    if cfg.phase == 'pretrain':
        cfg.build_occupancy_tree_config.update({'resolution': resolution})
    elif cfg.phase == 'distill':
        cfg.fix_resolution = resolution
        cfg.total_num_networks = reduce(lambda x, y: x * y, resolution)
        cfg.data['train'].cfg.update({'fixed_resolution': resolution})
        cfg.data['val'].cfg.update({'fixed_resolution': resolution})
    else:
        cfg.model['mlp'].update({'resolution': resolution})
    return cfg


def update_config(dataname, cfg):
    cfg = replace_dataname(dataname, cfg)
    if cfg.method == 'kilo_nerf':
        cfg = kilo_replace(dataname, cfg)
    return cfg


def update_loadfrom(load_from, cfg):
    if len(load_from) > 0:
        cfg.load_from = os.path.join(cfg.work_dir, load_from)
    return cfg


# ------------------------------------------------------------------------------------------ builders
def _device(cfg):
    return torch.device(cfg.get('device', 'cuda' if torch.cuda.is_available() else 'cpu'))


def _refuse(cfg):
    if cfg.get('distributed', False):
        raise NotImplementedError('distributed=True: xrnerf_amd.apis runs a single process (multi-GPU training: xrnerf_amd.dist)')
    if _is_ngp(cfg):
        missing = [k for k in ('sampler', 'mlp', 'render') if k not in cfg.model]
        data_type = cfg.get('data', {}).get('train', {}).get('type')
        if missing or data_type != 'HashNerfDataset':
            raise NotImplementedError('a HashNerfNetwork runs as the instant-ngp config only (sampler, mlp and render in the model dict, '
                                      'HashNerfDataset data): %s' % ('the model dict has no %s' % ', '.join(missing) if missing else
                                                                     'data.train is a %r' % (data_type,)))


def _is_ngp(cfg):
    return (cfg.get('model', None) or {}).get('type') == 'HashNerfNetwork'


def build_dataloader(cfg, mode='train'):
    """helper.py:83-110 -> (loader, dataset): the dataset on the run's device behind an in-process loader of batch size 1"""
    dataset = pipelines.build_dataset(dict(cfg.data[mode], device=_device(cfg)))
    return _runner.DataLoader(dataset), dataset


def get_optimizer(model, cfg):
    """helper.py:113-120: Adam over the model's parameters (animatable_nerf: over model.get_params(), lr alone) with torch.optim.Adam's
    defaults where cfg.optimizer is silent -- as train.FusedAdam (one launch for all tensors) where the parameters are on the GPU, as
    torch.optim.Adam for host tensors"""
    from .train import FusedAdam
    opt = dict(cfg.optimizer)
    kind = opt.pop('type', 'Adam')
    if kind != 'Adam':
        raise NotImplementedError('optimizer type %r: the reference configs all train with Adam' % (kind,))
    if cfg.get('method') == 'animatable_nerf':
        params, opt = model.get_params(), {'lr': opt['lr']}
    else:
        params = [p for p in model.parameters() if p.requires_grad]
    if _is_ngp(cfg):
        # the three NGP tensors (the direction encoding has none) in train.FusedAdam, whose fused EMA state is what the config's EMAHook keeps
        params = [p for p in params if p.numel() > 0]
        ema = [h for h in cfg.get('custom_hooks', None) or [] if h.get('type') == 'EMAHook']
        if ema:
            from .ngp_hooks import EMAHook
            hook = EMAHook(**{k: v for k, v in ema[0].items() if k not in ('type', 'priority')})
            ema_kw = dict(ema_momentum=hook.momentum, ema_warm_up=hook.warm_up)
    if opt.pop('amsgrad', False):
        raise NotImplementedError('optimizer amsgrad=True')
    kw = dict(lr=opt.pop('lr', 1e-3), betas=tuple(opt.pop('betas', (0.9, 0.999))), eps=opt.pop('eps', 1e-8), weight_decay=opt.pop('weight_decay', 0))
    if opt:
        raise NotImplementedError('optimizer keys %r' % sorted(opt))
    if _is_ngp(cfg):
        return FusedAdam(params, **dict(kw, **(ema_kw if ema else {})))
    if params and all(p.is_cuda and p.dtype == torch.float32 for p in params):
        return FusedAdam(params, **kw)
    return torch.optim.Adam(params, **kw)


def _hook_classes():
    from . import evaluate, kilo_distill, kilo_tree, ngp_hooks
    mods = (pipelines, evaluate, kilo_tree, kilo_distill, _runner, ngp_hooks)
    names = ('PassDatasetHook', 'PassSamplerIterHook', 'ModifyBatchsizeHook', 'EMAHook', 'SetValPipelineHook', 'PassIterHook', 'ValidateHook', 'CalElapsedTimeHook', 'TestHook', 'SaveSpiralHook', 'NBSaveSpiralHook',
             'HashSaveSpiralHook', 'OccupationHook', 'SaveDistillResultsHook', 'DistllCycleHook', 'BuildOccupancyTreeHook', 'MipLrUpdaterHook')
    return {n: next(getattr(m, n) for m in mods if hasattr(m, n)) for n in names}


def register_hooks(hook_cfgs, **variables):
    """helper.py:123-138: every entry's `params` are keyword values, its `variables` name entries of the caller's environment"""
    runner = variables['runner']
    classes = _hook_classes()
    for hook_cfg in hook_cfgs:
        if hook_cfg['type'] not in classes:
            raise NotImplementedError('hook %r is not built (built: %r)' % (hook_cfg['type'], sorted(classes)))
        given = {k: variables[v_name] for k, v_name in hook_cfg.get('variables', {}).items()}
        runner.register_hook(classes[hook_cfg['type']](**dict(hook_cfg.get('params', {})), **given))
    return runner


get_runner = _runner.get_runner


def get_root_logger(log_level='INFO'):
    logger = logging.getLogger('xrnerf_amd')
    if not logger.handlers:
        logger.addHandler(logging.StreamHandler())
    logger.setLevel(log_level if isinstance(log_level, int) else getattr(logging, str(log_level).upper(), logging.INFO))
    return logger


# ------------------------------------------------------------------------------------------ entry points
def train_nerf(cfg):
    """core/apis/train.py:14-68 -> the runner, after runner.run(dataloaders, cfg.workflow, cfg.max_iters)"""
    _refuse(cfg)
    train_loader, trainset = build_dataloader(cfg, mode='train')
    val_loader, valset = build_dataloader(cfg, mode='val')
    dataloaders = [train_loader, val_loader]
    network = builder.build_network(cfg.model).to(_device(cfg))
    optimizer = get_optimizer(network, cfg)
    Runner = get_runner(cfg.train_runner)
    extra = {}
    if _is_ngp(cfg):
        # the config still says NerfTrainRunner: the instant-ngp model trains through the span runner over the native loop
        Runner, extra = _runner.NgpIterRunner, dict(trainset=trainset)
    runner = Runner(network, optimizer=optimizer, work_dir=cfg.work_dir, logger=get_root_logger(log_level=cfg.get('log_level', 'INFO')),
                    meta=None, **extra)
    runner.timestamp = cfg.get('timestamp', None)
    runner.register_training_hooks(cfg.lr_config, cfg.optimizer_config, cfg.checkpoint_config, cfg.log_config,
                                   custom_hooks_config=cfg.get('custom_hooks', None))
    register_hooks(cfg.train_hooks, **locals())
    # resume_from restores the run (iteration, epoch, optimiser state) as well, load_from the weights alone
    if cfg.get('resume_from', None):
        runner.resume(cfg.resume_from)
    elif cfg.get('load_from', None) and os.path.exists(cfg.load_from):
        runner.load_checkpoint(cfg.load_from)
    runner.run(dataloaders, cfg.workflow, cfg.max_iters)
    return runner


def test_nerf(cfg):
    """core/apis/test.py:13-52: one pass over the whole test set through val_step (phase 'test') -> the runner"""
    _refuse(cfg)
    cfg.workflow = [('val', 1)]
    test_loader, testset = build_dataloader(cfg, mode='test')
    dataloaders = [test_loader]
    network = builder.build_network(cfg.model).to(_device(cfg))
    Runner = get_runner(cfg.test_runner)
    runner = Runner(network, work_dir=cfg.work_dir, logger=get_root_logger(log_level=cfg.get('log_level', 'INFO')), meta=None)
    runner.timestamp = cfg.get('timestamp', None)
    register_hooks(cfg.test_hooks, **locals())
    runner.load_checkpoint(cfg.load_from)
    runner.run(data_loaders=dataloaders, workflow=cfg.workflow, max_epochs=1)
    return runner


def run_nerf(args):
    """core/apis/api.py:10-18"""
    cfg = load_config(args.config)
    cfg = update_config(args.dataname, cfg)
    cfg = update_loadfrom(args.load_from, cfg)
    if args.test_only or args.render_only:
        cfg['model']['cfg']['phase'] = 'test' if args.test_only else 'render'
        return test_nerf(cfg)
    return train_nerf(cfg)
