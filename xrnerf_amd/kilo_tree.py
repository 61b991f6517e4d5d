"""KiloNeRF distillation as the reference runs it (configs/kilonerf/kilonerf_distill_*.py): the discovery loop that grows the kd-tree of
student networks.  `KiloNerfDistillTrainRunner` (core/runner/kilonerf_runner.py:11-69) with the hooks `SaveDistillResultsHook`
(core/hooks/save_distill_results_hook.py), `DistllCycleHook` (core/hooks/distill_cycle_hook.py) and `OccupationHook`
(core/hooks/train_hooks.py:27-51) as plain classes -- there is no mmcv -- plus `kilo_replace` (core/apis/helper.py:52-65) and
`distill_from_config`, which wires them from a distill config.  Each cycle: validate, keep the best error per network, detect saturated
colour heads, decide per node whether it is fitted or split, pick the split plane, queue the children, save checkpoint.pth, rebuild
data, model and optimiser for the next batch of nodes.

The device side of a validation is ONE call, ops.kilo_val_metrics (xrnerf_amd/csrc/xr_kilotree.hip), and one
blocking read of its [N, 16] table; the tree bookkeeping (`format_error_log`, `process_node_batch`, `log_error_stats`) is a host
function of those per-network numbers.  kilo_distill.calculate_error_metrics / distill() stay as the fixed-resolution shortcut."""
import logging
import os
from collections import deque
from functools import reduce

import numpy as np
import torch

from . import builder, kilo, ops
from .kilodata import Node, calculate_volume
from .pipelines import build_dataset

METRICS = ('mse', 'mae', 'mape', 'quantile_se')
_COLUMN = {'mse': ops.KT_MSE, 'mae': ops.KT_MAE, 'mape': ops.KT_MAPE, 'quantile_se': ops.KT_QUANTILE}


# ------------------------------------------------------------------ the validation numbers
class _PointErrors(dict):
    """errors_per_point of the reference: metric -> [N, P] host tensor.  The row of the split metric comes from the kernel's workspace;
    any other is formed by tensor ops when (and only when) somebody asks for it.  'quantile_se' is None, as in the reference."""

    def __init__(self, out, targets, rows):
        super().__init__(quantile_se=None)
        self._out, self._targets, self._rows = out, targets, rows

    def __missing__(self, metric):
        if metric in self._rows:
            v = self._rows[metric].cpu()
        elif metric in ('mse', 'mae', 'mape'):
            d = self._out - self._targets
            e = {'mse': d * d, 'mae': d.abs()}.get(metric)
            if e is None:
                e = d.abs() / (self._targets.abs() + 0.1)
            v = e.mean(dim=2).cpu()
        else:
            raise KeyError(metric)
        self[metric] = v
        return v


def val_table(out, test_targets, cfg, test_points=None, split_axis=None):
    """one validation of N networks -> (the kernel's [N, 16] table on the HOST: the one blocking read; the split metric's per-point rows
    on the device, or None without split_axis)"""
    N, P = int(out.shape[0]), int(out.shape[1])
    quantile_index = int(P * cfg.quantile_se)
    if not 0 <= quantile_index < P:
        raise IndexError('index %d is out of bounds for dimension 1 with size %d' % (quantile_index, P))
    want_split = split_axis is not None
    table, rows = ops.kilo_val_metrics(out, test_targets, quantile_index, points=test_points if want_split else None, split_axis=split_axis,
                                       split_metric=cfg.get('equal_split_metric', 'mse'), want_point_metric=want_split)
    return table.cpu(), rows


def table_to_errors(host, cfg):
    """the kernel's table (host tensor) -> (errors_per_network, errors_per_network_color, errors_per_network_density, saturation,
    thresholds): the reference's dicts of [N] host tensors, a bool tensor, numpy fp32"""
    per_net, per_color, per_density = {}, {}, {}
    for m in ('mse', 'mape', 'mae', 'quantile_se'):
        c = _COLUMN[m]
        per_net[m] = host[:, c].clone()
        if cfg.outputs == 'density' and m != 'quantile_se':
            per_density[m] = per_net[m]
        if cfg.outputs == 'color_and_density' or m == 'quantile_se':
            per_color[m], per_density[m] = host[:, c + 1].clone(), host[:, c + 2].clone()
    return per_net, per_color, per_density, host[:, ops.KT_SATURATION] != 0, host[:, ops.KT_THRESHOLD].numpy().copy()


def calculate_error_metrics(out, test_targets, cfg, test_points=None, split_axis=None):
    """save_distill_results_hook.py:44-111 on the kernel: -> (errors_per_point, errors_per_network, errors_per_network_color,
    errors_per_network_density, saturation), host tensors as the reference's.  With `split_axis` ([N] ints, -1 = none wanted) and
    `test_points` a sixth value follows: the equal-error split thresholds [N] (numpy fp32, NaN where none was wanted or none exists) of
    cfg.equal_split_metric, from the same call."""
    host, rows = val_table(out, test_targets, cfg, test_points, split_axis)
    per_point = _PointErrors(out, test_targets, {cfg.get('equal_split_metric', 'mse'): rows} if rows is not None else {})
    per_net, per_color, per_density, saturation, thresholds = table_to_errors(host, cfg)
    if split_axis is not None:
        return per_point, per_net, per_color, per_density, saturation, thresholds
    return per_point, per_net, per_color, per_density, saturation


def get_equal_error_split_threshold(test_points, errors, split_axis):
    """save_distill_results_hook.py:24-41 on the kernel: the coordinate along split_axis of the first point, in ascending coordinate
    order, at which the running sum of `errors` exceeds half their total -> numpy fp32 (NaN when the total is zero or not finite).
    test_points [P, 3], errors [P] (non-negative).  The errors ride through the kernel as |e - 0| in all four channels, whose mean is e."""
    pts = torch.as_tensor(test_points, dtype=torch.float32)
    e = torch.as_tensor(errors, dtype=torch.float32)
    dev = pts.device if ops._on_device(pts) else e.device if ops._on_device(e) else torch.device('cuda')
    pts, e = pts.to(dev), e.to(dev)
    out = e.reshape(1, -1, 1).expand(1, e.numel(), 4).contiguous()
    table, _ = ops.kilo_val_metrics(out, torch.zeros_like(out), 0, points=pts.reshape(1, -1, 3), split_axis=[int(split_axis)], split_metric='mae')
    return table[0, ops.KT_THRESHOLD].cpu().numpy()[()]


# ------------------------------------------------------------------ the tree bookkeeping (host only)
def new_best_errors(num_networks):
    """three dicts metric -> [num_networks] of +inf (before_train_iter)"""
    return tuple({m: float('inf') * torch.ones(num_networks) for m in METRICS} for _ in range(3))


def format_error_log(error_log, cur_iter, per_net, per_color, per_density, saturation):
    """the per-network line after_val_iter appends to val_step's error_log entries (in place)"""
    for i in range(len(error_log)):
        error_log[i] += 'network_index:{}, it: {} | '.format(i, cur_iter)
        for m in METRICS:
            error_log[i] += m + ': {:.5f} '.format(per_net[m][i].item())
            error_log[i] += '(d: {:.5f}, c: {:.5f}) '.format(per_density[m][i].item(), per_color[m][i].item())
        if saturation[i]:
            error_log[i] += ' [saturation detected]'
        error_log[i] += '\n'
    return error_log


def longest_axis(node):
    return np.argmax(np.array(node.domain_max) - np.array(node.domain_min))


def process_node_batch(cfg, cp, node_batch, processing_saturated_nodes, best, best_color, best_density, saturation, thresholds=None,
                       get_network=None, cycles_run=None):
    """what after_val_iter does to the tree at a cycle boundary (save_distill_results_hook.py:273-387): per node, fitted (volume and
    best errors recorded, its network kept) or split (axis, threshold, two children queued) or, with saturation_detection, re-queued
    for the low-learning-rate pass.  Changes cp and the nodes in place; -> the number of nodes fitted.
    thresholds: the equal-error split thresholds per network (tree_type 'kdtree_equal_error_split').  cycles_run with cfg.max_tree_cycles:
    once that many cycles have run every node is fitted (not in the reference, whose loop has no bound)."""
    below = 0
    for i, node in enumerate(node_batch):
        split_further = 'stop_after_one_iteration' not in cfg
        if 'max_tree_cycles' in cfg and cycles_run is not None and cycles_run >= cfg.max_tree_cycles:
            split_further = False
        if 'test_error_metric_color' in cfg:
            split_further = split_further and bool(best_color[cfg.test_error_metric_color][i] > cfg.max_error_color or
                                                   best_density[cfg.test_error_metric_density][i] > cfg.max_error_density)
        else:
            split_further = split_further and bool(best[cfg.test_error_metric][i] > cfg.max_error)
        if 'termination_volume' in cfg:
            split_further = split_further and cp['fitted_volume'] / cp['total_volume'] < cfg.termination_volume
        if not split_further:
            below += 1
            cp['fitted_volume'] += calculate_volume(node.domain_min, node.domain_max)
            node.discovery_best_error = {m: best[m][i] for m in METRICS}
            node.discovery_best_error_color = {m: best_color[m][i] for m in METRICS}
            node.discovery_best_error_density = {m: best_density[m][i] for m in METRICS}
            node.network = get_network(i) if get_network is not None else None
            continue
        if 'saturation_detection' in cfg and saturation[i] and not processing_saturated_nodes:
            cp['saturated_nodes_to_process'].append(node)
            continue
        if cfg.tree_type == 'kdtree_random':
            node.split_axis = np.random.randint(low=0, high=3)
        elif cfg.tree_type in ('kdtree_longest', 'kdtree_equal_error_split'):
            node.split_axis = longest_axis(node)
        else:
            raise ValueError('tree_type %r: kdtree_random, kdtree_longest or kdtree_equal_error_split' % (cfg.tree_type,))
        if cfg.tree_type == 'kdtree_equal_error_split':
            node.split_threshold = thresholds[i]
            if node.split_threshold != node.split_threshold:
                raise ValueError('network %d (%s %s): no equal-error split threshold, its validation %s errors sum to zero or are not finite'
                                 % (i, node.domain_min, node.domain_max, cfg.equal_split_metric))
        else:
            lo, hi = node.domain_min[node.split_axis], node.domain_max[node.split_axis]
            node.split_threshold = lo + (hi - lo) / 2
        node.leq_child, node.gt_child = Node(), Node()
        node.leq_child.domain_min, node.leq_child.domain_max = node.domain_min.copy(), node.domain_max.copy()
        node.leq_child.domain_max[node.split_axis] = node.split_threshold
        node.gt_child.domain_min, node.gt_child.domain_max = node.domain_min.copy(), node.domain_max.copy()
        node.gt_child.domain_min[node.split_axis] = node.split_threshold
        queue = cp['saturated_nodes_to_process'] if processing_saturated_nodes else cp['nodes_to_process']
        queue.append(node.leq_child)
        queue.append(node.gt_child)
    cp['num_networks_fitted'] += below
    return below


def log_error_stats(initial_nodes, phase, cfg, filename):
    """save_distill_results_hook.py:114-189 for phase 'discovery': per metric, the volume-weighted mean, the mean and the worst node of the
    best errors recorded in the tree, appended to `filename`"""
    if phase != 'discovery':
        raise NotImplementedError("log_error_stats: only the 'discovery' phase (the reference's 'final' phase belongs to its fine-tuning)")
    both = cfg.outputs == 'color_and_density'
    mins, maxs, volumes = [], [], []
    kinds = ('total', 'color', 'density') if both else ('total',)
    attr = {'total': 'discovery_best_error', 'color': 'discovery_best_error_color', 'density': 'discovery_best_error_density'}
    best = {k: {m: [] for m in METRICS} for k in kinds}
    queue = deque(initial_nodes)
    while queue:
        node = queue.popleft()
        if hasattr(node, 'leq_child'):
            queue.append(node.leq_child)
            queue.append(node.gt_child)
        if hasattr(node, 'discovery_best_error'):
            mins.append(node.domain_min)
            maxs.append(node.domain_max)
            volumes.append(calculate_volume(node.domain_min, node.domain_max))
            for k in kinds:
                for m in METRICS:
                    best[k][m].append(getattr(node, attr[k])[m])
    if not mins:
        return
    volumes = torch.tensor(volumes)
    with open(filename, 'a') as f:
        for m in METRICS:
            f.write('[' + m + ']')
            for k in kinds:
                e = torch.tensor(best[k][m])
                worst = torch.argmax(e)
                f.write('\t{} | weighted mean: {:.5f}, mean: {:.5f}, max: {} {} {:.5f}'.format(
                    k, ((volumes * e).sum() / volumes.sum()).item(), e.mean().item(), mins[worst], maxs[worst], e[worst]) + '\n')


def leaves_to_checkpoint(cp):
    """the distillation's tree -> {'domain_mins', 'domain_maxs', 'state_dict', 'num_hidden_layers'}, leaves in the breadth-first order of
    kilonerf_mlp.py:53-62 (leq_child before gt_child): what KiloNerfMLP(distilled_checkpoint=...) and KiloNerfMLP.from_arrays read"""
    return kilo.tree_to_checkpoint(cp)


# ------------------------------------------------------------------ the hooks
class SaveDistillResultsHook:
    """save_distill_results_hook.py:192-417: keeps the best validation errors of the node batch and, at a cycle boundary, fits or splits
    its nodes and saves the tree to work_dir/checkpoint.pth"""

    def __init__(self, cfg=None, trainset=None):
        assert cfg, 'cfg not input in SaveDistillResultsHook'
        assert trainset, 'trainset not input in SaveDistillResultsHook'
        self.cfg, self.trainset = cfg, trainset

    def before_train_iter(self, runner):
        if runner.iter % self.cfg.max_iters == 0:
            self.best_errors_per_network, self.best_errors_per_network_color, self.best_errors_per_network_density = \
                new_best_errors(self.cfg.num_networks)

    def after_val_iter(self, runner):
        cfg = self.cfg
        axes = None
        if runner.iter % cfg.max_iters == 0 and cfg.tree_type == 'kdtree_equal_error_split':
            axes = [int(longest_axis(node)) for node in self.trainset.get_info()['node_batch']]
        host, _ = val_table(runner.outputs['out'], runner.outputs['target_s'], cfg,
                            test_points=runner.outputs['test_points'] if axes else None, split_axis=axes)
        self.after_val_table(runner, host)

    def after_val_table(self, runner, host):
        """everything after the device: `host` is the validation's [N, 16] table (host tensor)"""
        cfg, cur_iter = self.cfg, runner.iter
        self.error_log = runner.outputs['error_log']
        boundary = cur_iter % cfg.max_iters == 0
        datas = self.trainset.get_info()
        per_net, per_color, per_density, saturation, thresholds = table_to_errors(host, cfg)
        for m in METRICS:
            self.best_errors_per_network[m] = torch.min(per_net[m], self.best_errors_per_network[m])
            if cfg.outputs == 'color_and_density':
                self.best_errors_per_network_color[m] = torch.min(per_color[m], self.best_errors_per_network_color[m])
                self.best_errors_per_network_density[m] = torch.min(per_density[m], self.best_errors_per_network_density[m])
        format_error_log(self.error_log, cur_iter, per_net, per_color, per_density, saturation)
        if not boundary:
            return
        cp, node_batch = datas['cp'], datas['node_batch']
        model = getattr(runner.model, 'module', runner.model)
        below = process_node_batch(cfg, cp, node_batch, datas['processing_saturated_nodes'], self.best_errors_per_network,
                                   self.best_errors_per_network_color, self.best_errors_per_network_density, saturation, thresholds,
                                   get_network=model.multi_network.get_single_network, cycles_run=cur_iter // cfg.max_iters)
        runner.logger.info('detected saturated networks: {}'.format(saturation.sum().item()))
        runner.logger.info('num networks below threshold: {}/{}'.format(below, len(node_batch)))
        runner.logger.info('fitted volume: {}/{} ({}%), num networks fitted: {}'.format(
            cp['fitted_volume'], cp['total_volume'], 100 * cp['fitted_volume'] / cp['total_volume'], cp['num_networks_fitted']))
        runner.logger.info('number of nodes_to_process: {}'.format(len(cp['nodes_to_process'])))
        log = os.path.join(runner.work_dir, 'log.txt')
        with open(log, 'a') as f:
            f.write('\n'.join(self.error_log))
        log_error_stats(cp['root_nodes'], 'discovery', cfg, log)
        checkpoint = runner.work_dir + '/checkpoint.pth'
        torch.save(cp, checkpoint)
        runner.logger.info('Saved to {}'.format(checkpoint))
        all_nodes_processed = len(cp['nodes_to_process']) == 0 and len(cp['saturated_nodes_to_process']) == 0
        if not all_nodes_processed and cur_iter == runner._max_iters:
            runner._max_iters += cfg.max_iters


def _build_optimizer(net, cfg):
    opt = dict(cfg.optimizer)
    kind = opt.pop('type', 'Adam')
    return getattr(torch.optim, kind)(net.get_params(), **opt)


class DistllCycleHook:
    """distill_cycle_hook.py:15-99: the iteration budget from the number of nodes, and at every cycle boundary the next batch of nodes:
    datasets, network, optimiser and the SaveDistillResultsHook that watches them"""

    def __init__(self, cfg=None, build=None):
        assert cfg, 'cfg not input in DistllCycleHook'
        self.cfg = cfg
        self.build = build or build_cycle           # (cfg, index) -> (trainset, valset, network, optimizer)

    def before_run(self, runner):
        cycles = self.cfg.total_num_networks // self.cfg.max_num_networks
        if self.cfg.total_num_networks % self.cfg.max_num_networks != 0:
            cycles += 1
        runner._max_iters = cycles * self.cfg.max_iters

    def after_val_iter(self, runner):
        if runner.iter % self.cfg.max_iters == 0 and runner.iter < runner._max_iters:
            self._update_train_distill_cyle(runner, runner.iter // self.cfg.max_iters)

    def _update_train_distill_cyle(self, runner, index):
        if self.cfg.get('distributed', False):
            raise NotImplementedError('multi-GPU distillation: the node batches of one tree are distilled on one GPU')
        trainset, valset, net, optimizer = self.build(self.cfg, index, teacher=getattr(getattr(runner.model, 'module', runner.model),
                                                                                       'teacher_nerf', None))
        runner.iter_loaders = [IterLoader(trainset), IterLoader(valset)]
        runner.optimizer = optimizer
        runner.model = net
        for i, hook in enumerate(runner.hooks):
            if isinstance(hook, SaveDistillResultsHook):
                runner.hooks[i] = SaveDistillResultsHook(self.cfg, trainset)


def build_cycle(cfg, index, teacher=None):
    """datasets, network and optimiser of node batch `index` (what _update_train_distill_cyle rebuilds, and what distill_from_config
    starts from): batch_index in both dataset cfgs, num_networks in the three places of the cfg, lr 1e-4 while saturated nodes are
    processed"""
    cfg.data['train'].cfg.update({'batch_index': index})
    trainset = build_dataset(cfg.data['train'])
    cfg.data['val'].cfg.update({'batch_index': index})
    valset = build_dataset(cfg.data['val'])
    datas = trainset.get_info()
    n = len(datas['node_batch'])
    cfg.update({'num_networks': n})
    cfg.model.multi_network.update({'num_networks': n})
    cfg.model.multi_network.embedder.update({'num_networks': n})
    model = dict(cfg.model)
    if teacher is not None:
        model.pop('pretrained_kwargs', None)
        model['teacher'] = teacher
    net = builder.build_network(model).to(trainset.device)
    if datas['processing_saturated_nodes']:
        cfg.optimizer.update({'lr': 0.0001})
    return trainset, valset, net, _build_optimizer(net, cfg)


class OccupationHook:
    """train_hooks.py:27-51: work_dir/delete_me_to_stop is made on the first call; once somebody removes it the run stops"""

    def __init__(self):
        self.first_run = True

    def func(self, runner):
        flag_folder = os.path.join(runner.work_dir, 'delete_me_to_stop')
        if self.first_run:
            os.makedirs(flag_folder, exist_ok=True)
            self.first_run = False
        elif not os.path.exists(flag_folder):
            print('Stop now!!!', flush=True)
            raise SystemExit(0)

    def after_train_iter(self, runner):
        self.func(runner)

    def after_val_iter(self, runner):
        self.func(runner)


# ------------------------------------------------------------------ the runner
class IterLoader:
    """mmcv's IterLoader over a dataset whose items are whole batches: item k of the k-th call, wrapping around; every tensor gets the
    leading batch dimension of 1 the reference's DataLoader adds (train_step / val_step strip it)"""

    def __init__(self, dataset):
        self.dataset, self.k = dataset, 0

    def __next__(self):
        item = self.dataset[self.k % max(len(self.dataset), 1)]
        self.k += 1
        dev = self.dataset.device
        return {k: torch.as_tensor(v, dtype=torch.float32).to(dev)[None] if k in ('domain_mins', 'domain_maxs') or torch.is_tensor(v) else v
                for k, v in item.items()}

    def __iter__(self):
        return self


class KiloNerfDistillTrainRunner:
    """kilonerf_runner.py:11-69: mmcv's iteration-based runner with `iter_loaders` as a member, so that a hook can swap the loaders (and
    the model, the optimiser and the hooks) between two cycles.  train() is IterBasedRunner.train with OptimizerHook(grad_clip=None)
    folded in; val() is IterBasedRunner.val."""

    def __init__(self, model, optimizer=None, work_dir=None, logger=None, max_iters=None):
        self.model, self.optimizer, self.work_dir = model, optimizer, work_dir
        self.logger = logger or logging.getLogger('xrnerf_amd.kilo_tree')
        self.iter, self._max_iters, self._inner_iter = 0, max_iters, 0
        self.hooks, self.outputs, self.iter_loaders = [], None, None
        if work_dir:
            os.makedirs(work_dir, exist_ok=True)

    def register_hook(self, hook):
        self.hooks.append(hook)

    def call_hook(self, name):
        for hook in list(self.hooks):
            fn = getattr(hook, name, None)
            if fn is not None:
                fn(self)

    def train(self, loader, **kwargs):
        self.model.train()
        data = next(loader)
        self.call_hook('before_train_iter')
        self.outputs = self.model.train_step(data, self.optimizer, **kwargs)
        self.optimizer.zero_grad()
        self.outputs['loss'].backward()
        self.optimizer.step()
        self.call_hook('after_train_iter')
        self._inner_iter += 1
        self.iter += 1

    @torch.no_grad()
    def val(self, loader, **kwargs):
        self.model.eval()
        data = next(loader)
        ex = data['batch_examples']
        if ex.shape[-1] < 10:               # room for the teacher's targets (columns 6:10), which val_step fills
            data['batch_examples'] = torch.cat([ex, ex.new_zeros(ex.shape[:-1] + (10 - ex.shape[-1],))], -1)
        self.call_hook('before_val_iter')
        self.outputs = self.model.val_step(data, **kwargs)
        self.call_hook('after_val_iter')
        self._inner_iter += 1

    def run(self, data_loaders, workflow, max_iters=None, **kwargs):
        assert isinstance(data_loaders, list) and len(data_loaders) == len(workflow)
        if max_iters is not None:
            self._max_iters = max_iters
        self.call_hook('before_run')
        assert self._max_iters is not None, 'max_iters must be specified during instantiation'
        self.logger.info('workflow: %s, max: %d iters', workflow, self._max_iters)
        self.iter_loaders = [IterLoader(x) for x in data_loaders]
        self.call_hook('before_epoch')
        while self.iter < self._max_iters:
            for i, (mode, iters) in enumerate(workflow):
                self._inner_iter = 0
                if not isinstance(mode, str) or not hasattr(self, mode):
                    raise ValueError('runner has no method named "{}" to run a workflow'.format(mode))
                for _ in range(iters):
                    if mode == 'train' and self.iter >= self._max_iters:
                        break
                    getattr(self, mode)(self.iter_loaders[i], **kwargs)
        self.call_hook('after_epoch')
        self.call_hook('after_run')


# ------------------------------------------------------------------ from a config
def kilo_replace(dataname, cfg):
    """core/apis/helper.py:52-65: the scene's row of cfg.resolution_table into the places of the cfg its phase reads"""
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


HOOKS = {'SaveDistillResultsHook': SaveDistillResultsHook, 'DistllCycleHook': DistllCycleHook, 'OccupationHook': OccupationHook}


def build_distill_runner(cfg, teacher=None, logger=None):
    """datasets, network, optimiser, hooks and runner of a distill config -> (runner, [trainset, valset], workflow); cfg is wrapped and
    completed in place of the caller's: total_num_networks defaults to the number of root nodes, train_hooks to the three hooks of the
    shipped configs"""
    cfg = builder.ConfigDict.wrap(dict(cfg))
    if cfg.get('distributed', False):
        raise NotImplementedError('multi-GPU distillation: the node batches of one tree are distilled on one GPU')
    if cfg.get('train_runner', {'type': 'KiloNerfDistillTrainRunner'})['type'] != 'KiloNerfDistillTrainRunner':
        raise ValueError('distill_from_config runs KiloNerfDistillTrainRunner configs (got %r)' % (cfg.train_runner,))
    os.makedirs(cfg.work_dir, exist_ok=True)
    for mode in ('train', 'val'):
        cfg.data[mode].cfg.setdefault('work_dir', cfg.work_dir)
    trainset, valset, net, optimizer = build_cycle(cfg, 0, teacher=teacher)
    if 'total_num_networks' not in cfg:
        cfg.total_num_networks = len(trainset.get_info()['cp']['root_nodes'])
    runner = KiloNerfDistillTrainRunner(net, optimizer, cfg.work_dir, logger)
    given = {'cfg': cfg, 'trainset': trainset}
    for h in cfg.get('train_hooks', [dict(type=k, params={}, variables=v) for k, v in (
            ('SaveDistillResultsHook', dict(cfg='cfg', trainset='trainset')), ('DistllCycleHook', dict(cfg='cfg')), ('OccupationHook', {}))]):
        runner.register_hook(HOOKS[h['type']](**dict(h.get('params', {})), **{k: given[v] for k, v in h.get('variables', {}).items()}))
    return runner, [trainset, valset], [tuple(w) for w in cfg.workflow]


def distill_from_config(cfg, teacher=None, logger=None):
    """run a distill config (a dict with the keys of configs/kilonerf/kilonerf_distill_*.py, after kilo_replace) to the end of its
    discovery loop -> the final cp ({'root_nodes', 'fitted_volume', 'num_networks_fitted', ...}; work_dir/checkpoint.pth holds the same).
    teacher: the NerfMLP-like module to distil, in place of model.pretrained_kwargs."""
    runner, datasets, workflow = build_distill_runner(cfg, teacher, logger)
    runner.run(datasets, workflow)
    return final_cp(runner, datasets[0])


def final_cp(runner, trainset):
    """the tree as the last cycle's SaveDistillResultsHook left it"""
    save = [h for h in runner.hooks if isinstance(h, SaveDistillResultsHook)]
    return (save[0].trainset if save else trainset).get_info()['cp']
