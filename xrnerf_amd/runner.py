"""The training / test runners a reference config names (train_runner, test_runner) and the four hooks its lr_config, optimizer_config,
checkpoint_config and log_config stand for -- without mmcv.  What mmcv's IterBasedRunner / EpochBasedRunner do is restated here as the
reference's call sites use it (core/apis/train.py, test.py, core/runner/*.py), AS REMEMBERED AND UNVERIFIED AGAINST MMCV (DESIGN.md
section 26 lists every such rule: hook order and priorities, the 'step' LR policy, the checkpoint layout, resume).

Device side of an iteration, besides the family's own step: FusedAdam.step (one xr_adam_step_list launch for all of a network's tensors)
and LogWindow.update (one xr_log_window_add launch: the iteration's log scalars never leave the device until the logger's interval ends).
"""
import logging
import os
from collections import OrderedDict

import numpy as np
import torch

from . import ops

# mmcv's priority names (lower runs first; hooks of equal priority run in registration order)
PRIORITY = {'HIGHEST': 0, 'VERY_HIGH': 10, 'HIGH': 30, 'ABOVE_NORMAL': 40, 'NORMAL': 50, 'BELOW_NORMAL': 60, 'LOW': 70, 'VERY_LOW': 90,
            'LOWEST': 100}
# mmcv's Hook base class routes the mode-specific stages to the general ones (before_train_iter -> before_iter, ...)
_GENERAL = {'before_train_epoch': 'before_epoch', 'before_val_epoch': 'before_epoch', 'after_train_epoch': 'after_epoch',
            'after_val_epoch': 'after_epoch', 'before_train_iter': 'before_iter', 'before_val_iter': 'before_iter',
            'after_train_iter': 'after_iter', 'after_val_iter': 'after_iter'}


# ------------------------------------------------------------------------------------------ the log window
class LogWindow:
    """mmcv's LogBuffer over one logging interval, with the sums on the device: update() adds v * num_samples and num_samples per name,
    read() returns LogBuffer.average's value, sum(v n) / sum(n), per name and clears the window.  A device scalar (a one-element fp32
    tensor the library can take) goes into the device window by ONE launch per update, nothing is read back; read() is the only blocking
    read.  Host values (Python numbers, host tensors) take the same arithmetic -- double sums in update order -- on the host."""

    def __init__(self):
        self.names, self.window, self.host = [], None, OrderedDict()

    def update(self, log_vars, num_samples=1):
        n = int(num_samples)
        dev = []
        for k, v in log_vars.items():
            if isinstance(v, torch.Tensor) and ops._on_device(v) and v.numel() == 1 and ops.optim_kernels_available():
                dev.append((k, v))
            else:
                s = self.host.setdefault(k, [0.0, 0.0])
                s[0] += float(v) * float(n)
                s[1] += float(n)
        if not dev:
            return
        for k, _ in dev:
            if k not in self.names:
                if len(self.names) == ops.LOG_WINDOW_SLOTS:
                    raise ValueError('LogWindow holds %d device scalars (got %r beyond %r)' % (ops.LOG_WINDOW_SLOTS, k, self.names))
                self.names.append(k)
        if self.window is None:
            self.window = torch.zeros(2 * ops.LOG_WINDOW_SLOTS, dtype=torch.float64, device=dev[0][1].device)
        # slot order is first-seen order; names missing from this update keep their sums: one launch per run of consecutive slots
        vals = {k: (v.detach().reshape(1) if v.dtype == torch.float32 else v.detach().reshape(1).float()) for k, v in dev}
        run, start = [], 0
        for i, name in enumerate(self.names + [None]):
            if name in vals:
                if not run:
                    start = i
                run.append(vals[name])
            elif run:
                ops.log_window_add(run, n, self.window, first_slot=start)
                run = []

    def reserve(self, names, device):
        """named slots of the device window for a producer that adds to it itself (ops.ngp_log_add, the native instant-ngp loop): the window
        is made on `device` when there is none yet -> (window tensor, slot of names[0], slot of names[1], ...).  read() serves them like any
        other name."""
        device = torch.device(device)
        if self.window is None:
            self.window = torch.zeros(2 * ops.LOG_WINDOW_SLOTS, dtype=torch.float64, device=device)
        elif self.window.device != device:
            raise ValueError('LogWindow.reserve: the window lives on %s, not on %s' % (self.window.device, device))
        for k in names:
            if k not in self.names:
                if len(self.names) == ops.LOG_WINDOW_SLOTS:
                    raise ValueError('LogWindow holds %d device scalars (got %r beyond %r)' % (ops.LOG_WINDOW_SLOTS, k, self.names))
                self.names.append(k)
        return (self.window,) + tuple(self.names.index(k) for k in names)

    def read(self):
        """-> OrderedDict name -> float (the window's weighted average); the window starts again from zero"""
        out = OrderedDict()
        if self.window is not None and self.names:
            w = self.window.to('cpu', copy=True).numpy()     # the blocking read (a copy: a host window is cleared below)
            self.window.zero_()
            S = ops.LOG_WINDOW_SLOTS
            for i, k in enumerate(self.names):
                if w[S + i] > 0:
                    out[k] = float(w[i] / w[S + i])
        for k, (sv, sn) in self.host.items():
            if sn > 0:
                out[k] = float(np.float64(sv) / np.float64(sn))
        self.host = OrderedDict()
        return out


# ------------------------------------------------------------------------------------------ loaders
class _DatasetIter:
    """what iter(DataLoader) is to PassIterHook: `_dataset`, and the items of one pass (pipelines.iterate: views, no workers)"""

    def __init__(self, dataset):
        from . import pipelines
        self._dataset = dataset
        self._it = pipelines.iterate(dataset)

    def __next__(self):
        return next(self._it)


class DataLoader:
    """the in-process stand-in for DataLoader(dataset, batch_size=1): one pass over pipelines.iterate(dataset) per iter()"""

    def __init__(self, dataset):
        self.dataset = dataset

    def __iter__(self):
        return _DatasetIter(self.dataset)

    def __len__(self):
        return len(self.dataset)


class IterLoader:
    """mmcv's IterLoader: an endless iterator over a loader that counts its passes (`epoch`) and keeps the current pass as `iter_loader`"""

    def __init__(self, dataloader):
        self._dataloader = dataloader
        self.iter_loader = iter(dataloader)
        self._epoch = 0

    @property
    def epoch(self):
        return self._epoch

    def __next__(self):
        try:
            return next(self.iter_loader)
        except StopIteration:
            self._epoch += 1
            self.iter_loader = iter(self._dataloader)
            return next(self.iter_loader)

    def __len__(self):
        return len(self._dataloader)


# ------------------------------------------------------------------------------------------ built-in hooks
def every_n_iters(runner, n):
    return (runner.iter + 1) % n == 0 if n > 0 else False


class LrUpdaterHook:
    """mmcv's LrUpdaterHook for by_epoch=False without warm-up: base_lr is each group's initial_lr, and before every training iteration
    the groups get get_lr(runner, base_lr)"""

    def __init__(self, by_epoch=False, warmup=None, **kwargs):
        if by_epoch:
            raise NotImplementedError('lr_config by_epoch=True: the reference configs all step by iteration')
        if warmup is not None:
            raise NotImplementedError('lr_config warmup=%r' % (warmup,))
        if kwargs:
            raise NotImplementedError('lr_config keys %r' % sorted(kwargs))
        self.by_epoch, self.base_lr = by_epoch, []

    def before_run(self, runner):
        for group in runner.optimizer.param_groups:
            group.setdefault('initial_lr', group['lr'])
        self.base_lr = [group['initial_lr'] for group in runner.optimizer.param_groups]

    def before_train_iter(self, runner):
        for group, base in zip(runner.optimizer.param_groups, self.base_lr):
            group['lr'] = self.get_lr(runner, base)


class StepLrUpdaterHook(LrUpdaterHook):
    """policy='step': base_lr * gamma ** (iter // step) for an int step, gamma ** (milestones passed) for a list; min_lr clips"""

    def __init__(self, step, gamma=0.1, min_lr=None, **kwargs):
        super().__init__(**kwargs)
        if isinstance(step, (list, tuple)):
            assert all(isinstance(s, int) and s > 0 for s in step)
        elif not (isinstance(step, int) and step > 0):
            raise TypeError('"step" must be a list or a positive integer')
        self.step, self.gamma, self.min_lr = step, gamma, min_lr

    def get_lr(self, runner, base_lr):
        progress = runner.iter
        if isinstance(self.step, int):
            exp = progress // self.step
        else:
            exp = len(self.step)
            for i, s in enumerate(self.step):
                if progress < s:
                    exp = i
                    break
        lr = base_lr * self.gamma ** exp
        return max(lr, self.min_lr) if self.min_lr is not None else lr


class MipLrUpdaterHook(LrUpdaterHook):
    """core/hooks/train_hooks.py:55-84 (policy='Mip'): log-linear interpolation from lr_init to lr_final, times a delay factor"""

    def __init__(self, lr_init, lr_final, max_steps, lr_delay_steps=0, lr_delay_mult=1, **kwargs):
        super().__init__(**kwargs)
        self.lr_init, self.lr_final, self.max_steps = lr_init, lr_final, max_steps
        self.lr_delay_steps, self.lr_delay_mult = lr_delay_steps, lr_delay_mult

    def get_lr(self, runner, base_lr):
        step = runner.epoch if self.by_epoch else runner.iter
        if self.lr_delay_steps > 0:
            delay_rate = self.lr_delay_mult + (1 - self.lr_delay_mult) * np.sin(0.5 * np.pi * np.clip(step / self.lr_delay_steps, 0, 1))
        else:
            delay_rate = 1.
        t = np.clip(step / self.max_steps, 0, 1)
        log_lerp = np.exp(np.log(self.lr_init) * (1 - t) + np.log(self.lr_final) * t)
        return delay_rate * log_lerp


LR_POLICIES = {'step': StepLrUpdaterHook, 'Mip': MipLrUpdaterHook}


class OptimizerHook:
    """mmcv's OptimizerHook with grad_clip=None: zero_grad, backward, step after every training iteration"""

    def __init__(self, grad_clip=None, **kwargs):
        if grad_clip is not None:
            raise NotImplementedError('optimizer_config grad_clip=%r: gradient clipping is not built' % (grad_clip,))
        if kwargs:
            raise NotImplementedError('optimizer_config keys %r' % sorted(kwargs))

    def after_train_iter(self, runner):
        runner.optimizer.zero_grad()
        runner.outputs['loss'].backward()
        runner.optimizer.step()


class CheckpointHook:
    """mmcv's CheckpointHook for by_epoch=False: work_dir/iter_N.pth every `interval` iterations (N = iterations finished), latest.pth -> it"""

    def __init__(self, interval=-1, by_epoch=False, save_optimizer=True, out_dir=None, **kwargs):
        if by_epoch:
            raise NotImplementedError('checkpoint_config by_epoch=True')
        if kwargs:
            raise NotImplementedError('checkpoint_config keys %r' % sorted(kwargs))
        self.interval, self.save_optimizer, self.out_dir = interval, save_optimizer, out_dir

    def after_train_iter(self, runner):
        if every_n_iters(runner, self.interval):
            runner.save_checkpoint(self.out_dir or runner.work_dir, save_optimizer=self.save_optimizer)


class TextLoggerHook:
    """one line per `interval` training iterations: the iteration, the learning rate and the window's averages (LogWindow.read -- the
    one blocking read of the interval)"""

    def __init__(self, interval=10, by_epoch=False, **kwargs):
        self.interval = interval

    def after_train_iter(self, runner):
        if every_n_iters(runner, self.interval):
            avg = runner.log_buffer.read()
            avg.update(getattr(runner, 'log_extra', {}))
            lr = runner.optimizer.param_groups[0]['lr'] if runner.optimizer is not None else float('nan')
            runner.log_output = avg
            runner.log_history.append((runner.iter + 1, float(lr), dict(avg)))
            runner.logger.info('Iter [%d/%d]\tlr: %.3e, %s', runner.iter + 1, runner.max_iters, lr,
                               ', '.join('%s: %s' % (k, ('%.4f' % v) if isinstance(v, float) else v) for k, v in avg.items()))


# ------------------------------------------------------------------------------------------ runners
class BaseRunner:
    def __init__(self, model, optimizer=None, work_dir=None, logger=None, meta=None, max_iters=None, max_epochs=None):
        self.model, self.optimizer, self.work_dir, self.meta = model, optimizer, work_dir, meta
        self.logger = logger or logging.getLogger('xrnerf_amd')
        self._hooks, self._iter, self._epoch, self._inner_iter = [], 0, 0, 0
        self._max_iters, self._max_epochs = max_iters, max_epochs
        self.mode, self.outputs, self.data_loader, self.timestamp = None, None, None, None
        self.log_buffer, self.log_output, self.log_extra, self.log_history = LogWindow(), OrderedDict(), {}, []
        if work_dir:
            os.makedirs(work_dir, exist_ok=True)

    iter = property(lambda self: self._iter)
    epoch = property(lambda self: self._epoch)
    inner_iter = property(lambda self: self._inner_iter)
    max_iters = property(lambda self: self._max_iters)
    max_epochs = property(lambda self: self._max_epochs)
    hooks = property(lambda self: self._hooks)

    def register_hook(self, hook, priority='NORMAL'):
        """behind every registered hook of the same or a higher priority (mmcv's insertion rule)"""
        hook.priority = PRIORITY[priority] if isinstance(priority, str) else int(priority)
        at = len(self._hooks)
        while at > 0 and self._hooks[at - 1].priority > hook.priority:
            at -= 1
        self._hooks.insert(at, hook)

    def call_hook(self, name):
        for hook in list(self._hooks):
            fn = getattr(hook, name, None)
            if fn is None and name in _GENERAL:
                fn = getattr(hook, _GENERAL[name], None)
            if fn is not None:
                fn(self)

    def register_training_hooks(self, lr_config, optimizer_config=None, checkpoint_config=None, log_config=None, custom_hooks_config=None):
        """mmcv's order: LR (VERY_HIGH), optimiser (ABOVE_NORMAL), checkpoint (NORMAL), loggers (VERY_LOW)"""
        if lr_config is not None:
            cfg = dict(lr_config)
            policy = cfg.pop('policy')
            if policy not in LR_POLICIES:
                raise NotImplementedError('lr_config policy %r (built: %r)' % (policy, sorted(LR_POLICIES)))
            self.register_hook(LR_POLICIES[policy](**cfg), 'VERY_HIGH')
        if optimizer_config is not None:
            self.register_hook(OptimizerHook(**dict(optimizer_config)), 'ABOVE_NORMAL')
        if checkpoint_config is not None:
            self.register_hook(CheckpointHook(**dict(checkpoint_config)), 'NORMAL')
        if log_config is not None:
            for h in log_config.get('hooks', []):
                if h['type'] != 'TextLoggerHook':
                    raise NotImplementedError('log_config hook %r: only TextLoggerHook is built' % (h['type'],))
                self.register_hook(TextLoggerHook(interval=log_config.get('interval', 10), **{k: v for k, v in h.items() if k != 'type'}),
                                   'VERY_LOW')
        if custom_hooks_config:
            raise NotImplementedError('custom_hooks %r (EMAHook belongs to the instant-ngp path: train.Trainer)' % (custom_hooks_config,))

    # -------------------------------------------------------------- checkpoints
    def _module(self):
        return getattr(self.model, 'module', self.model)

    def save_checkpoint(self, out_dir, filename_tmpl='iter_{}.pth', save_optimizer=True, create_symlink=True):
        os.makedirs(out_dir, exist_ok=True)
        meta = dict(self.meta or {}, iter=self.iter + 1, epoch=self.epoch + 1)
        ckpt = {'meta': meta, 'state_dict': OrderedDict((k, v.detach().cpu()) for k, v in self._module().state_dict().items())}
        if save_optimizer and self.optimizer is not None:
            ckpt['optimizer'] = self.optimizer.state_dict()
        name = filename_tmpl.format(self.iter + 1)
        torch.save(ckpt, os.path.join(out_dir, name))
        if create_symlink:
            link = os.path.join(out_dir, 'latest.pth')
            if os.path.lexists(link):
                os.remove(link)
            os.symlink(name, link)

    def load_checkpoint(self, filename, map_location='cpu', strict=False):
        self.logger.info('load checkpoint from %s', filename)
        ckpt = torch.load(filename, map_location=map_location, weights_only=False)
        state = ckpt['state_dict'] if 'state_dict' in ckpt else ckpt
        state = OrderedDict((k[7:] if k.startswith('module.') else k, v) for k, v in state.items())
        self._module().load_state_dict(state, strict=strict)
        return ckpt

    def resume(self, checkpoint, resume_optimizer=True, map_location='cpu'):
        ckpt = self.load_checkpoint(checkpoint, map_location=map_location)
        self._epoch = ckpt['meta']['epoch']
        self._iter = ckpt['meta']['iter']
        self._inner_iter = ckpt['meta']['iter']
        if 'optimizer' in ckpt and resume_optimizer and self.optimizer is not None:
            self.optimizer.load_state_dict(ckpt['optimizer'])
        self.logger.info('resumed from epoch: %d, iter %d', self.epoch, self.iter)


class IterRunner(BaseRunner):
    """mmcv's IterBasedRunner as core/apis/train.py drives it: run(data_loaders, workflow, max_iters)"""

    def _log(self, outputs):
        if 'log_vars' in outputs:
            self.log_buffer.update(outputs['log_vars'], outputs['num_samples'])

    def train(self, data_loader, **kwargs):
        self.model.train()
        self.mode = 'train'
        self.data_loader = data_loader
        self._epoch = data_loader.epoch
        data_batch = next(data_loader)
        self.data_batch = data_batch
        self.call_hook('before_train_iter')
        outputs = self.model.train_step(data_batch, self.optimizer, **kwargs)
        if not isinstance(outputs, dict):
            raise TypeError('model.train_step() must return a dict')
        self._log(outputs)
        self.outputs = outputs
        self.call_hook('after_train_iter')
        del self.data_batch
        self._inner_iter += 1
        self._iter += 1

    @torch.no_grad()
    def val(self, data_loader, **kwargs):
        self.model.eval()
        self.mode = 'val'
        self.data_loader = data_loader
        data_batch = next(data_loader)
        self.data_batch = data_batch
        self.call_hook('before_val_iter')
        outputs = self.model.val_step(data_batch, **kwargs)
        if not isinstance(outputs, dict):
            raise TypeError('model.val_step() must return a dict')
        self._log(outputs)
        self.outputs = outputs
        self.call_hook('after_val_iter')
        del self.data_batch
        self._inner_iter += 1

    def run(self, data_loaders, workflow, max_iters=None, **kwargs):
        assert isinstance(data_loaders, list) and len(data_loaders) == len(workflow)
        workflow = [tuple(w) for w in workflow]
        if max_iters is not None:
            self._max_iters = max_iters
        assert self._max_iters is not None, 'max_iters must be specified'
        self.logger.info('workflow: %s, max: %d iters', workflow, self._max_iters)
        self.call_hook('before_run')
        iter_loaders = [x if isinstance(x, IterLoader) else IterLoader(x) for x in data_loaders]
        self.call_hook('before_epoch')
        while self.iter < self._max_iters:
            for i, (mode, iters) in enumerate(workflow):
                self._inner_iter = 0
                if not isinstance(mode, str) or not hasattr(self, mode):
                    raise ValueError('runner has no method named "{}" to run a workflow'.format(mode))
                iter_runner = getattr(self, mode)
                for _ in range(iters):
                    if mode == 'train' and self.iter >= self._max_iters:
                        break
                    iter_runner(iter_loaders[i], **kwargs)
        self.call_hook('after_epoch')
        self.call_hook('after_run')


class EpochRunner(BaseRunner):
    """mmcv's EpochBasedRunner as core/apis/test.py drives it: run(data_loaders, [('val', 1)], max_epochs=1).  A 'val' pass does not
    advance the epoch (the reference's TestHook / NBSaveSpiralHook do that themselves, in after_val_epoch)"""

    def run_iter(self, data_batch, train_mode, **kwargs):
        if train_mode:
            outputs = self.model.train_step(data_batch, self.optimizer, **kwargs)
        else:
            outputs = self.model.val_step(data_batch, self.optimizer, **kwargs)
        if not isinstance(outputs, dict):
            raise TypeError('"train_step()" or "val_step()" must return a dict')
        if 'log_vars' in outputs:
            self.log_buffer.update(outputs['log_vars'], outputs['num_samples'])
        self.outputs = outputs

    def train(self, data_loader, **kwargs):
        self.model.train()
        self.mode = 'train'
        self.data_loader = data_loader
        self._max_iters = self._max_epochs * len(self.data_loader)
        self.call_hook('before_train_epoch')
        for i, data_batch in enumerate(self.data_loader):
            self.data_batch = data_batch
            self._inner_iter = i
            self.call_hook('before_train_iter')
            self.run_iter(data_batch, train_mode=True, **kwargs)
            self.call_hook('after_train_iter')
            del self.data_batch
            self._iter += 1
        self.call_hook('after_train_epoch')
        self._epoch += 1

    @torch.no_grad()
    def val(self, data_loader, **kwargs):
        self.model.eval()
        self.mode = 'val'
        self.data_loader = data_loader
        self.call_hook('before_val_epoch')
        for i, data_batch in enumerate(self.data_loader):
            self.data_batch = data_batch
            self._inner_iter = i
            self.call_hook('before_val_iter')
            self.run_iter(data_batch, train_mode=False)
            self.call_hook('after_val_iter')
            del self.data_batch
        self.call_hook('after_val_epoch')

    def run(self, data_loaders, workflow, max_epochs=None, **kwargs):
        assert isinstance(data_loaders, list) and len(data_loaders) == len(workflow)
        workflow = [tuple(w) for w in workflow]
        if max_epochs is not None:
            self._max_epochs = max_epochs
        assert self._max_epochs is not None, 'max_epochs must be specified'
        self.call_hook('before_run')
        while self.epoch < self._max_epochs:
            before = self.epoch
            for i, (mode, epochs) in enumerate(workflow):
                if not isinstance(mode, str) or not hasattr(self, mode):
                    raise ValueError('runner has no method named "{}" to run an epoch'.format(mode))
                for _ in range(epochs):
                    if mode == 'train' and self.epoch >= self._max_epochs:
                        break
                    getattr(self, mode)(data_loaders[i], **kwargs)
            if self.epoch == before:
                raise RuntimeError('the workflow %r never advances the epoch: a test run needs a hook that does (TestHook, '
                                   'NBSaveSpiralHook)' % (workflow,))
        self.call_hook('after_run')


class NerfTrainRunner(IterRunner):
    """core/runner/base.py"""


class NerfTestRunner(EpochRunner):
    """core/runner/base.py"""


class KiloNerfTrainRunner(IterRunner):
    """core/runner/kilonerf_runner.py:72-74"""


class KiloNerfTestRunner(EpochRunner):
    """core/runner/kilonerf_runner.py:77-79"""


def bungee_stages(runner, data_batch, rands=None, **kwargs):
    """core/runner/bungeenerf_runner.py:18-33: one training step per stage of the batch, each with its own before / after hooks (the
    optimiser hook among them); a stage whose loss is exactly 0 (no ray of that scale in the batch) is skipped before it is logged or
    stepped.  Each stage gets a shallow copy of the batch (the reference hands every stage the same dict, which train_step mutates: its
    second stage would see the first stage's fine z_vals and fail on the 'samples' tuple).  rands: per-stage resampling draws, or None.
    Shared by BungeeNerfTrainRunner.train and bungee.train_iteration.  -> the per-stage train_step outputs."""
    outs = []
    scale_code = data_batch['scale_code']
    for stage in range(int(torch.max(scale_code) + 1)):
        kwargs['stage'] = stage
        if rands is not None:
            kwargs['rand'] = rands[stage]
        runner.call_hook('before_train_iter')
        outputs = runner.model.train_step(dict(data_batch), runner.optimizer, **kwargs)
        if not isinstance(outputs, dict):
            raise TypeError('model.train_step() must return a dict')
        outs.append(outputs)
        if 'log_vars' in outputs:
            if outputs['log_vars']['loss'] == 0.:
                continue
            runner.log_buffer.update(outputs['log_vars'], outputs['num_samples'])
            runner.log_extra['stage'] = stage
        runner.outputs = outputs
        runner.call_hook('after_train_iter')
    return outs


class BungeeNerfTrainRunner(IterRunner):
    """core/runner/bungeenerf_runner.py:10-36"""

    def train(self, data_loader, **kwargs):
        self.model.train()
        self.mode = 'train'
        self.data_loader = data_loader
        self._epoch = data_loader.epoch
        data_batch = next(data_loader)
        self.data_batch = data_batch
        bungee_stages(self, data_batch, **kwargs)
        del self.data_batch
        self._inner_iter += 1
        self._iter += 1


class BungeeNerfTestRunner(EpochRunner):
    """core/runner/bungeenerf_runner.py:39-41"""


def _kilo_distill_runner():
    from .kilo_tree import KiloNerfDistillTrainRunner
    return KiloNerfDistillTrainRunner


class _At:
    """what an LrUpdaterHook's get_lr reads of a runner, at a given iteration"""

    def __init__(self, it, epoch=0):
        self.iter, self.epoch = it, epoch


def _per_iteration_methods(hook):
    """the per-iteration stages a hook defines (mode-specific or general), by name"""
    return [n for n in ('before_train_iter', 'after_train_iter', 'before_iter', 'after_iter') if callable(getattr(hook, n, None))]


class NgpIterRunner(IterRunner):
    """The instant-ngp config's training runner: IterRunner whose ('train', n) pairs run as SPANS of the native loop
    -- one train.Trainer.run(k) per span, i.e. one native call per refresh window with the per-iteration path at the refreshes, exactly as
    bench.py drives it -- instead of one Python train_step per 0.34-ms iteration.  A span ends at the earliest of the pair's end, max_iters
    and the next iteration at which a hook is due:
      absorbed   LrUpdaterHook (-> the trainer's lr_at), OptimizerHook(grad_clip=None), EMAHook, PassSamplerIterHook, ModifyBatchsizeHook
                 (the trainer does their per-iteration work), PassIterHook and OccupationHook (run at every span's end: the dataset gets
                 the span's last iteration) -- never end a span
      interval   CheckpointHook, TextLoggerHook: due where (i + 1) % interval == 0
      other      a hook with a before_ / after_ _train_iter or _iter method: due every iteration (spans of 1: correct, only slow)
    At a span's end the due hooks' after_train_iter run in priority order with runner.iter = the span's last iteration.  Every iteration's
    loss and psnr reach the log window on the device (LogWindow.reserve -> Trainer(log_window=)).  `val` pairs are IterRunner.val.
    `engine`: anything with run(k) -> the last iteration's outputs and an `iter` attribute (default: a train.Trainer over `trainset`, built
    behind the before_run hooks)."""

    def __init__(self, model, optimizer=None, work_dir=None, logger=None, meta=None, max_iters=None, max_epochs=None, trainset=None,
                 engine=None, device=None):
        super().__init__(model, optimizer=optimizer, work_dir=work_dir, logger=logger, meta=meta, max_iters=max_iters, max_epochs=max_epochs)
        self.trainset, self.engine, self.device = trainset, engine, device
        self.lr_at = None

    def register_training_hooks(self, lr_config, optimizer_config=None, checkpoint_config=None, log_config=None, custom_hooks_config=None):
        """IterRunner's, and custom_hooks=[dict(type='EMAHook', ...)] (mmcv registers custom hooks at their `priority`, NORMAL by default)"""
        from .ngp_hooks import EMAHook
        super().register_training_hooks(lr_config, optimizer_config, checkpoint_config, log_config, None)
        for h in custom_hooks_config or []:
            h = dict(h)
            kind = h.pop('type')
            if kind != 'EMAHook':
                raise NotImplementedError('custom hook %r: only EMAHook is built' % (kind,))
            priority = h.pop('priority', 'NORMAL')
            self.register_hook(EMAHook(**h), priority)

    def resume(self, checkpoint, resume_optimizer=True, map_location='cpu'):
        super().resume(checkpoint, resume_optimizer=resume_optimizer, map_location=map_location)
        from .ngp_hooks import EMAHook
        for h in self._hooks:
            if isinstance(h, EMAHook) and h.registered:
                h.alias(self)                  # the optimiser's loaded state tensors are new ones: the buffers name them again

    # -------------------------------------------------------------- planning
    def _classify(self):
        from .kilo_tree import OccupationHook
        from .ngp_hooks import EMAHook, ModifyBatchsizeHook, PassDatasetHook, PassSamplerIterHook
        from .pipelines import PassIterHook
        absorbed = (LrUpdaterHook, OptimizerHook, EMAHook, PassSamplerIterHook, ModifyBatchsizeHook)
        self._span_end, self._interval, self._every = [], [], []
        for h in self._hooks:
            if isinstance(h, absorbed):
                continue
            if isinstance(h, (PassIterHook, OccupationHook)):
                self._span_end.append(h)
            elif isinstance(h, (CheckpointHook, TextLoggerHook)):
                self._interval.append(h)
            elif _per_iteration_methods(h):
                self._every.append(h)

    def _next_due(self, i):
        """the first iteration >= i at which an interval hook or a per-iteration hook is due (None: never)"""
        if self._every:
            return i
        due = [i + (-(i + 1)) % h.interval for h in self._interval if h.interval and h.interval > 0]
        return min(due) if due else None

    def _make_engine(self):
        from .train import Trainer
        lr_hooks = [h for h in self._hooks if isinstance(h, LrUpdaterHook)]
        if lr_hooks:
            hook, base = lr_hooks[0], lr_hooks[0].base_lr[0]
            self.lr_at = lambda it: float(hook.get_lr(_At(it), base))
        else:
            lr = self.optimizer.param_groups[0]['lr']
            self.lr_at = lambda it: lr
        if self.engine is None:
            device = torch.device(self.device) if self.device is not None else next(self.model.parameters()).device
            self.engine = Trainer(device, dataset=self.trainset, net=self._module(), optimizer=self.optimizer, lr_at=self.lr_at,
                                  log_window=self.log_buffer.reserve(('loss', 'psnr'), device))
        self.engine.iter = self.iter               # (a resumed run goes on at its iteration)

    def train_span(self, data_loader, n):
        """up to `n` training iterations of one ('train', n) workflow pair, as spans"""
        self.model.train()
        self.mode = 'train'
        self.data_loader = data_loader
        self._epoch = data_loader.epoch
        end = min(self.iter + n, self._max_iters)
        while self.iter < end:
            first = self.iter
            due = self._next_due(first)
            last = end - 1 if due is None else min(end - 1, due)
            k = last - first + 1
            for h in self._every:                  # (spans of 1: runner.iter is the iteration about to run)
                fn = getattr(h, 'before_train_iter', None) or getattr(h, 'before_iter', None)
                if fn is not None:
                    fn(self)
            outputs = self.engine.run(k)
            if not isinstance(outputs, dict):
                raise TypeError('the engine\'s run() must return a dict')
            self.outputs = outputs
            self._iter, self._inner_iter = last, self._inner_iter + k - 1
            if self.optimizer is not None:         # what the text logger prints: the last iteration's
                for group in self.optimizer.param_groups:
                    group['lr'] = self.lr_at(last)
            for h in list(self._hooks):            # priority order
                if h in self._span_end or h in self._every or (h in self._interval and every_n_iters(self, h.interval)):
                    fn = getattr(h, 'after_train_iter', None) or getattr(h, 'after_iter', None)
                    if fn is not None:
                        fn(self)
            self._inner_iter += 1
            self._iter += 1

    def run(self, data_loaders, workflow, max_iters=None, **kwargs):
        # (apis.train_nerf always hands the train and the val loader: a workflow of ('train', n) alone uses the first)
        assert isinstance(data_loaders, list) and len(data_loaders) >= len(workflow)
        workflow = [tuple(w) for w in workflow]
        if max_iters is not None:
            self._max_iters = max_iters
        assert self._max_iters is not None, 'max_iters must be specified'
        self.logger.info('workflow: %s, max: %d iters', workflow, self._max_iters)
        self.call_hook('before_run')
        self._classify()
        self._make_engine()
        iter_loaders = [x if isinstance(x, IterLoader) else IterLoader(x) for x in data_loaders]
        self.call_hook('before_epoch')
        while self.iter < self._max_iters:
            for i, (mode, iters) in enumerate(workflow):
                self._inner_iter = 0
                if not isinstance(mode, str) or not hasattr(self, mode):
                    raise ValueError('runner has no method named "{}" to run a workflow'.format(mode))
                if mode == 'train':
                    self.train_span(iter_loaders[i], iters)
                else:
                    for _ in range(iters):
                        getattr(self, mode)(iter_loaders[i], **kwargs)
        self.call_hook('after_epoch')
        self.call_hook('after_run')


RUNNERS = {c.__name__: c for c in (NerfTrainRunner, NerfTestRunner, KiloNerfTrainRunner, KiloNerfTestRunner, BungeeNerfTrainRunner,
                                   BungeeNerfTestRunner)}


def get_runner(runner_cfg):
    """core/apis/helper.py:141-145: the class a config's train_runner / test_runner names"""
    name = runner_cfg['type']
    if name == 'KiloNerfDistillTrainRunner':
        return _kilo_distill_runner()
    if name not in RUNNERS:
        raise KeyError('%s is not a runner (built: %r)' % (name, sorted(RUNNERS) + ['KiloNerfDistillTrainRunner']))
    return RUNNERS[name]
