"""The hooks configs/instant_ngp/*.py name besides the common ones: PassDatasetHook, PassSamplerIterHook, ModifyBatchsizeHook
(core/hooks/hash_hook.py:12-42) and mmcv's EMAHook (custom_hooks), the latter restated AS REMEMBERED AND UNVERIFIED AGAINST MMCV like the rest
of DESIGN.md section 26.  Under runner.NgpIterRunner the three per-iteration ones are absorbed by train.Trainer, which does their work inside
its loop; on a plain IterRunner they do it themselves."""


def _module(runner):
    return getattr(runner.model, 'module', runner.model)


class PassDatasetHook:
    """dataset.get_alldata() / get_info() -> the network's sampler, once (hash_hook.py:12-22)"""

    def __init__(self, dataset=None):
        self.dataset = dataset

    def before_run(self, runner):
        _module(runner).sampler.set_data(self.dataset.get_alldata(), self.dataset.get_info())
        del self.dataset


class PassSamplerIterHook:
    """runner.iter -> sampler.set_iter before every training iteration (hash_hook.py:25-29)"""

    def before_train_iter(self, runner):
        _module(runner).sampler.set_iter(runner.iter)


class ModifyBatchsizeHook:
    """the sampler's n_rays_per_batch -> dataset.set_batchsize whenever it changed (hash_hook.py:32-42)"""

    def __init__(self):
        self.bs = 0

    def after_train_iter(self, runner):
        bs = _module(runner).sampler.n_rays_per_batch
        if bs != self.bs:
            self.bs = bs
            runner.data_loader.iter_loader._dataset.set_batchsize(self.bs)


class EMAHook:
    """mmcv's EMAHook for an iteration-based run on train.FusedAdam: the averages are the optimiser's own EMA state (one fused pass over
    p, g, m, v, ema per tensor), registered on the model as buffers `ema_<parameter name with . -> _>` that ALIAS that storage -- no second
    copy, no extra launch, and state_dict() / iter_N.pth carry them.  momentum and warm_up are the optimiser's ema_momentum / ema_warm_up
    (min(momentum, (1 + iter) / (warm_up + iter))).  `resume_from` resumes behind the registration.  The parameters are never swapped with
    the averages here: mmcv swaps in before/after_train_epoch only, which an iteration-based run never reaches."""

    def __init__(self, momentum=0.0002, interval=1, warm_up=100, resume_from=None):
        if interval != 1:
            raise NotImplementedError('EMAHook interval=%r: the fused optimiser averages at every update (interval=1)' % (interval,))
        assert 0 < momentum < 1
        self.momentum, self.interval, self.warm_up, self.checkpoint = momentum, interval, warm_up, resume_from
        self.registered = False

    @staticmethod
    def buffer_name(param_name):
        return 'ema_' + param_name.replace('.', '_')

    def alias(self, runner):
        """every optimised parameter's EMA state exists and the model's buffer of its name IS that tensor"""
        model, opt = _module(runner), runner.optimizer
        names = {id(p): n for n, p in model.named_parameters(recurse=True)}
        for group in opt.param_groups:
            group['ema_momentum'], group['ema_warm_up'] = self.momentum, self.warm_up
            for p in group['params']:
                if id(p) not in names or p.numel() == 0:
                    continue
                st = opt._state(p, group)
                if 'ema' not in st:                      # (state made before the momentum was known, or loaded without one)
                    st['ema'] = p.detach().clone()
                name = self.buffer_name(names[id(p)])
                old = model._buffers.get(name)
                if old is not None and old is not st['ema'] and old.shape == st['ema'].shape and old.device == st['ema'].device:
                    old.copy_(st['ema'])                 # keep the registered storage (whoever holds the buffer keeps seeing the average)
                    st['ema'] = old
                else:
                    model.register_buffer(name, st['ema'])
        # mmcv registers a buffer for EVERY named parameter: one without elements (the direction encoding's) has nothing to average and no
        # optimiser state; any other parameter outside the optimiser would keep a stale average and is refused
        optimised = {id(p) for group in opt.param_groups for p in group['params']}
        for n, p in model.named_parameters(recurse=True):
            if id(p) in optimised:
                continue
            if p.numel() != 0:
                raise NotImplementedError('EMAHook: parameter %r is not in the optimiser, whose fused EMA state the averages are' % n)
            if self.buffer_name(n) not in model._buffers:
                model.register_buffer(self.buffer_name(n), p.detach().clone())
        self.registered = True

    def before_run(self, runner):
        if not hasattr(runner.optimizer, '_state') or 'ema_momentum' not in runner.optimizer.defaults:
            raise NotImplementedError('EMAHook needs train.FusedAdam (the averages are its fused EMA state), got %s' % type(runner.optimizer).__name__)
        self.alias(runner)
        if self.checkpoint is not None:
            runner.resume(self.checkpoint)
            self.alias(runner)
