"""The bodies of the instant-ngp runner checks on the GPU (tests/test_gpu_ngp_runner.py).

Scene: tests/test_datasets.write_scene(root, H=64, W=64, n=(6, 2, 2)) -- 8 table images x 4096 rays of random RGBA -- under a config dict
with the key names of the reference's configs/instant_ngp/nerf_blender_local01.py: its own `model` dict (train.ngp_lego_model_cfg, pinned to
the file by tests/test_capi_and_host.py), N_rand_per_sampler = 1024, val_n = 1, 40 iterations.  They cross the grid refreshes at 0, 16 and 32
and the sampler's two batch-size updates behind iterations 15 and 31 (on this scene the first changes the size, the second keeps it).
Every training run is made once and shared (`Runs`); the global generator is seeded before each build."""
import contextlib
import copy
import logging
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from test_datasets import write_scene  # noqa: E402

DATANAME = 'tiny'
N_RAND = 1024
MAX_ITERS = 40
U64, U32 = 2.0 ** -53, 2.0 ** -24          # unit roundoffs

TRAIN_HOOKS = [  # configs/instant_ngp/nerf_blender_local01.py:32-45, verbatim
    dict(type='SetValPipelineHook', params=dict(), variables=dict(valset='valset')),
    dict(type='ValidateHook', params=dict(save_folder='visualizations/validation')),
    dict(type='OccupationHook', params=dict()),
    dict(type='PassIterHook', params=dict()),
    dict(type='PassDatasetHook', params=dict(), variables=dict(dataset='trainset')),
    dict(type='ModifyBatchsizeHook', params=dict()),
    dict(type='PassSamplerIterHook', params=dict()),
]
TEST_HOOKS = [  # :47-57
    dict(type='SetValPipelineHook', params=dict(), variables=dict(valset='testset')),
    dict(type='PassDatasetHook', params=dict(), variables=dict(dataset='testset')),
    dict(type='HashSaveSpiralHook', params=dict(save_folder='visualizations/spirals', ), variables=dict(cfg='cfg')),
]
TRAIN_PIPELINE = [dict(type='HashBatchSample', N_rand=N_RAND), dict(type='RandomBGColor'), dict(type='DeleteUseless', keys=['rays_rgb', 'iter_n', 'idx'])]
TEST_PIPELINE = [dict(type='HashGetRays', enable=True), dict(type='FlattenRays', enable=True), dict(type='HashSetImgids', enable=True),
                 dict(type='DeleteUseless', enable=True, keys=['pose', 'idx'])]


def config_dict(root, work, log_interval=8, workflow=(('train', MAX_ITERS),), ckpt_interval=10000):
    from xrnerf_amd.train import ngp_lego_model_cfg
    base = dict(dataset_type='blender', N_rand_per_sampler=N_RAND, datadir=root, half_res=False, testskip=1, white_bkgd=False, load_alpha=True,
                is_batching=True, mode='train', val_n=1)
    return dict(
        method='nerf', optimizer=dict(type='Adam', lr=1e-2, betas=(0.9, 0.99), eps=1e-15, weight_decay=1e-6), optimizer_config=dict(grad_clip=None),
        max_iters=MAX_ITERS, lr_config=dict(policy='step', step=10000, gamma=0.2, by_epoch=False),
        checkpoint_config=dict(interval=ckpt_interval, by_epoch=False), custom_hooks=[dict(type='EMAHook', momentum=0.05)], log_level='INFO',
        log_config=dict(interval=log_interval, by_epoch=False, hooks=[dict(type='TextLoggerHook')]), workflow=[tuple(w) for w in workflow],
        train_hooks=copy.deepcopy(TRAIN_HOOKS), test_hooks=copy.deepcopy(TEST_HOOKS), train_runner=dict(type='NerfTrainRunner'),
        test_runner=dict(type='NerfTestRunner'), num_gpus=1, distributed=False, work_dir=work, N_rand_per_sampler=N_RAND,
        model=ngp_lego_model_cfg(N_RAND),
        data=dict(train_loader=dict(batch_size=1, num_workers=0), train=dict(type='HashNerfDataset', cfg=dict(base), pipeline=copy.deepcopy(TRAIN_PIPELINE)),
                  val_loader=dict(batch_size=1, num_workers=0), val=dict(type='HashNerfDataset', cfg=dict(base, mode='val'), pipeline=copy.deepcopy(TEST_PIPELINE)),
                  test_loader=dict(batch_size=1, num_workers=0),
                  test=dict(type='HashNerfDataset', cfg=dict(base, mode='test', testskip=100), pipeline=copy.deepcopy(TEST_PIPELINE))))


def wrap(cfg_dict):
    from xrnerf_amd import apis
    from xrnerf_amd.builder import ConfigDict
    return apis.update_config(DATANAME, ConfigDict.wrap(copy.deepcopy(cfg_dict)))


@contextlib.contextmanager
def recorded_spans(spans, first=None):
    """train.Trainer.run wrapped for the duration: every call appends (iteration it starts at, k, the batch size of its last iteration);
    `first(trainer)` is called in front of the first one"""
    from xrnerf_amd import train
    orig = train.Trainer.run

    def run(self, k, iter_events=None):
        if first is not None and not spans:
            first(self)
        at = self.iter
        out = orig(self, k, iter_events)
        spans.append((at, k, int(out['num_samples'])))
        return out
    train.Trainer.run = run
    try:
        yield
    finally:
        train.Trainer.run = orig


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


@contextlib.contextmanager
def log_lines():
    h = _Lines()
    logger = logging.getLogger('xrnerf_amd')
    logger.addHandler(h)
    try:
        yield h.lines
    finally:
        logger.removeHandler(h)


def state_of(net, opt):
    """every tensor the issue names: table, both weight tensors, Adam m / v / step, the three EMA tensors -- host copies"""
    mlp = net.mlp
    out = {}
    for name, p in (('table', mlp.embedder_pos.params), ('w_density', mlp.density_net.params), ('w_color', mlp.color_net.params)):
        st = opt.state[p]
        out[name] = p.detach().cpu().clone()
        out[name + '.m'], out[name + '.v'], out[name + '.ema'] = st['m'].cpu().clone(), st['v'].cpu().clone(), st['ema'].cpu().clone()
        out[name + '.step'] = int(st['step'])
    return out


def assert_same_bits(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        if isinstance(a[k], int):
            assert a[k] == b[k], (what, k, a[k], b[k])
        else:
            assert a[k].shape == b[k].shape and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), '%s: %s differs' % (what, k)


def build_by_hand(cfg, dev):
    """what train_nerf builds, in its order, from the same seed: the three datasets' two, the network"""
    from xrnerf_amd import apis, builder
    torch.manual_seed(0)
    _, trainset = apis.build_dataloader(cfg, 'train')
    val_loader, valset = apis.build_dataloader(cfg, 'val')
    net = builder.build_network(cfg.model).to(dev)
    return trainset, valset, val_loader, net


class Runs:
    """the training runs the checks share, each made on first use"""

    def __init__(self, dev, tmp):
        self.dev, self.tmp, self.made = dev, tmp, {}
        self.root = os.path.join(tmp, 'scene_' + DATANAME)
        write_scene(self.root, H=64, W=64, n=(6, 2, 2))

    def work(self, name):
        return os.path.join(self.tmp, 'work_' + name)

    def cfg(self, name):
        kw = {'log8': dict(log_interval=8), 'log1': dict(log_interval=1),
              'val': dict(log_interval=20, workflow=(('train', 20), ('val', 1)), ckpt_interval=20)}[name]
        return config_dict(self.root, self.work(name), **kw)

    def get(self, name):
        """-> dict(runner=, spans=, lines=, state=) of train_nerf on the named config, or dict(trainer=, state=) of the hand-driven run"""
        if name not in self.made:
            self.made[name] = getattr(self, '_' + name)() if hasattr(self, '_' + name) else self._train(name)
        return self.made[name]

    def _train(self, name):
        from xrnerf_amd import apis
        spans = []
        torch.manual_seed(0)
        with recorded_spans(spans), log_lines() as lines:
            runner = apis.train_nerf(wrap(self.cfg(name)))
        torch.cuda.synchronize()
        return dict(runner=runner, spans=spans, lines=list(lines), state=state_of(runner.model, runner.optimizer))

    def _hand40(self):
        """Trainer(dev, dataset=..., net=...) after run(40): the benchmarked path on the same data and weights"""
        from xrnerf_amd.train import Trainer
        trainset, _, _, net = build_by_hand(wrap(self.cfg('log8')), self.dev)
        tr = Trainer(self.dev, dataset=trainset, net=net)
        tr.run(MAX_ITERS)
        torch.cuda.synchronize()
        return dict(trainer=tr, state=state_of(net, tr.opt))

    def _hand_val(self):
        """Trainer.run(20) + val_step + run(20) + val_step, driven by hand"""
        from xrnerf_amd import runner as R
        from xrnerf_amd.train import Trainer
        trainset, valset, val_loader, net = build_by_hand(wrap(self.cfg('val')), self.dev)
        tr = Trainer(self.dev, dataset=trainset, net=net)
        net.set_val_pipeline(valset.pipeline)
        loader = R.IterLoader(val_loader)
        frames = []
        for _ in range(2):
            net.train()
            tr.run(20)
            net.eval()
            with torch.no_grad():
                frames.append(net.val_step(next(loader)))
        torch.cuda.synchronize()
        return dict(trainer=tr, state=state_of(net, tr.opt), frames=frames)


# ------------------------------------------------------------------------------------------ 1
def check_runner_is_the_benchmarked_path(runs):
    """train_nerf, workflow [('train', 40)], log interval 8 == Trainer(dev, dataset=, net=).run(40), bit for bit"""
    from xrnerf_amd import runner as R
    got, want = runs.get('log8'), runs.get('hand40')
    runner = got['runner']
    assert type(runner) is R.NgpIterRunner and runner.iter == MAX_ITERS and runner.engine.iter == MAX_ITERS
    assert [(a, k) for a, k, _ in got['spans']] == [(0, 8), (8, 8), (16, 8), (24, 8), (32, 8)]
    sizes = [n for _, _, n in got['spans']]
    # the sampler sets the batch size behind iterations 15 and 31 (n target / measured samples, rounded up to 128 rays): the first update
    # changes it, the second finds the same samples per ray and keeps it
    assert sizes[0] == sizes[1] == N_RAND and sizes[2] == sizes[3] == sizes[4] != N_RAND and sizes[2] % 128 == 0, sizes
    assert got['state']['table.step'] == MAX_ITERS
    assert_same_bits(got['state'], want['state'], 'runner against Trainer.run(40)')
    assert not torch.equal(got['state']['table'], got['state']['table.ema'])                     # (an average, not a copy)
    # the log lines: five, each the average of its eight iterations, the lr the last iteration's
    assert [h[0] for h in runner.log_history] == [8, 16, 24, 32, 40] and all(h[1] == 1e-2 for h in runner.log_history)
    assert all(sorted(h[2]) == ['loss', 'psnr'] and np.isfinite(h[2]['loss']) and h[2]['loss'] > 0 and np.isfinite(h[2]['psnr']) for h in runner.log_history)
    assert sum('Iter [' in line and '/40]' in line and 'psnr:' in line for line in got['lines']) == 5
    assert runner.log_buffer.names == ['loss', 'psnr'] and os.path.isdir(os.path.join(runs.work('log8'), 'delete_me_to_stop'))
    assert runner.trainset.iter_n == MAX_ITERS - 1                                              # PassIterHook: the last span's last iteration


# ------------------------------------------------------------------------------------------ 2
def window_average(values, sizes, name):
    """LogWindow's arithmetic over one window in float64: sum(v n) / sum(n) in iteration order -> (average, bound).
    The bound is for `values` that went through one window each before (v = fl(fl(p n) / n), the spans-of-one run): against the
    device's window over the same iterations, whose terms are the very fl(p n) the one-iteration windows divided, each reproduced
    term fl(v n) is off by two roundings (<= 2 u |p n|), each side's running sum rounds once per addition (<= 2 u |S_j| together) and
    each side divides once (<= 2 u |A|)."""
    s, cnt, terms, partial = np.float64(0), np.float64(0), 0.0, 0.0
    for v, n in zip(values, sizes):
        t = np.float64(v) * np.float64(n)
        s, cnt = s + t, cnt + np.float64(n)
        terms += abs(t)
        partial += abs(s)
    avg = s / cnt
    return float(avg), float((2 * U64 * terms + 2 * U64 * partial) / cnt + 2 * U64 * abs(avg))


def check_span_plan_does_not_matter(runs):
    """log interval 1 (spans of one) ends on the bits of log interval 8; its 40 one-iteration values reproduce the other runs' window
    averages -- loss exactly, psnr within window_average's bound.  The interval-8 windows lie between the batch-size changes (behind
    iterations 15 and 31), so the first window of the validation run (log interval 20: iterations 0 .. 19, the same trajectory up to its
    first validation) is compared as well: the size changes inside it, and an average that weighted by anything but n_rays is off."""
    one, eight, val = runs.get('log1'), runs.get('log8'), runs.get('val')
    assert [(a, k) for a, k, _ in one['spans']] == [(i, 1) for i in range(MAX_ITERS)]
    assert_same_bits(one['state'], eight['state'], 'spans of 1 against spans of 8')
    sizes = [n for _, _, n in one['spans']]
    hist = one['runner'].log_history
    assert [h[0] for h in hist] == list(range(1, MAX_ITERS + 1))
    loss, psnr = [h[2]['loss'] for h in hist], [h[2]['psnr'] for h in hist]
    windows = [(eight['runner'].log_history[w][2], range(8 * w, 8 * w + 8)) for w in range(5)] + [(val['runner'].log_history[0][2], range(0, 20))]
    assert len(set(sizes[:20])) == 2 and val['runner'].log_history[0][0] == 20                  # the batch size changes inside the last of them
    worst = 0.0
    for avg, its in windows:
        want_loss, _ = window_average([loss[i] for i in its], [sizes[i] for i in its], 'loss')
        want_psnr, bound = window_average([psnr[i] for i in its], [sizes[i] for i in its], 'psnr')
        print('window %d..%d: loss %.17g (logged %.17g), psnr %.17g (logged %.17g, bound %.3g)'
              % (its[0], its[-1], want_loss, avg['loss'], want_psnr, avg['psnr'], bound))
        assert avg['loss'] == want_loss                       # v n and the sums are the device's own float64 operations on the same fp32 values
        assert abs(avg['psnr'] - want_psnr) <= bound and bound < 1e-13 * abs(want_psnr) + 1e-300
        worst = max(worst, abs(avg['psnr'] - want_psnr))
    # a plain mean of the 20 values is NOT the window's average (the weights matter at this precision)
    assert abs(float(np.mean(loss[:20])) - windows[-1][0]['loss']) > 1e-9 * abs(windows[-1][0]['loss'])


# ------------------------------------------------------------------------------------------ 3
def check_psnr_is_the_references(runs):
    """one iteration's logged psnr against mse2psnr(img2mse(rgb alpha, target alpha)) in torch fp32 on the host, from that step's rgb_out
    and batch (networks/hashnerf.py:40-42)"""
    from xrnerf_amd import runner as R
    from xrnerf_amd.networks import img2mse, mse2psnr
    from xrnerf_amd.train import Trainer
    trainset, _, _, net = build_by_hand(wrap(runs.cfg('log8')), runs.dev)
    window = R.LogWindow()
    tr = Trainer(runs.dev, dataset=trainset, net=net, log_window=window.reserve(('loss', 'psnr'), runs.dev))
    drawn, orig = [], trainset.next_batch

    def next_batch(out=None):
        b = orig(out=out)
        drawn.append({k: v for k, v in b.items()})
        return b
    trainset.next_batch = next_batch
    out = tr.step()
    torch.cuda.synchronize()
    rgb = net._last['rgb'].detach().cpu().clone()
    batch = {k: v.detach().cpu().clone() for k, v in drawn[0].items()}
    logged = window.read()
    n = rgb.shape[0]
    assert n == N_RAND == int(out['num_samples']) and tuple(batch['target_s'].shape) == (n, 3) and tuple(batch['alpha'].shape) == (n, 1)
    alpha, target = batch['alpha'], batch['target_s']
    want = float(mse2psnr(img2mse(rgb * alpha, target * alpha)))
    assert float(out['log_vars']['loss']) == logged['loss']                                   # fl(fl(l n) / n) = l: the product is exact
    # The bound, from the fp32 roundings of the composition (u = 2^-24) over M = 3 n elements, D = (rgb - target) alpha:
    #   host element   fl(fl(rgb a) - fl(target a)) is off D by <= u (|rgb a| + |target a| + |D|) <= u (2 a + |D|): the squared sum moves by
    #                  <= 2 u (sum D^2 + 2 sum |D| a), relatively 2 u (1 + 2 R), R = sum |D| a / sum D^2 (taken from the data in float64); + u per square
    #   device element fl(fl(rgb - target) a), squared: three roundings relative to D^2's factors -> <= 5 u
    #   the sums       any order of M non-negative fp32 terms: <= (M - 1) u each side; the host's mean divides once (u), the device in double
    #   -10 log x / log 10 in fp32: log within 2 ulp, the product, the quotient and the rounded constant -> <= 6 u |psnr|; d psnr / d x = 10 / (x ln 10)
    D = (rgb.double() - target.double()) * alpha.double()
    M = D.numel()
    Rr = float((D.abs() * alpha.double()).sum() / (D * D).sum())
    rel_x = U32 * (2 * (1 + 2 * Rr) + 1 + 5 + 2 * (M - 1) + 1)
    bound = 10.0 / np.log(10.0) * rel_x / (1 - rel_x) + 6 * U32 * abs(want) + 1e-12
    exact = float(-10.0 * torch.log10((D * D).mean()))
    print('psnr: logged %.9g, host fp32 %.9g, float64 %.9g; |logged - fp32| = %.3g, bound %.3g (R = %.3g)'
          % (logged['psnr'], want, exact, abs(logged['psnr'] - want), bound, Rr))
    assert abs(logged['psnr'] - want) <= bound and bound < 5e-3
    # the lazily logged value of the same step (networks._LazyPsnr: fp32 on the device) is the same quantity
    assert abs(float(out['log_vars']['psnr']) - logged['psnr']) <= bound


# ------------------------------------------------------------------------------------------ 4
MODEL_KEYS = ['ema_mlp_color_net_params', 'ema_mlp_density_net_params', 'ema_mlp_embedder_dir_params', 'ema_mlp_embedder_pos_params',
              'mlp.color_net.params', 'mlp.density_net.params', 'mlp.embedder_dir.params', 'mlp.embedder_pos.params', 'sampler.density_grid_bitfield']


def check_end_to_end_with_validation(runs):
    """workflow [('train', 20), ('val', 1)], checkpoints every 20: the files, the log lines, ValidateHook's PNG and metrics, and the
    parameters of Trainer.run(20) + val_step + run(20) + val_step driven by hand; then a resume from iter_20.pth"""
    from PIL import Image
    from xrnerf_amd import apis
    got, want = runs.get('val'), runs.get('hand_val')
    runner, work = got['runner'], runs.work('val')
    assert [(a, k) for a, k, _ in got['spans']] == [(0, 20), (20, 20)] and runner.iter == MAX_ITERS
    assert_same_bits(got['state'], want['state'], 'runner with validation against the hand-driven trainer')
    assert os.readlink(os.path.join(work, 'latest.pth')) == 'iter_40.pth'
    ckpts = {}
    for it in (20, 40):
        ckpt = ckpts[it] = torch.load(os.path.join(work, 'iter_%d.pth' % it), map_location='cpu', weights_only=False)
        assert sorted(ckpt) == ['meta', 'optimizer', 'state_dict'] and ckpt['meta']['iter'] == it
        assert sorted(ckpt['state_dict']) == MODEL_KEYS
        assert ckpt['state_dict']['sampler.density_grid_bitfield'].any()
        steps = [int(st['step']) for st in ckpt['optimizer']['state'].values()]
        assert steps == [it] * 3
    final = ckpts[40]['state_dict']
    for key, name in (('mlp.embedder_pos.params', 'table'), ('mlp.density_net.params', 'w_density'), ('mlp.color_net.params', 'w_color')):
        assert torch.equal(final[key], got['state'][name])
        assert torch.equal(final['ema_' + key.replace('.', '_')], got['state'][name + '.ema'])
        assert not torch.equal(ckpts[20]['state_dict'][key], final[key])
    # the log lines and the validation: one PNG (prediction beside ground truth) and one metrics line per validation
    assert [h[0] for h in runner.log_history] == [20, 40]
    assert all(np.isfinite(h[2]['loss']) and h[2]['loss'] > 0 and np.isfinite(h[2]['psnr']) for h in runner.log_history)
    assert sum('Iter [20/40]' in line or 'Iter [40/40]' in line for line in got['lines']) == 2
    metrics = [line for line in got['lines'] if line.startswith('On testset, mse is')]
    assert len(metrics) == 2 and all('nan' not in line for line in metrics), got['lines']
    for it in (20, 40):
        folder = os.path.join(work, 'visualizations/validation', str(it))
        assert sorted(os.listdir(folder)) == ['000.png'] and Image.open(os.path.join(folder, '000.png')).size == (128, 64)
    frames = want['frames']
    assert np.array_equal(runner.outputs['rgbs'][0], frames[1]['rgbs'][0]) and runner.outputs['rgbs'][0].shape == (64, 64, 3)
    # resume from iter_20.pth: iteration, step counters and EMA tensors as the checkpoint holds them, then on to 40
    cfg = wrap(dict(runs.cfg('val'), work_dir=runs.work('resumed')))
    cfg.resume_from = os.path.join(work, 'iter_20.pth')
    seen, spans = {}, []

    def first(tr):
        seen['iter'] = tr.iter
        seen['state'] = state_of(tr.net, tr.opt)
        seen['aliased'] = all(getattr(tr.net, 'ema_mlp_%s_params' % k).data_ptr() == tr.opt.state[getattr(tr.net.mlp, k).params]['ema'].data_ptr()
                              for k in ('embedder_pos', 'density_net', 'color_net'))
    torch.manual_seed(0)
    with recorded_spans(spans, first):
        resumed = apis.train_nerf(cfg)
    opt20 = ckpts[20]['optimizer']['state']
    assert seen['iter'] == 20 and seen['aliased'] and [(a, k) for a, k, _ in spans] == [(20, 20)]
    for i, name in enumerate(('table', 'w_density', 'w_color')):
        assert seen['state'][name + '.step'] == 20
        for part in ('m', 'v', 'ema'):
            assert torch.equal(seen['state'][name + '.' + part], opt20[i][part].cpu()), (name, part)
        assert torch.equal(seen['state'][name + '.ema'], ckpts[20]['state_dict']['ema_mlp_%s_params' % ('embedder_pos', 'density_net', 'color_net')[i]])
    assert resumed.iter == MAX_ITERS and [h[0] for h in resumed.log_history] == [40]
    assert np.isfinite(resumed.log_history[0][2]['loss']) and np.isfinite(resumed.log_history[0][2]['psnr'])
    assert state_of(resumed.model, resumed.optimizer)['table.step'] == MAX_ITERS
    assert os.path.isfile(os.path.join(runs.work('resumed'), 'iter_40.pth'))


# ------------------------------------------------------------------------------------------ 5
def check_test_pass(runs):
    """run_nerf(--test_only --load_from iter_40.pth) on a config FILE: HashSaveSpiralHook's frames, frame 0 = train.render_frame"""
    from PIL import Image
    from xrnerf_amd import apis, builder, evaluate
    from xrnerf_amd.train import render_frame
    runs.get('val')
    work = runs.work('val')
    cfg_dict = runs.cfg('val')
    path = os.path.join(runs.tmp, 'ngp_config.py')
    with open(path, 'w') as f:
        f.write('import os\nfrom datetime import datetime\n')
        for k, v in cfg_dict.items():
            f.write('%s = %r\n' % (k, v))
    tested = apis.run_nerf(apis.parse_args(['--config', path, '--dataname', DATANAME, '--test_only', '--load_from', 'iter_40.pth']))
    assert tested.model.phase == 'test' and tested.epoch == 1
    ckpt = torch.load(os.path.join(work, 'iter_40.pth'), map_location='cpu', weights_only=False)['state_dict']
    assert torch.equal(tested.model.sampler.density_grid_bitfield.cpu(), ckpt['sampler.density_grid_bitfield'])     # loaded before any frame
    assert torch.equal(tested.model.mlp.embedder_pos.params.detach().cpu(), ckpt['mlp.embedder_pos.params'])
    folder = os.path.join(work, 'visualizations/spirals')
    names = ['%03d.png' % i for i in range(40)]
    assert sorted(os.listdir(os.path.join(folder, '40_rgb'))) == names and sorted(os.listdir(os.path.join(folder, '40_alpha'))) == names
    assert Image.open(os.path.join(folder, '40_rgb', '000.png')).size == (64, 64)
    hook = next(h for h in tested.hooks if isinstance(h, evaluate.HashSaveSpiralHook))
    idx, rgb0, alpha0 = hook.spiral_data[0]
    assert idx == 0 and len(hook.spiral_data) == 40
    # frame 0 by train.render_frame on a network of its own with the checkpoint's weights and bitfield
    cfg = wrap(cfg_dict)
    _, testset = apis.build_dataloader(cfg, 'test')
    model = dict(cfg.model)
    model['cfg'] = dict(model['cfg'], phase='test')
    net = builder.build_network(model).to(runs.dev)
    net.load_state_dict({k: v for k, v in ckpt.items() if not k.startswith('ema_')})
    net.sampler.set_data(testset.get_alldata(), testset.get_info())
    assert np.array_equal(testset.get_alldata()['poses'], testset.render_poses)
    rgb, alpha = render_frame(net, testset.render_poses[0], 64, 64, testset.focal)
    rgb, alpha = rgb.cpu().numpy(), alpha.cpu().numpy()
    assert np.array_equal(alpha0, alpha) and alpha.shape == (64, 64, 1) and np.isfinite(rgb).all()
    mask = (alpha >= 0.99).astype(np.float64)                                     # HashSaveSpiralHook.apply_mask
    assert np.array_equal(rgb0, rgb * mask + 1 * (1 - mask))
    assert np.array_equal(np.asarray(Image.open(os.path.join(folder, '40_rgb', '000.png'))), evaluate.to8b(rgb * mask + 1 * (1 - mask)))


# ------------------------------------------------------------------------------------------ 6
def check_logged_against_unlogged_entry_point(runs):
    """Trainer(log_window=...) and Trainer() reach the same parameter bits after 33 iterations (the refresh iterations 0, 16 and 32 on the
    per-iteration path, 30 inside the native loop); the window holds all 33"""
    from xrnerf_amd import runner as R
    from xrnerf_amd.train import Trainer
    states, sizes = [], []
    window = R.LogWindow()
    for logged in (False, True):
        trainset, _, _, net = build_by_hand(wrap(runs.cfg('log8')), runs.dev)
        tr = Trainer(runs.dev, dataset=trainset, net=net, log_window=window.reserve(('loss', 'psnr'), runs.dev) if logged else None)
        for k in (16, 16, 1):
            out = tr.run(k)
            if logged:
                sizes += [int(out['num_samples'])] * k
        torch.cuda.synchronize()
        assert tr.iter == 33 and tr._loop is not None and tr._loop.enqueued == 30            # (iterations 0, 16 and 32 refresh the grid)
        states.append(state_of(net, tr.opt))
    assert_same_bits(states[0], states[1], 'logged against unlogged loop')
    raw = window.window.cpu().numpy()
    S = R.ops.LOG_WINDOW_SLOTS
    assert raw[S + 0] == raw[S + 1] == float(sum(sizes)) and len(set(sizes)) == 2 and not raw[2:S].any() and not raw[S + 2:].any()
    avg = window.read()
    assert sorted(avg) == ['loss', 'psnr'] and np.isfinite(avg['loss']) and avg['loss'] > 0 and np.isfinite(avg['psnr'])
    # the same 33 iterations through the runs' shared interval-1 run: its values, weighted, are this window's average
    one = runs.get('log1')
    hist = one['runner'].log_history[:33]
    want, _ = window_average([h[2]['loss'] for h in hist], [n for _, _, n in one['spans'][:33]], 'loss')
    assert avg['loss'] == want
