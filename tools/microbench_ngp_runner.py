"""What the config-driven instant-ngp runner costs against the bare trainer, at the benchmark's own size (100 synthetic 800 x 800 cameras).

Rows, alternating window by window in one process; each window is `--steps` (>= 256, a multiple of the 16-iteration refresh period) warmed-up
iterations, synchronised at both ends, rays counted by the trainer:
  (a) Trainer.run                    the benchmarked path: xr_ngp_loop_run between the refreshes
  (b) Trainer.run + log window       the same with every iteration's loss and psnr added to a device log window (xr_ngp_loop_run_logged: one
                                     single-workgroup launch more per iteration)
  (c) NgpIterRunner                  what apis.train_nerf builds for the instant-ngp config -- FusedAdam from cfg.optimizer, the lr / optimizer /
                                     checkpoint / log hooks at the config's own intervals (log 500, checkpoint 10000), EMAHook, the config's
                                     train_hooks without the validation pair -- over the same synthetic ray table, spans planned by the runner
(b) against (a) is the price of the log launch.  (c) adds host work between spans only: its windows must overlap (b)'s.

  python tools/microbench_ngp_runner.py [--steps 256] [--n-img 100] [--out profiles/ngp_runner_microbench.txt]"""
import argparse
import logging
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_runner(dev, data, work_dir):
    """apis.train_nerf's steps for a HashNerfNetwork config, on a ray table that is already there"""
    from xrnerf_amd import apis, builder, runner as R
    from xrnerf_amd.builder import ConfigDict
    from xrnerf_amd.train import ngp_lego_model_cfg
    cfg = ConfigDict.wrap(dict(
        method='nerf', model=ngp_lego_model_cfg(), optimizer=dict(type='Adam', lr=1e-2, betas=(0.9, 0.99), eps=1e-15, weight_decay=1e-6),
        optimizer_config=dict(grad_clip=None), lr_config=dict(policy='step', step=10000, gamma=0.2, by_epoch=False),
        checkpoint_config=dict(interval=10000, by_epoch=False), custom_hooks=[dict(type='EMAHook', momentum=0.05)],
        log_config=dict(interval=500, by_epoch=False, hooks=[dict(type='TextLoggerHook')]),
        train_hooks=[dict(type='OccupationHook', params=dict()), dict(type='PassIterHook', params=dict()),
                     dict(type='PassDatasetHook', params=dict(), variables=dict(dataset='trainset')),
                     dict(type='ModifyBatchsizeHook', params=dict()), dict(type='PassSamplerIterHook', params=dict())]))
    torch.manual_seed(0)
    network = builder.build_network(cfg.model).to(dev)
    optimizer = apis.get_optimizer(network, cfg)
    logger = logging.getLogger('xrnerf_amd.microbench')
    logger.setLevel(logging.WARNING)
    runner = R.NgpIterRunner(network, optimizer=optimizer, work_dir=work_dir, logger=logger, trainset=data)
    runner.register_training_hooks(cfg.lr_config, cfg.optimizer_config, cfg.checkpoint_config, cfg.log_config, custom_hooks_config=cfg.custom_hooks)
    apis.register_hooks(cfg.train_hooks, runner=runner, trainset=data)
    return runner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=256, help='iterations per timing window (a multiple of 16, at least 256)')
    ap.add_argument('--n-img', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=512, help='un-timed iterations of every row before its first window')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.steps >= 256 and args.steps % 16 == 0 and args.warmup % 16 == 0
    from xrnerf_amd import runner as R
    from xrnerf_amd.train import SyntheticLego, Trainer
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    mk = lambda: SyntheticLego(dev, args.n_img, 800, 800, seed=1, shuffle_seed=1)
    plain = Trainer(dev, dataset=mk())
    window = R.LogWindow()
    logged = Trainer(dev, dataset=mk(), log_window=window.reserve(('loss', 'psnr'), dev))
    tmp = tempfile.mkdtemp(prefix='ngp_runner_microbench_')
    runner = build_runner(dev, mk(), tmp)
    loader = R.IterLoader(R.DataLoader(runner.trainset))
    # the runner's set-up (before_run hooks, the engine) and its warm-up through run() itself; the windows then go on span by span
    runner.run([R.DataLoader(runner.trainset)], [('train', args.warmup)], args.warmup)
    plain.run(args.warmup)
    logged.run(args.warmup)
    window.read()
    torch.cuda.synchronize()

    def runner_window(k):
        runner._max_iters = runner.iter + k
        runner.train_span(loader, k)

    rows = {'(a) Trainer.run': (plain, lambda k: plain.run(k)), '(b) Trainer.run + log window': (logged, lambda k: logged.run(k)),
            '(c) NgpIterRunner, config intervals': (runner.engine, runner_window)}
    rates = {k: [] for k in rows}
    for _ in range(args.windows):
        for name, (tr, go) in rows.items():
            torch.cuda.synchronize()
            r0, t0 = tr.rays_done, time.perf_counter()
            go(args.steps)
            torch.cuda.synchronize()
            rates[name].append((tr.rays_done - r0) / (time.perf_counter() - t0))
        window.read()
    iters = {name: tr.iter for name, (tr, _) in rows.items()}
    same = all(torch.equal(plain.net.mlp.embedder_pos.params, tr.net.mlp.embedder_pos.params) for tr in (logged, runner.engine))
    lines = ['instant-ngp training on %s, %d synthetic 800 x 800 cameras; rays/s, median (min .. max) of %d alternating windows of %d iterations '
             'after %d warm-up iterations' % (torch.cuda.get_device_name(0), args.n_img, args.windows, args.steps, args.warmup), '']
    stat = {k: (statistics.median(v), min(v), max(v)) for k, v in rates.items()}
    for k, (med, lo, hi) in stat.items():
        lines.append('  %-40s %8.3f M (%.3f .. %.3f)' % (k, med / 1e6, lo / 1e6, hi / 1e6))
    a, b, c = (stat[k] for k in rows)
    lines += ['', 'the log launch: (b) / (a) = %.4f (medians)' % (b[0] / a[0]),
              'the runner: (c) / (b) = %.4f (medians); windows %s' % (c[0] / b[0], 'overlap' if c[2] >= b[1] and b[2] >= c[1] else 'DO NOT overlap'),
              'iterations done %r, log lines of the runner at %r; the three tables are %s after them' % (
                  sorted(set(iters.values())), [h[0] for h in runner.log_history], 'bit-identical' if same else 'DIFFERENT')]
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
