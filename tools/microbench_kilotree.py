"""KiloNeRF distillation's validation numbers at the shipped configs' size: N = 512 networks x P = 20000 validation examples.

Rows, alternating window by window in one process, their outputs compared before they are timed:
  kernel           ops.kilo_val_metrics (csrc/xr_kilotree.hip: one launch) + the read of its [N, 16] table
  tensor ops       kilo_distill.calculate_error_metrics, the torch composition it replaces (about 30 ops, three sorts of [N, P]), + the
                   read of its thirteen [N] results
  kernel + split   the same launch with an equal-error split threshold asked of every network (the tensor ops have no such row: the
                   reference runs it on the host, one network at a time)
and one whole SaveDistillResultsHook.after_val_iter at a cycle boundary (kd-tree bookkeeping, log.txt and checkpoint.pth included), the
nodes' networks stood in for by their index.

  python tools/microbench_kilotree.py [--networks 512] [--points 20000] [--out profiles/kilotree_microbench.txt]"""
import argparse
import os
import statistics
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows(fns, n_windows=5, warmup=2):
    """fns: {name: (callable, calls per window)} -> {name: (median ms per call, min, max)}, the callables alternating window by window; a
    host clock around work that ends in a device synchronise"""
    for f, _ in fns.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(n_windows):
        for k, (f, calls) in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            torch.cuda.synchronize()
            times[k].append(1e3 * (time.perf_counter() - t0) / calls)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--networks', type=int, default=512)
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from xrnerf_amd import kilo_distill as KD, kilo_tree as T, ops
    from xrnerf_amd.builder import ConfigDict
    from xrnerf_amd.kilodata import Node, calculate_volume
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    N, P = args.networks, args.points
    g = torch.Generator(device=dev).manual_seed(0)
    ex = torch.zeros((N, P, 10), device=dev)
    ex[..., :3] = torch.rand((N, P, 3), device=dev, generator=g) * 1.6 - 0.8
    ex[..., 6:10] = torch.rand((N, P, 4), device=dev, generator=g)
    targets, points = ex[..., 6:10], ex[..., :3]
    out = targets + 0.05 * torch.randn((N, P, 4), device=dev, generator=g)
    qi = int(P * 0.99)
    axes = torch.tensor([n % 3 for n in range(N)], dtype=torch.int32, device=dev)

    def kernel():
        return ops.kilo_val_metrics(out, targets, qi)[0].cpu()

    def kernel_split():
        return ops.kilo_val_metrics(out, targets, qi, points=points, split_axis=axes, split_metric='mse')[0].cpu()

    def tensor_ops():
        a, b, c, sat = KD.calculate_error_metrics(out, targets, 0.99)
        return torch.stack([d[m] for m in ('mse', 'mae', 'mape') for d in (a, b, c)] + [d['quantile_se'] for d in (a, b, c)] + [sat.float()], 1).cpu()
    k, t = kernel(), tensor_ops()
    rel = ((k[:, :9] - t[:, :9]).abs() / t[:, :9].abs()).max().item()
    relq = ((k[:, 9:11] - t[:, 9:11]).abs() / t[:, 9:11].abs()).max().item()
    lines = ['KiloNeRF validation numbers on %s: %d networks x %d points, quantile 0.99' % (torch.cuda.get_device_name(0), N, P),
             'kernel against tensor ops: means, largest relative difference %.3e; total / colour quantile %.3e; density quantile %d of %d differ '
             'in their bits; saturation %d differ' % (rel, relq, int((k[:, 11] != t[:, 11]).sum()), N, int((k[:, 12] != t[:, 12]).sum()))]
    assert rel <= 1e-5 and relq <= 4 * 2.0 ** -24 and bool((k[:, 11] == t[:, 11]).all()) and bool((k[:, 12] == t[:, 12]).all()), lines[-1]
    r = windows({'kernel': (kernel, 10), 'tensor ops': (tensor_ops, 3), 'kernel + split': (kernel_split, 10)})
    lines += ['', 'median ms per validation (min .. max), 5 windows alternating; a host clock around a synchronised window, the read of the results inside', '']
    for name, (med, lo, hi) in r.items():
        lines.append('%-40s %9.4f (%.4f .. %.4f)' % (name, med, lo, hi))
    lines.append('tensor ops / kernel = %.1f x' % (r['tensor ops'][0] / r['kernel'][0]))

    # one whole after_val_iter at a cycle boundary
    cfg = ConfigDict.wrap(dict(max_iters=10, outputs='color_and_density', quantile_se=0.99, equal_split_metric='mse', num_networks=N,
                               tree_type='kdtree_equal_error_split', test_error_metric='quantile_se', max_error=1e-3))
    error_log = ['[0.0, 0.0, 0.0] [1.0, 1.0, 1.0]\n'] * N
    calls = []

    def after_val_iter():
        cp = {'fitted_volume': 0, 'num_networks_fitted': 0, 'phase': 'discovery', 'root_nodes': []}
        for n in range(N):
            node = Node()
            node.domain_min, node.domain_max = [float(n), -0.8, -0.8], [float(n) + 1.6, 0.8 + 0.1 * (n % 2), 0.8 + 0.2 * (n % 3 == 0)]
            cp['root_nodes'].append(node)
        from collections import deque
        cp['nodes_to_process'], cp['saturated_nodes_to_process'] = deque(), deque()
        cp['total_volume'] = sum(calculate_volume(n.domain_min, n.domain_max) for n in cp['root_nodes'])
        info = {'cp': cp, 'processing_saturated_nodes': False, 'node_batch': list(cp['root_nodes'])}
        with tempfile.TemporaryDirectory() as work:
            runner = types.SimpleNamespace(iter=10, _max_iters=10, work_dir=work, logger=types.SimpleNamespace(info=lambda *a: None),
                                           outputs={'out': out, 'target_s': targets, 'test_points': points, 'error_log': list(error_log)},
                                           model=types.SimpleNamespace(multi_network=types.SimpleNamespace(get_single_network=lambda i: int(i))))
            hook = T.SaveDistillResultsHook(cfg, types.SimpleNamespace(get_info=lambda: info))
            runner.iter = 0
            hook.before_train_iter(runner)
            runner.iter = 10
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hook.after_val_iter(runner)
            calls.append(1e3 * (time.perf_counter() - t0))
        return cp
    cp = after_val_iter()
    for _ in range(5):
        after_val_iter()
    lines += ['', 'SaveDistillResultsHook.after_val_iter at a cycle boundary, kdtree_equal_error_split, %d nodes (%d split, %d fitted): median %.2f ms '
              '(%.2f .. %.2f) of 5 calls' % (N, len(cp['nodes_to_process']) // 2, cp['num_networks_fitted'], statistics.median(calls[1:]),
                                             min(calls[1:]), max(calls[1:]))]
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
