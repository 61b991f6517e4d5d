"""The optimiser step and the log update of one training iteration, on the parameter sets of three families:
  nerf         the vanilla NerfNetwork of configs/nerf/nerf_blender_base01.py (coarse + fine 8 x 256 MLPs: 48 tensors)
  neuralbody   the NeuralBody network of tests/golden/neuralbody_model_cfg.json (sparse convolutions: the most tensors)
  kilonerf     the KiloNeRF multi-network at 1440 networks (12 packed tensors)

Rows, alternating window by window in one process, their parameters compared before they are timed.  Each timed step is one optimiser
step plus one log update of three scalars:
  torch Adam + 3 .item()     torch.optim.Adam.step (multi-tensor kernels) and three blocking reads: what the hand-written loops do today
  FusedAdam (4 per launch)   the step FusedAdam.step took before the list kernel (xr_adam_step_multi, up to 4 tensors per launch) and
                             the same three reads
  list kernel + LogWindow    FusedAdam.step through xr_adam_step_list and LogWindow.update (one launch, nothing read); the window is
                             read once at the end of each timing window

  python tools/microbench_optim.py [--steps 200] [--out profiles/optim_microbench.txt]"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NERF_MLP = dict(type='NerfMLP', skips=[4], netdepth=8, netwidth=256, netchunk=1024 * 32, output_ch=5, use_viewdirs=True,
                embedder=dict(type='BaseEmbedder', i_embed=0, multires=10, multires_dirs=4))
NERF_MODEL = dict(type='NerfNetwork', cfg=dict(phase='train', N_importance=128, is_perturb=True, chunk=1024 * 32, bs_data='rays_o'),
                  mlp=NERF_MLP, mlp_fine=copy.deepcopy(NERF_MLP), render=dict(type='NerfRender', white_bkgd=True, raw_noise_std=0))


def shapes(name):
    import xrnerf_amd
    from xrnerf_amd import kilo
    if name == 'nerf':
        net = xrnerf_amd.build_network(NERF_MODEL)
    elif name == 'neuralbody':
        net = xrnerf_amd.build_network(json.load(open(os.path.join(ROOT, 'tests', 'golden', 'neuralbody_model_cfg.json')))['model'])
    else:
        net = kilo.MultiNetwork(1440, 63, 27)
    return [tuple(p.shape) for p in net.parameters() if p.requires_grad]


def parent_step(opt, grad_scale=1.0):
    """FusedAdam.step as it was before the list kernel: tensors that share a step count go out in launches of up to 4"""
    from xrnerf_amd import ops
    for group in opt.param_groups:
        todo = []
        for p in group['params']:
            if p.grad is None or p.numel() == 0:
                continue
            st = opt._state(p, group)
            st['step'] += 1
            todo.append((p, p.grad if p.grad.is_contiguous() else p.grad.contiguous(), st))
        while todo:
            chunk = [t for t in todo[:4] if t[2]['step'] == todo[0][2]['step']]
            todo = [t for t in todo if all(t is not c for c in chunk)]
            ops.adam_step_multi([c[0] for c in chunk], [c[1] for c in chunk], [c[2]['m'] for c in chunk], [c[2]['v'] for c in chunk],
                                chunk[0][2]['step'], group['lr'], group['betas'][0], group['betas'][1], group['eps'], group['weight_decay'],
                                None, 0.0, grad_scale=grad_scale)


def windows(fns, calls, n_windows=5, warmup=20):
    """fns: {name: (step, end of window)} -> {name: (median us per step, min, max)}, the rows alternating window by window; a host clock
    around a window that ends in a device synchronise"""
    for step, end in fns.values():
        for _ in range(warmup):
            step()
        end()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(n_windows):
        for k, (step, end) in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                step()
            end()
            torch.cuda.synchronize()
            times[k].append(1e6 * (time.perf_counter() - t0) / calls)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200, help='steps per timing window')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from xrnerf_amd import ops
    from xrnerf_amd.runner import LogWindow
    from xrnerf_amd.train import FusedAdam
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    assert ops.optim_kernels_available()
    dev = torch.device('cuda:0')
    kw = dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    lines = ['optimiser step + log update on %s; us per step, median (min .. max) of 5 alternating windows of %d steps' % (
        torch.cuda.get_device_name(0), args.steps), '']
    for name in ('nerf', 'neuralbody', 'kilonerf'):
        shp = shapes(name)
        g = torch.Generator(device=dev).manual_seed(0)
        init = [torch.randn(s, device=dev, generator=g) * 0.1 for s in shp]
        grads = [torch.randn(s, device=dev, generator=g) * 0.01 for s in shp]
        scalars = [torch.rand((), device=dev, generator=g) for _ in range(3)]
        sets = {}
        for row in ('torch', 'parent', 'list'):
            ps = [torch.nn.Parameter(t.clone()) for t in init]
            for p, gr in zip(ps, grads):
                p.grad = gr.clone()
            sets[row] = (ps, torch.optim.Adam(ps, **kw) if row == 'torch' else FusedAdam(ps, **kw))
        window = LogWindow()

        def read3():
            return [s.item() for s in scalars]
        steps = {
            'torch Adam + 3 .item()': (lambda: (sets['torch'][1].step(), read3()), lambda: None),
            'FusedAdam (4 per launch) + 3 .item()': (lambda: (parent_step(sets['parent'][1]), read3()), lambda: None),
            'list kernel + LogWindow': (lambda: (sets['list'][1].step(), window.update({'loss': scalars[0], 'psnr': scalars[1], 'reg': scalars[2]}, 4096)),
                                        window.read),
        }
        # outputs first: two steps of every row from the same parameters and gradients
        for step, end in steps.values():
            step(), step(), end()
        torch.cuda.synchronize()
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(sets['parent'][0], sets['list'][0]))
        rel = max(float((a.detach() - b.detach()).abs().max() / b.detach().abs().max()) for a, b in zip(sets['list'][0], sets['torch'][0]))
        assert same, 'the list kernel and xr_adam_step_multi differ'
        assert rel <= 1e-5, rel
        r = windows(steps, args.steps)
        n_float = sum(p.numel() for p in sets['list'][0])
        cap = ops.adam_list_capacity()
        lines.append('%s: %d tensors, %d floats (%d of them under 1024 floats); launches per step: %d of 4 tensors, %d of the list kernel; list '
                     'kernel = FusedAdam (4 per launch) in every bit, against torch Adam %.1e of the largest parameter' % (
                         name, len(shp), n_float, sum(p.numel() < 1024 for p in sets['list'][0]), -(-len(shp) // 4), -(-len(shp) // cap), rel))
        for row, (med, lo, hi) in r.items():
            lines.append('  %-40s %9.1f (%.1f .. %.1f)' % (row, med, lo, hi))
        new = r['list kernel + LogWindow']
        for row in list(r)[:2]:
            verdict = 'not slower' if new[0] <= r[row][0] + (r[row][2] - r[row][1]) + (new[2] - new[1]) else 'SLOWER'
            lines.append('  list kernel + LogWindow against %s: %.2f x, %s beyond the spread between windows' % (row, r[row][0] / new[0], verdict))
        lines.append('')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
