"""Vanilla-NeRF microbenchmark at config #1's own sizes (configs/nerf/nerf_blender_base01.py: 8 x 256 MLPs, N_rand_per_sampler = 4096 rays,
64 coarse + N_importance = 128 fine samples): ms per training step (train_step + backward + a torch Adam step) with the per-entry-point
device spans of one step (ops.KernelTimer), and ms per 800 x 800 test frame through batchify_forward.  Public API only
(xrnerf_amd.build_network, train_step, backward, torch.optim.Adam), so the same file measures any commit of this repository.

Every figure is the median of --repeats windows after warm-up, with the smallest and the largest window beside it; a window is --steps
training steps between two device events.  One JSON line.  Needs the GPU: it fails without one."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows(fn, repeats, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return {'median': statistics.median(out), 'min': min(out), 'max': max(out), 'windows': out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=int, default=4096)
    ap.add_argument('--samples', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--frame', type=int, default=800, help='side of the test frame (0: skip)')
    ap.add_argument('--frame-repeats', type=int, default=5)
    ap.add_argument('--label', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('microbench_vanilla needs the GPU')
    import xrnerf_amd
    from xrnerf_amd import ops, vanilla
    dev = torch.device('cuda')
    cfg = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'ngp_model_cfg.json')))['vanilla_model']
    torch.manual_seed(0)
    net = xrnerf_amd.build_network(cfg).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    n = a.rays
    g = torch.Generator().manual_seed(1)
    cam = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1) * 4.0
    rays_o = cam.to(dev)
    rays_d = torch.nn.functional.normalize(-cam + torch.randn(n, 3, generator=g) * 0.5, dim=-1).to(dev)
    target = torch.rand(n, 3, generator=g).to(dev)

    def step():
        z = vanilla.get_z_vals(rays_o, 2., 6., a.samples, randomized=True)
        batch = {'rays_o': rays_o[None], 'rays_d': rays_d[None], 'viewdirs': rays_d[None], 'z_vals': z[None],
                 'pts': vanilla.get_pts(rays_o, rays_d, z)[None], 'target_s': target[None]}
        out = net.train_step(batch, opt)
        opt.zero_grad(set_to_none=True)
        out['loss'].backward()
        opt.step()
        return out

    res = {'label': a.label, 'rays': n, 'coarse': a.samples, 'fine': net.N_importance, 'netwidth': 256,
           'train_step_ms': windows(step, a.repeats, a.steps, a.warmup)}
    # per-entry-point device spans of ONE step (events around every library call: the step itself is slower under the timer)
    ops.TIMER = ops.KernelTimer()
    out = step()
    torch.cuda.synchronize()
    res['spans_us'] = {k: {'launches': c, 'total_us': round(1e3 * ms, 1)} for k, (c, ms, _) in sorted(ops.TIMER.summary().items())}
    ops.TIMER = None
    res['loss'] = float(out['loss'].detach())
    if a.frame:
        F = a.frame
        j, i = torch.meshgrid(torch.arange(F, dtype=torch.float32), torch.arange(F, dtype=torch.float32), indexing='ij')
        d = torch.stack([(i - 0.5 * F) / (1.3889 * F), -(j - 0.5 * F) / (1.3889 * F), -torch.ones_like(i)], -1).reshape(-1, 3)
        o = torch.tensor([0., 0., 4.]).expand_as(d)
        o, d = o.contiguous().to(dev), d.to(dev)
        vd = torch.nn.functional.normalize(d, dim=-1)
        z = vanilla.get_z_vals(o, 2., 6., a.samples).contiguous()

        def frame():
            with torch.no_grad():
                ret = net.batchify_forward({'rays_o': o, 'rays_d': d, 'viewdirs': vd, 'z_vals': z, 'pts': vanilla.get_pts(o, d, z)},
                                           is_test=True)
            return ret['rgb']
        res['frame_ms'] = windows(frame, a.frame_repeats, 1, 1)
        res['frame'] = [F, F]
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
