"""The scene data pipelines at the shapes of the vanilla NeRF configs: the train item of configs/nerf/nerf_blender_base01.py (a 400 x 400
image, 4096 selected rays x 64 samples, perturbed) and its 800 x 800 x 64 test frame.

Rows, alternating window by window in one process, their outputs compared before they are timed (same select_inds / t_rand):
  fused        the config-shaped list through Compose: one xr_pipe_ray_front launch (csrc/xr_pipeline.hip)
  tensor ops   the same Compose forced to the step-by-step path (Compose.fuse = False) on the device -- what the launch replaces
The timed calls make their own draws (torch.randperm / torch.rand on the device) in both rows.

  python tools/microbench_pipeline.py [--out profiles/pipeline_microbench.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows(fns, n_windows=5, warmup=3):
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


def lists(H, W, focal, n_rays, S):
    """train_pipeline (from GetRays on) and test_pipeline of configs/nerf/nerf_blender_base01.py with the datainfo of an H x W scene"""
    info = dict(H=H, W=W, focal=focal, K=np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]]), hwf=[H, W, focal], near=2., far=6.)
    tail = lambda train: [dict(type='GetViewdirs', enable=True), dict(type='ToNDC', enable=False), dict(type='GetBounds', enable=True),
                          dict(type='GetZvals', enable=True, lindisp=False, N_samples=S), dict(type='PerturbZvals', enable=train),
                          dict(type='GetPts', enable=True)]
    train = [dict(type='ToTensor', enable=True, keys=['pose', 'target_s']), dict(type='GetRays', enable=True),
             dict(type='SelectRays', enable=True, sel_n=n_rays, precrop_iters=500, precrop_frac=0.5)] + tail(True) + \
            [dict(type='DeleteUseless', enable=True, keys=['pose', 'iter_n'])]
    test = [dict(type='ToTensor', enable=True, keys=['pose']), dict(type='GetRays', enable=True), dict(type='FlattenRays', enable=True)] + tail(False) + \
           [dict(type='DeleteUseless', enable=True, keys=['pose'])]
    return [dict(s, **info) for s in train], [dict(s, **info) for s in test]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from xrnerf_amd import pipelines
    from xrnerf_amd.datasets import pose_spherical
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    pose = torch.from_numpy(pose_spherical(30.0, -30.0, 4.0)[:3, :4].copy()).to(dev)
    lines = ['scene data pipelines on %s (median of 5 alternating windows, ms per item; min .. max)' % torch.cuda.get_device_name(0)]
    for what, H, n_rays, S, calls in (('train item 400 x 400, 4096 rays x 64', 400, 4096, 64, 50), ('test frame 800 x 800 x 64', 800, 0, 64, 5)):
        focal = 0.5 * H / np.tan(0.5 * 0.6911112070083618)
        train, test = lists(H, H, focal, n_rays, S)
        image = torch.rand((H, H, 3), device=dev)
        fused, plain = pipelines.Compose(train if n_rays else test), pipelines.Compose(train if n_rays else test)
        plain.fuse = False
        assert fused.fused is not None
        first = (lambda: {'pose': pose, 'target_s': image, 'iter_n': 1000}) if n_rays else (lambda: {'pose': pose})
        # the two rows on the same draws: the same keys, shapes and dtypes; the largest difference per output
        draws = {'select_inds': torch.randperm(H * H, device=dev)[:n_rays], 't_rand': torch.rand((n_rays, S), device=dev)} if n_rays else {}
        a, b = fused(dict(first(), **draws)), plain(dict(first(), **draws))
        torch.cuda.synchronize()
        assert sorted(a) == sorted(b) and all(tuple(a[k].shape) == tuple(b[k].shape) and a[k].dtype == b[k].dtype for k in a)
        diff = {k: float((a[k].double() - b[k].double()).abs().max()) for k in a if k != 'src_shape'}
        lines.append('%s: max |fused - tensor ops| %s' % (what, '  '.join('%s %.2e' % kv for kv in diff.items())))
        del a, b
        res = windows({'fused': (lambda: fused(first()), calls), 'tensor ops': (lambda: plain(first()), calls)})
        for k, (med, lo, hi) in res.items():
            lines.append('    %-11s %9.4f   (%.4f .. %.4f)' % (k, med, lo, hi))
        lines.append('    tensor ops / fused: %.1f x' % (res['tensor ops'][0] / res['fused'][0]))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
