"""The Mip-NeRF multiscale data side at the shapes of configs/mipnerf/mipnerf_multiscale.py on Lego: 100 views x 4 levels of 800 x 800
(8.5e7 rays), a training item of 1024 rays x 129 samples (randomised), and the test frame of each of the four sizes.

Rows, alternating window by window in one process, their outputs compared before they are timed (same ray_indices / t_rand):
  fused    the config's train_pipeline through Compose over the CameraTable: one xr_ms_rays launch (csrc/xr_multiscale.hip)
  table    the same Compose over the materialised fp32 tables on the device (eight index gathers and GetZvals' tensor ops) -- what a
           straight port of the reference does, and what the launch replaces
  frames   the seven ray arrays and z_vals of one test frame per size (one range launch and a [1, S] row, expanded)
The timed calls make their own draws (torch.randint / torch.rand on the device) in both rows.  The resident bytes of both forms are
printed beside the times; the pyramid of the 100 base views (xr_ms_pyramid) is timed once.

  python tools/microbench_multiscale.py [--out profiles/multiscale_microbench.txt] [--views 100]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from microbench_pipeline import windows  # noqa: E402

KEYS = ['rays_o', 'rays_d', 'viewdirs', 'radii', 'lossmult', 'near', 'far']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--views', type=int, default=100)
    ap.add_argument('--size', type=int, default=800)
    args = ap.parse_args()
    from xrnerf_amd import multiscale, ops, pipelines
    from xrnerf_amd.datasets import pose_spherical
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    N, H, n_down, n_rand, S = args.views, args.size, 4, 1024, 129
    focal = 0.5 * H / np.tan(0.5 * 0.6911112070083618)
    rng = np.random.default_rng(0)
    meta = {k: [] for k in ('cam2world', 'width', 'height', 'focal', 'near', 'far', 'lossmult', 'pix2cam')}
    for i in range(N):
        c2w = pose_spherical(float(rng.uniform(-180, 180)), float(rng.uniform(-60, -10)), 4.0).astype(np.float64)
        for j in range(n_down):
            h, f = H >> j, focal / 2 ** j
            meta['cam2world'].append(c2w), meta['width'].append(h), meta['height'].append(h), meta['focal'].append(f)
            meta['near'].append(2.), meta['far'].append(6.), meta['lossmult'].append(4. ** j)
            meta['pix2cam'].append([[1. / f, 0., -.5 * h / f], [0., -1. / f, .5 * h / f], [0., 0., -1.]])
    lines = ['Mip-NeRF multiscale data on %s: %d views x %d levels of %d x %d (median of 5 alternating windows, ms per item; min .. max)'
             % (torch.cuda.get_device_name(0), N, n_down, H, H)]
    # the converter's pyramid of the base views, timed once (after one warm-up call on two views)
    base = torch.randint(0, 256, (N, H, H, 4), dtype=torch.uint8, device=dev)
    ops.ms_pyramid(base[:2], n_down, True, want=('pixels',))
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    packed = ops.ms_pyramid(base, n_down, True, want=('pixels',))['pixels']
    stop.record()
    torch.cuda.synchronize()
    lines.append('pyramid of %d x %d x %d x 4 bytes -> %d packed pixels: %.2f ms (one call)' % (N, H, H, packed.shape[0], start.elapsed_time(stop)))
    del base
    table = multiscale.CameraTable({k: np.array(v) for k, v in meta.items()}, packed, dev)
    native = table.images.numel() * 4 + table.cams.numel() * 8 + table.hw.numel() * 4 + table.prefix.numel() * 8
    # the reference's form: one fp32 table per key, filled frame by frame by the kernel
    tabs = {k: torch.empty((table.total, 1 if k in ('radii', 'lossmult', 'near', 'far') else 3), device=dev) for k in KEYS}
    for i in range(len(table)):
        lo, hi = int(table.offsets[i]), int(table.offsets[i + 1])
        for k, v in table.frame(i).items():
            tabs[k][lo:hi] = v.reshape(hi - lo, -1)
    tabs['target_s'] = table.images
    straight = sum(v.numel() * 4 for v in tabs.values())
    lines.append('resident: images + camera table %.3f GB; the materialised 16-float tables %.3f GB (%d rays)' % (native / 1e9, straight / 1e9, table.total))
    steps = [dict(type='MipMultiScaleSample', keys=['target_s'] + KEYS, N_rand=n_rand), dict(type='GetZvals', enable=True, lindisp=False, N_samples=S, randomized=True),
             dict(type='ToTensor', keys=['target_s'] + KEYS)]
    fused, plain = pipelines.Compose(steps), pipelines.Compose(steps)
    assert type(fused.fused).__name__ == 'MultiscaleRun'
    draws = lambda: {'ray_indices': idx.clone(), 't_rand': t_rand.clone()}
    idx, t_rand = torch.randint(0, table.total, (n_rand,), device=dev), torch.rand((n_rand, S), device=dev)
    a, b = fused(dict({'camera_table': table}, **draws())), plain(dict(tabs, **draws()))
    torch.cuda.synchronize()
    assert sorted(a) == sorted(b) and all(tuple(a[k].shape) == tuple(b[k].shape) and a[k].dtype == b[k].dtype for k in a)
    lines.append('train item %d rays x %d: max |fused - table| %s' % (n_rand, S, '  '.join('%s %.2e' % (k, float((a[k].double() - b[k].double()).abs().max())) for k in a)))
    res = windows({'fused': (lambda: fused({'camera_table': table}), 50), 'table': (lambda: plain(dict(tabs)), 50)})
    for k, (med, lo, hi) in res.items():
        lines.append('    %-11s %9.4f   (%.4f .. %.4f)' % (k, med, lo, hi))
    lines.append('    table / fused: %.2f x' % (res['table'][0] / res['fused'][0]))

    def frame(i):
        out = table.frame(i)
        out['z_vals'] = table.z_row(i, S, False).expand(out['near'].shape[0], out['near'].shape[1], S)
        return out
    res = windows({'%d x %d' % table.sizes[j]: ((lambda j=j: frame(j)), 10) for j in range(n_down)})
    lines.append('test frame (seven ray arrays, z_vals [1, %d] expanded):' % S)
    for k, (med, lo, hi) in res.items():
        lines.append('    %-11s %9.4f   (%.4f .. %.4f)' % (k, med, lo, hi))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
