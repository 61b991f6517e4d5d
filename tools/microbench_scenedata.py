"""The BungeeNeRF data side at the shapes of configs/bungeenerf/bungeenerf_multiscale_google.py: a training item of 2048 rays x 65 edges
over a synthetic multi-altitude set, and a validation frame of 360 x 640 (the 1080 x 1920 captures at factor 3).

Rows, alternating window by window in one process, their outputs compared before they are timed (same permutation):
  item  fused     BungeeState.item: one xr_bgd_item launch (csrc/xr_bungeedata.hip)
        composed  what the parent commit has for the same work: BungeeRayTable.batch (slices of the materialised [N H W, 3, 3] table and
                  GetViewdirs' tensor ops) + bungee.bungee_zvals (one xr_bungee_zvals launch)
  frame fused     ops.bgd_frame: one xr_bgd_frame launch
        composed  bungee.make_val_pipeline: pose_rays' tensor ops + one xr_bungee_zvals launch
BungeeRayTable normalises the camera directions in fp32 and divides by a Python-float focal, so its rays differ from the float64 chain
in the last bits (printed); bounds and z-values are compared exactly against ops.bungee_zvals of the fused rays.  The resident bytes per
ray of both forms are printed beside the times.

  python tools/microbench_scenedata.py [--out profiles/scenedata_microbench.txt] [--per-scale 8]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from microbench_pipeline import windows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--per-scale', type=int, default=8)
    args = ap.parse_args()
    from xrnerf_amd import bungee, bungeedata, ops
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    H, W, n_rand, S, stage = 360, 640, 2048, 65, 2
    c = bungee.synthetic_city(H=H, W=W, n_per_scale=args.per_scale, seed=1)
    n = c['poses'].shape[0]
    focal, origin, scale = np.float64(c['focal']), tuple(float(v) for v in c['scene_origin']), float(c['scene_scale'])
    i_test = np.arange(n)[::16]
    i_train = np.array([i for i in range(n) if i not in i_test])
    codes = bungeedata.scale_codes(n, n, c['scale_split'], stage)
    state = bungeedata.BungeeState(H, W, focal, c['poses'], c['images'], codes, i_train, dev, seed=0)
    table = bungee.BungeeRayTable(H, W, float(focal), c['poses'], c['images'], c['scale_split'], stage, i_data=i_train, perm=state.perm.cpu(), n_images=n, device=dev)
    lines = ['BungeeNeRF data on %s: %d train images of %d x %d, %d rays (median of 5 alternating windows, ms per call; min .. max)'
             % (torch.cuda.get_device_name(0), len(i_train), H, W, len(state))]
    held = sum(t.numel() * t.element_size() for t in (table.rays_rgb, table.radii, table.scale_code))
    lines.append('resident bytes per ray: images + camera table + permutation %.1f; the fp32 tables of BungeeRayTable %.1f; the reference float64 tables 88'
                 % (state.bytes_per_ray(), held / float(len(table))))
    kw = dict(S=S, ray_nearfar='sphere', scene_origin=origin, scaling=scale)
    fused = lambda idx=3: state.item(idx, n_rand, **kw)
    composed = lambda idx=3: bungee.bungee_zvals(table.batch(idx, n_rand), S, 'sphere', origin, scale)
    a, b = fused(), composed()
    near, far, z = ops.bungee_zvals(a['rays_o'], a['viewdirs'], None, None, S, 'sphere', origin, scale)
    torch.cuda.synchronize()
    assert sorted(a) == sorted(b) and torch.equal(a['near'], near) and torch.equal(a['far'], far) and torch.equal(a['z_vals'], z)
    assert torch.equal(a['target_s'], b['target_s']) and torch.equal(a['scale_code'], b['scale_code']) and torch.equal(a['rays_o'], b['rays_o'])
    diff = {k: float((a[k].double() - b[k].double()).abs().max()) for k in ('rays_d', 'viewdirs', 'radii')}
    assert diff['rays_d'] <= 4 * 2.0 ** -24 and diff['viewdirs'] <= 4 * 2.0 ** -24          # radii difference neighbouring directions: printed only
    lines.append('train item %d rays x %d: near / far / z_vals equal ops.bungee_zvals of the fused rays; rays_o, target_s, scale_code equal the table; max |fused - table| %s'
                 % (n_rand, S, '  '.join('%s %.2e' % kv for kv in diff.items())))
    res = windows({'fused': (fused, 50), 'composed': (composed, 50)})
    for k, (med, lo, hi) in res.items():
        lines.append('    %-11s %9.4f   (%.4f .. %.4f)' % (k, med, lo, hi))
    lines.append('    composed / fused: %.2f x' % (res['composed'][0] / res['fused'][0]))
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    pose = torch.from_numpy(np.ascontiguousarray(c['poses'][int(i_test[0])][:3, :4], dtype=np.float32)).to(dev)
    val = bungee.make_val_pipeline(H, W, K, S, 'sphere', origin, scale)
    frame_fused = lambda: ops.bgd_frame(pose, H, W, K, **kw)
    frame_composed = lambda: val({'pose': pose})
    a, b = frame_fused(), frame_composed()
    near, far, z = ops.bungee_zvals(a['rays_o'], a['viewdirs'], None, None, S, 'sphere', origin, scale)
    host = bungee.pose_rays(pose.cpu(), H, W, K)
    torch.cuda.synchronize()
    assert torch.equal(a['near'], near) and torch.equal(a['far'], far) and torch.equal(a['z_vals'], z)
    assert all(torch.equal(a[k].cpu(), host[k]) for k in ('rays_o', 'rays_d', 'viewdirs'))
    # radii: against the same lines in numpy (IEEE square root and division) on the host's rays_d.  torch.sqrt on a host tensor is a vector
    # library's and, depending on the machine, not correctly rounded for every argument: the rays where pose_rays' own radii differ are counted
    d = host['rays_d'].view(H, W, 3).numpy()
    e = d[:-1] - d[1:]
    dx = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
    ieee = torch.from_numpy(((np.concatenate([dx, dx[-2:-1]], 0) * np.float32(2)) / np.sqrt(np.float32(12))).reshape(-1, 1))
    assert ieee.dtype == torch.float32 and torch.equal(a['radii'].cpu(), ieee)
    off = int((host['radii'].view(torch.int32) != ieee.view(torch.int32)).sum())
    diff = {k: float((a[k].double() - b[k].double()).abs().max()) for k in ('rays_d', 'viewdirs', 'radii')}
    lines.append('validation frame %d x %d x %d: rays_o, rays_d, viewdirs equal pose_rays on host tensors, radii equal the same lines in numpy (pose_rays on host tensors differs '
                 'from those in %d of %d rays: this host\'s torch.sqrt); near / far / z_vals equal ops.bungee_zvals of them; max |fused - device tensor ops| %s'
                 % (H, W, S, off, ieee.numel(), '  '.join('%s %.2e' % kv for kv in diff.items())))
    res = windows({'fused': (frame_fused, 20), 'composed': (frame_composed, 20)})
    for k, (med, lo, hi) in res.items():
        lines.append('    %-11s %9.4f   (%.4f .. %.4f)' % (k, med, lo, hi))
    lines.append('    composed / fused: %.2f x' % (res['composed'][0] / res['fused'][0]))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
