"""The ZJU-MoCap / H36M data side at the shapes of configs/neuralbody/nb_zjumocap_313.py: a 512 x 512 prepared picture (1024 x 1024 at
ratio 0.5), a training item of 1024 rays x 64 samples (perturbed) and the whole test frame.

Rows, alternating window by window in one process, their outputs compared for equality before they are timed (same ray_draws / t_rand):
  fused-2    NBGetRays .. GetPts through Compose over the prepared picture: xr_body_sample (one workgroup, the rounds inside) and
             xr_body_points (one thread per (ray, sample)) -- csrc/xr_bodydata.hip
  fused-1    the same with z_vals and pts written by the sampling workgroup itself (BodyRun.fused_points): one launch
  stepwise   the same Compose with fuse = False: every transform on its own, numpy on the host in the reference's arithmetic (float64
             rays of every pixel, six polygon fills, two argwheres, the rejection loop) -- what the reference does per item after its
             disk read, and what the fused run replaces.  There is no device tensor-op form of these transforms
  frame      the whole test frame, fused (count, one read of the survivor count, write, points) and stepwise
The one-time work per picture (xr_body_prepare of a 1024 x 1024 picture at ratio 0.5 with a nonzero D, and xr_body_masks) is timed apart.

  python tools/microbench_bodydata.py [--out profiles/bodydata_microbench.txt] [--size 512]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from microbench_pipeline import windows  # noqa: E402


def lists(n_rays, S):
    head = [dict(type='NBGetRays', enable=True)]
    tail = lambda train: [dict(type='GetZvals', enable=True, lindisp=False, N_samples=S), dict(type='PerturbZvals', enable=train), dict(type='GetPts', enable=True)]
    train = head + [dict(type='NBSelectRays', enable=True, sel_n=n_rays), dict(type='ToTensor', enable=True, keys=['rays_o', 'rays_d', 'target_s', 'near', 'far'])] + tail(True)
    test = head + [dict(type='NBSelectRays', enable=True, sel_all=True),
                   dict(type='ToTensor', enable=True, keys=['rays_o', 'rays_d', 'target_s', 'near', 'far', 'mask_at_box'])] + tail(False)
    return train, test


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--size', type=int, default=512)
    args = ap.parse_args()
    from xrnerf_amd import bodydata, builder, ops, pipelines
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    H = W = args.size
    n_rays, S, ratio = 1024, 64, 0.5
    rng = np.random.default_rng(0)
    lines = ['ZJU-MoCap / H36M data on %s: a %d x %d picture, %d rays x %d samples (median of 5 alternating windows, ms per item; min .. max)'
             % (torch.cuda.get_device_name(0), H, W, n_rays, S)]
    # ---- the one-time work per picture
    Hs, Ws = int(H / ratio), int(W / ratio)
    K_raw = np.array([[1.1 * Ws, 0, 0.5 * Ws], [0, 1.1 * Ws, 0.5 * Hs], [0, 0, 1]])
    D = np.array([-0.08, 0.02, 0.001, -0.001, 0.0])
    yy, xx = np.mgrid[:Hs, :Ws]
    msk8 = (((xx - 0.5 * Ws) / (0.22 * Ws)) ** 2 + ((yy - 0.5 * Hs) / (0.42 * Hs)) ** 2 < 1).astype(np.uint8)
    img8, msk8 = torch.from_numpy(rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)).to(dev), torch.from_numpy(msk8).to(dev)
    R = np.eye(3)
    T = np.array([[0.0], [0.0], [3.0]])
    verts = rng.uniform([-0.45, -0.9, -0.2], [0.45, 0.9, 0.2], (6890, 3)).astype(np.float32)
    bounds = bodydata.body_bounds(verts)

    def prepare():
        img, msk = ops.body_prepare(img8, msk8, K_raw, D, ratio, False)
        K = K_raw.copy()
        K[:2] *= ratio
        pic = bodydata.PreparedPicture(img, msk, K, R, T, 'bench')
        pic.lists(bounds)
        return pic
    pic = prepare()
    res = windows({'prepare + lists': (prepare, 3)})
    bound, body = pic.lists(bounds)
    lines.append('one-time per picture: xr_body_prepare of %d x %d at ratio %.1f + xr_body_masks (bound list %d, body list %d): %.3f ms (%.3f .. %.3f); resident %.2f MB'
                 % ((Hs, Ws, ratio, bound.numel(), body.numel()) + res['prepare + lists'] + (pic.nbytes / 1e6,)))
    # ---- the training item
    cfg = builder.ConfigDict(dict(mode='train'))
    short = torch.zeros(1, dtype=torch.int32, device=dev)
    base = lambda mode='train': dict(cfg=builder.ConfigDict(dict(mode=mode)), img=pic.img, msk=pic.msk, cam_K=pic.K.copy(), cam_R=pic.R.copy(), cam_T=pic.T.copy(),
                                     smpl_verts=verts, body_picture=pic, short_items=short)
    train, test = lists(n_rays, S)
    two, one, step = pipelines.Compose(train), pipelines.Compose(train), pipelines.Compose(train)
    assert type(two.fused).__name__ == 'BodyRun'
    one.fused.fused_points, step.fuse = True, False
    draws, t_rand = torch.randint(0, 1 << 62, (ops.BODY_ROUNDS, n_rays), device=dev), torch.rand((n_rays, S), device=dev)
    pinned = lambda: dict(base(), ray_draws=draws.clone(), t_rand=t_rand.clone())
    a, b, c = two(pinned()), one(pinned()), step(pinned())
    torch.cuda.synchronize()
    keys = ('rays_o', 'rays_d', 'near', 'far', 'target_s', 'z_vals', 'pts')
    for k in keys:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k].cpu(), c[k].cpu()), k
    lines.append('train item: fused-2, fused-1 and stepwise give identical %s; items short so far %d' % (', '.join(keys), int(short.item())))
    res = windows({'fused-2': (lambda: two(base()), 50), 'fused-1': (lambda: one(base()), 50), 'stepwise': (lambda: step(base()), 2)})
    for k, (med, lo, hi) in res.items():
        lines.append('    %-11s %9.4f   (%.4f .. %.4f)' % (k, med, lo, hi))
    lines.append('    stepwise / fused-2: %.1f x;  fused-1 / fused-2: %.2f x' % (res['stepwise'][0] / res['fused-2'][0], res['fused-1'][0] / res['fused-2'][0]))
    # ---- the test frame
    ff, fs = pipelines.Compose(test), pipelines.Compose(test)
    fs.fuse = False
    a, c = ff(base('test')), fs(base('test'))
    torch.cuda.synchronize()
    for k in keys + ('mask_at_box',):
        assert torch.equal(a[k].cpu(), c[k].cpu()), k
    res = windows({'fused': (lambda: ff(base('test')), 20), 'stepwise': (lambda: fs(base('test')), 2)})
    lines.append('test frame %d x %d (%d of %d rays hit the box), identical outputs:' % (H, W, a['rays_o'].shape[0], H * W))
    for k, (med, lo, hi) in res.items():
        lines.append('    %-11s %9.4f   (%.4f .. %.4f)' % (k, med, lo, hi))
    lines.append('    stepwise / fused: %.1f x' % (res['stepwise'][0] / res['fused'][0]))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
