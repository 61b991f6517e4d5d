"""GNR's body depth maps at the shape of configs/gnr/gnr_genebody.py: four source views at 512 x 512 of synthetic_mesh(5, 0) -- 10 242
vertices and 20 480 faces, the subdivision nearest to SMPL's 6 890 / 13 776 -- in gnr_render.synthetic_scene's cameras.

Rows: depth_maps on the kernels (four views in one call; the projection and the rasteriser separately), then one view of it -- the
kernel path against the module's own tensor-op path (gnr_raster.TENSOR_OPS_STAGES: per face, vectorised over its box, on the device),
the two alternating window by window in one process, their maps compared bit for bit before they are timed.  The tensor-op path makes
some hundred launches per face, so its windows hold one call of one view (the comparison run is its warm-up).  Next to them the render_rays training call with its
backward at the same scene (1024 rays x 256 samples, the configuration's GNRMLP: the last row of tools/microbench_gnr_render.py, code
this module does not touch), in front of which the maps are made once per frame, and the maps' share of it.

  python tools/microbench_gnr_raster.py [--out profiles/gnr_raster_microbench.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows(fns, n_windows=5, n_calls=10, warmup=3):
    """fns: {name: callable}; -> {name: (median ms per call, min, max)}, the callables alternating window by window"""
    for f in fns.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(n_windows):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n_calls):
                f()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) / n_calls)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=int, default=1024)
    ap.add_argument('--samples', type=int, default=256)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--map', type=int, default=128)
    ap.add_argument('--subdivisions', type=int, default=5)
    ap.add_argument('--tensor-op-windows', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from xrnerf_amd import builder, gnr_raster as RA, gnr_render as GR
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    R, S, V, size = args.rays, args.samples, 4, args.size
    sc = GR.synthetic_scene(0, R, S, V, size, args.channels, args.map, args.map, args.subdivisions)
    d = lambda t: t.to(dev)
    verts, faces, calibs, persps = d(sc['smpl']['verts']), d(sc['smpl']['faces']), d(sc['calibs']), d(sc['persps'])
    lines = ['GNR body depth maps on %s: %d views at %d x %d, %d vertices, %d faces' % (torch.cuda.get_device_name(0), V, size, size, verts.shape[0],
                                                                                      faces.shape[0])]
    maps = RA.depth_maps(verts, faces, calibs, persps, size, size)
    pv = RA.projected_vertices(verts, calibs, persps)

    def tensor_ops_one_view():
        RA.TENSOR_OPS_STAGES = True
        try:
            return RA.depth_maps(verts, faces, calibs[:1], persps[:1], size, size)
        finally:
            RA.TENSOR_OPS_STAGES = False
    print('comparing the two paths on one view ...', flush=True)
    one_t = tensor_ops_one_view()
    one_k = RA.depth_maps(verts, faces, calibs[:1], persps[:1], size, size)
    torch.cuda.synchronize()
    covered = int((maps > 0).sum())
    lines += ['covered pixels: %d of %d (%.1f %%); dilated stand-in of the scene: %d; covered outside the scene\'s dilated mask: %d'
              % (covered, maps.numel(), 100.0 * covered / maps.numel(), int((sc['smpl']['depth'] > 0).sum()), int(((maps > 0) & ~(d(sc['masks']) > 0)).sum())),
              'one view, kernel path against tensor-op path on the device: %d of %d map values differ in their bits'
              % (int((one_k.view(torch.int32) != one_t.view(torch.int32)).sum()), one_k.numel()), '',
              'median ms per call (min .. max)', '']
    k4 = windows({'depth_maps': lambda: RA.depth_maps(verts, faces, calibs, persps, size, size),
                  'projection': lambda: RA.projected_vertices(verts, calibs, persps),
                  'rasteriser': lambda: RA.rasterize(pv, faces, size, size, True, 1e-6, True)})
    for name in ('depth_maps', 'projection', 'rasteriser'):
        lines.append('%-44s %9.4f (%.4f .. %.4f)   5 windows of 10 calls' % (('four views, kernels: %s' % name,) + k4[name]))
    print('timing the pair ...', flush=True)
    pair = windows({'kernel': lambda: RA.depth_maps(verts, faces, calibs[:1], persps[:1], size, size), 'tensor ops': tensor_ops_one_view},
                   n_windows=args.tensor_op_windows, n_calls=1, warmup=0)          # (the comparison above was the warm-up)
    lines.append('%-44s kernel %9.4f (%.4f .. %.4f)   tensor ops %11.2f (%.2f .. %.2f)   tensor ops / kernel = %.0f x   %d windows of 1 call'
                 % (('one view, depth_maps',) + pair['kernel'] + pair['tensor ops'] + (pair['tensor ops'][0] / pair['kernel'][0], args.tensor_op_windows)))

    # the render_rays training call with its backward, as tools/microbench_gnr_render.py's last row builds it
    with open(os.path.join(ROOT, 'tests', 'golden', 'gnr_render_cfg.json')) as f:
        cfg = json.load(f)
    mlp = builder.build_mlp(dict(type='GNRMLP', opt=dict(cfg['nerf'], input_ch_feat=args.channels))).to(dev)
    ren = builder.build_render(dict(type='GnrRenderer', opt=dict(cfg['nerf_renderer'], model=None, N_samples=S, loadSize=size, N_rand=R)))
    ren.nerf = mlp
    param = {'center': d(sc['mesh_param']['center']), 'spatial_freq': sc['mesh_param']['spatial_freq']}
    feats, images, masks, rays, gt, t_rand, noise = (d(sc[k]) for k in ('feats', 'images', 'masks', 'rays', 'rgb_gt', 't_rand', 'noise'))

    def step(depth):
        smpl = dict({k: d(v) for k, v in sc['smpl'].items()}, depth=depth)

        def run():
            rgb, _ = ren.render_rays(rays, feats, images, masks, calibs, smpl, param, persps=persps, q_persps=sc['q_persps'], is_train=True, t_rand=t_rand,
                                     noise=noise)
            mlp.zero_grad(set_to_none=True)
            ren.cal_loss(rgb, gt).backward()
        return run
    print('timing render_rays ...', flush=True)
    r = windows({'dilated stand-in': step(d(sc['smpl']['depth'])), 'rasterised maps': step(maps)})
    lines.append('')
    for name in ('dilated stand-in', 'rasterised maps'):
        lines.append('%-44s %9.4f (%.4f .. %.4f)   5 windows of 10 calls' % (('render_rays training call + backward, %s' % name,) + r[name]))
    call = r['rasterised maps']
    lines += ['', 'the maps are made once per frame in front of that call: %.4f ms = %.2f %% of it; the call\'s own spread over its windows is %.4f ms = %.2f %%'
              % (k4['depth_maps'][0], 100.0 * k4['depth_maps'][0] / call[0], call[2] - call[1], 100.0 * (call[2] - call[1]) / call[0])]
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
