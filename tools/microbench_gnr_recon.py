"""GNR's mesh reconstruction at the shape of configs/gnr/gnr_genebody.py: N_grid = 512 (513^3 = 135 005 697 grid points), loadSize = 512,
4 source views, on the generated scene (gnr_render.synthetic_scene(size=512)).

Rows: the grid hull, the first level's select (reso 8), the fold at reso 8, the iso-surface, the vertex transform with 5 rounds of
smoothing, and the colour pass's point rows -- each kernel path against the tensor-op composition of xrnerf_amd/gnr_recon.py run on
device tensors.  The volume the fold and the surface work on is analytic (a smooth body-sized blob), so that the rows do not depend on a
network.  Device events around single calls, median of 3 after one warm-up call (the tensor-op sides move gigabytes per call); the two
sides' results are compared before they are timed.  The last row is GnrRenderer.reconstruct as a whole with a seeded
GNRMLP(W=64, input_ch_feat=16) whose raw densities straddle zero on this scene (weights drawn here; no trained checkpoint): kernels only -- the reference's host-side path (a 3.2 GB coordinate array, 257 hull chunks) has no device form to time.

  python tools/microbench_gnr_recon.py [--out profiles/gnr_recon_microbench.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, n=3):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


MLP_OPT = dict(input_ch_feat=16, smpl_type='smplx', use_smpl_sdf=True, use_t_pose=True, use_nml=True, use_attention=True, weighted_pool=True,
               use_sh=True, use_viewdirs=True, use_occlusion=True, use_smpl_depth=True, use_occlusion_net=True, angle_diff=False, use_bn=False,
               skips=[2, 4, 6], num_views=4)
RENDER_OPT = dict(N_samples=16, ddp=False, train_encoder=False, projection_mode='perspective', loadSize=512, num_views=4, N_rand=48, use_nml=True,
                  use_attention=True, debug=False, use_vgg=False, use_smpl_sdf=True, use_t_pose=True, use_smpl_depth=True, regularization=False,
                  angle_diff=False, use_occlusion=True, use_occlusion_net=True, use_vh_free=False, use_white_bkgd=False, chunk=524288,
                  N_rand_infer=4096, use_vh=True, laplacian=5, vh_overhead=1)


def renderer(dev, n_grid):
    """GnrRenderer with a GNRMLP(W=64) whose matrices are the default initialisation scaled by 3 under a fixed seed and whose density bias
    is -1.8, so that the occupancy crosses the threshold inside the hull"""
    from xrnerf_amd import builder, gnr_render  # noqa: F401
    mlp = builder.build_mlp(dict(type='GNRMLP', opt=dict(MLP_OPT), W=64))
    torch.manual_seed(5)
    with torch.no_grad():
        for name, p in mlp.named_parameters():
            if name.endswith('weight'):
                torch.nn.init.kaiming_uniform_(p, a=5 ** 0.5)
                p.mul_(3.0)
            elif name.endswith('bias'):
                p.uniform_(-0.1, 0.1)
        mlp.alpha_out_linear.bias.fill_(-1.8)
    ren = builder.build_render(dict(type='GnrRenderer', opt=dict(RENDER_OPT, model=None, N_grid=n_grid)))
    ren.nerf = mlp.to(dev)
    return ren


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--n-grid', type=int, default=512)
    args = ap.parse_args()
    from xrnerf_amd import gnr_recon as R
    from xrnerf_amd.gnr_render import synthetic_scene
    dev = torch.device('cuda')
    N = args.n_grid + 1
    sc = synthetic_scene(size=512)
    d = lambda t: t.to(dev)
    calibs, persps, masks = d(sc['calibs']), d(sc['persps']), R.dilate_masks(d(sc['masks']))
    sf, center = sc['mesh_param']['spatial_freq'], d(sc['mesh_param']['center'])
    grid = R.Grid(N, [-256.0] * 3, [256.0] * 3, sf, center)
    lines = []

    def both(name, fn, same=None):
        R.TENSOR_OPS_STAGES = False
        k = fn()
        R.TENSOR_OPS_STAGES = True
        t = fn()
        if same is not None:
            same(k, t)
        R.TENSOR_OPS_STAGES = False
        tk = timed(fn)
        R.TENSOR_OPS_STAGES = True
        tt = timed(fn)
        R.TENSOR_OPS_STAGES = False
        lines.append('%-46s kernels %9.3f ms (%.3f .. %.3f)   tensor ops %10.3f ms (%.3f .. %.3f)   x %.1f' % ((name,) + tk + tt + (tt[0] / tk[0],)))
        print(lines[-1], flush=True)
        return k

    state = both('grid hull, %d^3 points' % N, lambda: R.grid_hull(grid, calibs, persps, masks, 512, 512), lambda a, b: torch.equal(a, b) or sys.exit('hull differs'))
    share = float(state.float().mean())
    reso = max(N // 64, 1)
    sel = both('level select, reso %d' % reso, lambda: R.level_select(grid, reso, state, calibs, persps, 512, 512),
               lambda a, b: torch.equal(a[0], b[0]) or sys.exit('select differs'))
    # an analytic body-sized volume
    g = torch.arange(N, device=dev, dtype=torch.float32) - N / 2
    r = torch.sqrt(g[:, None, None] ** 2 * 0.6 + g[None, :, None] ** 2 * 0.25 + g[None, None, :] ** 2)
    vol0 = torch.sigmoid((N * 0.11 - r) * (64.0 / N))
    del r

    def fold():
        v, s = vol0.clone(), state.clone()
        if R.TENSOR_OPS_STAGES:
            R._fold_tensor_ops(reso, v, s)
        else:
            from xrnerf_amd import ops
            ops.gnr_recon_fold(reso, v, s)
        return v
    if reso > 1:
        both('fold at reso %d (with two volume copies)' % reso, fold, lambda a, b: torch.equal(a, b) or sys.exit('fold differs'))
    mesh = both('iso-surface', lambda: R.marching_cubes(vol0, 0.5), lambda a, b: torch.equal(a[1], b[1]) or sys.exit('faces differ'))
    verts_idx, faces, normals = mesh
    world = both('vertex transform + 5 smoothing rounds', lambda: R.laplacian_smooth(R.to_world(verts_idx, N, (0, 512), sf, center)[0], faces, 5))
    pts = world.float()
    both('point rows of the colour pass', lambda: R.point_rows(pts, normals, calibs, persps, 512, 512, d(sc['smpl']['rot'][0])))
    lines.append('(hull share of the grid %.4f; first level %d points; surface %d vertices, %d triangles)' % (share, sel[0].shape[0], verts_idx.shape[0], faces.shape[0]))
    del vol0, mesh, world
    ren = renderer(dev, args.n_grid)
    a = dict(feats=d(sc['feats']), images=d(sc['images']), masks=d(sc['masks']), calibs=calibs, bbox=(0, 512, 0, 512), smpl={k: d(v) for k, v in sc['smpl'].items()},
             mesh_param={'center': center, 'spatial_freq': sf}, persps=persps)
    out = []
    t = timed(lambda: out.append(ren.reconstruct(**a)), n=3)
    lines.append('%-46s kernels %9.3f ms (%.3f .. %.3f)   levels %s, %d vertices, %d triangles' % (('GnrRenderer.reconstruct, GNRMLP(W=64)',) + t + (ren.recon_levels, len(out[-1][0]), len(out[-1][1]))))
    print(lines[-1], flush=True)
    text = '# tools/microbench_gnr_recon.py on %s, N_grid = %d, loadSize = 512, 4 views; median of 3 calls (min .. max)\n' % (torch.cuda.get_device_name(0), args.n_grid) + '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
