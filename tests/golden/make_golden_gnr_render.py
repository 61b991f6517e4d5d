"""Generates tests/golden/ref_gnr_render.npz from the REFERENCE'S OWN GnrRenderer.render_rays and GNRMLP, in the build container only:
    python tests/golden/make_golden_gnr_render.py

The machinery is make_golden_gnr.py's (imported unchanged): the reference's mesh_grid kernels compiled for the host behind its own
MeshGridSearcher, and gnr_render.py imported unmodified.  On top of it: `lpips` is stubbed, the reference's networks/utils/gnr.py and
embedders/gnr_embedder.py are imported from where they lie, `index`, `orthogonal`, `perspective` are set on the loaded gnr_render
module and PositionalEncoding / SphericalHarmonics on the `embedders` package shell, so mlps/gnr_mlp.py imports unmodified too.

Inputs are generated (xrnerf_amd.gnr_render.synthetic_scene), not stored: 48 rays x 16 samples, 4 source views, 64 x 64 images,
feature maps [4, 16, 12, 20], GNRMLP(W=64, input_ch_feat=16) with every option of configs/gnr/gnr_genebody.py.  With default
initialisation every raw density is negative (image and gradients exactly zero), so the weight matrices are scaled by 3 and
alpha_out_linear.bias is set (to -1.8 on this scene's inputs) so that the raw densities straddle zero; the asserts at the end of run() hold the reference alone to a scene in which something is rendered.

Stored per mode (`inf.`: is_train=False; `trn.`: one training call with the stored draws, torch.rand / torch.randn patched inside the
reference's module), from the float32 run and, suffix 64, from a float64 run that is handed the float32 run's hull flags, smpl_vis and
mesh-query results (CastingSearcher), so the two differ by rounding only:
    inside [R S], boundary [R S] (float64 distance in pixels of the nearest view's source index from a rounding boundary across which the
    mask's sign changes: decision_distance),
    vis_margin [M,V] (float64 |z - d|; 0 where another depth pixel is one rounding away), t_vals, pts, xy, z, smpl_vis, attdirs, nerf_input (float64 run: its sampled columns, gathered64), source_rgb, net (the network output,
    occlusion columns stripped), rgb_map, depth, weights, loss, d_net (gradient of the loss in net), d_feats
A second file, ref_gnr_render_params.npz (each committed file stays under 1 MiB), holds the weights under their state_dict keys
(`w.<key>`) and the training call's parameter gradients (`trn.g.<key>` float32 run, `trn.gd.<key>` = float64 run minus float32 run).
gnr_render_cfg.json holds the two option dicts.  The maker asserts a non-zero gradient for every parameter tensor and for the feature
maps (the occlusion head gets its gradient through the attention softmax it weights)."""
import importlib
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_gnr as MG  # noqa: E402
from gnr_render_restatement import decision_distance as _dd  # noqa: E402


def decision_distance(src, maps, positive):
    """gnr_render_restatement.decision_distance on source indices: it takes normalised coordinates"""
    V, H, W = maps.shape
    xy = torch.stack([(src[:, 0] * 2 + 1) / W - 1, (src[:, 1] * 2 + 1) / H - 1], 1)
    return _dd(xy, maps, positive)
import ref_import  # noqa: E402

MLP_OPT = dict(input_ch_feat=16, smpl_type='smplx', use_smpl_sdf=True, use_t_pose=True, use_nml=True, use_attention=True,
               weighted_pool=True, use_sh=True, use_viewdirs=True, use_occlusion=True, use_smpl_depth=True, use_occlusion_net=True,
               angle_diff=False, use_bn=False, skips=[2, 4, 6], num_views=4)
RENDER_OPT = dict(model=None, N_samples=16, ddp=False, train_encoder=False, projection_mode='perspective', loadSize=64, num_views=4,
                  N_rand=48, N_grid=512, use_nml=True, use_attention=True, debug=False, use_vgg=False, use_smpl_sdf=True, use_t_pose=True,
                  use_smpl_depth=True, regularization=False, angle_diff=False, use_occlusion=True, use_occlusion_net=True,
                  use_vh_free=False, use_white_bkgd=False, chunk=524288, N_rand_infer=4096, use_vh=True, laplacian=5, vh_overhead=1)
WEIGHT_SEED, WEIGHT_SCALE, ALPHA_BIAS = 5, 3.0, -1.8


def load_reference(searcher_cls):
    """-> (the loaded gnr_render module, GnrRenderer, GNRMLP)"""
    renderer_cls = MG.load_reference_renderer(searcher_cls)
    if 'lpips' not in sys.modules:
        sys.modules['lpips'] = types.ModuleType('lpips')

    def from_file(name, *path):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref_import.REF, 'xrnerf', 'models', *path))
        mod = importlib.util.module_from_spec(spec)
        mod.__package__ = name.rpartition('.')[0]
        spec.loader.exec_module(mod)
        return mod
    utils = from_file('xrnerf.models.networks.utils._gnr_leaf', 'networks', 'utils', 'gnr.py')
    emb = from_file('xrnerf.models.embedders._gnr_embedder_leaf', 'embedders', 'gnr_embedder.py')
    mod = sys.modules['xrnerf.models.renders.gnr_render']
    mod.index, mod.orthogonal, mod.perspective = utils.index, utils.orthogonal, utils.perspective
    shell = sys.modules['xrnerf.models.embedders']
    shell.PositionalEncoding, shell.SphericalHarmonics = emb.PositionalEncoding, emb.SphericalHarmonics
    mlp_cls = importlib.import_module('xrnerf.models.mlps.gnr_mlp').GNRMLP
    return mod, renderer_cls, mlp_cls


def gnr_weights(mlp):
    """the fixture's weights: default initialisation under a fixed seed, matrices scaled, the density bias raised"""
    torch.manual_seed(WEIGHT_SEED)
    with torch.no_grad():
        for name, p in mlp.named_parameters():
            if name.endswith('weight'):
                torch.nn.init.kaiming_uniform_(p, a=5 ** 0.5)
                p.mul_(WEIGHT_SCALE)
            elif name.endswith('bias'):
                p.uniform_(-0.1, 0.1)
        mlp.alpha_out_linear.bias.fill_(ALPHA_BIAS)


class _PatchedTorch:
    """`torch` as the reference's module sees it during the training call: rand / randn return the stored draws"""

    def __init__(self, rand, randn):
        self._rand, self._randn = rand, randn

    def __getattr__(self, k):
        return getattr(torch, k)

    def rand(self, shape, device=None):
        assert tuple(shape) == tuple(self._rand.shape)
        return self._rand.clone()

    def randn(self, shape, device=None):
        assert tuple(shape) == tuple(self._randn.shape)
        return self._randn.clone()


def run(mod, renderer_cls, mlp, searcher, scene, dtype, is_train, handed=None):
    """one render_rays call of the reference -> dict of recorded tensors.  handed = (inside, smpl_vis) of the float32 run."""
    cast = lambda t: t.to(dtype) if t.is_floating_point() else t
    opt = ref_import.Cfg(RENDER_OPT)
    opt['model'] = mlp
    ren = renderer_cls(opt)
    ren.mesh_searcher = MG.CastingSearcher(searcher)
    rec = {}
    smpl = {k: cast(v) for k, v in scene['smpl'].items()}
    feats = cast(scene['feats']).clone().requires_grad_()
    args = dict(feats=feats, images=cast(scene['images']), masks=cast(scene['masks']), calibs=cast(scene['calibs']), smpl=smpl,
                mesh_param={'center': cast(scene['mesh_param']['center']), 'spatial_freq': scene['mesh_param']['spatial_freq']},
                persps=cast(scene['persps']), q_persps=cast(scene['q_persps']))
    vh = ren.inside_pts_vh

    def inside_pts_vh(pts, masks, smpl_, calibs, persps=None):
        rec['all_pts'] = pts.detach()
        inside, vis, scan_vis = vh(pts, masks, smpl_, calibs, persps)
        if handed is not None:
            inside, vis = handed
        rec['inside'], rec['smpl_vis'] = inside, vis
        return inside, vis, scan_vis
    att = ren.make_att_input

    def make_att_input(pts, viewdirs, calibs, smpl_):
        rec['pts'] = pts.detach()
        rec['attdirs'] = att(pts, viewdirs, calibs, smpl_)
        return rec['attdirs']
    mni = ren.make_nerf_input

    def make_nerf_input(*a, **k):
        rec['nerf_input'], rec['source_rgb'] = mni(*a, **k)
        return rec['nerf_input'], rec['source_rgb']
    mno = ren.make_nerf_output

    def make_nerf_output(nerf_output, t_vals, norm, source_rgb, is_train=True):
        rec['t_vals'] = t_vals.detach()
        rgb_map, weights = mno(nerf_output, t_vals, norm, source_rgb, is_train=is_train)
        rec['weights'] = weights.detach()
        return rgb_map, weights

    def nerf(x, attdirs, smpl_vis=None):
        out = mlp(x, attdirs, smpl_vis=smpl_vis)
        out.retain_grad()
        rec['net_full'] = out
        return out
    ren.inside_pts_vh, ren.make_att_input, ren.make_nerf_input, ren.make_nerf_output, ren.nerf = \
        inside_pts_vh, make_att_input, make_nerf_input, make_nerf_output, nerf
    saved = mod.torch
    if is_train:
        mod.torch = _PatchedTorch(cast(scene['t_rand']), cast(scene['noise']))
    try:
        rgb_map, depth = ren.render_rays(cast(scene['rays']), is_train=is_train, **args)
    finally:
        mod.torch = saved
    loss = ren.cal_loss(rgb_map, cast(scene['rgb_gt']))
    mlp.zero_grad()
    loss.backward()
    V = RENDER_OPT['num_views']
    rec.update(rgb_map=rgb_map.detach(), depth=depth.detach(), loss=loss.detach(), net=rec['net_full'].detach()[:, :4 + V + 1],
               d_net=rec['net_full'].grad[:, :4 + V + 1], d_feats=feats.grad, nerf_input=rec['nerf_input'].detach(),
               source_rgb=rec['source_rgb'].detach(), attdirs=rec['attdirs'].detach())
    assert rec['net_full'].grad[:, 4 + V + 1:].abs().max() == 0          # (the occlusion columns of the output: no scan, so no loss on them)
    for name, p in mlp.named_parameters():
        assert p.grad is not None and p.grad.abs().max() > 0, 'zero gradient in %s' % name
    assert feats.grad.abs().max() > 0
    rec['param_grads'] = {name: p.grad.detach().clone() for name, p in mlp.named_parameters()}
    return rec


def projections(mod, rec, scene, dtype):
    """the hull's projection once more through the reference's own perspective(): xy [V,2,N] normalised and z [V,N] of ALL points"""
    pts = rec['all_pts'].to(dtype)
    V = scene['calibs'].shape[0]
    xyz = mod.perspective(pts.permute((1, 0))[None, ...].expand([V, -1, -1]), scene['calibs'].to(dtype), scene['persps'].to(dtype))
    xy = xyz[:, :2, :] / torch.tensor([[[scene['width']], [scene['width']]]], dtype=dtype) * 2 - 1
    return xy, xyz[:, 2, :]


def main():
    assert ref_import.available(), 'needs the reference checkout (run in the build container)'
    from xrnerf_amd.gnr_render import synthetic_scene
    scene = synthetic_scene()
    R, S = scene['t_rand'].shape
    V, size = scene['calibs'].shape[0], scene['width']
    params = {}
    out = {'weight_seed': np.int64(WEIGHT_SEED), 'weight_scale': np.float64(WEIGHT_SCALE), 'alpha_bias': np.float64(ALPHA_BIAS)}
    with tempfile.TemporaryDirectory() as tmp:
        lib = MG.build_reference_kernels(tmp)
        searcher_cls = MG.load_reference_searcher(MG.mesh_grid_module(lib))
        mod, renderer_cls, mlp_cls = load_reference(searcher_cls)
        mlp32 = mlp_cls(ref_import.Cfg(MLP_OPT), W=64)
        gnr_weights(mlp32)
        torch.set_default_dtype(torch.float64)
        try:
            mlp64 = mlp_cls(ref_import.Cfg(MLP_OPT), W=64)
        finally:
            torch.set_default_dtype(torch.float32)
        mlp64.load_state_dict({k: v.double() for k, v in mlp32.state_dict().items()}, strict=True)
        for mode, is_train in (('inf', False), ('trn', True)):
            r32 = run(mod, renderer_cls, mlp32, searcher_cls(), scene, torch.float32, is_train)
            torch.set_default_dtype(torch.float64)
            try:
                r64 = run(mod, renderer_cls, mlp64, searcher_cls(), scene, torch.float64, is_train, handed=(r32['inside'], r32['smpl_vis']))
            finally:
                torch.set_default_dtype(torch.float32)
            inside = r32['inside'].numpy()
            M = int(inside.sum())
            # how far every point is from a rounding boundary of the nearest-sample index, in float64 on the float32 points
            xy64, z64 = projections(mod, r32, scene, torch.float64)
            src = ((xy64 + 1) * size - 1) / 2
            boundary = decision_distance(src, scene['masks'][:, 0].double(), True).amin(0).numpy()
            vis_boundary = decision_distance(src, scene['smpl']['depth'][:, 0].double(), False).permute(1, 0)[torch.from_numpy(inside)].numpy()
            d = mod.index(scene['smpl']['depth'].double(), xy64, 'nearest').squeeze(1)
            vis_margin = (z64 - d).abs().permute(1, 0)[torch.from_numpy(inside)].numpy()
            vis_margin = np.where(vis_boundary <= 1e-3, 0.0, vis_margin)          # (another depth pixel one rounding away: not compared)
            xy32, z32 = projections(mod, r32, scene, torch.float32)
            sel = torch.from_numpy(inside)
            share = float((boundary <= 1e-3).mean())
            rays_hit = (boundary.reshape(R, S) <= 1e-3).any(1)
            net = r32['net'].numpy()
            acc = r32['weights'].sum(1).numpy()
            crossing = inside.reshape(R, S).any(1)
            print(mode, 'raw density quantiles', np.quantile(net[:, 3], [0, .1, .25, .5, .75, .9, 1]).round(2))
            pos = float((net[:, 3] + (scene['noise'].reshape(-1)[sel].numpy() if is_train else 0) > 0).mean())
            mid = float(((acc > 0.05) & (acc < 0.95))[crossing].mean())
            print('%s: %d points, %d inside, %d rays cross the hull, %d all-inside rays, smpl_vis true %.2f, positive density %.2f, '
                  'acc in (0.05, 0.95) for %.2f of the crossing rays, raw density %.2f .. %.2f, loss %.6f' % (
                      mode, R * S, M, int(crossing.sum()), int((inside.reshape(R, S).all(1)).sum()), float(r32['smpl_vis'].float().mean()),
                      pos, mid, float(net[:, 3].min()), float(net[:, 3].max()), float(r32['loss'])))
            print('%s: %.4f of the points within 1e-3 pixel of a rounding boundary (bar 0.01), %.4f of the rays hold one (bar 0.05), '
                  '%.4f of the visibility margins below 1e-4 (bar 0.01)' % (mode, share, float(rays_hit.mean()), float((vis_margin < 1e-4).mean())))
            assert 0.2 <= pos <= 0.8 and mid >= 0.5
            assert share <= 0.01 and rays_hit.mean() <= 0.05 and (vis_margin < 1e-4).mean() <= 0.01
            assert r32['d_net'].abs().max() > 0 and M > 0
            o = {'inside': inside, 'boundary': boundary, 'vis_margin': vis_margin, 't_vals': r32['t_vals'].numpy(),
                 'smpl_vis': r32['smpl_vis'].numpy(), 'xy': xy32[:, :, sel].permute(2, 0, 1).numpy(), 'z': z32[:, sel].permute(1, 0).numpy(),
                 'xy64': xy64[:, :, sel].permute(2, 0, 1).numpy(), 'z64': z64[:, sel].permute(1, 0).numpy()}
            for k in ('pts', 'attdirs', 'nerf_input', 'source_rgb', 'net', 'rgb_map', 'depth', 'weights', 'loss', 'd_net', 'd_feats'):
                o[k], o[k + '64'] = r32[k].numpy(), r64[k].numpy()
                assert o[k].dtype == np.float32 and o[k + '64'].dtype == np.float64, k
            n_emb = o['nerf_input'].shape[-1] - scene['feats'].shape[1] - 3
            o['gathered64'] = o.pop('nerf_input64')[..., n_emb:]                 # (size cap: the float64 run's sampled columns only)
            o['nerf_input_dev'] = np.abs(r32['nerf_input'].double() - r64['nerf_input']).amax(dim=(0, 1)).numpy()
            o['nerf_input_max'] = r64['nerf_input'].abs().amax(dim=(0, 1)).numpy()
            for k, v in o.items():
                out[mode + '.' + k] = v
            if is_train:
                # the weights under their state_dict keys; the training call's parameter gradients as the float32 run's and the float64
                # run's difference from it (float32 holds that difference to 2^-24 of itself: the float64 gradient is g + gd)
                for name, w in mlp32.state_dict().items():
                    params['w.' + name] = w.numpy()
                for name, g32 in r32['param_grads'].items():
                    params['trn.g.' + name] = g32.numpy()
                    params['trn.gd.' + name] = (r64['param_grads'][name] - g32.double()).float().numpy()
    import json
    with open(os.path.join(HERE, 'gnr_render_cfg.json'), 'w') as f:
        json.dump({'nerf': dict(MLP_OPT), 'nerf_W': 64, 'nerf_renderer': {k: v for k, v in RENDER_OPT.items() if k != 'model'}}, f, indent=1, sort_keys=True)
        f.write('\n')
    ppath = os.path.join(HERE, 'ref_gnr_render_params.npz')
    np.savez_compressed(ppath, **params)
    print('wrote %s (%d bytes)' % (ppath, os.path.getsize(ppath)))
    assert os.path.getsize(ppath) < 1 << 20
    path = os.path.join(HERE, 'ref_gnr_render.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
