"""Registry entries of the BungeeNeRF path (configs/bungeenerf/bungeenerf_multiscale_google.py): `BungeeNerfNetwork`,
`BungeeNerfMLP`, `BungeeEmbedder`, `BungeeNerfRender`, the device-side data glue (bounds + z-values, ray table, validation rays,
the google-data loader) and the runner's stage loop (`train_iteration`).  Constructor signatures, `data` dict keys, sub-module /
parameter names and numerics follow
  /root/reference/xrnerf/models/networks/bungeenerf.py, mlps/bungeenerf_mlp.py, embedders/bungee_embedder.py,
  renders/bungeenerf_render.py, networks/utils/mip.py:132-176, core/runner/bungeenerf_runner.py,
  datasets/pipelines/create.py (BungeeBatchSample, GetRays(include_radius), BungeeGetZvals, BungeeGetBounds),
  datasets/load_data/get_rays.py (get_rays_np_bungee, load_rays_bungee), load_multiscale_google.py and load.py:145-171.

Every stage between the ray batch and the loss is a HIP launch (xrnerf_amd/csrc/xr_bungee.hip: bounds + z-values, cast_rays +
embedding, renderer forward / backward; the Mip-NeRF resampler, xr_mip.hip), and the residual MLP is ONE autograd node on the strided
linear kernels (`_BungeeMlpFn`).  No CPU path: host tensors raise.
"""
import json
import os

import numpy as np
import torch
from torch import nn

from . import builder, mlp_graph as G, ops
from .builder import EMBEDDERS, MLPS, NETWORKS, RENDERS
from .mip import MipSamples, resample_along_rays, sample_along_rays
from .networks import BaseNerfNetwork, get_dist_info, img2mse, mse2psnr, recover_shape, unfold_batching
from .renders import RayRender
from .vanilla import merge_ret


# ------------------------------------------------------------------ data glue
def bungee_zvals(data, N_samples=65, ray_nearfar='sphere', scene_origin=(0., 0., 0.), scene_scaling_factor=1.0):
    """BungeeGetBounds + BungeeGetZvals on the device: data['rays_o'], data['viewdirs'] (and data['near'] / data['far'] when
    ray_nearfar is None) -> data['near'], data['far'] [R,1], data['z_vals'] [R,N_samples]"""
    near, far, z = ops.bungee_zvals(data['rays_o'], data['viewdirs'], data.get('near'), data.get('far'), int(N_samples), ray_nearfar,
                                    scene_origin, scene_scaling_factor)
    data['near'], data['far'], data['z_vals'] = near, far, z
    return data


def pose_rays(pose, H, W, K):
    """GetRays(include_radius=True) + FlattenRays + GetViewdirs for one validation pose [3|4, 4] on its device.  Like the reference,
    these rays_d are NOT normalised (K^-1 pixel directions), while the training table's are; viewdirs are normalised in both."""
    dev = pose.device
    c2w = pose[:3, :4].to(torch.float32)
    i, j = torch.meshgrid(torch.linspace(0, W - 1, W, device=dev), torch.linspace(0, H - 1, H, device=dev), indexing='ij')
    i, j = i.t(), j.t()
    dirs = torch.stack([(i - K[0][2]) / K[0][0], -(j - K[1][2]) / K[1][1], -torch.ones_like(i)], -1)
    rays_d = torch.sum(dirs[..., None, :] * c2w[:3, :3], -1)
    rays_o = c2w[:3, -1].expand(rays_d.shape)
    dx = torch.sqrt(torch.sum((rays_d[:-1, :, :] - rays_d[1:, :, :]) ** 2, -1))
    dx = torch.cat([dx, dx[-2:-1, :]], 0)
    radii = dx[..., None] * 2 / torch.sqrt(torch.tensor(12.0, device=dev))
    data = {'src_shape': torch.tensor([H, W, 3]), 'rays_o': rays_o.reshape(-1, 3).contiguous(),
            'rays_d': rays_d.reshape(-1, 3).contiguous(), 'radii': radii.reshape(-1, 1).contiguous()}
    data['viewdirs'] = (data['rays_d'] / torch.norm(data['rays_d'], dim=-1, keepdim=True)).contiguous()
    return data


def make_val_pipeline(H, W, K, N_samples=65, ray_nearfar='sphere', scene_origin=(0., 0., 0.), scene_scaling_factor=1.0):
    """the config's test_pipeline (GetRays, FlattenRays, GetViewdirs, BungeeGetBounds, BungeeGetZvals) as a `set_val_pipeline` func"""
    def pipeline(d):
        data = pose_rays(d['pose'], H, W, K)
        return bungee_zvals(data, N_samples, ray_nearfar, scene_origin, scene_scaling_factor)
    return pipeline


class BungeeRayTable:
    """load_rays_bungee (get_rays.py) on the device + BungeeBatchSample.  poses [N,3,4+], images [N,H,W,3] are the dataset's images
    from scale_split[cur_stage] on (load.py slices them so), n_images the dataset's total (default N + scale_split[cur_stage]); scale
    codes as the reference assigns them (the first n_images - scale_split[0] of these images get code 0, ...); perm = the permutation
    of the flattened rays (default torch.randperm on the host generator, the reference's draw)."""

    def __init__(self, H, W, focal, poses, images, scale_split, cur_stage, i_data=None, perm=None, n_images=None, device='cuda'):
        poses = torch.as_tensor(np.asarray(poses, np.float64), device=device)[:, :3, :4]
        images = torch.as_tensor(np.asarray(images, np.float32), device=device)
        n = poses.shape[0]
        codes, prev = [], n + scale_split[cur_stage] if n_images is None else n_images
        for cur, spl in enumerate(scale_split[:cur_stage + 1]):
            codes += [cur] * (prev - spl)
            prev = spl
        if len(codes) != n or images.shape[0] != n:
            raise ValueError('BungeeRayTable: %d poses / %d images, but scale_split %s at stage %d gives %d scale codes'
                             % (n, images.shape[0], list(scale_split), cur_stage, len(codes)))
        if i_data is not None and not all(0 <= int(i) < n for i in np.asarray(i_data).ravel()):
            raise ValueError('BungeeRayTable: i_data out of range')
        codes = torch.tensor(codes, dtype=torch.int64, device=device)
        i, j = torch.meshgrid(torch.arange(W, dtype=torch.float32, device=device), torch.arange(H, dtype=torch.float32, device=device),
                              indexing='xy')
        dirs = torch.stack([(i - W * .5) / focal, -(j - H * .5) / focal, -torch.ones_like(i)], -1)
        dirs = dirs / torch.linalg.norm(dirs, dim=-1)[..., None]
        rays_d = torch.sum(dirs[None, ..., None, :].to(torch.float64) * poses[:, None, None, :3, :3], -1)      # [N,H,W,3]
        rays_o = poses[:, None, None, :3, 3].expand(rays_d.shape)
        dx = torch.sqrt(torch.sum((rays_d[:, :-1] - rays_d[:, 1:]) ** 2, -1))
        dx = torch.cat([dx, dx[:, -2:-1]], 1)
        radii = dx[..., None] * 2 / np.sqrt(12)
        sel = torch.arange(n, device=device) if i_data is None else torch.as_tensor(np.asarray(i_data), device=device)
        rays_rgb = torch.stack([rays_o, rays_d, images.to(torch.float64)[:, :H, :W, :3]], 3)[sel]      # [n,H,W,3,3]
        self.rays_rgb = rays_rgb.reshape(-1, 3, 3).to(torch.float32)
        self.radii = radii[sel].reshape(-1, 1).to(torch.float32)
        self.scale_code = codes[sel][:, None, None].expand(len(sel), H, W).reshape(-1, 1)
        if perm is None:
            perm = torch.randperm(self.rays_rgb.shape[0])
        perm = torch.as_tensor(perm)
        if sorted(perm.tolist()) != list(range(self.rays_rgb.shape[0])):
            raise ValueError('BungeeRayTable: perm must be a permutation of the %d rays' % self.rays_rgb.shape[0])
        self.perm = perm.to(device)
        self.rays_rgb, self.radii, self.scale_code = self.rays_rgb[self.perm], self.radii[self.perm], self.scale_code[self.perm]

    def __len__(self):
        return self.rays_rgb.shape[0]

    def batch(self, idx, N_rand):
        """BungeeBatchSample(idx) + GetViewdirs: rays_o, rays_d, target_s, radii, scale_code, viewdirs"""
        s = slice(N_rand * idx, N_rand * idx + N_rand)
        b = self.rays_rgb[s]
        d = {'rays_o': b[:, 0].contiguous(), 'rays_d': b[:, 1].contiguous(), 'target_s': b[:, 2].contiguous(),
             'radii': self.radii[s].contiguous(), 'scale_code': self.scale_code[s].contiguous()}
        d['viewdirs'] = (d['rays_d'] / torch.norm(d['rays_d'], dim=-1, keepdim=True)).contiguous()
        return d


def load_google_data(datadir, factor=None):
    """load_multiscale_google.py: images/*.{jpg,png,...} + poses_enu.json -> (imgs [N,H,W,C] in [0,1], poses [N,3,5], scene_scale,
    scene_origin, scale_split).  Images are read with PIL (cv2 is not a dependency here) and shrunk by an integer `factor` with a
    box filter: the same mean over factor x factor blocks as cv2.INTER_AREA for integer factors, but not pinned against cv2's rounding."""
    from PIL import Image
    imgdir = os.path.join(datadir, 'images')
    files = [os.path.join(imgdir, f) for f in sorted(os.listdir(imgdir)) if f.endswith(('JPG', 'jpg', 'png', 'jpeg', 'PNG'))]
    factor = int(factor or 1)
    imgs, sh = [], None
    for f in files:
        im = np.asarray(Image.open(f))
        if sh is None:
            sh = np.array(im.shape)
        im = im.astype(np.float32)
        h, w = sh[0] // factor, sh[1] // factor
        im = im[:h * factor, :w * factor].reshape(h, factor, w, factor, -1).mean((1, 3))
        imgs.append(im / 255)
    imgs = np.stack(imgs, 0).astype(np.float32)
    with open(os.path.join(datadir, 'poses_enu.json')) as fh:
        data = json.load(fh)
    poses = np.array(data['poses'])[:, :-2].reshape([-1, 3, 5])
    poses[:, :2, 4] = np.array(sh[:2] // factor).reshape([1, 2])
    poses[:, 2, 4] = poses[:, 2, 4] * 1. / factor
    return imgs, poses, data['scene_scale'], np.array(data['scene_origin']), data['scale_split']


def synthetic_city(H=32, W=40, n_per_scale=4, n_scales=3, seed=0, scene_scale=1.0 / 400):
    """A small procedural multi-altitude scene in the google data's conventions: cameras looking down (slightly tilted) at
    n_scales altitudes, the highest first (scale codes 0..n_scales-1 through scale_split), positions in scaled metres on an
    earth-sized globe (scene_origin = globe centre in metres below the local origin, scene_scale), images = a smooth colour
    pattern of the ground point each pixel sees.  Returns numpy arrays: poses [N,3,4], images [N,H,W,3]."""
    rng = np.random.default_rng(seed)
    heights = [3000.0 * 0.4 ** k for k in range(n_scales)]           # 3000, 1200, 480 m
    poses, imgs = [], []
    focal = 1.2 * W
    for k in range(n_scales):
        for _ in range(n_per_scale):
            h = heights[k] * scene_scale
            pos = np.array([rng.uniform(-1, 1) * 600 * scene_scale, rng.uniform(-1, 1) * 600 * scene_scale, h])
            tilt, yaw = rng.uniform(0.05, 0.3), rng.uniform(0, 2 * np.pi)
            fwd = np.array([np.sin(tilt) * np.cos(yaw), np.sin(tilt) * np.sin(yaw), -np.cos(tilt)])
            right = np.cross(fwd, [0., 1., 0.]); right /= np.linalg.norm(right)
            up = np.cross(right, fwd)
            c2w = np.stack([right, up, -fwd, pos], 1)
            i, j = np.meshgrid(np.arange(W) + 0.0, np.arange(H) + 0.0, indexing='xy')
            d = np.stack([(i - W * .5) / focal, -(j - H * .5) / focal, -np.ones_like(i)], -1) @ c2w[:3, :3].T
            t = -pos[2] / d[..., 2]
            gx, gy = (pos[0] + t * d[..., 0]) / scene_scale, (pos[1] + t * d[..., 1]) / scene_scale
            img = np.stack([0.5 + 0.4 * np.sin(gx / 90.0), 0.5 + 0.4 * np.cos(gy / 70.0), 0.5 + 0.3 * np.sin((gx + gy) / 150.0)], -1)
            poses.append(c2w)
            imgs.append(img)
    n = n_per_scale * n_scales
    return {'poses': np.stack(poses).astype(np.float64), 'images': np.stack(imgs).astype(np.float32), 'H': H, 'W': W, 'focal': focal,
            'scene_scale': scene_scale, 'scene_origin': np.array([0.0, 0.0, -ops.EARTH_RADIUS]),
            'scale_split': [n - n_per_scale * (k + 1) for k in range(n_scales)]}


# ------------------------------------------------------------------ embedder
@EMBEDDERS.register_module()
class BungeeEmbedder(nn.Module):
    """[mean, sin(mean 2^l) exp(-0.5 4^l cov), cos(...) exp(...)]_{l<multires} + [d, sin(d 2^l), cos(d 2^l)]_{l<multires_dirs}"""

    def __init__(self, i_embed=0, multires=10, multires_dirs=4, input_ch=3, **kwargs):
        super().__init__()
        if i_embed == -1:
            # the reference's Identity over the 6 (mean, cov) columns contradicts its own get_embed_ch (3): no semantics to follow
            raise NotImplementedError('BungeeEmbedder(i_embed=-1) is inconsistent in the reference (6 columns, get_embed_ch says 3)')
        if input_ch != 3:
            raise NotImplementedError('input_ch must be 3')
        self.multires, self.multires_dirs = int(multires), int(multires_dirs)
        self.embed_ch, self.embed_ch_dirs = input_ch * (1 + 2 * self.multires), input_ch * (1 + 2 * self.multires_dirs)

    def get_embed_ch(self):
        return self.embed_ch, self.embed_ch_dirs

    def forward(self, data):
        s = data['samples']
        if isinstance(s, MipSamples):
            R, S = s.z_vals.shape[0], s.z_vals.shape[1] - 1
            data['embedded'] = ops.bungee_encode(data['viewdirs'], self.multires, self.multires_dirs,
                                                 frustum=(s.rays_o, s.rays_d, s.radii, s.z_vals), ray_shape=s.ray_shape)
        else:                                   # the reference's (means, covs) tuple
            means, covs = s
            R, S = means.shape[:2]
            data['embedded'] = ops.bungee_encode(data['viewdirs'], self.multires, self.multires_dirs, gaussians=(means, covs))
        data['unflatten_shape'] = torch.Size((R, S))
        return data


# ------------------------------------------------------------------ residual MLP
class BungeeNerfBaseBlock(nn.Module):
    def __init__(self, netwidth=256, input_ch=3, input_ch_views=3):
        super().__init__()
        self.pts_linears = nn.ModuleList([nn.Linear(input_ch, netwidth)] + [nn.Linear(netwidth, netwidth) for _ in range(3)])
        self.views_linear = nn.Linear(input_ch_views + netwidth, netwidth // 2)
        self.feature_linear = nn.Linear(netwidth, netwidth)
        self.alpha_linear = nn.Linear(netwidth, 1)
        self.rgb_linear = nn.Linear(netwidth // 2, 3)


class BungeeNerfResBlock(nn.Module):
    def __init__(self, netwidth=256, input_ch=3, input_ch_views=3):
        super().__init__()
        self.pts_linears = nn.ModuleList([nn.Linear(input_ch + netwidth, netwidth), nn.Linear(netwidth, netwidth)])
        self.views_linear = nn.Linear(input_ch_views + netwidth, netwidth // 2)
        self.feature_linear = nn.Linear(netwidth, netwidth)
        self.alpha_linear = nn.Linear(netwidth, 1)
        self.rgb_linear = nn.Linear(netwidth // 2, 3)


def _block_params(blk):
    ps = []
    for layer in blk.pts_linears:
        ps += [layer.weight, layer.bias]
    for layer in (blk.views_linear, blk.feature_linear, blk.alpha_linear, blk.rgb_linear):
        ps += [layer.weight, layer.bias]
    return ps


@MLPS.register_module()
class BungeeNerfMLP(nn.Module):
    """baseblock (4 trunk layers) + cur_stage residual blocks (2 trunk layers on [x_pts | h]); every block has its own alpha / feature /
    view / rgb heads; raw [M, 1 + cur_stage, 4] = [rgb | alpha] per head (mlps/bungeenerf_mlp.py)"""

    def __init__(self, cur_stage=0, netwidth=256, netchunk=1024 * 64, embedder=None, **kwarg):
        super().__init__()
        self.chunk = netchunk
        self.embedder = builder.build_embedder(embedder)
        self.num_resblocks = cur_stage
        self.live_heads = None            # heads whose raw columns the loss reads (set by BungeeNerfNetwork.train_step)
        W = netwidth
        self.input_ch, self.input_ch_dirs = self.embedder.get_embed_ch()
        self.baseblock = BungeeNerfBaseBlock(netwidth=W, input_ch=self.input_ch, input_ch_views=self.input_ch_dirs)
        self.resblocks = nn.ModuleList([BungeeNerfResBlock(netwidth=W, input_ch=self.input_ch, input_ch_views=self.input_ch_dirs)
                                        for _ in range(self.num_resblocks)])

    def run_mlp(self, x):
        W = self.baseblock.feature_linear.weight.shape[0]
        if not (ops._on_device(x) and x.dtype == torch.float32 and x.dim() == 2 and W % 8 == 0):
            raise ops._lib.XrError('BungeeNerfMLP runs on ROCm device float32 [M, C] batches with netwidth a multiple of 8 '
                                   '(there is no CPU path)')
        params = _block_params(self.baseblock)
        for blk in self.resblocks:
            params += _block_params(blk)
        live = self.num_resblocks + 1 if self.live_heads is None else int(self.live_heads)
        return _BungeeMlpFn.apply(x, self.input_ch, self.input_ch_dirs, self.num_resblocks, live, *params)

    def batchify_run_mlp(self, x):
        # netchunk only bounds the reference's activation memory: on the device the whole batch goes through in one piece
        return self.run_mlp(x)

    def forward(self, data):
        data = self.embedder(data)
        out = self.batchify_run_mlp(data['embedded'])
        data['raw'] = out.reshape(list(data['unflatten_shape']) + list(out.shape[1:]))
        del data['unflatten_shape']
        return data


def _block_layout(k):
    """block k's place in the flat parameter list of _block_params: (offset, trunk layers); 2 n_trunk + 8 tensors per block"""
    return (0, 4) if k == 0 else (16 + 12 * (k - 1), 2)


class _BungeeMlpFn(torch.autograd.Function):
    """BungeeNerfMLP.run_mlp as one autograd node over the shared trunk / view-head graph (mlp_graph.py, which explains the buffer
    layouts; the pattern of vanilla._NerfMlpFn).  Here:
      * each residual block's input [x_pts | h] is ONE buffer: x_pts copied once, h written into it by the previous trunk's last layer;
      * each block's view head writes its column range of raw [M, H, 4] through the output row stride;
      * the backward runs block by block from the last; blocks at or above `live` heads have an exactly-zero output gradient (the
        renderer's heads above the stage), so their products are skipped and their parameters get zero tensors (Adam still moves
        them through its moments, as in the reference)."""

    @staticmethod
    def forward(ctx, x, ic, idr, n_res, live, *params):
        xr, _ = ops._rows(x.detach())
        ps = [p.detach() for p in params]
        M, W, Kx = xr.shape[0], ps[0].shape[0], G.ceil4(ic)
        if xr.shape[1] < Kx or xr.shape[1] < ic + idr:
            raise ops._lib.XrError('BungeeNerfMLP: the embedding has %d columns, expected %d' % (xr.shape[1], ic + idr))
        H = n_res + 1
        x_pts, x_dir = xr[:, :Kx], xr[:, ic:ic + idr]
        raw = torch.empty((M, H, 4), dtype=torch.float32, device=xr.device)
        blocks = []
        h = x_pts
        for k in range(H):
            off, n_trunk = _block_layout(k)
            tw = ps[off:off + 2 * n_trunk]
            nxt = None                           # the next residual block's [x_pts | h] buffer
            if k < H - 1:
                nxt = torch.empty((M, Kx + W), dtype=torch.float32, device=xr.device)
                nxt[:, :Kx].copy_(x_pts)
            trunk, y = G.trunk_forward(h, list(zip(tw[0::2], tw[1::2])), ic, out=None if nxt is None else nxt[:, Kx:])
            head = G.view_head_forward(y, x_dir, ps[off + 2 * n_trunk:off + 2 * n_trunk + 8], raw[:, k, :])
            blocks.append((trunk, y, head))
            h = nxt
        ctx.cfg = (ic, n_res, min(max(int(live), 0), H), Kx)
        ctx.blocks = blocks
        ctx.shapes = [p.shape for p in ps]
        return raw

    @staticmethod
    def backward(ctx, d_raw):
        ic, n_res, live, Kx = ctx.cfg
        d_raw = d_raw.contiguous()
        grads = [None] * len(ctx.shapes)
        d_next = None                             # gradient of the next block's [x_pts | h] input
        for k in range(n_res, -1, -1):
            off, n_trunk = _block_layout(k)
            n_p = 2 * n_trunk + 8
            if k >= live:
                for j in range(off, off + n_p):
                    grads[j] = torch.zeros(ctx.shapes[j], dtype=torch.float32, device=d_raw.device)
                continue
            trunk, y, head = ctx.blocks[k]
            grads[off + 2 * n_trunk:off + n_p], dh = G.view_head_backward(d_raw[:, k, :], head, y)
            if d_next is not None:
                dh = dh + d_next[:, Kx:]          # the trunk's output feeds its own head and the next block
            grads[off:off + 2 * n_trunk], d_next = G.trunk_backward(dh, trunk, ic, first=k == 0)
        ctx.blocks = None
        return (None, None, None, None, None) + tuple(grads)


# ------------------------------------------------------------------ renderer
@RENDERS.register_module()
class BungeeNerfRender(nn.Module):
    """renders/bungeenerf_render.py: heads 0..stage summed, midpoint distances times |viewdirs|, cumprod weights"""

    def __init__(self, stage=0, white_bkgd=False, raw_noise_std=0, rgb_padding=0, density_bias=-1, density_activation='softplus',
                 **kwarg):
        super().__init__()
        if density_activation not in ('softplus', 'relu'):
            raise NotImplementedError
        self.white_bkgd, self.raw_noise_std, self.rgb_padding = white_bkgd, raw_noise_std, rgb_padding
        self.density_bias, self.stage, self.density_activation = density_bias, stage, density_activation

    def forward(self, data, is_test=False, noise=None):
        raw, z_vals = data['raw'], data['z_vals']
        if raw.dim() != 4 or raw.shape[1] != z_vals.shape[1] - 1:
            raise ValueError('BungeeNerfRender expects raw [R, S, heads, 4] and interval edges z_vals [R, S+1]')
        noise_std = 0 if is_test else self.raw_noise_std
        if noise is None and noise_std > 0.:
            noise = (torch.randn(raw.shape[:2]) * noise_std).to(raw.device)          # drawn on the host, as the reference does
        rgb, disp, acc, w = RayRender.apply(ops.bungee_render_forward, ops.bungee_render_backward, raw, z_vals, data['viewdirs'],
                                            noise if noise_std > 0. else None, int(self.stage), float(self.density_bias),
                                            float(self.rgb_padding), bool(self.white_bkgd), self.density_activation)
        data['weights'] = w
        return data, {'rgb': rgb, 'disp': disp, 'acc': acc}


# ------------------------------------------------------------------ network
@NETWORKS.register_module()
class BungeeNerfNetwork(BaseNerfNetwork):
    """networks/bungeenerf.py: coarse pass (sample_along_rays) and fine pass (resample_along_rays) through ONE MLP, loss masked by
    scale_code <= stage"""

    def __init__(self, cfg, mlp=None, render=None):
        super().__init__()
        cfg = builder.ConfigDict.wrap(dict(cfg))
        self.phase = cfg.get('phase', 'train')
        self.chunk = cfg.get('chunk', 1024 * 32)
        self.bs_data = cfg.get('bs_data', 'rays_o')
        self.is_perturb = cfg.get('is_perturb', False)
        self.N_importance = cfg.get('N_importance', 0)
        self.resample_padding = cfg.resample_padding
        self.ray_shape = cfg.ray_shape
        if mlp is not None:
            self.mlp = builder.build_mlp(mlp)
        if render is not None:
            self.render = builder.build_render(render)

    def forward(self, data, is_test=False, rand=None):
        """rand: [R, n_z] uniform draws for the randomized resampling (None: drawn on the device)"""
        randomized = not is_test
        data = sample_along_rays(data, self.ray_shape)
        data, ret = self.render(self.mlp(data), is_test)
        if self.N_importance > 0:
            data = resample_along_rays(data, randomized, self.ray_shape, self.resample_padding, rand=rand)
            _, ret2 = self.render(self.mlp(data), is_test)
            ret = merge_ret(ret, ret2)
        return ret

    def batchify_forward(self, data, is_test=False):
        N = data[self.bs_data].shape[0]
        all_ret = {}
        for i in range(0, N, self.chunk):
            chunk = {k: (v[i:i + self.chunk] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == N else v) for k, v in data.items()}
            ret = self.forward(chunk, is_test)
            for k in ret:
                all_ret.setdefault(k, []).append(ret[k])
        return {k: torch.cat(v, 0) for k, v in all_ret.items()}

    def train_step(self, data, optimizer, **kwargs):
        for k in data:
            if torch.is_tensor(data[k]):
                data[k] = unfold_batching(data[k])
        stage = int(kwargs['stage'])
        self.render.stage = stage
        self.mlp.live_heads = stage + 1
        try:
            ret = self.forward(data, is_test=False, rand=kwargs.get('rand'))
        finally:
            self.mlp.live_heads = None
        mask = data['scale_code'] <= stage
        img_loss = img2mse(ret['rgb'] * mask, data['target_s'] * mask)
        psnr = mse2psnr(img_loss)
        loss = img_loss
        if 'coarse_rgb' in ret:
            loss = loss + img2mse(ret['coarse_rgb'] * mask, data['target_s'] * mask)
        log_vars = {'loss': loss.item(), 'psnr': psnr.item()}           # the reference's own logging (and the runner's 0-check)
        return {'loss': loss, 'log_vars': log_vars, 'num_samples': ret['rgb'].shape[0]}

    def _render_pose(self, pose):
        data = self.val_pipeline({'pose': pose})
        with torch.no_grad():
            ret = self.batchify_forward(data, is_test=True)
        return ret, data['src_shape']

    def val_step(self, data, optimizer=None, **kwargs):
        if self.phase == 'test':
            return self.test_step(data, **kwargs)
        rank, _ = get_dist_info()
        if rank != 0:
            return {}
        import time
        for k in data:
            data[k] = unfold_batching(data[k])
        rgbs, disps, gt_imgs, elapsed = [], [], [], []
        for i in range(data['poses'].shape[0]):
            t0 = time.time()
            ret, shape = self._render_pose(data['poses'][i])
            rgb, disp = recover_shape(ret['rgb'], shape), recover_shape(ret['disp'], shape)
            rgbs.append(rgb.cpu().numpy())
            disps.append(disp.cpu().numpy())
            gt_imgs.append(data['images'][i].cpu().numpy())
            elapsed.append(time.time() - t0)
        spiral_rgbs, spiral_disps = [], []
        for i in range(data['spiral_poses'].shape[0]):
            ret, shape = self._render_pose(data['spiral_poses'][i])
            spiral_rgbs.append(recover_shape(ret['rgb'], shape).cpu().numpy())
            spiral_disps.append(recover_shape(ret['disp'], shape).cpu().numpy())
        return {'spiral_rgbs': spiral_rgbs, 'spiral_disps': spiral_disps, 'rgbs': rgbs, 'disps': disps, 'gt_imgs': gt_imgs,
                'elapsed_time': elapsed}

    def test_step(self, data, **kwargs):
        rank, _ = get_dist_info()
        if rank != 0:
            return {}
        for k in data:
            data[k] = unfold_batching(data[k])
        image, idx = data['image'], data['idx'].item()
        ret, shape = self._render_pose(data['pose'])
        return {'rgb': recover_shape(ret['rgb'], shape).cpu().numpy(), 'gt_img': image.cpu().numpy(), 'idx': idx}

    def set_val_pipeline(self, func):
        self.val_pipeline = func


# ------------------------------------------------------------------ the runner's stage loop
def train_iteration(net, batch, optimizer, rands=None):
    """BungeeNerfTrainRunner.train for one batch: for stage in 0..max(scale_code), one train_step, then zero_grad / backward / step
    (mmcv's OptimizerHook), skipped entirely when the loss is exactly 0 (the runner `continue`s before after_train_iter).
    Each stage gets a shallow copy of the batch (the reference hands every stage the same dict, which train_step mutates: its second
    stage would see the first stage's fine z_vals and fail on the 'samples' tuple).  rands: per-stage resampling draws, or None.
    -> the per-stage train_step outputs."""
    from . import runner as _runner
    r = _runner.IterRunner(net, optimizer)
    r.register_hook(_runner.OptimizerHook(), 'ABOVE_NORMAL')
    return _runner.bungee_stages(r, batch, rands=rands)
