"""Registry entries of the vanilla-NeRF path (BASELINE config #1, configs/nerf/nerf_blender_base01.py):
`NerfNetwork`, `NerfMLP`, `BaseEmbedder`, `NerfRender`, plus stratified / hierarchical sampling.

This is the reference's only renderer that runs on a CPU as shipped and is
pure PyTorch there.  Host tensors take plain tensor code (the CPU-runnable parity case).  On the device a training step is
  encode (xr_nerf_encode) -> the MLP as ONE autograd node over the linear kernels (_NerfMlpFn) -> renderer forward / backward
  (xr_nerf_render_train_forward / xr_nerf_render_backward, renders.RayRender) -> resampling + merge + points (xr_nerf_sample_pdf)
and the same again for the fine network (xrnerf_amd/csrc/xr_vanilla.hip; DESIGN.md "Vanilla NeRF (config #1)").  Constructor signatures, `data` dict keys,
sub-module / parameter names (`pts_linears.N`, `views_linears.0`, `feature_linear`, `alpha_linear`,
`rgb_linear`) and numerics follow
  /root/reference/xrnerf/models/embedders/base.py:8-77, mlps/nerf_mlp.py:11-94,
  renders/nerf_render.py:10-98, networks/utils/hierarchical_sample.py:6-53, networks/nerf.py:16-92
  and datasets/pipelines/create.py:486-531,577-601, augment.py:261-283.
"""
import torch
import torch.nn.functional as F
from torch import nn

from . import builder
from .builder import EMBEDDERS, MLPS, NETWORKS, RENDERS
from .networks import BaseNerfNetwork, img2mse, mse2psnr, unfold_batching
from .renders import RayRender


# ------------------------------------------------------------------ positional encoding
@EMBEDDERS.register_module()
class BaseEmbedder(nn.Module):
    """gamma(p) = (p, sin(2^k p), cos(2^k p))_{k<multires}; directions with multires_dirs"""

    def __init__(self, i_embed=0, multires=10, multires_dirs=4, input_ch=3, **kwargs):
        super().__init__()
        self.input_ch = input_ch
        if i_embed == -1:
            self.freqs, self.freqs_dirs = None, None
            self.embed_ch = self.embed_ch_dirs = input_ch
        else:
            self.multires, self.multires_dirs = int(multires), int(multires_dirs)
            self.freqs = [float(2.0 ** k) for k in range(multires)]          # 2**linspace(0, L-1, L)
            self.freqs_dirs = [float(2.0 ** k) for k in range(multires_dirs)]
            self.embed_ch = input_ch * (1 + 2 * multires)
            self.embed_ch_dirs = input_ch * (1 + 2 * multires_dirs)

    def get_embed_ch(self):
        return self.embed_ch, self.embed_ch_dirs

    @staticmethod
    def run_embed(x, freqs):
        if freqs is None:
            return x
        parts = [x]
        for f in freqs:
            parts.append(torch.sin(x * f))
            parts.append(torch.cos(x * f))
        return torch.cat(parts, -1)

    def _kernel_ok(self, pts, viewdirs):
        from . import ops
        if self.freqs is None or self.input_ch != 3 or self.multires > 16 or self.multires_dirs > 16:
            return False
        if not (ops._on_device(pts) and ops._on_device(viewdirs) and pts.dtype == viewdirs.dtype == torch.float32):
            return False
        if pts.shape[-1] != 3 or viewdirs.shape[-1] != 3 or pts.numel() == 0:
            return False
        if torch.is_grad_enabled() and (pts.requires_grad or viewdirs.requires_grad):
            return False                              # the kernel has no backward: a differentiable input keeps the tensor ops
        # [R, S, 3] points with one direction per ray, or one direction per point
        shared = pts.dim() == viewdirs.dim() + 1 and pts.shape[:-2] == viewdirs.shape[:-1]
        return (shared or pts.shape == viewdirs.shape) and ops.vanilla_kernels_available()

    def forward(self, data):
        pts, viewdirs = data['pts'], data['viewdirs']
        data['unflatten_shape'] = pts.shape[:-1]
        if self._kernel_ok(pts, viewdirs):
            # device: one launch; rows padded to a multiple of 4 floats (zeros), which NerfMLP's linear kernels read in place
            from . import ops
            data['embedded'] = ops.nerf_encode(pts, viewdirs, self.multires, self.multires_dirs)
            return data
        if pts.dim() > viewdirs.dim():
            viewdirs = viewdirs[:, None].expand(pts.shape)
        e_pts = self.run_embed(pts.reshape(-1, pts.shape[-1]), self.freqs)
        e_dir = self.run_embed(viewdirs.reshape(-1, viewdirs.shape[-1]), self.freqs_dirs)
        data['embedded'] = torch.cat([e_pts, e_dir], -1)
        return data


# ------------------------------------------------------------------ 8 x 256 MLP with a skip and a view branch
@MLPS.register_module()
class NerfMLP(nn.Module):
    def __init__(self, skips=[4], netdepth=8, netwidth=256, output_ch=4, use_viewdirs=True, netchunk=1024 * 32,
                 embedder=None, **kwarg):
        super().__init__()
        self.skips = list(skips)
        self.chunk = netchunk
        self.use_viewdirs = use_viewdirs
        self.embedder = builder.build_embedder(embedder)
        D, W = netdepth, netwidth
        self.input_ch, self.input_ch_dirs = self.embedder.get_embed_ch()
        layers = [nn.Linear(self.input_ch, W)]
        for i in range(D - 1):
            layers.append(nn.Linear(W + self.input_ch if i in self.skips else W, W))
        self.pts_linears = nn.ModuleList(layers)
        if use_viewdirs:
            self.views_linears = nn.ModuleList([nn.Linear(self.input_ch_dirs + W, W // 2)])
            self.feature_linear = nn.Linear(W, W)
            self.alpha_linear = nn.Linear(W, 1)
            self.rgb_linear = nn.Linear(W // 2, 3)
        else:
            self.output_linear = nn.Linear(W, output_ch)

    def _device_graph_ok(self, x):
        W = self.pts_linears[0].weight.shape[0]
        from . import ops
        if not (ops._on_device(x) and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] > 0 and self.use_viewdirs and len(self.views_linears) == 1
                and W % 4 == 0 and (W // 2) % 4 == 0 and (len(self.pts_linears) - 1) not in self.skips
                and all(l.weight.shape[0] == W for l in self.pts_linears)):
            return False
        if torch.is_grad_enabled() and x.requires_grad:
            return False                                  # the node has no input gradient: the per-layer graph provides it
        if any(p.dtype != torch.float32 or p.device != x.device for p in self.parameters()):
            return False
        if self.input_ch % 4:
            # the first trunk layer and the skip buffer read ceil4(input_ch) columns of x in place (part of the vanilla-NeRF device path)
            return x.shape[1] >= (self.input_ch + 3) // 4 * 4 and ops.vanilla_kernels_available()
        return True

    def run_mlp(self, x):
        if self._device_graph_ok(x):
            # device: the whole MLP as ONE autograd node over the linear kernels, every activation in a buffer of its own layout
            # (_NerfMlpFn below): no concatenations, splits, paddings or per-layer autograd glue between the products
            params = []
            for layer in self.pts_linears:
                params += [layer.weight, layer.bias]
            v = self.views_linears[0]
            params += [v.weight, v.bias, self.feature_linear.weight, self.feature_linear.bias, self.alpha_linear.weight, self.alpha_linear.bias,
                       self.rgb_linear.weight, self.rgb_linear.bias]
            return _NerfMlpFn.apply(x, tuple(self.skips), self.input_ch, self.input_ch_dirs, *params)
        x_pts, x_dir = torch.split(x, [self.input_ch, self.input_ch_dirs], dim=-1)
        if x.is_cuda:
            # device: linear + bias + relu (and their gradients) on the fp32-MFMA kernels (xrnerf_amd/linear.py); same
            # maths, summation order aside.  alpha and feature heads share one product (rows of one weight matrix).
            from .linear import linear_act_padded as lin
            x_pts = x_pts.contiguous()
        else:
            def lin(t, w, b, relu=False):
                y = F.linear(t, w, b)
                return F.relu(y) if relu else y
        h = x_pts
        for i, layer in enumerate(self.pts_linears):
            h = lin(h, layer.weight, layer.bias, True)
            if i in self.skips:
                h = torch.cat([x_pts, h], -1)
        if not self.use_viewdirs:
            return lin(h, self.output_linear.weight, self.output_linear.bias)
        if x.is_cuda:
            W = self.feature_linear.weight.shape[0]
            both = lin(h, torch.cat([self.feature_linear.weight, self.alpha_linear.weight], 0),
                       torch.cat([self.feature_linear.bias, self.alpha_linear.bias], 0))
            feature, alpha = both[:, :W], both[:, W:W + 1]
        else:
            alpha = self.alpha_linear(h)
            feature = self.feature_linear(h)
        h = torch.cat([feature, x_dir], -1)
        for layer in self.views_linears:
            h = lin(h, layer.weight, layer.bias, True)
        return torch.cat([lin(h, self.rgb_linear.weight, self.rgb_linear.bias), alpha], -1)

    def batchify_run_mlp(self, x):
        # netchunk only bounds the reference's activation memory; on the device the whole batch goes through in one piece
        # (same rows, same maths; 288 GB of HBM, and the GEMM tiles fill the chip better)
        if self.chunk is None or x.is_cuda:
            return self.run_mlp(x)
        return torch.cat([self.run_mlp(x[i:i + self.chunk]) for i in range(0, x.shape[0], self.chunk)], 0)

    def forward(self, data):
        data = self.embedder(data)
        out = self.batchify_run_mlp(data['embedded'])
        data['raw'] = out.reshape(list(data['unflatten_shape']) + [out.shape[-1]])
        del data['unflatten_shape']
        return data


class _NerfMlpFn(torch.autograd.Function):
    """NerfMLP.run_mlp on the device (nerf_mlp.py:62-94) as one autograd node over the shared trunk / view-head graph (mlp_graph.py, which
    explains the buffer layouts).  Here: the trunk cut into runs that end at a skip layer, each writing into the [x_pts | h] buffer the
    next run reads, and the parameter layout (D trunk layers, then views, feature, alpha, rgb).
    x: the embedded batch [M, input_ch + input_ch_dirs], rows 16-byte aligned (ops.mip_encode pads its rows for this; otherwise one copy)."""

    @staticmethod
    def forward(ctx, x, skips, ic, idr, *params):
        from . import mlp_graph as G, ops
        D = (len(params) - 8) // 2
        ps = [p.detach() for p in params]
        xr, _ = ops._rows(x.detach())
        M, W, Kx = xr.shape[0], ps[0].shape[0], G.ceil4(ic)
        if xr.shape[1] < Kx or xr.shape[1] < ic + idr:
            raise ops._lib.XrError('NerfMLP: the embedding has %d columns, expected %d' % (xr.shape[1], ic + idr))
        x_pts, x_dir = xr[:, :Kx], xr[:, ic:ic + idr]
        # the trunk in runs [lo, hi) that end behind a skip layer; a run's first layer reads x_pts (zero weight columns under its padding)
        ends = sorted({i + 1 for i in skips if 0 <= i < D - 1} | {D})
        runs = list(zip([0] + ends[:-1], ends))
        trunks, h = [], x_pts
        for lo, hi in runs:
            cat = None                           # the next run's [x_pts | h] buffer
            if hi < D:
                cat = torch.empty((M, Kx + W), dtype=torch.float32, device=xr.device)
                cat[:, :Kx].copy_(x_pts)
            state, y = G.trunk_forward(h, list(zip(ps[2 * lo:2 * hi:2], ps[2 * lo + 1:2 * hi:2])), ic, out=None if cat is None else cat[:, Kx:])
            trunks.append(state)
            h = y if cat is None else cat
        raw = torch.empty((M, 4), dtype=torch.float32, device=xr.device)
        ctx.head = G.view_head_forward(h, x_dir, ps[2 * D:], raw)
        ctx.cfg = (ic, Kx, runs)
        ctx.trunks, ctx.h_last = trunks, h
        return raw

    @staticmethod
    def backward(ctx, d_raw):
        from . import mlp_graph as G, ops
        if ctx.needs_input_grad[0]:
            raise ops._lib.XrError('_NerfMlpFn has no gradient with respect to its input: NerfMLP.run_mlp takes the per-layer graph for '
                                   'an input that requires one')
        ic, Kx, runs = ctx.cfg
        head_grads, dh = G.view_head_backward(d_raw.contiguous(), ctx.head, ctx.h_last)
        grads = [None] * (2 * runs[-1][1])
        for (lo, hi), state in zip(reversed(runs), reversed(ctx.trunks)):
            grads[2 * lo:2 * hi], dh_in = G.trunk_backward(dh, state, ic, first=lo == 0)
            if lo > 0:
                dh = dh_in[:, Kx:]                             # the skip layer's output is that column range of [x_pts | h]
        ctx.trunks = ctx.h_last = ctx.head = None
        return (None, None, None, None) + tuple(grads) + tuple(head_grads)


# ------------------------------------------------------------------ classic volume rendering
@RENDERS.register_module()
class NerfRender(nn.Module):
    def __init__(self, white_bkgd=False, raw_noise_std=0, rgb_padding=0, density_bias=0, density_activation='relu',
                 **kwarg):
        super().__init__()
        self.white_bkgd, self.raw_noise_std = white_bkgd, raw_noise_std
        self.rgb_padding, self.density_bias = rgb_padding, density_bias
        if density_activation == 'softplus':
            self.density_activation = F.softplus
        elif density_activation == 'relu':
            self.density_activation = F.relu
        else:
            raise NotImplementedError

    @staticmethod
    def get_weights(density_delta):
        """w_k = alpha_k * prod_{j<k} (1 - alpha_j + 1e-10)"""
        alpha = 1 - torch.exp(-density_delta)
        ones = torch.ones((alpha.shape[0], 1), device=alpha.device, dtype=alpha.dtype)
        trans = torch.cumprod(torch.cat([ones, 1. - alpha + 1e-10], -1), -1)[:, :-1]
        return alpha * trans

    @staticmethod
    def get_disp_map(weights, z_vals):
        depth = torch.sum(weights * z_vals, -1)
        return 1. / torch.max(1e-10 * torch.ones_like(depth), depth / torch.sum(weights, -1))

    def forward(self, data, is_test=False):
        raw, z_vals, rays_d = data['raw'], data['z_vals'], data['rays_d']
        noise_std = 0 if is_test else self.raw_noise_std
        from . import ops
        if (torch.is_grad_enabled() and raw.requires_grad and ops._on_device(raw) and raw.dtype == torch.float32
                and self.density_activation is F.relu and self.rgb_padding == 0 and self.density_bias == 0
                and raw.dim() == 3 and raw.shape[-1] == 4 and raw.shape[0] > 0 and 1 <= raw.shape[1] <= 4096
                and tuple(z_vals.shape) == tuple(raw.shape[:2]) and tuple(rays_d.shape) == (raw.shape[0], 3)
                and not z_vals.requires_grad and not rays_d.requires_grad and ops.vanilla_kernels_available()):
            # training on the device: one launch forward, one backward (renders.RayRender); gradients flow from the colours
            noise = torch.randn(raw.shape[:2], device=raw.device) * noise_std if noise_std > 0. else None
            rgb_map, disp, acc, weights = RayRender.apply(ops.nerf_render_train_forward, ops.nerf_render_backward, raw, z_vals, rays_d,
                                                          noise, bool(self.white_bkgd))
            data['weights'] = weights
            return data, {'rgb': rgb_map, 'disp': disp, 'acc': acc}
        if (raw.is_cuda and not (torch.is_grad_enabled() and raw.requires_grad) and noise_std == 0
                and self.density_activation is F.relu and self.rgb_padding == 0 and self.density_bias == 0
                and raw.dim() == 3 and raw.shape[-1] == 4 and tuple(z_vals.shape) == tuple(raw.shape[:2])):
            # inference on the device: one launch (xr_nerf_render_forward) instead of ~25 tensor ops
            rgb_map, disp, acc, weights = ops.nerf_render_forward(raw, z_vals, rays_d, self.white_bkgd)
            data['weights'] = weights
            return data, {'rgb': rgb_map, 'disp': disp, 'acc': acc}
        dists = z_vals[..., 1:] - z_vals[..., :-1]
        if dists.shape[1] != raw.shape[1]:          # z_vals are sample positions, not interval edges
            far = torch.full_like(dists[..., :1], 1e10)
            dists = torch.cat([dists, far], -1)
        dists = dists * torch.norm(rays_d[..., None, :], dim=-1)
        rgb = torch.sigmoid(raw[..., :3]) * (1 + 2 * self.rgb_padding) - self.rgb_padding
        noise = torch.randn(raw[..., 3].shape, device=raw.device) * noise_std if noise_std > 0. else 0.
        weights = self.get_weights(self.density_activation(raw[..., 3] + noise + self.density_bias) * dists)
        rgb_map = torch.sum(weights[..., None] * rgb, -2)
        acc_map = torch.sum(weights, -1)
        ret = {'rgb': rgb_map + (1. - acc_map[..., None]) if self.white_bkgd else rgb_map,
               'disp': self.get_disp_map(weights, z_vals), 'acc': acc_map}
        data['weights'] = weights
        return data, ret


# ------------------------------------------------------------------ sampling along rays
def get_z_vals(rays_o, near, far, n_samples=64, lindisp=False, randomized=False):
    """GetZvals (datasets/pipelines/create.py:486-531)"""
    t = torch.linspace(0., 1., steps=n_samples, device=rays_o.device)
    z = near * (1. - t) + far * t if not lindisp else 1. / (1. / near * (1. - t) + 1. / far * t)
    if randomized:
        return perturb_z_vals(z.expand(list(rays_o.shape[:-1]) + [n_samples]))
    return z.expand(list(rays_o.shape[:-1]) + [n_samples])


def perturb_z_vals(z_vals, t_rand=None):
    """PerturbZvals (datasets/pipelines/augment.py:261-283): one uniform draw inside each sample's bin"""
    mids = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
    upper = torch.cat([mids, z_vals[..., -1:]], -1)
    lower = torch.cat([z_vals[..., :1], mids], -1)
    if t_rand is None:
        t_rand = torch.rand(z_vals.shape, device=z_vals.device)
    return lower + (upper - lower) * t_rand


def get_pts(rays_o, rays_d, z_vals):
    """GetPts (create.py:577-601)"""
    return rays_o[..., None, :] + rays_d[..., None, :] * z_vals[..., :, None]


def sample_pdf(data, N_samples, is_perturb=False, is_test=False, u=None):
    """hierarchical re-sampling from the coarse weights (networks/utils/hierarchical_sample.py:6-53)"""
    z_vals, rays_o, rays_d = data['z_vals'], data['rays_o'], data['rays_d']
    det = True if is_test else (not is_perturb)
    from . import ops
    if (ops._on_device(z_vals) and z_vals.dtype == torch.float32 and z_vals.dim() == 2 and z_vals.shape[0] > 0 and 3 <= z_vals.shape[1] <= 1024
            and 1 <= N_samples <= 1024 and data['weights'].shape == z_vals.shape and tuple(rays_o.shape) == (z_vals.shape[0], 3)
            and rays_d.shape == rays_o.shape and ops.vanilla_kernels_available()):
        # device: inversion, merge, sort and the new points in one launch; the draws are made on the device (no host draw, no copy)
        if u is None and not det:
            u = torch.rand((z_vals.shape[0], N_samples), device=z_vals.device)
        elif u is not None:
            u = u.to(z_vals.device).expand(z_vals.shape[0], N_samples)
        data['z_vals'], data['pts'] = ops.nerf_sample_pdf(z_vals, data['weights'], rays_o, rays_d, N_samples, u)
        return data
    weights = data['weights'][..., 1:-1] + 1e-5
    bins = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
    pdf = weights / torch.sum(weights, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    if u is None:
        if det:
            u = torch.linspace(0., 1., steps=N_samples).expand(list(cdf.shape[:-1]) + [N_samples])
        else:
            u = torch.rand(list(cdf.shape[:-1]) + [N_samples])
    u = u.to(cdf.device).contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below = torch.clamp(inds - 1, min=0)
    above = torch.clamp(inds, max=cdf.shape[-1] - 1)
    cdf_lo, cdf_hi = torch.gather(cdf, -1, below), torch.gather(cdf, -1, above)
    bin_lo, bin_hi = torch.gather(bins, -1, below), torch.gather(bins, -1, above)
    denom = cdf_hi - cdf_lo
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    z_samples = (bin_lo + (u - cdf_lo) / denom * (bin_hi - bin_lo)).detach()
    z_all, _ = torch.sort(torch.cat([z_vals, z_samples], -1), -1)
    data['pts'], data['z_vals'] = get_pts(rays_o, rays_d, z_all), z_all
    return data


def merge_ret(ret, fine_ret):
    for k in ('rgb', 'disp', 'acc'):
        ret['coarse_' + k] = ret[k]
        ret[k] = fine_ret[k]
    return ret


# ------------------------------------------------------------------ coarse + fine network
@NETWORKS.register_module()
class NerfNetwork(BaseNerfNetwork):
    def __init__(self, cfg, mlp=None, mlp_fine=None, render=None):
        super().__init__()
        cfg = builder.ConfigDict.wrap(dict(cfg))
        self.phase = cfg.get('phase', 'train')
        if 'chunk' in cfg: self.chunk = cfg.chunk
        if 'bs_data' in cfg: self.bs_data = cfg.bs_data
        if 'is_perturb' in cfg: self.is_perturb = cfg.is_perturb
        if 'N_importance' in cfg: self.N_importance = cfg.N_importance
        if mlp is not None: self.mlp = builder.build_mlp(mlp)
        if mlp_fine is not None: self.mlp_fine = builder.build_mlp(mlp_fine)
        if render is not None: self.render = builder.build_render(render)

    def forward(self, data, is_test=False):
        data, ret = self.render(self.mlp(data), is_test)
        if self.N_importance > 0:
            data = sample_pdf(data, self.N_importance, self.is_perturb, is_test)
            _, fine_ret = self.render(self.mlp_fine(data), is_test)
            ret = merge_ret(ret, fine_ret)
        return ret

    def batchify_forward(self, data, is_test=False):
        N = data[self.bs_data].shape[0]
        all_ret = {}
        for i in range(0, N, self.chunk):
            chunk = {k: (v[i:i + self.chunk] if v.shape[0] == N else v) for k, v in data.items()}
            for k, v in self.forward(chunk, is_test).items():
                all_ret.setdefault(k, []).append(v)
        return {k: torch.cat(v, 0) for k, v in all_ret.items()}

    def train_step(self, data, optimizer, **kwargs):
        for k in data:
            data[k] = unfold_batching(data[k])
        ret = self.forward(data, is_test=False)
        loss = img2mse(ret['rgb'], data['target_s'])
        psnr = mse2psnr(loss)
        if 'coarse_rgb' in ret:
            loss = loss + img2mse(ret['coarse_rgb'], data['target_s'])
        return {'loss': loss, 'log_vars': {'loss': loss.item(), 'psnr': psnr.item()}, 'num_samples': ret['rgb'].shape[0]}

    def val_step(self, data, optimizer=None, **kwargs):
        """networks/nerf.py:93-142: render the validation poses (timed per frame, pipeline included) and the spiral
        poses through `val_pipeline` (set by the validation hook) in `chunk`-sized pieces; rank 0 only"""
        import time
        from .networks import get_dist_info, recover_shape, unfold_batching
        if self.phase == 'test':
            return self.test_step(data, **kwargs)
        rank, _ = get_dist_info()
        if rank != 0:
            return {}
        for k in data:
            data[k] = unfold_batching(data[k])
        poses, images, spiral_poses = data['poses'], data['images'], data['spiral_poses']
        rgbs, disps, gt_imgs, elapsed = [], [], [], []
        with torch.no_grad():
            for i in range(poses.shape[0]):
                start = time.time()
                frame = self.val_pipeline({'pose': poses[i]})
                ret = self.batchify_forward(frame, is_test=True)
                rgb = recover_shape(ret['rgb'], frame['src_shape']).cpu().numpy()     # the read-back ends the frame
                elapsed.append(time.time() - start)
                rgbs.append(rgb)
                disps.append(recover_shape(ret['disp'], frame['src_shape']).cpu().numpy())
                gt_imgs.append(images[i].cpu().numpy())
            spiral_rgbs, spiral_disps = [], []
            for i in range(spiral_poses.shape[0]):
                frame = self.val_pipeline({'pose': spiral_poses[i]})
                ret = self.batchify_forward(frame, is_test=True)
                spiral_rgbs.append(recover_shape(ret['rgb'], frame['src_shape']).cpu().numpy())
                spiral_disps.append(recover_shape(ret['disp'], frame['src_shape']).cpu().numpy())
        return {'spiral_rgbs': spiral_rgbs, 'spiral_disps': spiral_disps, 'rgbs': rgbs, 'disps': disps, 'gt_imgs': gt_imgs,
                'elapsed_time': elapsed}

    def test_step(self, data, **kwargs):
        """networks/nerf.py:144-168 (the runner only knows train_step / val_step: val_step + phase == 'test')"""
        from .networks import get_dist_info, recover_shape, unfold_batching
        rank, _ = get_dist_info()
        if rank != 0:
            return {}
        for k in data:
            data[k] = unfold_batching(data[k])
        image, idx = data['image'], data['idx'].item()
        with torch.no_grad():
            frame = self.val_pipeline({'pose': data['pose']})
            ret = self.batchify_forward(frame, is_test=True)
        rgb = recover_shape(ret['rgb'], frame['src_shape']).cpu().numpy()
        return {'rgb': rgb, 'gt_img': image.cpu().numpy(), 'idx': idx}

    def set_val_pipeline(self, func):
        self.val_pipeline = func
