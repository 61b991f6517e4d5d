"""BungeeNeRF's maths restated in composed torch (any dtype, any device), written from the formulas: the bounds and z-values, cast_rays
+ the embedding, the multi-head renderer, the resampler, the residual MLP (same sub-module names as xrnerf_amd.bungee.BungeeNerfMLP,
so state dicts load both ways) and the training step / stage loop.  In float64 it is the oracle of tests/test_emu_bungee.py and
tests/test_gpu_bungee.py; in float32 it is the composed-torch baseline of tools/microbench_bungee.py and the trajectory test."""
import torch
import torch.nn.functional as F
from torch import nn

EARTH = 6371011.0


def bounds(o, v, mode, origin, s):
    """near, far [R, 1]"""
    if mode == 'sphere':
        c = torch.tensor([x * s for x in origin], dtype=o.dtype, device=o.device)
        oc = o - c
        b = (oc * v).sum(-1)
        vv = (v * v).sum(-1)
        cc = (oc * oc).sum(-1)

        def hit(r):
            t = (-b - torch.sqrt(b * b - vv * (cc - r * r))) / vv
            return (t[:, None] * v).norm(dim=-1, keepdim=True)
        return hit((EARTH + 250) * s) * 0.9, hit(EARTH * s) * 1.1
    near = ((250 * s - o[:, 2] * s) / (v[:, 2] * s)).clamp(min=1e-6)
    far = (-o[:, 2] * s) / (v[:, 2] * s)
    return near[:, None], far[:, None]


def zvals(near, far, N):
    n1 = (2 * N) // 3
    t = torch.linspace(0, 1, N, dtype=near.dtype, device=near.device)
    zd = (1 / (1 / near * (1 - t) + 1 / far * t))[:, :n1]
    t2 = torch.linspace(0, 1, N - n1 + 1, dtype=near.dtype, device=near.device)
    zl = zd[:, -1:] * (1 - t2) + far * t2
    return torch.sort(torch.cat([zd, zl[:, 1:]], -1), -1)[0]


def gaussians(z, o, d, radii, cone=True):
    t0, t1 = z[:, :-1], z[:, 1:]
    r = radii.reshape(-1, 1)
    if cone:
        mu, hw = (t0 + t1) / 2, (t1 - t0) / 2
        den = 3 * mu ** 2 + hw ** 2
        t_mean = mu + 2 * mu * hw ** 2 / den
        t_var = hw ** 2 / 3 - 4 / 15 * hw ** 4 * (12 * mu ** 2 - hw ** 2) / den ** 2
        r_var = r ** 2 * (mu ** 2 / 4 + 5 / 12 * hw ** 2 - 4 / 15 * hw ** 4 / den)
    else:
        t_mean, t_var, r_var = (t0 + t1) / 2, (t1 - t0) ** 2 / 12, (r ** 2 / 4).expand_as(t0)
    d2 = d ** 2
    null = 1 - d2 / d2.sum(-1, keepdim=True).clamp_min(1e-10)
    means = o[:, None] + d[:, None] * t_mean[..., None]
    covs = t_var[..., None] * d2[:, None] + r_var[..., None] * null[:, None]
    return means, covs


def embed(means, covs, viewdirs, L=10, Ld=4):
    m, c = means.reshape(-1, 3), covs.reshape(-1, 3)
    parts = [m]
    for l in range(L):
        e = torch.exp(-0.5 * 4.0 ** l * c)
        parts += [torch.sin(m * 2.0 ** l) * e, torch.cos(m * 2.0 ** l) * e]
    v = viewdirs[:, None].expand(means.shape).reshape(-1, 3)
    dp = [v]
    for l in range(Ld):
        dp += [torch.sin(v * 2.0 ** l), torch.cos(v * 2.0 ** l)]
    return torch.cat(parts + dp, -1)


def render(raw, z, viewdirs, stage, noise=None, density_bias=-1.0, rgb_padding=0.0, white_bkgd=False, act='softplus'):
    """-> rgb, disp, acc, weights (differentiable in raw)"""
    zm = .5 * (z[:, 1:] + z[:, :-1])
    dist = torch.cat([zm[:, 1:] - zm[:, :-1], torch.full_like(zm[:, :1], 1e10)], -1) * viewdirs.norm(dim=-1, keepdim=True)
    a = raw[:, :, :stage + 1].sum(2)
    rgb = (1 + 2 * rgb_padding) / (1 + torch.exp(-a[..., :3])) - rgb_padding
    x = a[..., 3] + (0 if noise is None else noise) + density_bias
    dens = F.softplus(x) if act == 'softplus' else F.relu(x)
    alpha = 1 - torch.exp(-dens * dist)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha + 1e-10], -1), -1)[:, :-1]
    w = alpha * T
    acc = w.sum(-1)
    rgb_map = (w[..., None] * rgb).sum(1)
    if white_bkgd:
        rgb_map = rgb_map + (1 - acc[:, None])
    depth = (w * zm).sum(-1)
    disp = 1 / torch.max(torch.full_like(depth, 1e-10), depth / acc)
    return rgb_map, disp, acc, w


def resample(z, w, padding, rand=None):
    """max-blur, padding, piecewise-constant inverse cdf (the Mip-NeRF resampler)"""
    wp = torch.cat([w[:, :1], w, w[:, -1:]], -1)
    wm = torch.maximum(wp[:, :-1], wp[:, 1:])
    w = 0.5 * (wm[:, :-1] + wm[:, 1:]) + padding
    n = z.shape[1]
    ws = w.sum(-1, keepdim=True)
    pad = torch.clamp(1e-5 - ws, min=0)
    w = w + pad / w.shape[-1]
    ws = ws + pad
    pdf = w / ws
    cdf = torch.cat([torch.zeros_like(pdf[:, :1]), torch.clamp(torch.cumsum(pdf[:, :-1], -1), max=1), torch.ones_like(pdf[:, :1])], -1)
    eps = torch.finfo(torch.float32).eps
    if rand is not None:
        s = 1 / n
        u = torch.arange(n, dtype=z.dtype, device=z.device) * s
        u = torch.clamp(u + rand.to(z.dtype) * (s - eps), max=1 - eps)
    else:
        u = torch.linspace(0, 1 - eps, n, dtype=z.dtype, device=z.device).expand(z.shape[0], n)
    mask = u[..., None, :] >= cdf[..., :, None]
    b0 = torch.where(mask, z[..., :, None], z[..., :1, None]).max(-2)[0]
    b1 = torch.where(~mask, z[..., :, None], z[..., -1:, None]).min(-2)[0]
    c0 = torch.where(mask, cdf[..., :, None], cdf[..., :1, None]).max(-2)[0]
    c1 = torch.where(~mask, cdf[..., :, None], cdf[..., -1:, None]).min(-2)[0]
    t = torch.clamp(torch.nan_to_num((u - c0) / (c1 - c0), 0), 0, 1)
    return (b0 + t * (b1 - b0)).detach()


class _Block(nn.Module):
    def __init__(self, W, ic, idr, n_trunk, first_in):
        super().__init__()
        self.pts_linears = nn.ModuleList([nn.Linear(first_in, W)] + [nn.Linear(W, W) for _ in range(n_trunk - 1)])
        self.views_linear = nn.Linear(idr + W, W // 2)
        self.feature_linear = nn.Linear(W, W)
        self.alpha_linear = nn.Linear(W, 1)
        self.rgb_linear = nn.Linear(W // 2, 3)

    def forward(self, x, views):
        h = x
        for l in self.pts_linears:
            h = F.relu(l(h))
        alpha = self.alpha_linear(h)
        h0 = F.relu(self.views_linear(torch.cat([self.feature_linear(h), views], -1)))
        return self.rgb_linear(h0), alpha, h


class RestatedMLP(nn.Module):
    """the residual MLP as nn.Linear layers (state-dict compatible with BungeeNerfMLP's)"""

    def __init__(self, cur_stage=0, netwidth=256, ic=63, idr=27):
        super().__init__()
        self.ic, self.idr = ic, idr
        self.baseblock = _Block(netwidth, ic, idr, 4, ic)
        self.resblocks = nn.ModuleList([_Block(netwidth, ic, idr, 2, ic + netwidth) for _ in range(cur_stage)])

    def forward(self, x):
        pts, views = x[:, :self.ic], x[:, self.ic:self.ic + self.idr]
        rgb, alpha, h = self.baseblock(pts, views)
        rgbs, alphas = [rgb], [alpha]
        for b in self.resblocks:
            rgb, alpha, h = b(torch.cat([pts, h], -1), views)
            rgbs.append(rgb)
            alphas.append(alpha)
        return torch.cat([torch.stack(rgbs, 1), torch.stack(alphas, 1)], -1)


class RestatedNetwork(nn.Module):
    """coarse + fine pass through one MLP; train_step masked by scale_code <= stage (flat [R, ...] batches)"""

    def __init__(self, cur_stage=0, netwidth=256, resample_padding=0.01, N_importance=65):
        super().__init__()
        self.mlp = RestatedMLP(cur_stage, netwidth)
        self.resample_padding, self.N_importance = resample_padding, N_importance

    def forward(self, b, stage, rand=None, is_test=False):
        z = b['z_vals']
        out = []
        for level in range(2 if self.N_importance > 0 else 1):
            if level == 1:
                z = resample(z, out[-1][3], self.resample_padding, None if is_test else rand)
            means, covs = gaussians(z, b['rays_o'], b['rays_d'], b['radii'])
            raw = self.mlp(embed(means, covs, b['viewdirs'])).reshape(z.shape[0], z.shape[1] - 1, -1, 4)
            out.append(render(raw, z, b['viewdirs'], stage))
        return out

    def train_step(self, b, stage, rand=None):
        out = self.forward(b, stage, rand)
        m = b['scale_code'] <= stage
        loss = sum(torch.mean((o[0] * m - b['target_s'] * m) ** 2) for o in out)
        return loss


def train_iteration(net, b, opt, rands=None):
    losses = []
    for stage in range(int(torch.max(b['scale_code'])) + 1):
        loss = net.train_step(b, stage, None if rands is None else rands[stage])
        losses.append(loss.item())
        if losses[-1] == 0.:
            continue
        opt.zero_grad()
        loss.backward()
        opt.step()
    return losses
