"""Float64 restatements of GNR's renderer stages for shapes the fixture does not hold (tests/golden/ref_gnr_render.npz): written from
the reference's lines (gnr_render.py:189-526, networks/utils/gnr.py:286-349), independently of xrnerf_amd/gnr_render.py, and themselves
held to the fixture by tests/test_gnr_render_host.py.  Every function takes the dtype of its inputs, so the float32 run of the same
lines gives the `ref32` of a bar."""
import numpy as np
import torch
import torch.nn.functional as F


def project(pts, calibs, persps, width, height):
    """pts [N,3] -> (xy [V,2,N] normalised, z [V,N])"""
    p = torch.einsum('vjk,nk->vjn', calibs[:, :3, :3], pts) + calibs[:, :3, 3:4]
    z = p[:, 2]
    u, v = p[:, 0] / z.clamp(min=1e-9), p[:, 1] / z.clamp(min=1e-9)
    cam = persps[:, :, None]
    if persps.shape[1] > 6:
        r2 = u * u + v * v
        c = 1 + r2 * (cam[:, 4] + r2 * (cam[:, 5] + r2 * cam[:, 8]))
        u, v = (c * u + cam[:, 6] * 2 * u * v + cam[:, 7] * (r2 + 2 * u * u),
                c * v + cam[:, 7] * 2 * u * v + cam[:, 6] * (r2 + 2 * v * v))
    px, py = cam[:, 0] * u + cam[:, 2], cam[:, 1] * v + cam[:, 3]
    return torch.stack([px / width * 2 - 1, py / height * 2 - 1], 1), z


def nearest(maps, xy):
    """maps [V,H,W], xy [V,2,N] -> [V,N]: grid_sample's nearest mode (align_corners=False, zeros), written out"""
    V, H, W = maps.shape
    x, y = torch.round(((xy[:, 0] + 1) * W - 1) / 2), torch.round(((xy[:, 1] + 1) * H - 1) / 2)
    ok = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
    val = maps[torch.arange(V)[:, None], torch.nan_to_num(y).clamp(0, H - 1).long(), torch.nan_to_num(x).clamp(0, W - 1).long()]
    return torch.where(ok, val, torch.zeros_like(val))


def decision_distance(xy, maps, positive):
    """[V,N]: distance in pixels of the source index from the nearest rounding boundary across which the sampled value (its sign test,
    with `positive`) changes; 1e9 where no neighbouring pixel differs (make_golden_gnr_render.decision_distance)"""
    V, H, W = maps.shape
    x, y = ((xy[:, 0] + 1) * W - 1) / 2, ((xy[:, 1] + 1) * H - 1) / 2
    ix, iy = torch.round(x), torch.round(y)
    dx, dy = 0.5 - (x - ix).abs(), 0.5 - (y - iy).abs()
    sx, sy = torch.where(x >= ix, 1.0, -1.0), torch.where(y >= iy, 1.0, -1.0)

    def value(px, py):
        ok = (px >= 0) & (px < W) & (py >= 0) & (py < H)
        v = maps[torch.arange(V)[:, None], py.clamp(0, H - 1).long(), px.clamp(0, W - 1).long()]
        v = torch.where(ok, v, torch.zeros_like(v))
        return (v > 0) if positive else v
    here = value(ix, iy)
    out = torch.full_like(x, 1e9)
    for px, py, dist in ((ix + sx, iy, dx), (ix, iy + sy, dy), (ix + sx, iy + sy, torch.maximum(dx, dy))):
        out = torch.where(value(px, py) != here, torch.minimum(out, dist), out)
    return out


def hull(rays, t_vals, calibs, persps, masks, width, height, depth=None, rot=None):
    """-> dict: inside [R S] bool, boundary [R S], pts / xy / z / vis / vis_margin / attdirs of the survivors (ascending flat index)"""
    R, S = t_vals.shape
    V = calibs.shape[0]
    pts = (rays[:, None, 3:6] * t_vals[..., None] + (1 - t_vals[..., None]) * rays[:, None, 0:3]).reshape(-1, 3)
    xy, z = project(pts, calibs, persps, width, height)
    m = masks.reshape(V, masks.shape[-2], masks.shape[-1])
    inside = (nearest(m, xy) > 0).all(0) & torch.isfinite(xy).all(1).all(0)
    out = {'inside': inside, 'boundary': decision_distance(torch.nan_to_num(xy), m, True).amin(0), 'pts': pts[inside],
           'xy': xy[:, :, inside].permute(2, 0, 1), 'z': z[:, inside].permute(1, 0)}
    if depth is not None:
        dm = depth.reshape(V, depth.shape[-2], depth.shape[-1])
        d = nearest(dm, xy)[:, inside].permute(1, 0)
        out['vis'] = ((out['z'] - d) <= 0) & (d > 0)
        near = decision_distance(torch.nan_to_num(xy), dm, False)[:, inside].permute(1, 0) <= 1e-3
        out['vis_margin'] = torch.where(near, torch.zeros_like(d), (out['z'] - d).abs())
    cam_c = torch.inverse(calibs)[:, :3, 3]
    view = (rays[:, 0:3] - rays[:, 3:6])[:, None, :].expand(-1, S, -1).reshape(-1, 3)[inside]
    dirs = torch.cat([view[:, None], cam_c[None] - out['pts'][:, None]], 1)
    if rot is not None:
        dirs = dirs @ rot
    out['attdirs'] = dirs / dirs.norm(dim=-1, keepdim=True).clamp(min=1e-9)
    return out


def gather(xy, feats, images):
    """xy [M,V,2], feats [V,C,h,w], images [V,3,H,W] -> [M,V,C+3] through F.grid_sample (bilinear, align_corners=False, zeros)"""
    g = xy.permute(1, 0, 2)[:, :, None, :]
    a = F.grid_sample(feats, g, mode='bilinear', padding_mode='zeros', align_corners=False)[..., 0]
    b = F.grid_sample(images, g, mode='bilinear', padding_mode='zeros', align_corners=False)[..., 0]
    return torch.cat([a, b], 1).permute(2, 0, 1)


def composite_dense(net, source_rgb, inside, t_vals, noise=None, z_near_far=None, white=False):
    """the dense formulation: net [M, 4 + V + 1] and source_rgb [M,V,3] scattered to [R, S] with -1e4 in channels 0 .. 3 outside
    the hull -> (rgb_map [R,6], depth [R], acc [R], weights [R,S]); differentiable in net"""
    R, S = t_vals.shape
    V = source_rgb.shape[1]
    where = torch.nonzero(inside.reshape(-1)).reshape(-1)
    base = torch.zeros((R * S, 4 + V + 1), dtype=net.dtype)
    base[:, :4] = -1e4
    full = base.index_put((where,), net[:, :4 + V + 1]).view(R, S, -1)
    src = torch.zeros((R * S, V, 3), dtype=net.dtype).index_put((where,), source_rgb).view(R, S, V, 3)
    rgb = torch.sigmoid(full[..., :3])
    raw = full[..., 3] + (noise if noise is not None else 0)
    alpha = 1 - torch.exp(-torch.relu(raw))
    keep = 1 - alpha + 1e-10
    trans = torch.cat([torch.ones((R, 1), dtype=net.dtype), torch.cumprod(keep, -1)[:, :-1]], -1)
    weights = alpha * trans
    blend = (torch.cat([rgb[:, :, None], src], 2) * full[..., 4:, None]).sum(2)
    rgb_map = torch.cat([(weights[..., None] * rgb).sum(1), (weights[..., None] * blend).sum(1)], -1)
    acc = weights.sum(-1)
    if white:
        rgb_map = rgb_map + (1 - acc[:, None])
    z = t_vals * z_near_far[0] + (1 - t_vals) * z_near_far[1] if z_near_far is not None else 2 * t_vals - 1
    return rgb_map, (weights * z).sum(-1), acc, weights


def loss(rgb_map, rgb_gt):
    """cal_loss with attention and nothing else switched on"""
    return ((rgb_map[:, :3] - rgb_gt) ** 2).mean() + ((rgb_map[:, 3:6] - rgb_gt) ** 2).mean()


# ---------------------------------------------------------------- GNRMLP (mlps/gnr_mlp.py), the options of configs/gnr/gnr_genebody.py
def pose_embed(x, num_freqs=10, spatial_freq=1 / 256):
    bands = torch.linspace(spatial_freq * 0.1 * np.pi * 2, spatial_freq * 10 * np.pi * 2, steps=num_freqs).to(x.dtype)   # (float32 bands, as stored)
    return torch.cat([x] + [f(x * b) for b in bands for f in (torch.sin, torch.cos)], -1)


def sh9(d):
    """rank-3 harmonics with the reference's slot quirks written out: [c0, c1 y, c1 z, -c1 x, ...]"""
    x, y, z = d[..., 0:1], d[..., 1:2], d[..., 2:3]
    c0, c1, c2 = np.sqrt(1 / np.pi / 4), np.sqrt(3 / np.pi / 4), np.sqrt(5 / np.pi / 4)
    p3 = -((x * x + y * y) * 3 + 2 * z * (-3 * z)) / 6
    a = -c2 * np.sqrt(2) / np.sqrt(6)
    b = -a / 2
    return torch.cat([c0 * torch.ones_like(z), c1 * y, c1 * z, -c1 * x, b * 3 * (y * x + x * y), a * (-3 * z) * y, c2 * p3, a * (-1) * x,
                      b * z * (x * x - y * y)], -1)


def gnr_mlp(sd, x, attdirs, smpl_vis=None, alpha_only=False, skips=(2, 4, 6), D=8):
    """sd: state_dict (tensors of x's dtype); x [M, V, 3 + 7 + C + 3]; attdirs [M, V + 1, 3] -> [M, 4 + (V + 1) + V] (or alpha [M, 1])"""
    lin = lambda h, name: F.linear(h, sd[name + '.weight'], sd[name + '.bias'])
    M, V = x.shape[0], x.shape[1]
    W = sd['alpha_out_linear.weight'].shape[1]
    pts, smpl, feats = x[..., :3], x[..., 3:10], x[..., 10:]
    upts, usmpl = pts[:, 0], smpl[:, 0]
    fp, fs, ff = pts.reshape(M * V, 3), smpl.reshape(M * V, 7), feats.reshape(M * V, -1)
    qry, src = attdirs[:, :1], attdirs[:, 1:]
    d = src.reshape(-1, 3)
    mom = torch.cross(fp, d, dim=-1)
    o = torch.relu(lin(torch.cat([fs, d, mom, ff], -1), 'occ_linears.0'))
    o = torch.relu(lin(o, 'occ_linears.1'))
    occ = torch.sigmoid(lin(torch.cat([fs, d, mom, o], -1), 'occ_linears.2')).view(M, V)
    h = torch.cat([pose_embed(fp), fs, ff], -1)
    per_view = None
    for i in range(D):
        h = torch.relu(lin(h, 'alpha_linears.%d' % i))
        if i in skips:
            if i == skips[0]:
                per_view = h
                h = h.view(M, V, W).mean(1)
            h = torch.cat([pose_embed(upts), usmpl, h], -1)
    alpha = lin(h, 'alpha_out_linear')
    if alpha_only:
        return alpha
    wts = torch.exp(sd['s'] * ((src * qry).sum(-1) - 1))
    wts = wts / (wts.sum(-1, keepdim=True) + 1e-8)
    pooled = (per_view.view(M, V, W) * wts[..., None]).sum(1)
    h = torch.relu(lin(torch.cat([pose_embed(upts), usmpl, pooled], -1), 'rgb_linears.0'))
    h = torch.relu(lin(torch.cat([sh9(-qry[:, 0]), h], -1), 'rgb_linears.1'))
    h = lin(torch.relu(lin(h, 'rgb_linears.2')), 'rgb_linears.3')
    dirs = sh9(attdirs.reshape(-1, 3))
    val = torch.cat([pose_embed(torch.cat([upts, fp], 0)), dirs, torch.cat([pooled, per_view], 0)], -1)
    val = torch.cat([dirs, torch.relu(lin(val, 'value_linears.0'))], -1)
    val = torch.cat([dirs, torch.relu(lin(val, 'value_linears.1'))], -1)
    val = lin(val, 'value_linears.2').view(M, V + 1, -1)
    q = sh9(qry[:, 0])
    key = torch.cat([q, torch.relu(lin(torch.cat([pose_embed(upts), q, pooled], -1), 'key_linears.0'))], -1)
    key = torch.cat([q, torch.relu(lin(key, 'key_linears.1'))], -1)
    key = lin(key, 'key_linears.2')
    att = (val * key[:, None]).sum(-1)
    e = torch.exp(att - att.max(1, keepdim=True)[0])
    e = torch.cat([e[:, :1], e[:, 1:] * occ], 1)
    att = e / (e.sum(-1, keepdim=True) + 1e-8)
    return torch.cat([h, alpha, att, occ], -1)
