"""The stages of GNR's renderer around the network (configs/gnr/gnr_genebody.py; the reference's GnrRenderer.render_rays,
gnr_render.py:359-526), on the kernels of csrc/xr_gnr_render.hip:

    visual_hull    inside_pts_vh and the sample points of render_rays: which points every source mask sees, compacted in the order of
                   torch.nonzero, with per survivor the point, its flat index, per view the normalised image coordinates, the depth and
                   smpl_vis, and make_att_input's directions -- so nothing is projected a second time
    pixel_gather   the `feats is not None` half of make_nerf_input: bilinear samples of channel-last feature maps and of the images,
                   written at a row stride into the buffer the network's first layer reads
    composite      make_nerf_output and the lines around it, per ray over the ray's survivors only (exact: outside the hull the
                   reference's -1e4 gives alpha = 0 and a transmittance factor of exactly 1.0f); differentiable in the network output
    synthetic_scene  a small generated scene (body, ring of source cameras, masks, depth maps, maps, rays): the fixture's inputs

    GNRMLP, GnrRenderer   the reference's classes on these stages, registered with the builder; reconstruct / octree_reconstruct run on
                   gnr_recon.py's stages

Device tensors run the kernels; host tensors take the tensor-op path -- the reference's lines restated, which is also the timing
baseline of tools/microbench_gnr_render.py."""
import numpy as np
import torch
import torch.nn.functional as F

from . import ops


TENSOR_OPS_STAGES = False        # measurements only: the three stages take their tensor-op path on device tensors too


def _use_kernels(t):
    """device tensors run the kernels; a library handle without the entry points is an error, not a quiet tensor-op run"""
    if not ops._on_device(t) or TENSOR_OPS_STAGES:
        return False
    if not ops.gnr_render_kernels_available():
        from . import _lib
        raise _lib.XrError('the loaded library has no xr_gnr_render entry points (stale build?)')
    return True


# ---------------------------------------------------------------- the reference's lines (host path, timing baseline)
def perspective(points, w2c, camera):
    """networks/utils/gnr.py:324-349: points [V,3,N], w2c [V,4,4], camera [V,cols] -> [V,3,N] (pixel x, pixel y, camera depth)"""
    rot, trans = w2c[:, :3, :3], w2c[:, :3, 3:4]
    points = torch.baddbmm(trans, rot, points)
    xy = points[:, :2, :] / torch.clamp(points[:, 2:3, :], 1e-9)
    if camera.shape[1] > 6:
        x2 = xy[:, 0, :] * xy[:, 0, :]
        y2 = xy[:, 1, :] * xy[:, 1, :]
        xy_ = xy[:, 0, :] * xy[:, 1, :]
        r2 = x2 + y2
        c = (1 + r2 * (camera[:, 4:5] + r2 * (camera[:, 5:6] + r2 * camera[:, 8:9])))
        xy = c.unsqueeze(1) * xy + torch.cat([(camera[:, 6:7] * 2 * xy_ + camera[:, 7:8] * (r2 + 2 * x2)).unsqueeze(1),
                                              (camera[:, 7:8] * 2 * xy_ + camera[:, 6:7] * (r2 + 2 * y2)).unsqueeze(1)], 1)
    xy = camera[:, 0:2, None] * xy + camera[:, 2:4, None]
    return torch.cat([xy, points[:, 2:3, :]], 1)


def index(feat, uv, mode='bilinear'):
    """networks/utils/gnr.py:286-302: feat [V,C,H,W] (or [V,H,W]), uv [V,2,N] -> [V,C,N]"""
    if feat.dim() == 3:
        feat = feat.unsqueeze(1)
    return F.grid_sample(feat, uv.transpose(1, 2).unsqueeze(2), mode=mode, align_corners=False)[:, :, :, 0]


def sample_points(rays, t_vals):
    rays_s, rays_e = rays[:, 0:3], rays[:, 3:6]
    return (rays_e[:, None, :] * t_vals[..., None] + (1 - t_vals[..., None]) * rays_s[:, None, :]).reshape(-1, 3)


def att_directions(pts, viewdirs, calibs, rot):
    """make_att_input, perspective branch -> [M, V+1, 3]"""
    cam_c = torch.inverse(calibs)[:, :3, 3]
    V = calibs.shape[0]
    attdirs = cam_c[None, :, :].expand(pts.shape[0], -1, -1) - pts[:, None, :].expand(-1, V, -1)
    if rot is not None:
        viewdirs = viewdirs @ rot
        attdirs = (attdirs.reshape(-1, 3) @ rot).view(attdirs.shape)
    attdirs = torch.cat([viewdirs[:, None, :], attdirs], dim=1)
    return attdirs / torch.clamp(torch.norm(attdirs, dim=-1, keepdim=True), min=1e-9)


def hull_tensor_ops(rays, t_vals, calibs, persps, masks, width, height, depth=None, rot=None, attention=True):
    """inside_pts_vh and the lines of render_rays around it as tensor ops -> the dict of visual_hull().  One deviation, shared with
    the kernel: a point with a non-finite projected coordinate is outside."""
    R, S = t_vals.shape
    V = calibs.shape[0]
    pts = sample_points(rays, t_vals)
    xyz = perspective(pts.permute(1, 0)[None].expand(V, -1, -1), calibs, persps)
    xy = xyz[:, :2, :] / torch.tensor([[[width], [height]]], dtype=xyz.dtype, device=xyz.device) * 2 - 1
    finite = torch.isfinite(xy).all(1).all(0)
    m = masks.reshape(V, 1, masks.shape[-2], masks.shape[-1])
    inside = (index(m, torch.nan_to_num(xy), 'nearest').squeeze(1) > 0).all(0) & finite
    idx = torch.nonzero(inside).reshape(-1)
    count = inside.view(R, S).sum(1)
    table = torch.stack([count, torch.cumsum(count, 0) - count], 1).to(torch.int32)
    out = {'M': int(idx.numel()), 'table': table, 'idx': idx.to(torch.int32), 'pts': pts[idx],
           'xy': xy[:, :, idx].permute(2, 0, 1).contiguous(), 'z': xyz[:, 2, idx].permute(1, 0).contiguous(), 'vis': None, 'attdirs': None}
    if depth is not None:
        d = index(depth.reshape(V, 1, depth.shape[-2], depth.shape[-1]), torch.nan_to_num(xy), 'nearest').squeeze(1).permute(1, 0)[idx]
        out['vis'] = ((out['z'] - d) <= 0) & (d > 0)
    if attention:
        viewdirs = (rays[:, 0:3] - rays[:, 3:6])[:, None, :].expand(-1, S, -1).reshape(-1, 3)[idx]
        out['attdirs'] = att_directions(out['pts'], viewdirs, calibs, rot)
    return out


def gather_tensor_ops(xy, feats, images):
    """the reference's two index() calls, permute and cat: xy [M,V,2], feats [V,C,h,w], images [V,3,H,W] ->
    (latent [M,V,C+3], source_rgb [M,V,3])"""
    uv = xy.permute(1, 2, 0)
    latent = index(feats, uv).permute(2, 0, 1)
    source_rgb = index(images, uv).permute(2, 0, 1)
    return torch.cat([latent, source_rgb], -1), source_rgb


def composite_tensor_ops(net, source_rgb, idx, R, S, t_vals, noise=None, z_near_far=None, white=False):
    """render_rays:447-481 and make_nerf_output as the reference's dense tensor ops: the compact network output is scattered to
    [R S] with -1e4 in the first four channels outside the hull -> (rgb_map [R,6], depth [R], acc [R], weights [R,S])"""
    V = source_rgb.shape[1]
    idx = idx.long()
    full = net.new_zeros((R * S, 4 + V + 1))
    full[:, :4] = -1e4
    full = full.index_copy(0, idx, net[:, :4 + V + 1])
    src = source_rgb.new_zeros((R * S, V, 3)).index_copy(0, idx, source_rgb)
    full = full.view(R, S, -1)
    rgb = torch.sigmoid(full[..., :3])
    alpha = 1. - torch.exp(-F.relu(full[..., 3] + (noise if noise is not None else 0)))
    weights = alpha * torch.cumprod(torch.cat([torch.ones((R, 1), dtype=net.dtype, device=net.device), 1. - alpha + 1e-10], -1), -1)[:, :-1]
    rgb_map = torch.sum(weights[..., None] * rgb, -2)
    att = full[..., 4:]
    blend = torch.sum(torch.cat([rgb.unsqueeze(-2), src.view(R, S, V, 3)], dim=-2) * att[..., None], dim=-2)
    rgb_map = torch.cat([rgb_map, torch.sum(weights[..., None] * blend, -2)], -1)
    acc = torch.sum(weights, -1)
    if white:
        rgb_map = rgb_map + (1. - acc[..., None])
    z_vals = t_vals * z_near_far[0] + (1 - t_vals) * z_near_far[1] if z_near_far is not None else 2 * t_vals - 1
    return rgb_map, torch.sum(weights * z_vals, -1), acc, weights


# ---------------------------------------------------------------- the stages
def visual_hull(rays, t_vals, calibs, persps, masks, width, height, depth=None, rot=None, attention=True):
    """rays [R,6] (start, end), t_vals [R,S], calibs [V,4,4], persps [V,cols], masks / depth [V,1,H,W] or [V,H,W], rot [3,3] ->
    dict: M, table [R,2] int32 (count, base), idx [M] int32, pts [M,3], xy [M,V,2], z [M,V], vis [M,V] bool / None,
    attdirs [M,V+1,3] / None.  One blocking read (M), where the reference has `len(pts) == 0`."""
    if persps is None:
        raise ValueError('projection: only the perspective projection (persps) is built')
    if not _use_kernels(rays):
        return hull_tensor_ops(rays, t_vals, calibs, persps, masks, width, height, depth, rot, attention)
    cam_c = torch.inverse(calibs)[:, :3, 3].contiguous() if attention else None
    return ops.gnr_hull(rays, t_vals, calibs, persps, masks, width, height, depth, cam_c, rot if attention else None)


def channel_last(feats):
    """[V,C,h,w] -> [V,h,w,C] contiguous: once per frame"""
    return feats.permute(0, 2, 3, 1).contiguous()


class _Gather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats_last, xy, images, out, col0):
        rows, source_rgb = ops.gnr_gather(xy, feats_last, images, out, col0)
        ctx.save_for_backward(xy)
        ctx.col0, ctx.shape = col0, tuple(feats_last.shape)
        ctx.mark_non_differentiable(source_rgb)
        if out is not None:
            ctx.mark_dirty(out)
        return rows, source_rgb

    @staticmethod
    def backward(ctx, d_rows, d_source_rgb):
        xy, = ctx.saved_tensors
        return ops.gnr_gather_backward(xy, d_rows.contiguous(), ctx.col0, ctx.shape), None, None, None, None


def pixel_gather(xy, feats_last, images, out=None, col0=0):
    """xy [M,V,2]; feats_last [V,h,w,C] (channel_last(feats)); images [V,3,H,W] -> (rows [M,V,ld], source_rgb [M,V,3]): columns
    col0 .. col0 + C + 3 of every row are the sampled features and colour, the rest up to ld zeros.  When the feature maps require
    grad (train_encoder) the rows carry their gradient back to them, bit-repeatably; nothing flows to xy (`regularization`) or to the
    images, and source_rgb carries none."""
    if not _use_kernels(xy):
        latent, source_rgb = gather_tensor_ops(xy, feats_last.permute(0, 3, 1, 2), images)
        if latent.requires_grad:                                   # the kernel's rule: a NaN or infinite upstream entry contributes nothing
            latent.register_hook(lambda g: torch.where(torch.isfinite(g), g, torch.zeros_like(g)))
        M, V, n = latent.shape
        ld = out.shape[2] if out is not None else (col0 + n + 3) // 4 * 4
        rows = torch.cat([out[:, :, :col0] if out is not None else latent.new_zeros((M, V, col0)), latent, latent.new_zeros((M, V, ld - col0 - n))], -1)
        if out is not None and not rows.requires_grad:
            out.copy_(rows)
            rows = out
        return rows, source_rgb.detach().contiguous()
    if feats_last.requires_grad:
        return _Gather.apply(feats_last, xy, images, out, col0)
    return ops.gnr_gather(xy, feats_last, images, out, col0)


class _Composite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, source_rgb, idx, table, t_vals, noise, z_near_far, white):
        rgb_map, depth, acc, weights, trans = ops.gnr_composite_forward(net, source_rgb, idx, table, t_vals, noise, z_near_far, white)
        ctx.save_for_backward(net, source_rgb, idx, table, t_vals, noise, trans)
        ctx.white = white
        ctx.mark_non_differentiable(depth, acc, weights)
        return rgb_map, depth, acc, weights

    @staticmethod
    def backward(ctx, d_rgb_map, d_depth, d_acc, d_weights):
        net, source_rgb, idx, table, t_vals, noise, trans = ctx.saved_tensors
        d = ops.gnr_composite_backward(net, source_rgb, idx, table, t_vals, noise, ctx.white, d_rgb_map.contiguous(), trans)
        if d.shape[1] != net.shape[1]:                       # (columns behind the attention, the occlusion head's: no gradient from here)
            d = torch.cat([d, d.new_zeros((d.shape[0], net.shape[1] - d.shape[1]))], 1)
        return d, None, None, None, None, None, None, None


def composite(net, source_rgb, idx, table, t_vals, noise=None, z_near_far=None, white=False):
    """net [M, >= 4 + V + 1] (colour 3, density 1, attention V + 1; further columns are ignored), source_rgb [M,V,3], idx [M] and
    table [R,2] as visual_hull() gives them, t_vals [R,S], noise [R,S] or None (the reference adds unit-variance noise when training,
    whatever raw_noise_std says), z_near_far = (q_persps[-2], q_persps[-1]) or None -> (rgb_map [R,6], depth [R], acc [R],
    weights [R,S]).  The gradient reaches `net` through rgb_map only (depth, acc and weights are not differentiated, as in the
    reference's loss)."""
    if not _use_kernels(t_vals):
        R, S = t_vals.shape
        return composite_tensor_ops(net, source_rgb, idx, R, S, t_vals, noise, z_near_far, white)
    return _Composite.apply(net, source_rgb, idx, table, t_vals, noise, z_near_far, white)


# ---------------------------------------------------------------- the synthetic scene
def _look_at(pos, target):
    f = target - pos
    f = f / np.linalg.norm(f)
    right = np.cross(np.array([0.0, -1.0, 0.0]), f)
    right = right / np.linalg.norm(right)
    down = np.cross(f, right)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, down, f, pos
    return np.linalg.inv(c2w)


def _project64(verts, w2c, cam):
    """float64 numpy restatement of perspective() for one view: -> (pixel xy [N,2], depth [N])"""
    p = verts @ w2c[:3, :3].T + w2c[:3, 3]
    xy = p[:, :2] / np.maximum(p[:, 2:3], 1e-9)
    x, y = xy[:, 0], xy[:, 1]
    x2, y2, xy_ = x * x, y * y, x * y
    r2 = x2 + y2
    c = 1 + r2 * (cam[4] + r2 * (cam[5] + r2 * cam[8]))
    x, y = c * x + cam[6] * 2 * xy_ + cam[7] * (r2 + 2 * x2), c * y + cam[7] * 2 * xy_ + cam[6] * (r2 + 2 * y2)
    return np.stack([cam[0] * x + cam[2], cam[1] * y + cam[3]], 1), p[:, 2]


def synthetic_scene(seed=0, R=48, S=16, V=4, size=64, C=16, fh=12, fw=20, subdivisions=3, distance=3.0, dilate=5, depth='dilated'):
    """the generated inputs of one render_rays call, float32 host tensors: a synthetic_mesh body; V source cameras on a ring at
    `distance` looking at the body's centre and one query camera, 11-entry camera rows (fx, fy, cx, cy, k1, k2, p1, p2, k3, near,
    far) with non-zero distortion; masks and smpl['depth'] = the projected vertices dilated by `dilate` pixels; images [V,3,size,size];
    feature maps [V,C,fh,fw]; R rays (start, end) through random pixels of the query view's central three quarters; ground-truth colours; the
    training draws t_rand and noise.  depth='raster': smpl['depth'] = the body's real depth maps (gnr_raster.depth_maps) instead of the
    dilated stand-in"""
    if depth not in ('dilated', 'raster'):
        raise ValueError("depth is 'dilated' or 'raster'")
    kind = depth
    from .gnr import synthetic_mesh
    rng = np.random.default_rng([seed, 77])
    mesh = synthetic_mesh(subdivisions, seed)
    verts = mesh['verts'].numpy().astype(np.float64)
    centre = (verts.max(0) + verts.min(0)) / 2
    focal = size * 1.25

    def camera(angle, height):
        pos = centre + distance * np.array([np.sin(angle), height, np.cos(angle)]) / np.sqrt(1 + height * height)
        row = np.array([focal * rng.uniform(0.97, 1.03), focal * rng.uniform(0.97, 1.03), size / 2 + rng.uniform(-1, 1),
                        size / 2 + rng.uniform(-1, 1), rng.uniform(-0.06, 0.06), rng.uniform(-0.02, 0.02), rng.uniform(-0.004, 0.004),
                        rng.uniform(-0.004, 0.004), rng.uniform(-0.01, 0.01), distance - 1.2, distance + 1.2])
        return _look_at(pos, centre), row
    cams = [camera(2 * np.pi * v / V + 0.2, 0.1 * (v % 2)) for v in range(V)]
    q_calib, q_persp = camera(0.55, 0.05)
    masks = torch.zeros((V, 1, size, size))
    depth = torch.zeros((V, 1, size, size))
    for v, (w2c, row) in enumerate(cams):
        pix, z = _project64(verts, w2c, row)
        px, py = np.rint(pix[:, 0]).astype(np.int64), np.rint(pix[:, 1]).astype(np.int64)
        ok = (px >= 0) & (px < size) & (py >= 0) & (py < size)
        zmap = np.zeros((size, size))
        np.maximum.at(zmap, (py[ok], px[ok]), z[ok])
        depth[v, 0] = torch.from_numpy(zmap.astype(np.float32))
        masks[v, 0] = (depth[v, 0] > 0).float()
    k = 2 * dilate + 1
    masks = F.max_pool2d(masks, k, 1, dilate)
    depth = F.max_pool2d(depth, k, 1, dilate)
    # rays of the query view, the reference's get_rays_perspective restated in float64
    lo, hi = size // 8, size - size // 8
    pj, pi = rng.integers(lo, hi, R).astype(np.float64), rng.integers(lo, hi, R).astype(np.float64)
    x, y = (pj - q_persp[2]) / q_persp[0], (pi - q_persp[3]) / q_persp[1]
    xp, yp = x, y
    for _ in range(3):
        x2, y2, xy_ = x * x, y * y, x * y
        r2 = x2 + y2
        c = 1 + r2 * (q_persp[4] + r2 * (q_persp[5] + r2 * q_persp[8]))
        x, y = (xp - q_persp[6] * 2 * xy_ - q_persp[7] * (r2 + 2 * x2)) / (c + 1e-9), (yp - q_persp[7] * 2 * xy_ - q_persp[6] * (r2 + 2 * y2)) / (c + 1e-9)
    d = np.stack([x, y, np.ones_like(x)], -1)
    c2w = np.linalg.inv(q_calib)
    rays = np.concatenate([(d * q_persp[-2]) @ c2w[:3, :3].T + c2w[:3, 3], (d * q_persp[-1]) @ c2w[:3, :3].T + c2w[:3, 3]], 1)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    smpl = dict(mesh)
    smpl['depth'] = depth
    if kind == 'raster':
        from .gnr_raster import depth_maps
        smpl['depth'] = depth_maps(mesh['verts'], mesh['faces'], f32(np.stack([c[0] for c in cams])), f32(np.stack([c[1] for c in cams])), size, size)
    return {'smpl': smpl, 'calibs': f32(np.stack([c[0] for c in cams])), 'persps': f32(np.stack([c[1] for c in cams])),
            'q_calib': f32(q_calib), 'q_persps': f32(q_persp), 'masks': masks, 'images': f32(rng.uniform(0, 1, (V, 3, size, size))),
            'feats': f32(rng.normal(0, 1, (V, C, fh, fw))), 'rays': f32(rays), 'rgb_gt': f32(rng.uniform(0, 1, (R, 3))),
            'mesh_param': {'center': f32(centre), 'spatial_freq': 0.7 * (size / 2)}, 'width': size,
            't_rand': f32(rng.uniform(0, 1, (R, S))), 'noise': f32(rng.normal(0, 1, (R, S))), 'N_samples': S}


# ---------------------------------------------------------------- embedders (gnr_embedder.py:83-177 restated)
class PositionalEncoding:
    """x -> [x | sin(x f), cos(x f) for f in num_freqs frequencies spaced linearly from min_freq 2 pi to max_freq 2 pi]"""

    def __init__(self, d, num_freqs=10, min_freq=None, max_freq=None):
        import math
        lo = 0 if min_freq is None else min_freq
        hi = 2 ** (num_freqs - 1) if max_freq is None else max_freq
        self.freq_bands = torch.linspace(lo * math.pi * 2, hi * math.pi * 2, steps=num_freqs)
        self.out_dim = d * (1 + 2 * num_freqs)

    def embed(self, x):
        out = [x]
        for f in self.freq_bands.tolist() if x.dtype == torch.float32 else self.freq_bands.to(x.dtype).tolist():
            out += [torch.sin(x * f), torch.cos(x * f)]
        return torch.cat(out, -1)


class SphericalHarmonics:
    """real spherical harmonics of rank 3 (9 values) by the reference's recurrences, its index quirks included: the order-m terms of
    degree l read the Legendre slots l(l+1)/2 + m and l(l+1)/2 - m"""

    def __init__(self, d=3, rank=3):
        assert d % 3 == 0
        self.rank = max(int(rank), 0)
        self.out_dim = self.rank * self.rank * (d // 3)

    def embed(self, xyz):
        import math
        cs, sn, z = xyz[..., 0:1], xyz[..., 1:2], xyz[..., 2:3]
        omx = cs * cs + sn * sn
        n = self.rank
        P = [None] * ((n + 1) * n // 2)
        P[0] = torch.ones_like(z)
        for l in range(1, n):
            b = (l * l + l) // 2
            P[b + l] = -P[b - 1] * (2 * l - 1)
            P[b + l - 1] = P[b - 1] * (2 * l - 1) * z
            for m in range(l, 1, -1):
                P[b + m - 2] = -(omx * P[b + m] + 2 * (m - 1) * z * P[b + m - 1]) / ((l - m + 2) * (l + m - 1))
        H = [None] * (n * n)
        for l in range(n):
            b = l * l + l
            a = float(np.sqrt((2 * l + 1) / math.pi / 4))
            H[b] = a * P[b // 2]
            a = float(a * np.sqrt(2))
            s_m, c_m = sn, cs
            for m in range(1, l + 1):
                a = float(-a / np.sqrt((l + m) * (l + 1 - m)))
                H[b - m] = a * P[b // 2 + m] * s_m
                H[b + m] = a * P[b // 2 - m] * c_m
                s_m, c_m = s_m * cs + c_m * sn, c_m * cs - s_m * sn
        return torch.cat(H, -1)


# ---------------------------------------------------------------- GNRMLP (mlps/gnr_mlp.py)
from torch import nn  # noqa: E402

from .builder import MLPS, RENDERS  # noqa: E402


def _lin(x, layer, relu=False, weight=None):
    """every nn.Linear through the linear kernels with exact fp32 products, forward and backward, as NB_NeRFMLP:
    the bars are 4 x the reference's own float32 error, which the default split arithmetic does not meet"""
    from .linear import linear_act_padded
    return linear_act_padded(x, layer.weight if weight is None else weight, layer.bias, relu, exact=True)


@MLPS.register_module()
class GNRMLP(nn.Module):
    """the reference's GNRMLP: same constructor, same state_dict keys, same forward(x, attdirs, alpha_only, smpl_vis); forward_rows takes
    the kernel-made input rows instead of the reference's [M, V, 3 + 7 + C + 3] layout"""

    def __init__(self, opt, D=8, W=256, input_ch=3, input_ch_atts=3, output_ch=4, activation='relu', pose_freqs=10, att_freqs=6,
                 spatial_freq=1 / 256):
        super().__init__()
        if activation != 'relu':
            raise ValueError("activation=%r: only 'relu' is built (the reference's swish branch stores a class, not a function)" % (activation,))
        if opt.use_attention and not opt.weighted_pool:
            raise ValueError('use_attention without weighted_pool: the reference reads an undefined h0 there')
        if opt.use_bn:
            raise ValueError('use_bn: the reference constructs the batch-norm layers and never calls them')
        self.D, self.W = D, W
        self.use_smpl_sdf, self.use_t_pose, self.angle_diff = opt.use_smpl_sdf, opt.use_t_pose, opt.angle_diff
        self.use_occ_net = opt.use_occlusion_net
        self.input_ch_pos_enc = input_ch
        self.input_ch_smpl = (4 if self.use_smpl_sdf else 0) + (3 if self.use_t_pose else 0)
        self.use_smpl = self.input_ch_smpl != 0
        self.input_ch_feat = opt.input_ch_feat + 3
        self.skips = list(opt.skips)
        self.use_viewdirs = opt.use_viewdirs and opt.use_attention
        self.num_views = opt.num_views
        self.input_ch_atts = 0 if not opt.use_attention else (1 if self.angle_diff else 3)
        self.use_sh = opt.use_sh if not self.angle_diff else False
        self.use_attention, self.use_bn, self.spatial_freq = opt.use_attention, opt.use_bn, spatial_freq
        self.pose_embeder = PositionalEncoding(input_ch, num_freqs=pose_freqs, min_freq=spatial_freq * 0.1, max_freq=spatial_freq * 10)
        self.att_embeder = SphericalHarmonics(d=self.input_ch_atts) if self.use_sh else PositionalEncoding(self.input_ch_atts, num_freqs=att_freqs)
        self.pose_embed_fn, self.att_embed_fn = self.pose_embeder.embed, self.att_embeder.embed
        self.weighted_pool = opt.weighted_pool and self.use_attention
        pe, ae, sm = self.pose_embeder.out_dim, self.att_embeder.out_dim, self.input_ch_smpl
        self.alpha_linears = nn.ModuleList([nn.Linear(pe + sm + self.input_ch_feat, W)] +
                                           [nn.Linear(W + pe + sm, W) if i in self.skips else nn.Linear(W, W) for i in range(0, D - 1)])
        self.alpha_out_linear = nn.Linear(W, 1)
        self.rgb_linears = nn.ModuleList([nn.Linear(W + pe + sm, W // 4), nn.Linear(W // 4 + ae, W // 8) if self.use_viewdirs else nn.Linear(W // 4, W // 8),
                                          nn.Linear(W // 8, W // 16), nn.Linear(W // 16, 3)])
        if self.weighted_pool:
            self.s = nn.Parameter(torch.ones(1))
        if self.use_attention:
            self.value_linears = nn.ModuleList([nn.Linear(pe + ae + W, W // 4), nn.Linear(W // 4 + ae, W // 8), nn.Linear(W // 8 + ae, W // 16)])
            self.key_linears = nn.ModuleList([nn.Linear(pe + ae + W, W // 4), nn.Linear(W // 4 + ae, W // 8), nn.Linear(W // 8 + ae, W // 16)])
        if self.use_occ_net:
            self.occ_linears = nn.ModuleList([nn.Linear(sm + 6 + self.input_ch_feat, W // 4), nn.Linear(W // 4, W // 16), nn.Linear(W // 16 + sm + 6, 1)])

    # the row the first alpha layer reads: [pose_embed (pe) | body shape (sm) | features and colour | zero padding]
    def row_layout(self):
        """-> (col0, ld): the column at which the gathered features start and the row stride, a multiple of 4"""
        col0 = self.pose_embeder.out_dim + self.input_ch_smpl
        return col0, (col0 + self.input_ch_feat + 3) // 4 * 4

    def forward(self, x, attdirs=None, alpha_only=False, smpl_vis=None):
        pts, smpl, feats = torch.split(x, [self.input_ch_pos_enc, self.input_ch_smpl, self.input_ch_feat], dim=-1)
        col0, ld = self.row_layout()
        M, V = x.shape[0], x.shape[1]
        rows = torch.cat([self.pose_embed_fn(pts), smpl, feats, x.new_zeros((M, V, ld - col0 - self.input_ch_feat))], -1)
        return self.forward_rows(pts[:, 0], smpl[:, 0], rows, attdirs, alpha_only, smpl_vis)

    def forward_rows(self, pts, smpl, rows, attdirs=None, alpha_only=False, smpl_vis=None):
        """pts [M,3] (normalised), smpl [M, input_ch_smpl], rows [M,V,ld] in row_layout() (pixel_gather writes its part in place)"""
        V, W = self.num_views, self.W
        M, ld = rows.shape[0], rows.shape[2]
        col0 = self.row_layout()[0]
        relu_all = True
        feats = rows[:, :, col0:col0 + self.input_ch_feat].reshape(-1, self.input_ch_feat)
        pe_u = self.pose_embed_fn(pts)
        ipts = pts[:, None].expand(-1, V, -1).reshape(-1, self.input_ch_pos_enc)
        ismpl = smpl[:, None].expand(-1, V, -1).reshape(-1, self.input_ch_smpl)
        have_att = self.use_attention and attdirs is not None
        if have_att:
            qry, src = torch.split(attdirs, [1, V], dim=-2)
        occ_out = None
        if self.use_occ_net and attdirs is not None:
            d = src.reshape(-1, 3)
            m = torch.cross(ipts, d, dim=-1)
            occ_h = torch.cat([ismpl, d, m, feats], dim=-1)
            for i, l in enumerate(self.occ_linears):
                occ_h = _lin(occ_h, l, relu=i < len(self.occ_linears) - 1)
                if i == 1:
                    occ_h = torch.cat([ismpl, d, m, occ_h], dim=-1)
            occ_out = torch.sigmoid(occ_h).view(-1, V, 1)
        first = self.alpha_linears[0]
        w0 = F.pad(first.weight, (0, ld - first.weight.shape[1]))          # zero weight columns under the padding
        h, tmp_h = rows.reshape(-1, ld), None
        for i, l in enumerate(self.alpha_linears):
            h = _lin(h, l, relu=relu_all, weight=w0 if i == 0 else None)
            if i in self.skips:
                if i == self.skips[0]:
                    tmp_h = h
                    h = torch.mean(h.view(-1, V, W), dim=1)
                h = torch.cat([pe_u, smpl, h], dim=-1)
        alpha = _lin(h, self.alpha_out_linear)
        if alpha_only:
            return alpha
        if self.use_attention and self.weighted_pool:
            wts = torch.exp(self.s * (torch.sum(src * qry, dim=-1) - 1))
            wts = wts / (torch.sum(wts, dim=-1, keepdim=True) + 1e-8)
            h = torch.sum(tmp_h.view(-1, V, W) * wts[..., None], dim=1)
            h0 = h
        else:
            h = torch.mean(tmp_h.view(-1, V, W), dim=1)
        h = torch.cat([pe_u, smpl, h], -1)
        for i, l in enumerate(self.rgb_linears):
            h = _lin(h, l, relu=i < len(self.rgb_linears) - 1)
            if i == 0 and self.use_viewdirs:
                h = torch.cat([self.att_embed_fn(-qry.squeeze(1)), h], dim=-1)
        outputs = torch.cat([h, alpha], dim=-1)
        if have_att:
            flat = attdirs.reshape(-1, self.input_ch_atts)
            ae_all = self.att_embed_fn(flat)
            ae_q = self.att_embed_fn(qry.squeeze(1))
            # rows of the value head: per point the query direction first, then the V source views (the reference stacks all query
            # rows in front of all source rows and reads them back [M, V + 1]: the same pairing is restated, quirk included)
            val = torch.cat([self.pose_embed_fn(torch.cat([pts, ipts], dim=0)), ae_all, torch.cat([h0, tmp_h], dim=0)], dim=-1)
            for i, l in enumerate(self.value_linears):
                val = _lin(val, l, relu=i < len(self.value_linears) - 1)
                if i < len(self.value_linears) - 1:
                    val = torch.cat([ae_all, val], dim=-1)
            key = torch.cat([pe_u, ae_q, h0], dim=-1)
            for i, l in enumerate(self.key_linears):
                key = _lin(key, l, relu=i < len(self.key_linears) - 1)
                if i < len(self.key_linears) - 1:
                    key = torch.cat([ae_q, key], dim=-1)
            val = val.view(M, V + 1, -1)
            attention = torch.matmul(val, key.unsqueeze(1).permute(0, 2, 1)).squeeze(-1)
            if self.use_occ_net:
                attention = self.weighted_softmax(attention, occ_out.squeeze(-1))
            elif smpl_vis is not None:
                attention = self.weighted_softmax(attention, smpl_vis.float())
            else:
                attention = F.softmax(attention, dim=-1)
            outputs = torch.cat([outputs, attention], dim=-1)
        if self.use_occ_net and occ_out is not None:
            outputs = torch.cat([outputs, occ_out.squeeze(-1)], dim=-1)
        return outputs

    def weighted_softmax(self, attention, weight):
        e = torch.exp(attention - torch.max(attention, 1, keepdim=True)[0])
        e = torch.cat([e[:, :1], e[:, 1:] * weight], dim=1)
        return e / (torch.sum(e, dim=-1, keepdim=True) + 1e-8)


# ---------------------------------------------------------------- GnrRenderer (renders/gnr_render.py)
@RENDERS.register_module()
class GnrRenderer:
    """the reference's GnrRenderer on the stages above: render_rays = hull -> mesh queries on the survivors only -> shape embedding and
    gather into the network's input rows -> GNRMLP -> compositor.  Same constructor, signatures and return values; render_rays also takes
    `t_rand` [R,S] (uniform draws) and `noise` [R,S] (unit normal draws), drawn on the device by default."""

    def __init__(self, opt, nerf_fine=None, projection='perspective', vgg_loss=None, threshold=0.5):
        from .gnr import MeshGridSearcher
        for name in ('use_vh_free', 'debug', 'regularization', 'angle_diff'):
            if opt.get(name, False):
                raise NotImplementedError('%s is not built%s' % (name, ' (the reference\'s branch slices with a float tensor)' if name == 'use_vh_free' else ''))
        if projection != 'perspective' or opt.get('projection_mode', 'perspective') != 'perspective':
            raise NotImplementedError('projection: only the perspective projection is built')
        if not opt.use_vh or not opt.use_attention:
            raise NotImplementedError('use_vh and use_attention must be on: the compaction and the blend compositor are the path built here')
        self.opt, self.nerf, self.nerf_fine = opt, opt.model, nerf_fine
        self.use_fine = nerf_fine is not None
        self.width = self.height = opt.loadSize
        self.N_samples, self.num_views, self.N_rand, self.N_grid = opt.N_samples, opt.num_views, opt.N_rand, opt.N_grid + 1
        self.projection_mode, self.chunk, self.N_rand_infer = projection, opt.chunk, opt.N_rand_infer
        self.mse_loss = nn.MSELoss()
        self.mesh_searcher = MeshGridSearcher()
        self.use_nml, self.use_attention, self.threshold, self.debug = opt.use_nml, opt.use_attention, threshold, False
        self.rgb_ch = 6
        self.use_vgg, self.vgg_loss = opt.use_vgg, vgg_loss
        self.use_smpl_sdf, self.use_t_pose, self.use_smpl_depth = opt.use_smpl_sdf, opt.use_t_pose, opt.use_smpl_depth
        self.regularization, self.angle_diff = False, False
        self.use_occlusion = opt.use_occlusion and self.use_smpl_depth
        self.use_occlusion_net = opt.use_occlusion_net
        self.gamma, self.omega_reg = 1, 0.01
        self.pts_nml = self.alpha_grad = self.alpha_gt = self.alpha_smpl = self.alpha = self.occ = self.occ_gt = None
        self.nerf_out_ch = 8
        self.use_vh, self.vh_overhead, self.use_vh_free = True, opt.vh_overhead, False
        self.use_white_bkgd = opt.use_white_bkgd
        self.default_rgb = torch.ones if self.use_white_bkgd else torch.zeros
        self._feats_last = None

    def cal_loss(self, rgb, rgb_gt):
        loss = {'nerf': self.mse_loss(rgb[:, :3], rgb_gt), 'att': self.mse_loss(rgb[:, 3:6], rgb_gt)}
        if self.alpha_gt is not None and self.alpha is not None:
            loss['alpha'] = self.mse_loss(self.alpha, self.alpha_gt)
        if self.use_occlusion_net and self.occ is not None and self.occ_gt is not None:
            loss['occ'] = self.mse_loss(self.occ, self.occ_gt)
        return sum(loss.values())

    def get_rays_perspective(self, bbox, w2c, cam):
        """bbox [top, bottom, left, right]; cam [fx, fy, cx, cy, (k1, k2, p1, p2, k3), near, far] -> (rays_s, rays_e) [h, w, 3]"""
        top, bottom, left, right = (int(v) for v in bbox)
        near, far = cam[-2], cam[-1]
        i, j = torch.meshgrid(torch.linspace(top, bottom - 1, bottom - top, device=w2c.device),
                              torch.linspace(left, right - 1, right - left, device=w2c.device), indexing='ij')
        x, y = (j - cam[2]) / cam[0], (i - cam[3]) / cam[1]
        if len(cam) > 6:
            xp, yp = x, y
            for _ in range(3):                                     # three fixed-point sweeps undo the distortion
                x2, y2, xy = x * x, y * y, x * y
                r2 = x2 + y2
                c = (1 + r2 * (cam[4] + r2 * (cam[5] + r2 * cam[8])))
                x, y = (xp - cam[6] * 2 * xy - cam[7] * (r2 + 2 * x2)) / (c + 1e-9), (yp - cam[7] * 2 * xy - cam[6] * (r2 + 2 * y2)) / (c + 1e-9)
        z = torch.ones_like(x)
        starts, ends = torch.stack([x * near, y * near, z * near], -1), torch.stack([x * far, y * far, z * far], -1)
        c2w = torch.inverse(w2c)
        rot, t = c2w[:3, :3], c2w[:3, 3]
        return torch.sum(starts[..., None, :] * rot, -1) + t, torch.sum(ends[..., None, :] * rot, -1) + t

    def make_att_input(self, pts, viewdirs, calibs, smpl):
        return att_directions(pts, viewdirs, calibs, smpl['rot'][0] if smpl is not None else None)

    def inside_pts_vh(self, pts, masks, smpl, calibs, persps=None):
        """the reference's signature on any points (tensor ops) -> (inside [N] bool, smpl_vis [n_inside, V] or None, scan_vis or None)"""
        if persps is None:
            raise NotImplementedError('projection: only the perspective projection is built')
        V = calibs.shape[0]
        xyz = perspective(pts.permute(1, 0)[None].expand(V, -1, -1), calibs, persps)
        xy = xyz[:, :2, :] / torch.tensor([[[self.width], [self.height]]], dtype=xyz.dtype, device=xyz.device) * 2 - 1
        m = masks.reshape(V, 1, masks.shape[-2], masks.shape[-1])
        inside = (index(m, torch.nan_to_num(xy), 'nearest').squeeze(1) > 0).all(0) & torch.isfinite(xy).all(1).all(0)

        def vis(depth_maps):
            d = index(depth_maps.reshape(V, 1, depth_maps.shape[-2], depth_maps.shape[-1]), torch.nan_to_num(xy), 'nearest').squeeze(1).permute(1, 0)[inside]
            return ((xyz[:, 2, :].permute(1, 0)[inside] - d) <= 0) & (d > 0)
        smpl_vis = vis(smpl['depth']) if self.use_occlusion else None
        scan_vis = vis(smpl['scan_depth']) if self.use_occlusion_net and 'scan_depth' in smpl else None
        return inside, smpl_vis, scan_vis

    def scan_depth_maps(self, scan, calibs, persps):
        """scan = [verts [N,3], faces [F,3]] -> the scan's depth maps [V,1,height,width] in the source views (gnr_raster.depth_maps).
        Nothing calls it by itself: a caller that puts the result into smpl['scan_depth'] switches the occlusion head's supervision
        (occ_gt = scan_vis) on, a loss existing runs do not have."""
        from .gnr_raster import depth_maps
        if persps is None:
            raise NotImplementedError('projection: only the perspective projection is built')
        return depth_maps(scan[0], scan[1], calibs[:self.num_views], persps[:self.num_views], self.height, self.width)

    def make_nerf_input(self, pts, feats, images, smpl, calibs, mesh_param, persps=None, is_train=True):
        """the reference's layout [N, V, 3 + 7 + C + 3] and source_rgb [N, V, 3] (render_rays builds the network's rows directly instead)"""
        from .gnr import body_shape_embedding
        emb, self.alpha_smpl = body_shape_embedding(pts, smpl, mesh_param, self.width, self.use_nml, self.use_t_pose, self.use_smpl_sdf,
                                                    searcher=self.mesh_searcher)
        self.pts_nml = emb[:, :3]
        if feats is None:
            return emb, None
        V = calibs.shape[0]
        xyz = perspective(pts.permute(1, 0)[None].expand(V, -1, -1), calibs, persps)
        xy = xyz[:, :2, :] / torch.tensor([[[self.width], [self.height]]], dtype=xyz.dtype, device=xyz.device) * 2 - 1
        latent, source_rgb = gather_tensor_ops(xy.permute(2, 0, 1), feats, images[:self.num_views])
        return torch.cat([emb[:, None, :].expand(-1, V, -1), latent], -1), source_rgb

    def make_nerf_output(self, nerf_output, t_vals, norm, source_rgb, is_train=True, noise=None):
        """the dense formulation: nerf_output [R, S, 4 + V + 1] -> (rgb_map [R, 6], weights [R, S]); `norm` is unused, as in the reference"""
        R, S = t_vals.shape
        if is_train and noise is None:
            noise = torch.randn((R, S), device=nerf_output.device)
        idx = torch.arange(R * S, device=nerf_output.device)
        rgb_map, _, _, weights = composite_tensor_ops(nerf_output.reshape(R * S, -1), source_rgb.reshape(R * S, self.num_views, 3), idx, R, S, t_vals,
                                                      noise if is_train else None, None, self.use_white_bkgd)
        return rgb_map, weights

    def _channel_last(self, feats):
        if feats.requires_grad:
            return feats.permute(0, 2, 3, 1).contiguous()
        import weakref
        c = self._feats_last
        if c is None or c[0]() is not feats or c[1] != feats._version:                 # once per frame; the caller's maps are not kept alive
            self._feats_last = c = (weakref.ref(feats), feats._version, channel_last(feats))
        return c[2]

    def render_rays(self, ray_batch, feats, images, masks, calibs, smpl, mesh_param, scan=None, persps=None, q_persps=None, is_train=True,
                    t_rand=None, noise=None):
        from .gnr import embed
        if persps is None:
            raise NotImplementedError('projection: only the perspective projection is built')
        self.alpha = None
        dev = ray_batch.device
        R, S, V = ray_batch.shape[0], self.N_samples, self.num_views
        t_vals = torch.linspace(0., 1., steps=S, device=dev).repeat([R, 1])
        if is_train:
            t_rand = torch.rand(t_vals.shape, device=dev) if t_rand is None else t_rand
            t_vals = t_vals + (t_rand - 0.5) / (S - 1)
            noise = torch.randn(t_vals.shape, device=dev) if noise is None else noise
        else:
            noise = None
        h = visual_hull(ray_batch[:, :6].contiguous(), t_vals, calibs, persps, masks, self.width, self.height,
                        smpl['depth'] if self.use_occlusion else None, smpl['rot'][0], True)
        if h['M'] == 0:                                            # nothing is launched after the hull
            return self.default_rgb([R, self.rgb_ch], dtype=torch.float32, device=dev), torch.zeros([R], dtype=torch.float32, device=dev)
        pts = h['pts']
        if is_train and scan is not None:
            self.mesh_searcher.set_mesh(scan[0], scan[1])
            self.alpha_gt = (self.mesh_searcher.inside_mesh(pts) + 1) / 2
        # body-shape embedding: the mesh queries see the survivors only
        self.mesh_searcher.set_mesh(smpl['verts'], smpl['faces'])
        closest_pts, closest_idx = self.mesh_searcher.nearest_points(pts)
        signs = self.mesh_searcher.inside_mesh(pts) if self.use_smpl_sdf else None
        emb, self.alpha_smpl = embed(pts, closest_pts, closest_idx, signs, smpl, mesh_param, self.width, self.use_nml, self.use_t_pose, self.use_smpl_sdf)
        self.pts_nml = emb[:, :3]
        # the network's input rows: [pose_embed | body shape | gathered features and colour | zero padding], no [M, V, 269] tensor
        col0, ld = self.nerf.row_layout()
        rows = torch.empty((h['M'], V, ld), dtype=torch.float32, device=dev)
        rows[:, :, :col0] = torch.cat([self.nerf.pose_embed_fn(emb[:, :3]), emb[:, 3:]], -1)[:, None, :]
        rows, source_rgb = pixel_gather(h['xy'], self._channel_last(feats), images[:V], rows, col0)
        net = torch.cat([self.nerf.forward_rows(emb[i:i + self.chunk, :3], emb[i:i + self.chunk, 3:], rows[i:i + self.chunk], h['attdirs'][i:i + self.chunk],
                                                smpl_vis=h['vis'][i:i + self.chunk] if h['vis'] is not None else None)
                         for i in range(0, h['M'], self.chunk)], 0)
        self.alpha = torch.sigmoid(net[..., 3] * self.gamma)
        if self.use_occlusion_net and is_train and scan is not None and 'scan_depth' in smpl:
            d = index(smpl['scan_depth'].reshape(V, 1, *smpl['scan_depth'].shape[-2:]), h['xy'].permute(1, 2, 0), 'nearest').squeeze(1).permute(1, 0)
            self.occ_gt = (((h['z'] - d) <= 0) & (d > 0)).float()
            self.occ = net[:, -V:]
        z_near_far = (float(q_persps[-2]), float(q_persps[-1])) if q_persps is not None else None
        rgb_map, depth, _, _ = composite(net, source_rgb, h['idx'], h['table'], t_vals, noise, z_near_far, self.use_white_bkgd)
        return rgb_map, depth

    def render(self, feats, images, masks, calibs, bbox, mesh_param, smpl=None, scan=None, persps=None):
        """one training batch of N_rand rays of the last view -> {'loss', 'num_samples'}"""
        rays_s, rays_e = self.get_rays_perspective(bbox, calibs[-1], persps[-1])
        top, bottom, left, right = (int(v) for v in bbox)
        gt = images[-1].permute((1, 2, 0))[top:bottom, left:right]
        n = (bottom - top) * (right - left)
        sel = torch.from_numpy(np.random.choice(n, size=[self.N_rand * self.vh_overhead], replace=False)).to(calibs.device)
        batch_rays = torch.cat([rays_s.reshape(-1, 3)[sel], rays_e.reshape(-1, 3)[sel]], 1)
        rgb, _ = self.render_rays(batch_rays, feats, images[:self.num_views], masks[:self.num_views], calibs[:self.num_views], smpl, mesh_param,
                                  scan, persps[:self.num_views])
        return {'loss': self.cal_loss(rgb, gt.reshape(-1, 3)[sel]), 'num_samples': rgb.shape[0]}

    def render_path(self, feats, images, masks, calibs, bbox, mesh_param, smpl=None, scan=None, persps=None):
        """every query view behind the num_views source views -> (rgbs [Q, H, W, 6], depths [Q, H, W])"""
        top, bottom, left, right = (int(v) for v in bbox)
        height, width = max(self.height, bottom - top), max(self.width, right - left)
        V = self.num_views
        rgbs, depths = [], []
        for q in range(V, calibs.shape[0]):
            rays_s, rays_e = self.get_rays_perspective(bbox, calibs[q], persps[q])
            batch_rays = torch.cat([rays_s.reshape(-1, 3), rays_e.reshape(-1, 3)], 1)
            rgb, depth = [], []
            for i in range(0, batch_rays.shape[0], self.N_rand_infer):
                c, d = self.render_rays(batch_rays[i:i + self.N_rand_infer].detach(), feats, images[:V], masks[:V], calibs[:V], smpl, mesh_param,
                                        persps=persps[:V], q_persps=persps[q], is_train=False)
                rgb.append(c[:, :self.rgb_ch])
                depth.append(d)
            img = self.default_rgb((height, width, self.rgb_ch), dtype=torch.float32, device=calibs.device)
            dimg = torch.zeros((height, width), dtype=torch.float32, device=calibs.device)
            img[top:bottom, left:right] = torch.cat(rgb, 0).view(bottom - top, right - left, self.rgb_ch)
            dimg[top:bottom, left:right] = torch.cat(depth, 0).view(bottom - top, right - left)
            rgbs.append(img)
            depths.append(dimg)
        return torch.stack(rgbs, dim=0), torch.stack(depths, dim=0)

    # ---- mesh reconstruction (gnr_recon.py)
    def _network_rows(self, pts, xy, feats_last, images, smpl, mesh_param):
        """the network's input rows of a chunk of points: mesh queries (set_mesh is the caller's), shape embedding, pixel gather in place
        into rows -> (emb, rows, source_rgb); feats_last = self._channel_last(feats)"""
        from .gnr import embed
        closest_pts, closest_idx = self.mesh_searcher.nearest_points(pts)
        signs = self.mesh_searcher.inside_mesh(pts) if self.use_smpl_sdf else None
        emb, _ = embed(pts, closest_pts, closest_idx, signs, smpl, mesh_param, self.width, self.use_nml, self.use_t_pose, self.use_smpl_sdf)
        col0, ld = self.nerf.row_layout()
        rows = torch.empty((pts.shape[0], self.num_views, ld), dtype=torch.float32, device=pts.device)
        rows[:, :, :col0] = torch.cat([self.nerf.pose_embed_fn(emb[:, :3]), emb[:, 3:]], -1)[:, None, :]
        rows, source_rgb = pixel_gather(xy, feats_last, images[:self.num_views], rows, col0)
        return emb, rows, source_rgb

    @torch.no_grad()
    def octree_reconstruct(self, coords, masks, **kwargs):
        """The reference's signature: coords [N,N,N,3] (array or tensor) or None -- then kwargs['grid'] = (bb_min, bb_max) and the points
        are made where they are used; masks [V,1,H,W]; kwargs: feats, images, smpl, calibs, mesh_param, persps.  -> the occupancy volume
        [N,N,N], a float32 tensor that stays on the device (the reference returns a float64 numpy array).  self.recon_levels keeps the
        number of evaluated points per level."""
        if kwargs.get('persps') is None:
            raise NotImplementedError('projection: only the perspective projection is built')
        from . import gnr_recon as R
        calibs, persps = kwargs['calibs'][:self.num_views].contiguous(), kwargs['persps'][:self.num_views].contiguous()
        feats, images, smpl, mesh_param = kwargs['feats'], kwargs['images'], kwargs['smpl'], kwargs['mesh_param']
        dev, N = calibs.device, self.N_grid
        if coords is None:
            bb_min, bb_max = kwargs['grid']
            grid = R.Grid(N, bb_min, bb_max, mesh_param['spatial_freq'], mesh_param['center'].to(dev))
        else:
            grid = R.Grid(N, [0, 0, 0], [1, 1, 1], 1.0, torch.zeros(3, device=dev), torch.as_tensor(np.asarray(coords, dtype=np.float32) if not torch.is_tensor(coords) else coords).to(dev))
        state = R.grid_hull(grid, calibs, persps, R.dilate_masks(masks[:self.num_views]), self.width, self.height)
        self.mesh_searcher.set_mesh(smpl['verts'], smpl['faces'])              # once for the whole reconstruction

        feats_last = self._channel_last(feats)

        def evaluate(flat, pts, xy):
            out = []
            for i in range(0, pts.shape[0], self.chunk):
                emb, rows, _ = self._network_rows(pts[i:i + self.chunk], xy[i:i + self.chunk], feats_last, images, smpl, mesh_param)
                out.append(self.nerf.forward_rows(emb[:, :3], emb[:, 3:], rows, alpha_only=True))
            return torch.cat(out, 0)
        select = lambda reso, st: R.level_select(grid, reso, st, calibs, persps, self.width, self.height)
        vol, _, self.recon_levels = R.octree(N, kwargs.get('reso0', N // 64), state, evaluate, select, gamma=self.gamma)
        return vol

    @torch.no_grad()
    def vertex_colours(self, pts, normals, feats, images, calibs, persps, smpl, mesh_param):
        """the colouring lines of reconstruct: the network at the vertices pts [Nv,3] with the normals as view directions (no smpl_vis),
        sigmoid of channels 0-2 blended with the source colours by the attention channels -> [Nv,3]"""
        self.mesh_searcher.set_mesh(smpl['verts'], smpl['faces'])
        return self._vertex_colours(pts, normals, feats, images, calibs, persps, smpl, mesh_param)

    def _vertex_colours(self, pts, normals, feats, images, calibs, persps, smpl, mesh_param):
        """vertex_colours on the mesh the searcher already holds (reconstruct: set_mesh once per reconstruction)"""
        from . import gnr_recon as R
        V = self.num_views
        feats_last = self._channel_last(feats)
        xy, attdirs = R.point_rows(pts.contiguous(), normals.float().contiguous(), calibs, persps, self.width, self.height, smpl['rot'][0] if smpl is not None else None)
        rgbs = []
        for i in range(0, pts.shape[0], self.chunk):
            emb, rows, source_rgb = self._network_rows(pts[i:i + self.chunk], xy[i:i + self.chunk], feats_last, images, smpl, mesh_param)
            net = self.nerf.forward_rows(emb[:, :3], emb[:, 3:], rows, attdirs[i:i + self.chunk])
            rgb = torch.sigmoid(net[:, :3])
            att = net[:, 4:4 + V + 1]
            rgbs.append(torch.sum(torch.cat([rgb[:, None], source_rgb.view(-1, V, 3)], dim=-2) * att[..., None], dim=-2))
        return torch.cat(rgbs, 0)

    def reconstruct(self, feats, images, masks, calibs, bbox, mesh_param, smpl=None, scan=None, persps=None):
        """The reference's signature -> (verts float64 [Nv,3], faces int32 [T,3], rgbs float32 [Nv,3]) as numpy.  An empty hull or a volume
        that never crosses the threshold gives three empty arrays (scikit-image would raise); masks, calibs and persps are cut to
        num_views.  The grid spans 0 .. 512 along x and z whatever loadSize is, as in the reference."""
        if persps is None:
            raise NotImplementedError('projection: only the perspective projection is built')
        from . import gnr_recon as R
        with torch.no_grad():
            V, N = self.num_views, self.N_grid
            top, bottom = float(bbox[0]), float(bbox[1])
            bb_min = [0 - self.width / 2, top - self.height / 2, 0 - self.width / 2]
            bb_max = [512 - self.width / 2, bottom - self.height / 2, 512 - self.width / 2]
            calibs, persps, masks = calibs[:V].contiguous(), persps[:V].contiguous(), masks[:V]
            center = mesh_param['center'].to(calibs.device)
            kwargs = {'feats': feats, 'images': images, 'smpl': smpl, 'calibs': calibs, 'mesh_param': mesh_param, 'persps': persps}
            vol = self.octree_reconstruct(None, masks, grid=(bb_min, bb_max), **kwargs)
            if sum(self.recon_levels) == 0:
                return R.empty_mesh()
            verts_idx, faces, normals = R.marching_cubes(vol, self.threshold)
            if verts_idx.shape[0] == 0 or faces.shape[0] == 0:
                return R.empty_mesh()
            verts, pts = R.to_world(verts_idx, N, (top, bottom), mesh_param['spatial_freq'], center)
            if self.opt.get('laplacian', 0) > 0:
                verts = R.laplacian_smooth(verts, faces, int(self.opt.laplacian))
                pts = verts.float()
            rgbs = self._vertex_colours(pts, normals, feats, images, calibs, persps, smpl, mesh_param)
            return verts.cpu().numpy(), faces.cpu().numpy(), rgbs.float().cpu().numpy()
