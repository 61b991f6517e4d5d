"""The float64 lines of the BungeeNeRF training rays in plain numpy: what get_rays_np_bungee / load_rays_bungee
(xrnerf/datasets/load_data/get_rays.py:156-206) evaluate under numpy 2 with the types load_data hands over -- an fp32 meshgrid, a Python
float W * .5 (which leaves the difference fp32), an np.float64 focal (which moves the chain to float64) and float64 poses -- followed by
GetViewdirs on the float64 rays (torch.norm accumulates acc = fma(x, x, acc)).  tests/golden/make_golden_scenedata.py asserts, element by
element, that these values rounded to fp32 are the reference's values cast to fp32; xr_bgd_item (xrnerf_amd/csrc/xr_bungeedata.hip)
states the same lines in device code."""
from fractions import Fraction

import numpy as np


def fma(a, b, c):
    """a b + c rounded once (exact rational arithmetic, then the correctly rounded conversion)"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def image_rays(H, W, focal, c2w):
    """rays_o, rays_d [H, W, 3], radii [H, W, 1], viewdirs [H, W, 3] of one train image, float64"""
    H, W, focal, c2w = int(H), int(W), np.float64(focal), np.asarray(c2w, np.float64)
    i, j = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing='xy')
    xf, yf = i - np.float32(W * .5), -(j - np.float32(H * .5))                   # fp32
    x, y, z = xf.astype(np.float64) / focal, yf.astype(np.float64) / focal, -np.ones((H, W))
    n = np.sqrt((x * x + y * y) + z * z)
    u = [x / n, y / n, z / n]
    d = np.stack([(u[0] * c2w[r, 0] + u[1] * c2w[r, 1]) + u[2] * c2w[r, 2] for r in range(3)], -1)
    e = d[:-1] - d[1:]
    dx = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
    dx = np.concatenate([dx, dx[-2:-1]], 0)
    radii = (dx[..., None] * 2) / np.sqrt(12.0)
    nd = np.array([[np.sqrt(fma(p[2], p[2], fma(p[1], p[1], p[0] * p[0]))) for p in row] for row in d])
    return np.broadcast_to(c2w[:3, 3], d.shape), d, radii, d / nd[..., None]


def table(H, W, focal, poses, images, codes, i_train, perm):
    """the shuffled tables of a stage: dict of float64 / int64 arrays rays_o, rays_d, target_s, viewdirs [T H W, 3], radii, scale_code [.,1]"""
    o, d, r, v, rgb, c = [], [], [], [], [], []
    for i in i_train:
        ro, rd, rr, rv = image_rays(H, W, focal, poses[i])
        o.append(ro.reshape(-1, 3)); d.append(rd.reshape(-1, 3)); r.append(rr.reshape(-1, 1)); v.append(rv.reshape(-1, 3))
        rgb.append(np.asarray(images[i], np.float64).reshape(-1, 3))
        c.append(np.full((H * W, 1), codes[i], np.int64))
    cat = lambda xs: np.concatenate(xs, 0)[np.asarray(perm)]
    return dict(rays_o=cat(o), rays_d=cat(d), target_s=cat(rgb), radii=cat(r), scale_code=cat(c), viewdirs=cat(v))
