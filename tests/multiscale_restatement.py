"""The specification of xr_ms_rays and xr_ms_pyramid (xrnerf_amd/csrc/xr_multiscale.hip) in numpy: float64, every product and sum written
out in the order the kernel takes them, nothing handed to a matmul or a reduction.  tests/golden/make_golden_multiscale.py asserts,
element by element, that these round to the same fp32 as the reference's load_rays_multiscale + flatten, and that the pyramid gives the
reference converter's bytes; the host path of xrnerf_amd/multiscale.py builds its tables from the same lines."""
import numpy as np


def frame_rays(pix2cam, cam2world, H, W, lossmult, near, far):
    """the seven per-ray arrays of one H x W image, float64, [H, W, .]; H < 3 raises ValueError (the reference returns fewer radii)"""
    H, W = int(H), int(W)
    if H < 3:
        raise ValueError('multiscale rays need H >= 3 (got %d)' % H)
    P, C = np.asarray(pix2cam, np.float64), np.asarray(cam2world, np.float64)
    x = (np.arange(W, dtype=np.float64) + 0.5)[None, :] * np.ones((H, 1))
    y = (np.arange(H, dtype=np.float64) + 0.5)[:, None] * np.ones((1, W))
    cam = [(x * P[r, 0] + y * P[r, 1]) + P[r, 2] for r in range(3)]
    d = np.stack([(cam[0] * C[r, 0] + cam[1] * C[r, 1]) + cam[2] * C[r, 2] for r in range(3)], -1)
    n = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    e = d[:-1] - d[1:]
    dx = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
    dx = np.concatenate([dx, dx[-2:-1]], 0)                      # the last row takes dx[H - 3], not dx[H - 2]
    ones = np.ones((H, W, 1))
    return dict(rays_o=np.broadcast_to(C[:3, 3], (H, W, 3)).copy(), rays_d=d, viewdirs=d / n[..., None], radii=(dx[..., None] * 2) / np.sqrt(12.0),
                lossmult=float(lossmult) * ones, near=float(near) * ones, far=float(far) * ones)


RAY_KEYS = ('rays_o', 'rays_d', 'viewdirs', 'radii', 'lossmult', 'near', 'far')


def tables(meta):
    """the reference's flattened fp32 tables of a whole split: {key: [total, .] float32}"""
    frames = [frame_rays(meta['pix2cam'][i], meta['cam2world'][i], meta['height'][i], meta['width'][i], meta['lossmult'][i], meta['near'][i],
                         meta['far'][i]) for i in range(len(meta['height']))]
    return {k: np.concatenate([f[k].reshape(-1, f[k].shape[-1]) for f in frames], 0).astype(np.float32) for k in RAY_KEYS}


def z_vals(near, far, S, lindisp=False, t_rand=None):
    """GetZvals in float32 on [R,1] near / far: torch.linspace's two-sided formula, then the bins"""
    near, far = np.asarray(near, np.float32), np.asarray(far, np.float32)
    one, step = np.float32(1), (np.float32(1) / np.float32(S - 1) if S > 1 else np.float32(0))
    j = np.arange(S)
    # torch.linspace: step j below the middle, 1 - step (S - 1 - j) from it on, each ONE rounding (the product is exact in double)
    t = np.where(j < S // 2, np.float64(step) * j, 1.0 - np.float64(step) * (S - 1 - j)).astype(np.float32) if S > 1 else np.zeros(1, np.float32)
    z = near * (one - t) + far * t if not lindisp else one / (one / near * (one - t) + one / far * t)
    if t_rand is None:
        return z.astype(np.float32)
    mids = np.float32(.5) * (z[..., 1:] + z[..., :-1])
    upper, lower = np.concatenate([mids, z[..., -1:]], -1), np.concatenate([z[..., :1], mids], -1)
    return (lower + (upper - lower) * np.asarray(t_rand, np.float32)).astype(np.float32)


def down2(img):
    """(((a + b) + c) + d) / 4 in float32: the association numpy's np.mean(reshape, (1, 3)) takes"""
    img = np.asarray(img, np.float32)
    a, b, c, d = img[0::2, 0::2], img[0::2, 1::2], img[1::2, 0::2], img[1::2, 1::2]
    return (((a + b) + c) + d) / np.float32(4)


def pyramid(base, n_down, white_bkgd=True):
    """one [H,W,C] uint8 view -> ([bytes of level j], [loaded fp32 [h,w,3] pixels of level j])"""
    H, W = base.shape[:2]
    if H % (1 << (n_down - 1)) or W % (1 << (n_down - 1)):
        raise ValueError('a %d x %d image cannot be halved %d times' % (H, W, n_down - 1))
    img = base.astype(np.float32) / np.float32(255)
    saved, loaded = [], []
    for j in range(n_down):
        b = (img * np.float32(255)).astype(np.uint8)
        saved.append(b)
        px = b.astype(np.float32) / np.float32(255)
        if white_bkgd:
            px = px[..., :3] * px[..., -1:] + (np.float32(1) - px[..., -1:])
        loaded.append(px[..., :3])
        if j + 1 < n_down:
            img = down2(img)
    return saved, loaded


def pix2cam(focal, width, height):
    """convert_blender_data.py:103-114 for one image, in double"""
    fx = fy = float(focal)
    cx, cy = float(width) * .5, float(height) * .5
    return np.array([[1. / fx, 0., -cx / fx], [0., -1. / fy, cy / fy], [0., 0., -1.]])
