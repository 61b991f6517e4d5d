"""The integer and float specification of the GeneBody frame preparation (xrnerf_amd/csrc/xr_genebody.hip), in numpy,
one operation per line where the bits matter.  This file IS the specification of the two OpenCV resizes: cv2 is not installed here, so
`resize_nearest` and `resize_cubic_u8` are written from OpenCV's resize.cpp as it is remembered and their equality with OpenCV itself is
UNVERIFIED.  tests/golden/make_golden_genebody.py hands them to the reference's own GeneBodyDataset as `cv2.resize`.

  crop_box         GeneBodyDataset.image_cropping (genebody_dataset.py:116-158) with its quirks: `left` padded by bbox_h, the 10 % padding
                   in double and truncated, three placement branches per axis, the whole (non-square) picture for an empty mask
  resize_nearest   INTER_NEAREST: sx = min(floor(x * scale), n - 1), scale = 1 / (S / (double) n)
  resize_cubic_u8  8-bit INTER_CUBIC in fixed point: fx = (float)((x + 0.5) scale - 0.5), four float coefficients with A = -0.75f, each
                   short(rint(c * 2048)), taps sx - 1 .. sx + 2 clamped to the crop, int32 sums, (v + 2^21) >> 22 saturated
  assemble         mask > 128 (| depth > 0 for input views), ToTensor, Normalize or the white background, the mask product, the mask's box
  calib            the adjusted K, near / far, spatial_freq, the item's bbox and center (float64 where the reference's BLAS order is open)
"""
import numpy as np

COEF_BITS = 11
A = np.float32(-0.75)
f32 = np.float32


def crop_box(mask):
    """(top, left, bottom, right) of a raw mask [h, w]"""
    h, w = int(mask.shape[0]), int(mask.shape[1])
    rows, cols = np.nonzero(mask != 0)[:2]
    if len(rows) == 0:
        return 0, 0, h, w
    top, left, bottom, right = int(rows.min()), int(cols.min()), int(rows.max()), int(cols.max())
    bbox_h, bbox_w = bottom - top, right - left
    bottom = min(int(bbox_h * 0.1 + bottom), h)
    top = max(int(top - bbox_h * 0.1), 0)
    right = min(int(bbox_w * 0.1 + right), w)
    left = max(int(left - bbox_h * 0.1), 0)                 # bbox_h: the reference's line, kept
    bbox_h, bbox_w = bottom - top, right - left
    if bbox_h >= bbox_w:
        c, size = (left + right) / 2, bbox_h
        if c - size / 2 < 0:
            left, right = 0, size
        elif c + size / 2 >= w:
            left, right = w - size, w
        else:
            left = int(c - size / 2)
            right = left + size
    else:
        c, size = (top + bottom) / 2, bbox_w
        if c - size / 2 < 0:
            top, bottom = 0, size
        elif c + size / 2 >= h:
            top, bottom = h - size, h
        else:
            top = int(c - size / 2)
            bottom = top + size
    return top, left, bottom, right


def check_box(box, h, w):
    """the crops the reference itself breaks on: a side beyond the picture"""
    top, left, bottom, right = box
    if top < 0 or left < 0 or bottom > h or right > w or bottom <= top or right <= left:
        raise ValueError('crop (%d, %d, %d, %d) does not lie inside the %d x %d picture: its side exceeds the other dimension' % (top, left, bottom, right, h, w))


def _scale(n, S):
    return 1. / (S / float(n))


def nearest_index(n, S):
    x = np.arange(S, dtype=np.float64)
    return np.minimum(np.floor(x * _scale(n, S)).astype(np.int64), n - 1)


def resize_nearest(src, S):
    """src [h, w] of any dtype -> [S, S]"""
    return np.ascontiguousarray(src[nearest_index(src.shape[0], S)][:, nearest_index(src.shape[1], S)])


def cubic_taps(n, S):
    """-> (index [S, 4] clamped to 0 .. n - 1, coefficient [S, 4] int32)"""
    x = np.arange(S, dtype=np.float64)
    fx = ((x + 0.5) * _scale(n, S) - 0.5).astype(np.float32)
    sx = np.floor(fx)
    f = (fx - sx).astype(np.float32)
    t = f + f32(1)
    c0 = ((A * t - f32(-3.75)) * t + f32(-6)) * t - f32(-3)
    c1 = ((f32(1.25) * f - f32(2.25)) * f) * f + f32(1)
    g = f32(1) - f
    c2 = ((f32(1.25) * g - f32(2.25)) * g) * g + f32(1)
    c3 = ((f32(1) - c0) - c1) - c2
    c = np.stack([c0, c1, c2, c3], axis=1)
    assert c.dtype == np.float32
    coef = np.clip(np.rint(c * f32(1 << COEF_BITS)), -32768, 32767).astype(np.int32)
    idx = np.clip(sx.astype(np.int64)[:, None] + np.arange(-1, 3)[None], 0, n - 1)
    return idx, coef


def resize_cubic_u8(src, S):
    """src [h, w, C] uint8 -> [S, S, C] uint8"""
    assert src.dtype == np.uint8 and src.ndim == 3
    iy, cy = cubic_taps(src.shape[0], S)
    ix, cx = cubic_taps(src.shape[1], S)
    s = src.astype(np.int64)
    hor = (s[:, ix, :] * cx[None, :, :, None]).sum(axis=2)                     # [h, S, C], no shift
    ver = (hor[iy] * cy[:, :, None, None]).sum(axis=1)                         # [S, S, C]
    assert np.abs(hor).max(initial=0) < 2 ** 31 and np.abs(ver).max(initial=0) < 2 ** 31 - 2 ** 21
    return np.clip((ver + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def prepare_view(img, mask, depth16, S):
    """what the view store keeps: (rgb [S,S,3] uint8, mask byte [S,S] uint8, depth [S,S] fp32 or None, box)"""
    if mask.dtype != np.uint8 or mask.ndim != 2:
        raise ValueError('a mask must be single-channel uint8')
    box = crop_box(mask)
    check_box(box, mask.shape[0], mask.shape[1])
    t, l, b, r = box
    depth = None
    if depth16 is not None:
        depth = resize_nearest((depth16.astype(np.float32) / f32(1000.0))[t:b, l:r], S)
    return resize_cubic_u8(img[t:b, l:r], S), resize_nearest(mask[t:b, l:r], S), depth, box


def mask_box(m):
    S = m.shape[0]
    rows, cols = np.nonzero(m)
    if len(rows) == 0:
        return [[0, 0], [S, S]]
    return [[int(rows.min()), int(cols.min())], [int(rows.max()), int(cols.max())]]


def assemble_view(rgb, m8, depth, is_input, white):
    """-> (img [3,S,S] fp32, mask [S,S] fp32, box [[r0,c0],[r1,c1]])"""
    m = m8 > 128
    if is_input and depth is not None:
        m = m | (depth > 0)
    mf = m.astype(np.float32)
    x = rgb.astype(np.float32).transpose(2, 0, 1) / f32(255)
    if is_input:
        x = (x - f32(0.5)) / f32(0.5)
    elif white:
        x = x * mf + (f32(1) - mf)
    return mf[None] * x, mf, mask_box(m)


def adjusted_K(K, box, S):
    """genebody_dataset.py:292-297 on a float32 K: every step rounds to fp32"""
    t, l, b, r = box
    K = np.array(K, dtype=np.float32)
    K[0, 2] = f32(K[0, 2] - f32(l))
    K[1, 2] = f32(K[1, 2] - f32(t))
    K[0, :] = K[0, :] * f32(S / float(r - l))
    K[1, :] = K[1, :] * f32(S / float(b - t))
    return K


def project64(verts, w2c):
    """camera coordinates of float32 vertices in float64, and the bound 4 x 2^-24 x (sum |a b| + |t|) of a float32 evaluation in any order"""
    v, R, t = verts.astype(np.float64), w2c[:3, :3].astype(np.float64), w2c[:3, 3].astype(np.float64)
    return v @ R.T + t, 4 * 2.0 ** -24 * (np.abs(v) @ np.abs(R).T + np.abs(t))


def near_far64(verts, w2c):
    """-> (near, far, the largest bound of a z coordinate) in float64"""
    vp, err = project64(verts, w2c)
    lo, hi = vp[:, 2].min(), vp[:, 2].max()
    return lo - (hi - lo) / 2, hi + (hi - lo) / 2, err[:, 2].max()


def spatial_freq64(verts, box, w2c, K):
    """get_realworld_scale in float64 -> (spatial_freq, smallest extent / largest magnitude of the coordinates it divides by)"""
    vp, _ = project64(verts, w2c)
    p = vp @ K.astype(np.float64).T
    uv = p[:, :2] / (p[:, 2:] + float(f32(1e-8)))
    lo, hi = uv.min(0), uv.max(0)
    smin, smax = verts.astype(np.float64).min(0), verts.astype(np.float64).max(0)
    bh, bw = box[1][0] - box[0][0], box[1][1] - box[0][1]
    a = 1 if bh > bw else 0
    long_axis = (bh if a else bw) / (hi[a] - lo[a]) * (smax[a] - smin[a])
    rel = min((hi[a] - lo[a]) / np.abs(uv[:, a]).max(), (smax[a] - smin[a]) / np.abs(verts[:, a]).max())
    return 180 / long_axis / 0.5, rel


def item_bbox(boxes, S):
    """boxes: the mask boxes [[r0,c0],[r1,c1]] of the views that count -> float64 [4]"""
    pts = np.array(boxes).reshape(-1, 2)
    centroid = np.array([S, S]) / 2
    b = (np.max(np.abs(pts - centroid), axis=0) * np.array([1, np.sqrt(2)])).astype(np.int32)
    return np.clip(np.array([centroid - b, centroid + b]).T.reshape(-1), 0, S)


def center(verts):
    return (verts.max(0) + verts.min(0)) / 2
