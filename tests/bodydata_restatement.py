"""The specification of the human-data kernels (xrnerf_amd/csrc/xr_bodydata.hip), independent of the package: float64 and exact integer
numpy.  prepare() and fill() ARE the specification of the prepared picture and of the box silhouette (OpenCV's undistort, resize and
fillPoly are not available where the fixture is made: their equality with these functions is unverified).  rays(), box() and sample()
restate the reference's NBGetRays / get_near_far / sample_rays; tests/golden/make_golden_bodydata.py asserts element by element that they
round to the reference's own fp32 outputs."""
import numpy as np

FACES = ((0, 1, 3, 2, 0), (4, 5, 7, 6, 5), (0, 1, 5, 4, 0), (2, 3, 7, 6, 2), (0, 2, 6, 4, 0), (1, 3, 7, 5, 1))
ROUNDS = 8
# roundings between a source byte and a prepared pixel: byte / 255 (1), the weights ax, 1 - ax, ay, 1 - ay (4), two row blends (3 each, the
# larger counted once per tap pair: 3), the column blend (3), s s - 1 additions and the division of the block mean (4 at s = 2): 15, stated 16
PREPARE_DEPTH = 16


def prepare(img8, msk8, K, D, s, white_bkgd):
    """(img [H,W,3] float64, msk [H,W] uint8) of include/xrnerf_mi355_bodydata.h's xr_body_prepare, every product and sum in float64"""
    img8, msk8 = np.asarray(img8), np.asarray(msk8)
    Hs, Ws = img8.shape[:2]
    Hm, Wm = msk8.shape
    src = img8.astype(np.float64) / 255.0
    vv, uu = np.meshgrid(np.arange(Hs), np.arange(Ws), indexing='ij')
    msrc = lambda y, x: msk8[(y * Hm) // Hs, (x * Wm) // Ws] != 0
    D = np.asarray(D, np.float64)
    if not D.any():
        und, mund = src, msrc(vv, uu)
    else:
        fx, fy, cx, cy = K[0][0], K[1][1], K[0][2], K[1][2]
        k1, k2, p1, p2, k3 = D
        x, y = (uu - cx) / fx, (vv - cy) / fy
        r2 = x * x + y * y
        kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = (x * kr + p1 * (2.0 * x * y)) + p2 * (r2 + 2.0 * x * x)
        yd = (y * kr + p1 * (r2 + 2.0 * y * y)) + p2 * (2.0 * x * y)
        us, vs = fx * xd + cx, fy * yd + cy
        und, mund = np.zeros((Hs, Ws, 3)), np.zeros((Hs, Ws), bool)
        tap = lambda yy, xx: src[yy, xx] if 0 <= yy < Hs and 0 <= xx < Ws else np.zeros(3)
        for v in range(Hs):
            for u in range(Ws):
                a, b = us[v, u], vs[v, u]
                if not (a > -2.0 and a < Ws + 1.0 and b > -2.0 and b < Hs + 1.0):
                    continue
                x0, y0 = int(np.floor(a)), int(np.floor(b))
                ax, ay = a - x0, b - y0
                top = tap(y0, x0) * (1 - ax) + tap(y0, x0 + 1) * ax
                bot = tap(y0 + 1, x0) * (1 - ax) + tap(y0 + 1, x0 + 1) * ax
                und[v, u] = top * (1 - ay) + bot * ay
                xn, yn = int(np.floor(a + 0.5)), int(np.floor(b + 0.5))
                mund[v, u] = 0 <= xn < Ws and 0 <= yn < Hs and bool(msrc(yn, xn))
    H, W = Hs // s, Ws // s
    img = und.reshape(H, s, W, s, 3).transpose(0, 2, 1, 3, 4).reshape(H, W, s * s, 3).sum(2) / float(s * s) if s > 1 else und.copy()
    msk = mund[::s, ::s].astype(np.uint8)
    img[msk == 0] = 1.0 if white_bkgd else 0.0
    return img, msk


def fill_one(pts, H, W):
    """one closed polygon over integer vertices (x, y), the last joined to the first, Python integers: a pixel is set when it lies on an
    edge or inside by the even-odd rule -> bool [H,W]"""
    pts = [(int(x), int(y)) for x, y in np.asarray(pts)]
    out = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            inside = on_edge = False
            for e in range(len(pts)):
                (ax, ay), (bx, by) = pts[e], pts[(e + 1) % len(pts)]
                cross = (bx - ax) * (y - ay) - (x - ax) * (by - ay)
                if cross == 0 and min(ax, bx) <= x <= max(ax, bx) and min(ay, by) <= y <= max(ay, by):
                    on_edge = True
                if (ay > y) != (by > y) and ((cross > 0) == (by > ay)):
                    inside = not inside
            out[y, x] = inside or on_edge
    return out


def fill(corners, H, W):
    """the six polygons of get_bound_2d_mask over the eight integer corners -> uint8 [H,W]"""
    c = np.asarray(corners)
    out = np.zeros((H, W), bool)
    for face in FACES:
        out |= fill_one(c[list(face)], H, W)
    return out.astype(np.uint8)


def lists(msk, corners):
    """(bound_list, body_list): flat pixel indices in argwhere order"""
    H, W = msk.shape
    b = fill(corners, H, W)
    return np.flatnonzero(b.reshape(-1) == 1).astype(np.int32), np.flatnonzero((msk * b).reshape(-1) != 0).astype(np.int32)


def camera(K, R, T):
    K, R, T = np.asarray(K, np.float64), np.asarray(R, np.float64), np.asarray(T, np.float64).reshape(3, 1)
    return np.linalg.inv(K), R, T.ravel(), -np.dot(R.T, T).ravel()


def rays(K, R, T, pix, W):
    """normalised float64 directions of flat pixels `pix`, in the kernel's order of operations -> (rays_o [3], d [n,3])"""
    Ki, R, T, o = camera(K, R, T)
    pix = np.asarray(pix, np.int64)
    x, y = (pix % W).astype(np.float64), (pix // W).astype(np.float64)
    pc = [((x * Ki[r, 0] + y * Ki[r, 1]) + Ki[r, 2]) - T[r] for r in range(3)]
    d = np.stack([((pc[0] * R[0, k] + pc[1] * R[1, k]) + pc[2] * R[2, k]) - o[k] for k in range(3)], -1)
    n = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return o, d / n[:, None]


def box(bounds, o, d, dtype=np.float64):
    """get_near_far in `dtype`: (near, far, hit) for every ray, un-compacted"""
    t = dtype
    bounds, o, d = np.asarray(bounds).astype(t), np.asarray(o).astype(t), np.asarray(d).astype(t)
    nd = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    v = d / nd[:, None]
    v = np.where((v < t(1e-5)) & (v > t(-1e-10)), t(1e-5), v)
    v = np.where((v > t(-1e-5)) & (v < t(1e-10)), t(-1e-5), v)
    tmin, tmax = (bounds[0] - o) / v, (bounds[1] - o) / v
    near, far = np.minimum(tmin, tmax).max(-1), np.maximum(tmin, tmax).min(-1)
    return near / nd, far / nd, near < far


def clamp_margin(d):
    """the smallest distance of a viewdir component to one of the four clamp thresholds"""
    v = np.asarray(d, np.float64)
    return min(np.abs(v - th).min() for th in (1e-5, -1e-10, -1e-5, 1e-10))


def sample(K, R, T, W, bounds, img, bound_list, body_list, draws, sel_n):
    """xr_body_sample: dict of fp32 arrays (NaN tail when short) and the number of rounds used, the survivors per round"""
    out = {k: [] for k in ('rays_o', 'rays_d', 'near', 'far', 'target_s')}
    count, rounds, per_round = 0, 0, []
    img = np.asarray(img).reshape(-1, 3)
    while count < sel_n and rounds < ROUNDS:
        rem = sel_n - count
        n_body = rem // 2
        pix = np.concatenate([body_list[draws[rounds, :n_body] % len(body_list)], bound_list[draws[rounds, n_body:rem] % len(bound_list)]])
        o, d = rays(K, R, T, pix, W)
        near, far, hit = box(bounds, o[None], d)
        out['rays_o'].append(np.broadcast_to(o, d.shape)[hit])
        out['rays_d'].append(d[hit])
        out['near'].append(near[hit][:, None])
        out['far'].append(far[hit][:, None])
        out['target_s'].append(img[pix[hit]])
        count += int(hit.sum())
        per_round.append(int(hit.sum()))
        rounds += 1
    res = {}
    for k, v in out.items():
        a = np.concatenate(v, 0).astype(np.float32)
        res[k] = np.concatenate([a, np.full((sel_n - count, a.shape[1]), np.nan, np.float32)], 0)
    return res, rounds, per_round


def frame(K, R, T, H, W, bounds, img=None):
    """select_all_rays: rays in float64 rounded to fp32, then the box in fp32"""
    o, d = rays(K, R, T, np.arange(H * W), W)
    o32, d32 = np.broadcast_to(o, d.shape).astype(np.float32), d.astype(np.float32)
    near, far, hit = box(np.asarray(bounds, np.float32), o32[:1], d32, np.float32)
    res = {'rays_o': o32[hit], 'rays_d': d32[hit], 'near': near[hit][:, None], 'far': far[hit][:, None], 'mask_at_box': hit}
    if img is not None:
        res['target_s'] = np.asarray(img, np.float32).reshape(-1, 3)[hit]
    return res
