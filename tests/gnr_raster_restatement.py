"""The z-buffer rasteriser of the reference's extensions/mesh_grid (render.h: zbuffer_forward, process_one_tri, normalize_coeff) as a
SERIAL float32 numpy restatement: one face after the other, one pixel after the other, every operation a np.float32 scalar operation in
the order written there.  It is the specification of xrnerf_amd/csrc/xr_gnr_raster.hip away from the fixture
(tests/golden/ref_gnr_raster.npz, which it equals bit for bit) -- nothing here is shared with the package.

Quirks kept: the perspective z is a double division rounded to float; the orthographic z takes c[2] twice; a perspective pixel whose
coefficient sum is <= eps `continue`s past the pixel's vertex list; only `zbuf > z` wins, so the lowest face wins a tie and FLT_MAX
never wins; orthographic vertices and faces are not tested against eps."""
import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def process_one_tri(v, w, h, eps, double_face=False):
    """v: 9 np.float32 (already divided by z with persp) -> (type, bbox, Ainv); type 0 = draws nothing (Ainv = 'culled' where det > eps did it)"""
    umin = umax = v[0]
    vmin = vmax = v[1]
    for i in (1, 2):
        if umin > v[3 * i]:
            umin = v[3 * i]
        elif umax < v[3 * i]:
            umax = v[3 * i]
        if vmin > v[3 * i + 1]:
            vmin = v[3 * i + 1]
        elif vmax < v[3 * i + 1]:
            vmax = v[3 * i + 1]
    umin, umax, vmin, vmax = np.floor(umin), np.ceil(umax), np.floor(vmin), np.ceil(vmax)
    b = [f32(0) if umin < 0 else umin, f32(w - 1) if umax >= f32(w) else umax, f32(0) if vmin < 0 else vmin, f32(h - 1) if vmax >= f32(h) else vmax]
    if not (b[1] >= b[0]) or not (b[3] >= b[2]):
        return 0, None, None
    bbox = [int(x) for x in b]
    A = [f32(0)] * 9
    A[6] = v[3] * v[7] - v[6] * v[4]
    A[7] = v[6] * v[1] - v[0] * v[7]
    A[8] = v[0] * v[4] - v[3] * v[1]
    det = A[6] + A[7] + A[8]
    if not double_face and det > eps:
        return 0, None, 'culled'
    A[0] = v[4] - v[7]
    A[1] = v[7] - v[1]
    A[2] = v[1] - v[4]
    A[3] = v[6] - v[3]
    A[4] = v[0] - v[6]
    A[5] = v[3] - v[0]
    if det <= eps and det >= -eps:
        l2 = [A[0] * A[0] + A[3] * A[3], A[1] * A[1] + A[4] * A[4], A[2] * A[2] + A[5] * A[5]]
        i = 0 if l2[0] > l2[1] else 1
        i = i if l2[i] > l2[2] else 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        if l2[i] > eps * eps:
            t = (1 << j) + (1 << k)
            A[k] = (v[3 * k] - v[3 * j]) / l2[i]
            A[j] = -A[k]
            A[k + 3] = (v[3 * k + 1] - v[3 * j + 1]) / l2[i]
            A[j + 3] = -A[k + 3]
            A[j + 6] = (v[3 * k] * (v[3 * k] - v[3 * j]) + v[3 * k + 1] * (v[3 * k + 1] - v[3 * j + 1])) / l2[i]
            A[k + 6] = (v[3 * j] * (v[3 * j] - v[3 * k]) + v[3 * j + 1] * (v[3 * j + 1] - v[3 * k + 1])) / l2[i]
            ln = np.sqrt(l2[i])
            A[i] = (v[3 * j + 1] - v[3 * k + 1]) / ln
            A[i + 3] = (v[3 * k] - v[3 * j]) / ln
            A[i + 6] = (v[3 * j] * v[3 * k + 1] - v[3 * k] * v[3 * j + 1]) / ln
        else:
            t = 1 << i
            A[0] = v[3 * i]
            A[1] = v[3 * i + 1]
    else:
        t = 7
        A = [a / det for a in A]
    return t, bbox, A


def normalize_coeff(u, v, A, t, eps):
    """-> (inside, [c0, c1, c2])"""
    if t in (7, 3, 5, 6):
        c = [A[0] * u + A[3] * v + A[6], A[1] * u + A[4] * v + A[7], A[2] * u + A[5] * v + A[8]]
        if t == 7:
            return bool(c[0] >= -eps and c[1] >= -eps and c[2] >= -eps), c
        i = (7 - t) // 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        if c[i] * c[i] > eps * eps:
            return False, c
        c[i] = f32(0)
        return bool(c[j] >= -eps and c[k] >= -eps), c
    if t in (1, 2, 4):
        i = t // 2
        cj, ck = u - A[0], v - A[1]
        if cj * cj + ck * ck > eps * eps:
            return False, None
        c = [f32(0)] * 3
        c[i] = f32(1)
        return True, c
    return False, None


def _depth(c, vz, persp, eps):
    """the lines behind a successful normalize_coeff -> (go_on, c, z): go_on False is the reference's `continue`"""
    if persp:
        c = [c[0] / vz[0], c[1] / vz[1], c[2] / vz[2]]
        z = c[0] + c[1] + c[2]
        if z <= eps:
            return False, c, z
        c = [c[0] / z, c[1] / z, c[2] / z]
        return True, c, f32(1.0 / np.float64(z))
    return True, c, c[0] * vz[0] + c[2] * vz[1] + c[2] * vz[2]


def zbuffer_forward(verts, tri, h, w, persp, eps=1e-6, double_face=False, info=None):
    """verts [N,3] float32, tri [F,3] integer -> (index [h,w] int64, coeff [h,w,3] float32, visual [N] bool, zbuf [h,w] float32 with
    FLT_MAX where empty).  `info`: a dict that receives what the fixture's maker asserts on (pixels won per type, faces culled, ties)."""
    with np.errstate(all='ignore'):
        return _zbuffer_forward(np.ascontiguousarray(verts, f32), np.asarray(tri).astype(np.int64), int(h), int(w), bool(persp), f32(eps), double_face, info)


def _zbuffer_forward(v, tri, h, w, persp, eps, double_face, info):
    n = v.shape[0]
    index = np.full((h, w), -1, np.int64)
    coeff = np.zeros((h, w, 3), f32)
    vis = np.ones(n, bool)
    zbuf = np.full((h, w), FLT_MAX, f32)
    wtype = np.zeros((h, w), np.int64)
    tie_z = np.full((h, w), np.nan, f32)
    culled, occluded = 0, set()
    ibuf = {}
    for i in range(n):
        x, y = v[i, 0], v[i, 1]
        if persp:
            if v[i, 2] <= eps:
                vis[i] = False
                continue
            x, y = x / v[i, 2], y / v[i, 2]
        x, y = np.floor(x), np.floor(y)
        if not (x >= 0 and y >= 0 and x < f32(w) and y < f32(h)):
            vis[i] = False
            continue
        ibuf.setdefault((int(x), int(y)), []).append(i)
    for f in range(tri.shape[0]):
        ids = [int(tri[f, 0]), int(tri[f, 1]), int(tri[f, 2])]
        if persp and (v[ids[0], 2] <= eps or v[ids[1], 2] <= eps or v[ids[2], 2] <= eps):
            continue
        v_ = [v[ids[q // 3], q % 3] for q in range(9)]
        if persp:
            for j in range(3):
                v_[3 * j] = v_[3 * j] / v_[3 * j + 2]
                v_[3 * j + 1] = v_[3 * j + 1] / v_[3 * j + 2]
        t, bbox, A = process_one_tri(v_, w, h, eps, double_face)
        if not t:
            culled += A == 'culled'
            continue
        vz = (v_[2], v_[5], v_[8])
        for y in range(bbox[2], bbox[3] + 1):
            for x in range(bbox[0], bbox[1] + 1):
                inside, c = normalize_coeff(f32(x), f32(y), A, t, eps)
                if inside:
                    go_on, c, z = _depth(c, vz, persp, eps)
                    if not go_on:
                        continue
                    if z == zbuf[y, x] and index[y, x] >= 0:
                        tie_z[y, x] = z
                    if zbuf[y, x] > z:
                        zbuf[y, x] = z
                        index[y, x] = f
                        coeff[y, x] = c
                        wtype[y, x] = t
                for k in ibuf.get((x, y), ()):
                    if k in ids:
                        continue
                    pu, pv = v[k, 0], v[k, 1]
                    if persp:
                        pu, pv = pu / v[k, 2], pv / v[k, 2]
                    inside, c = normalize_coeff(pu, pv, A, t, eps)
                    if inside:
                        go_on, c, z = _depth(c, vz, persp, eps)
                        if not go_on:
                            continue
                        if z <= v[k, 2]:
                            vis[k] = False
                            occluded.add(k)
    if info is not None:
        info.update(full=int((wtype == 7).sum()), line=int(np.isin(wtype, (3, 5, 6)).sum()), point=int(np.isin(wtype, (1, 2, 4)).sum()),
                    culled=int(culled), ties=int((tie_z == zbuf).sum()), hidden=len(occluded))
    return index, coeff, vis, zbuf


def depth_of(zbuf, index):
    """the package's depth output: the z-buffer, 0 where no face won"""
    return np.where(index >= 0, zbuf, f32(0)).astype(f32)
