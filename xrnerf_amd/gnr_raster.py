"""GNR's body depth maps: the z-buffer rasteriser and vertex visibility of the reference's extensions/mesh_grid
(render.h / render.cpp, `_render.forward`) on the kernels of csrc/xr_gnr_raster.hip.

    render_forward   the reference's `_render.forward(verts, tri, h, w, persp, eps)` -> (index [h,w] int64, coeff [h,w,3], visual [n] bool)
    rasterize        the same over [N,3] or [V,N,3] vertices, with the z-buffer as a fourth value (0 where empty) and `double_face`
    projected_vertices, depth_maps   a body mesh -> the [V,1,H,W] camera-depth maps inside_pts_vh samples (smpl['depth'], 'scan_depth'):
                     the vertices go through gnr_render.perspective() -- lens distortion exactly as the hull applies it to a sample --
                     are shifted by -0.5 pixel (the hull's nearest rule, pixel i = rint(px - 0.5), puts the centre of pixel i at
                     px = i + 0.5; the rasteriser samples at integers) and handed over as (px z, py z, z)

Device tensors run the kernels; host tensors take the tensor-op path -- per face, vectorised over its box, the same fp32 operations in
the same order -- which is also the timing baseline of tools/microbench_gnr_raster.py.  No gradient flows through any of it: the maps
are inputs."""
import torch

from . import _lib, ops

TENSOR_OPS_STAGES = False        # measurements only: take the tensor-op path on device tensors too
MAX_SIDE = ops.GNR_RASTER_MAX_SIDE
FLT_MAX = 3.4028234663852886e38


def _use_kernels(t):
    """device tensors run the kernels; a library handle without the entry points is an error, not a quiet tensor-op run"""
    if not ops._on_device(t) or TENSOR_OPS_STAGES:
        return False
    if not ops.gnr_raster_kernels_available():
        raise _lib.XrError('the loaded library has no xr_gnr_raster entry points (stale build?)')
    return True


# ---------------------------------------------------------------- the reference's lines as tensor ops (host path, timing baseline)
def _setup(v, tri, h, w, persp, eps, double_face):
    """process_one_tri and the lines of zbuffer_forward in front of it for every face at once: elementwise fp32, so the same bits as
    face by face -> (draws [F] bool, type [F], box [F,4] = x0, x1, y0, y1, A [F,9], vz [F,3])"""
    c = v[tri]
    vx, vy, vz = c[..., 0], c[..., 1], c[..., 2]
    draws = torch.ones(tri.shape[0], dtype=torch.bool, device=v.device)
    if persp:
        draws = ~(vz <= eps).any(1)
        vx, vy = vx / vz, vy / vz
    umin, umax, vmin, vmax = torch.floor(vx.min(1)[0]), torch.ceil(vx.max(1)[0]), torch.floor(vy.min(1)[0]), torch.ceil(vy.max(1)[0])
    zero = torch.zeros_like(umin)
    bx0, bx1 = torch.where(umin < 0, zero, umin), torch.where(umax >= float(w), zero + float(w - 1), umax)
    by0, by1 = torch.where(vmin < 0, zero, vmin), torch.where(vmax >= float(h), zero + float(h - 1), vmax)
    draws = draws & (bx1 >= bx0) & (by1 >= by0)
    x0, x1, x2, y0, y1, y2 = vx[:, 0], vx[:, 1], vx[:, 2], vy[:, 0], vy[:, 1], vy[:, 2]
    a6, a7, a8 = x1 * y2 - x2 * y1, x2 * y0 - x0 * y2, x0 * y1 - x1 * y0
    det = a6 + a7 + a8
    if not double_face:
        draws = draws & ~(det > eps)
    rows = [torch.stack([y1 - y2, y2 - y0, y0 - y1], 1), torch.stack([x2 - x1, x0 - x2, x1 - x0], 1), torch.stack([a6, a7, a8], 1)]
    l2 = rows[0] * rows[0] + rows[1] * rows[1]
    i = torch.where(l2[:, 0] > l2[:, 1], 0, 1)
    i = torch.where(l2.gather(1, i[:, None])[:, 0] > l2[:, 2], i, 2)
    j = (i + 1) % 3
    k = (j + 1) % 3
    l2i = l2.gather(1, i[:, None])[:, 0]
    flat = (det <= eps) & (det >= -eps)
    line = flat & (l2i > eps * eps)
    point = flat & ~line
    at = lambda t, q: t.gather(1, q[:, None])[:, 0]
    xi, yi, xj, yj, xk, yk = at(vx, i), at(vy, i), at(vx, j), at(vy, j), at(vx, k), at(vy, k)
    ln = torch.sqrt(l2i)
    ak = [(xk - xj) / l2i, (yk - yj) / l2i, (xj * (xj - xk) + yj * (yj - yk)) / l2i]
    aj = [-ak[0], -ak[1], (xk * (xk - xj) + yk * (yk - yj)) / l2i]
    ai = [(yj - yk) / ln, (xk - xj) / ln, (xj * yk - xk * yj) / ln]
    A = []
    for r in range(3):
        lr = torch.zeros_like(rows[r]).scatter(1, i[:, None], ai[r][:, None]).scatter(1, j[:, None], aj[r][:, None]).scatter(1, k[:, None], ak[r][:, None])
        pr = rows[r]
        if r == 0:
            pr = torch.stack([xi, yi, rows[0][:, 2]], 1)
        A.append(torch.where(line[:, None], lr, torch.where(point[:, None], pr, rows[r] / det[:, None])))
    typ = torch.where(line, (1 << j) + (1 << k), torch.where(point, 1 << i, 7))
    box = torch.stack([bx0, bx1, by0, by1], 1)
    box = torch.where(draws[:, None], box, torch.zeros_like(box)).to(torch.int64)
    return draws, typ, box, torch.cat(A, 1), vz


def _coeff(A, t, u, v, eps):
    """normalize_coeff for one face over tensors of sample points -> (inside, [c0, c1, c2])"""
    if t in (7, 3, 5, 6):
        c = [A[q] * u + A[3 + q] * v + A[6 + q] for q in range(3)]
        if t == 7:
            return (c[0] >= -eps) & (c[1] >= -eps) & (c[2] >= -eps), c
        i = (7 - t) // 2
        j, k = (i + 1) % 3, (i + 2) % 3
        on = ~(c[i] * c[i] > eps * eps)
        c[i] = torch.zeros_like(c[i])
        return on & (c[j] >= -eps) & (c[k] >= -eps), c
    i = t // 2
    cj, ck = u - A[0], v - A[1]
    d = cj * cj + ck * ck
    c = [torch.ones_like(d) if q == i else torch.zeros_like(d) for q in range(3)]
    return ~(d > eps * eps), c


def _depth(c, vz, persp, eps):
    """the lines behind normalize_coeff -> (go_on, c, z); go_on False is the reference's `continue`.  The perspective z is a double
    division rounded to float, the orthographic z takes c[2] twice"""
    if persp:
        c = [c[q] / vz[q] for q in range(3)]
        s = c[0] + c[1] + c[2]
        return ~(s <= eps), [cq / s for cq in c], (1.0 / s.double()).float()
    z = c[0] * vz[0] + c[2] * vz[1] + c[2] * vz[2]
    return torch.ones_like(z, dtype=torch.bool), c, z


def _rasterize_view(v, tri, ok, h, w, persp, eps, double_face):
    dev, n = v.device, v.shape[0]
    index = torch.full((h, w), -1, dtype=torch.int64, device=dev)
    coeff = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    zbuf = torch.full((h, w), FLT_MAX, dtype=torch.float32, device=dev)
    pu, pv, pz = v[:, 0], v[:, 1], v[:, 2]
    vis = torch.ones(n, dtype=torch.bool, device=dev)
    if persp:
        vis = ~(pz <= eps)
        pu, pv = pu / pz, pv / pz
    fx, fy = torch.floor(pu), torch.floor(pv)
    vis = vis & (fx >= 0) & (fy >= 0) & (fx < float(w)) & (fy < float(h))
    ix, iy = torch.where(vis, fx, torch.zeros_like(fx)).long(), torch.where(vis, fy, torch.zeros_like(fy)).long()
    on_image = vis.clone()
    if tri.shape[0] == 0:
        return index, coeff, vis, zbuf * 0
    draws, typ, box, A, vz = _setup(v, tri, h, w, persp, eps, double_face)
    draws_h, typ_h, box_h = (draws & ok).tolist(), typ.tolist(), box.tolist()
    ids = torch.arange(n, device=dev)
    for f in range(tri.shape[0]):
        if not draws_h[f]:
            continue
        x0, x1, y0, y1 = box_h[f]
        t, Af, zf = typ_h[f], A[f], vz[f]
        xs = torch.arange(x0, x1 + 1, dtype=torch.float32, device=dev)[None, :]
        ys = torch.arange(y0, y1 + 1, dtype=torch.float32, device=dev)[:, None]
        inside, c = _coeff(Af, t, xs, ys, eps)
        go, c, z = _depth(c, zf, persp, eps)
        zb = zbuf[y0:y1 + 1, x0:x1 + 1]
        win = inside & go & (zb > z)
        zb.copy_(torch.where(win, z, zb))
        ib = index[y0:y1 + 1, x0:x1 + 1]
        ib.copy_(torch.where(win, torch.full_like(ib, f), ib))
        cb = coeff[y0:y1 + 1, x0:x1 + 1]
        cb.copy_(torch.where(win[..., None], torch.stack([cq.expand(win.shape) for cq in c], -1), cb))
        # the pixel's vertices: the ones whose pixel lies in the box, except the corners and -- the reference's `continue` -- the ones
        # at a pixel that is inside the face with a coefficient sum <= eps
        m = on_image & (ix >= x0) & (ix <= x1) & (iy >= y0) & (iy <= y1) & (ids != tri[f, 0]) & (ids != tri[f, 1]) & (ids != tri[f, 2])
        m = m & ~(inside & ~go).expand(win.shape)[(iy - y0).clamp(0, y1 - y0), (ix - x0).clamp(0, x1 - x0)]
        inside_v, cv = _coeff(Af, t, pu, pv, eps)
        go_v, cv, z_v = _depth(cv, zf, persp, eps)
        vis = vis & ~(m & inside_v & go_v & (z_v <= pz))
    return index, coeff, vis, torch.where(index >= 0, zbuf, torch.zeros_like(zbuf))


def rasterize_tensor_ops(verts, tri, h, w, persp, eps=1e-6, double_face=False):
    """rasterize() as tensor ops, on whatever device the tensors live: verts [V,N,3] -> (index [V,h,w], coeff [V,h,w,3],
    visual [V,N], depth [V,h,w])"""
    e = torch.tensor(eps, dtype=torch.float32, device=verts.device)
    tri = tri.long()
    ok = ((tri >= 0) & (tri < verts.shape[1])).all(1)            # a face with an index outside the mesh is dropped, as in the kernel
    tri = torch.where(ok[:, None], tri, torch.zeros_like(tri))
    out = [_rasterize_view(v, tri, ok, h, w, bool(persp), e, bool(double_face)) for v in verts]
    return tuple(torch.stack([o[q] for o in out]) for q in range(4))


# ---------------------------------------------------------------- public interface
def _checked(verts, tri, h, w, eps):
    if not isinstance(verts, torch.Tensor) or verts.dtype != torch.float32:
        raise _lib.XrError('rasterize takes float32 vertices (got %s)' % getattr(verts, 'dtype', type(verts)))
    if not isinstance(tri, torch.Tensor) or tri.dtype not in (torch.int32, torch.int64):
        raise _lib.XrError('rasterize takes int32 or int64 faces (got %s)' % getattr(tri, 'dtype', type(tri)))
    if verts.dim() not in (2, 3) or verts.shape[-1] != 3 or tri.dim() != 2 or tri.shape[-1] != 3:
        raise _lib.XrError('rasterize: verts [N,3] or [V,N,3], faces [F,3]')
    h, w = int(h), int(w)
    batched = verts.dim() == 3
    v3 = verts if batched else verts[None]
    V, N = v3.shape[0], v3.shape[1]
    if not float(eps) >= 0.0:
        raise _lib.XrError('rasterize: eps must not be negative (got %r)' % (eps,))
    if V < 1 or N < 1 or h < 1 or w < 1 or h > MAX_SIDE or w > MAX_SIDE or V * h * w >= 2 ** 31 - 1 or V * N > 2 ** 31 - 1 or tri.shape[0] >= 2 ** 32 - 1:
        raise _lib.XrError('rasterize: refused sizes (1 <= h, w <= %d; V h w and V N within int32; F < 2^32 - 1): V %d N %d F %d h %d w %d'
                           % (MAX_SIDE, V, N, tri.shape[0], h, w))
    return v3.contiguous(), h, w, batched


def rasterize(verts, tri, h, w, persp, eps=1e-6, double_face=False):
    """verts [N,3] or [V,N,3] float32 as the reference's render_forward takes them (with `persp`, x and y are divided by z inside; a
    vertex or face with z <= eps is dropped), tri [F,3] int32 / int64 shared by the views -> (index int64, -1 where empty; coeff;
    visual bool; depth = the z-buffer, 0 where empty), each with a leading view axis when verts has one.  A face with det > eps is
    culled unless double_face."""
    v3, h, w, batched = _checked(verts, tri, h, w, eps)
    with torch.no_grad():
        if _use_kernels(v3):
            out = ops.gnr_raster_forward(v3, tri.to(torch.int32).contiguous(), h, w, persp, double_face, eps)
        else:
            out = rasterize_tensor_ops(v3, tri, h, w, persp, eps, double_face)
    return out if batched else tuple(o[0] for o in out)


def render_forward(verts, tri, h, w, persp, eps=1e-6):
    """drop-in for the reference's extensions/mesh_grid `_render.forward`: verts [n,3] float32, tri [f,3] int64 ->
    (index [h,w] int64, coeff [h,w,3] float32, visual [n] bool)"""
    if verts.dim() != 2:
        raise _lib.XrError('render_forward takes [n,3] vertices (rasterize() takes views)')
    return rasterize(verts, tri, h, w, persp, eps)[:3]


def projected_vertices(verts, calibs, persps):
    """verts [N,3] (world), calibs [V,4,4], persps [V,cols] -> [V,N,3] = (px z, py z, z) with (px, py) the pixel coordinates of
    gnr_render.perspective() shifted by -0.5: what depth_maps hands to the rasteriser"""
    from .gnr_render import perspective
    V = calibs.shape[0]
    xyz = perspective(verts.reshape(-1, 3).permute(1, 0)[None].expand(V, -1, -1), calibs, persps)
    z = xyz[:, 2]
    return torch.stack([(xyz[:, 0] - 0.5) * z, (xyz[:, 1] - 0.5) * z, z], -1).contiguous()


def depth_maps(verts, faces, calibs, persps, height, width, double_face=True):
    """camera-depth maps of a mesh in every view -> [V,1,height,width] float32, 0 where no face covers the pixel: the layout
    inside_pts_vh samples.  double_face: a body mesh whose winding is not known (or mirrored) still gives its nearest surface."""
    with torch.no_grad():
        pv = projected_vertices(verts.to(torch.float32), calibs.to(torch.float32), persps.to(torch.float32))
        return rasterize(pv, faces, int(height), int(width), True, 1e-6, double_face)[3][:, None]
