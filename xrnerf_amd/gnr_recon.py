"""GNR's mesh reconstruction around the network (the reference's GnrRenderer.reconstruct / octree_reconstruct, gnr_render.py:643-815),
on the kernels of csrc/xr_gnr_recon.hip:

    grid_hull         the N^3 grid points (np.linspace, / spatial_freq + center in float64, rounded once) tested against the dilated
                      masks of every source view -> one state byte per point; no coordinate array exists
    octree            the coarse-to-fine levels: select the level's unprocessed lattice points in C order, evaluate them through a
                      callback, scatter, then skip-and-fill the cells whose 8 corners agree to 0.01 (last skipped cell wins)
    marching_cubes    iso-surface with welded vertices, outward normals and consistently wound triangles
    to_world          the reference's vertex transform (its N-for-N-1 kept), float64
    laplacian_smooth  trimesh's documented filter_laplacian defaults (lamb 0.5, volume constraint), float64
    point_rows        per vertex the normalised projections and make_att_input's directions for the colour pass

Device tensors run the kernels; host tensors take the tensor-op path (also the timing baseline of tools/microbench_gnr_recon.py).
DESIGN.md section 17."""
import os
import re

import numpy as np
import torch

from . import ops

TENSOR_OPS_STAGES = False        # measurements only: every stage takes its tensor-op path on device tensors too


def _use_kernels(t):
    """device tensors run the kernels; a library handle without the entry points is an error, not a quiet tensor-op run"""
    if not ops._on_device(t) or TENSOR_OPS_STAGES:
        return False
    if not ops.gnr_recon_kernels_available():
        from . import _lib
        raise _lib.XrError('the loaded library has no xr_gnr_recon entry points (stale build?)')
    return True


class Grid:
    """N points per axis between bb_min and bb_max (np.linspace), mapped to the body's frame by / spatial_freq + center; or the
    caller's own `coords` [N,N,N,3]"""

    def __init__(self, N, bb_min, bb_max, spatial_freq, center, coords=None):
        self.N, self.bb_min, self.bb_max = int(N), [float(v) for v in bb_min], [float(v) for v in bb_max]
        self.spatial_freq, self.center = float(spatial_freq), center.reshape(3).float()
        self.coords = None if coords is None else coords.reshape(-1, 3).float().contiguous()
        self._args = None

    def args(self):
        if self._args is None:
            self._args = ops.gnr_recon_grid(self.N, self.bb_min, self.bb_max, self.spatial_freq, self.center.contiguous(), self.coords)
        return self._args

    def points(self, flat=None):
        """tensor ops: the points [N^3,3] (or those at `flat`), bit for bit numpy's expression"""
        dev = self.center.device
        if self.coords is not None:
            return self.coords if flat is None else self.coords[flat.long()]
        N = self.N
        lin = []
        for a in range(3):
            step = (self.bb_max[a] - self.bb_min[a]) / (N - 1)
            y = torch.arange(N, dtype=torch.float64, device=dev) * step + self.bb_min[a]
            y[-1] = self.bb_max[a]
            lin.append(y / self.spatial_freq + self.center[a].double())
        if flat is None:
            g = torch.stack(torch.meshgrid(lin[0], lin[1], lin[2], indexing='ij'), -1).reshape(-1, 3)
        else:
            f = flat.long()
            g = torch.stack([lin[0][f // (N * N)], lin[1][f // N % N], lin[2][f % N]], -1)
        return g.float()


def dilate_masks(masks):
    """the reference's 5 x 5 box dilation of the source masks [V,1,H,W] (a tiny map: a tensor op)"""
    import torch.nn.functional as F
    m = masks.reshape(-1, 1, masks.shape[-2], masks.shape[-1]).float()
    return torch.clamp(F.conv2d(m, torch.ones((1, 1, 5, 5), dtype=torch.float32, device=m.device), padding=(2, 2)), 0, 1)


def _project(pts, calibs, persps, width, height):
    from .gnr_render import perspective
    V = calibs.shape[0]
    xyz = perspective(pts.permute(1, 0)[None].expand(V, -1, -1), calibs, persps)
    return xyz[:, :2, :] / torch.tensor([[[width], [height]]], dtype=xyz.dtype, device=xyz.device) * 2 - 1


def _hull_flags(pts, calibs, persps, masks, width, height):
    from .gnr_render import index
    V = calibs.shape[0]
    xy = _project(pts, calibs, persps, width, height)
    m = masks.reshape(V, 1, masks.shape[-2], masks.shape[-1])
    return (index(m, torch.nan_to_num(xy), 'nearest').squeeze(1) > 0).all(0) & torch.isfinite(xy).all(1).all(0), xy


def grid_hull(grid, calibs, persps, masks, width, height, chunk=1 << 20):
    """masks: the DILATED masks [V,1,H,W] -> state [N,N,N] uint8: 1 = unprocessed (inside the hull, all indices below N - 1), 0 = processed"""
    N = grid.N
    if _use_kernels(calibs):
        return ops.gnr_recon_hull(grid.args(), calibs, persps, masks, width, height)
    dev = calibs.device
    state = torch.zeros((N, N, N), dtype=torch.uint8, device=dev)
    state[:-1, :-1, :-1] = 1
    flat_state = state.reshape(-1)
    for i in range(0, N ** 3, chunk):
        flat = torch.arange(i, min(i + chunk, N ** 3), device=dev)
        inside, _ = _hull_flags(grid.points(flat), calibs, persps, masks, width, height)
        flat_state[i:i + chunk] *= inside.to(torch.uint8)
    return state


def level_select(grid, reso, state, calibs, persps, width, height):
    """-> (flat [M] int32, pts [M,3], xy [M,V,2]) of the points whose indices are multiples of reso and whose state is 1, in C order"""
    if _use_kernels(state):
        return ops.gnr_recon_select(grid.args(), reso, state, calibs, persps, width, height)
    lattice = torch.zeros_like(state, dtype=torch.bool)
    lattice[::reso, ::reso, ::reso] = True
    flat = torch.nonzero((lattice & (state == 1)).reshape(-1)).reshape(-1)
    pts = grid.points(flat)
    xy = _project(pts, calibs, persps, width, height).permute(2, 0, 1).contiguous() if calibs is not None else None
    return flat.to(torch.int32), pts, xy


def _fold_tensor_ops(reso, vol, state):
    N = vol.shape[0]
    dev = vol.device
    g = torch.arange(0, N, reso, device=dev)
    n = g.numel() - 1
    v = vol[g][:, g][:, :, g].double()
    corners = torch.stack([v[a:a + n, b:b + n, c:c + n] for a in (0, 1) for b in (0, 1) for c in (0, 1)], 0)
    lo, hi = corners.min(0)[0], corners.max(0)[0]
    mid = g[:-1] + reso // 2
    skip = ((hi - lo) < 0.01) & (state[mid][:, mid][:, :, mid] == 1)
    fill = (0.5 * (lo + hi)).to(vol.dtype)
    P = n * reso + 1
    p = torch.arange(P, device=dev)
    hi_c = torch.clamp(p // reso, max=n - 1)
    lo_c = torch.clamp((p + reso - 1) // reso - 1, min=0)
    taken = torch.zeros((P, P, P), dtype=torch.bool, device=dev)
    sub_v, sub_s = vol[:P, :P, :P], state[:P, :P, :P]
    for cx in (hi_c, lo_c):                                        # the last covering cell in C order first
        for cy in (hi_c, lo_c):
            for cz in (hi_c, lo_c):
                s = skip[cx][:, cy][:, :, cz] & ~taken
                sub_v[s] = fill[cx][:, cy][:, :, cz][s]
                sub_s[s] = 0
                taken |= s
    return int(skip.sum())


def octree(N, reso0, state, eval_fn, select=None, gamma=None):
    """The coarse-to-fine levels reso0, reso0 // 2 .. 1 on state [N,N,N] (uint8, changed in place).  eval_fn(flat [M] int32, pts, xy) ->
    values [M]; `select(reso, state)` -> (flat, pts, xy) makes a level's test set (default: flat only, pts = xy = None).  With `gamma` the
    values go through sigmoid(gamma v).  -> (volume [N,N,N] float32, state, [M per level]).  One blocking read (M) per level."""
    dev = state.device
    vol = torch.zeros((N, N, N), dtype=torch.float32, device=dev)
    kernels = _use_kernels(state)
    if select is None:
        bare = Grid(N, [0, 0, 0], [N - 1] * 3, 1.0, torch.zeros(3, device=dev))

        def select(reso, st):
            if not kernels:
                return level_select(bare, reso, st, None, None, 1.0, 1.0)[0], None, None
            eye = torch.eye(4, device=dev)[None].contiguous()
            return ops.gnr_recon_select(bare.args(), reso, st, eye, torch.ones((1, 4), device=dev), 1.0, 1.0)[0], None, None
    counts = []
    reso = int(reso0)
    while reso > 0:
        flat, pts, xy = select(reso, state)
        counts.append(int(flat.shape[0]))
        if flat.shape[0] == 0:
            break
        values = eval_fn(flat, pts, xy).reshape(-1).float()
        if kernels:
            ops.gnr_recon_scatter(flat, values.contiguous(), vol, state, gamma)
        else:
            vol.reshape(-1)[flat.long()] = torch.sigmoid(values * gamma) if gamma is not None else values
            state.reshape(-1)[flat.long()] = 0
        if reso <= 1:
            break
        if kernels:
            ops.gnr_recon_fold(reso, vol, state)
        else:
            _fold_tensor_ops(reso, vol, state)
        reso //= 2
    return vol, state, counts


# ---------------------------------------------------------------- iso-surface
_TABLE = None


def cube_table():
    """the 256 x 16 triangle table, read from the kernel source: ONE typed-in copy"""
    global _TABLE
    if _TABLE is None:
        src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc', 'xr_gnr_recon.hip')).read()
        body = src[src.index('GC_TRI[256][16] = {'):]
        body = body[body.index('{') + 1:body.index('};')]
        rows = [[int(v) for v in r.split(',')] for r in re.findall(r'\{([^{}]*)\}', body)]
        assert len(rows) == 256 and all(len(r) == 16 for r in rows)
        _TABLE = torch.tensor(rows, dtype=torch.int64)
    return _TABLE


def _edge_offsets():
    off = torch.zeros((12, 3), dtype=torch.int64)
    for e in range(12):
        axis, u, v = e // 4, e & 1, (e >> 1) & 1
        b, c = [a for a in range(3) if a != axis]
        off[e, b], off[e, c] = u, v
    return off


def _gradient(vol):
    g = []
    for a in range(3):
        v = vol.movedim(a, 0)
        d = torch.empty_like(v)
        d[1:-1] = (v[2:] - v[:-2]) * 0.5
        d[0], d[-1] = v[1] - v[0], v[-1] - v[-2]
        g.append(d.movedim(0, a))
    return torch.stack(g, -1)


def _surface_tensor_ops(vol, level):
    N, dev = vol.shape[0], vol.device
    inside = vol > level
    stride = (N * N, N, 1)
    cross = torch.zeros((N, N, N, 3), dtype=torch.bool, device=dev)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    slot = torch.nonzero(cross.reshape(-1)).reshape(-1)             # voxel C order, then axis order
    voxel, axis = slot // 3, slot % 3
    flat_v = vol.reshape(-1)
    other = voxel + torch.tensor(stride, device=dev)[axis]
    va, vb = flat_v[voxel], flat_v[other]
    t = (level - va) / (vb - va)
    verts = torch.stack([voxel // (N * N), voxel // N % N, voxel % N], -1).to(vol.dtype)
    verts[torch.arange(slot.numel(), device=dev), axis] += t
    grad = _gradient(vol).reshape(-1, 3)
    g = grad[voxel] + t[:, None] * (grad[other] - grad[voxel])
    normals = -g / torch.clamp(torch.norm(g, dim=-1, keepdim=True), min=1e-9)
    vid = torch.full((N ** 3 * 3,), -1, dtype=torch.int64, device=dev)
    vid[slot] = torch.arange(slot.numel(), device=dev)
    case = torch.zeros((N - 1, N - 1, N - 1), dtype=torch.int64, device=dev)
    for c in range(8):
        o = (c & 1, (c >> 1) & 1, (c >> 2) & 1)
        case += inside[o[0]:N - 1 + o[0], o[1]:N - 1 + o[1], o[2]:N - 1 + o[2]].long() << c
    table = cube_table().to(dev)
    cell = torch.nonzero(((case != 0) & (case != 255)).reshape(-1)).reshape(-1)
    M = N - 1
    ijk = torch.stack([cell // (M * M), cell // M % M, cell % M], -1)
    tri = table[case.reshape(-1)[cell]][:, :15].reshape(-1, 5, 3)   # cell C order, then table order
    valid = tri[..., 0] >= 0
    e = tri.clamp(min=0)
    q = ijk[:, None, None, :] + _edge_offsets().to(dev)[e]
    faces = vid[((q[..., 0] * N + q[..., 1]) * N + q[..., 2]) * 3 + e // 4][valid]
    return verts, faces.to(torch.int32).reshape(-1, 3), normals


def marching_cubes(volume, level):
    """volume [N,N,N]; a corner is inside when its value is > level -> (verts_idx [Nv,3], faces [T,3] int32, normals [Nv,3]): index
    coordinates, welded vertices in owner-voxel C order then axis order, triangles in cell C order then table order, normals towards
    lower values.  A volume that never crosses the level gives (0, 3) arrays."""
    if _use_kernels(volume):
        return ops.gnr_recon_surface(volume, level)
    return _surface_tensor_ops(volume, level)


def to_world(verts_idx, N, bbox, spatial_freq, center):
    """(v - N / 2) / N [512, bottom - top, 512], / spatial_freq + center in float64 -> (verts float64 [Nv,3], pts = its float32 rounding)"""
    extent = [512.0, float(bbox[1]) - float(bbox[0]), 512.0]
    if _use_kernels(verts_idx):
        return ops.gnr_recon_world(verts_idx, N, extent, spatial_freq, center.float().contiguous())
    v = (verts_idx.double() - N / 2) / N * torch.tensor([extent], dtype=torch.float64, device=verts_idx.device)
    v = v / float(spatial_freq) + center.reshape(1, 3).float().double()
    return v, v.float()


def neighbour_lists(faces, n_verts):
    """CSR lists of every vertex's edge neighbours, each once, ascending -> (rowptr [Nv+1] int32, cols int32)"""
    f = faces.long()
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    e = torch.unique(torch.cat([e, e.flip(1)], 0), dim=0)
    rowptr = torch.zeros((n_verts + 1,), dtype=torch.int64, device=faces.device)
    rowptr[1:] = torch.cumsum(torch.bincount(e[:, 0], minlength=n_verts), 0)
    return rowptr.to(torch.int32), e[:, 1].to(torch.int32).contiguous()


def _signed_volume(v, f):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return torch.sum(torch.sum(a * torch.cross(b, c, dim=-1), -1)) / 6.0


def laplacian_smooth(verts, faces, iterations, lamb=0.5):
    """trimesh.smoothing.filter_laplacian's documented defaults on float64 vertices [Nv,3]: v += lamb (mean of the edge neighbours - v),
    then every vertex is scaled about the origin by (vol0 / vol)^(1/3); `iterations` times -> a new tensor"""
    if iterations <= 0 or verts.shape[0] == 0 or faces.shape[0] == 0:
        return verts.clone()
    rowptr, cols = neighbour_lists(faces, verts.shape[0])
    if _use_kernels(verts):
        return ops.gnr_recon_smooth(verts, faces.contiguous(), rowptr, cols, iterations, lamb)
    f = faces.long()
    deg = (rowptr[1:] - rowptr[:-1]).to(verts.dtype)
    rows = torch.repeat_interleave(torch.arange(verts.shape[0], device=verts.device), (rowptr[1:] - rowptr[:-1]).long())
    v = verts.clone()
    vol0 = _signed_volume(v, f)
    for _ in range(iterations):
        mean = torch.zeros_like(v).index_add_(0, rows, v[cols.long()]) / torch.clamp(deg, min=1)[:, None]
        v = torch.where(deg[:, None] > 0, v + lamb * (mean - v), v)
        ratio = vol0 / _signed_volume(v, f)
        v = v * torch.sign(ratio) * torch.abs(ratio) ** (1.0 / 3.0)
    return v


def point_rows(pts, dirs, calibs, persps, width, height, rot=None):
    """-> (xy [n,V,2], attdirs [n,V+1,3]): the projections of the points and make_att_input's directions with query direction `dirs`"""
    from .gnr_render import att_directions
    if _use_kernels(pts):
        cam_c = torch.inverse(calibs)[:, :3, 3].contiguous()
        return ops.gnr_recon_point_rows(pts, dirs, calibs, persps, width, height, cam_c, rot)
    return _project(pts, calibs, persps, width, height).permute(2, 0, 1).contiguous(), att_directions(pts, dirs, calibs, rot)


def empty_mesh():
    return np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32)
