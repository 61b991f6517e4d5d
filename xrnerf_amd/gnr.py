"""GNR's body-shape embedding (configs/gnr/gnr_genebody.py): the reference's `extensions/mesh_grid` searcher and the embedding half of
GnrRenderer.make_nerf_input (gnr_render.py:236-281), on the kernels of csrc/xr_gnr.hip.

    MeshGridSearcher      the reference's interface (set_mesh, nearest_points, inside_mesh) and attributes (verts, faces, step, num,
                          minmax, tri_num, tri_idx); step / num / minmax come from the reference's torch lines in float32
    body_shape_embedding  [pts_nml | T-pose coordinates | reg_vecs / norm | tanh(20 sdf)] and alpha_smpl
    synthetic_mesh        a closed, deformed icosphere with posed vertices, T-pose vertices and a rotation (the fixture's mesh)

The reference's kernels are the specification, quirks included.  Device tensors run the kernels; host tensors
(or a library handle without the entry points) take the host path: numpy for the grid build and the two searches (gnr_host.py: the
kernels restated with the points side by side under masks), tensor ops for the embedding -- the same results.  GNR's renderer, image
encoder and attention heads are not here."""
import numpy as np
import torch

from . import gnr_host, ops


def _use_kernels(t):
    return ops._on_device(t) and ops.gnr_kernels_available()


def grid_geometry(verts):
    """MeshGridSearcher.set_mesh's torch lines (mesh_grid_searcher.py:15-23) in float32 -> (step 0-dim, num [4] int32, minmax [6]), HOST
    tensors.  The bounding box is taken where the vertices are (min / max are exact anywhere) and read once; the lines after it run on
    the host, so the cube root and the divisions round the same way for host and device meshes and two machines build the same grid."""
    box = torch.stack([torch.min(verts, 0)[0], torch.max(verts, 0)[0]]).cpu()
    _min, _max = box[0], box[1]
    step = (torch.cumprod(_max - _min, 0)[-1] / len(verts)) ** (1. / 3.)
    l = _max - _min
    c = (_max + _min) / 2
    l = torch.max(torch.floor(l / step), torch.zeros_like(l)) + 1
    _min_step = c - step * l / 2
    num = torch.cat([l, torch.cumprod(l, 0)[-1:]]).int()
    minmax = torch.cat([_min_step, _max])
    return step, num, minmax


def _box_cell(x, n):
    """x < 0 ? 0 : (x >= n ? n - 1 : floor(x)) on float32 x (a NaN goes to cell 0)"""
    if x < 0:
        return 0
    if x >= np.float32(n):
        return n - 1
    if x != x:
        return 0
    return int(np.floor(x))


def host_grid_build(verts, faces, step, min3, num3):
    """the grid build on the host, face by face in ascending order: what the reference's two passes give when run serially.
    -> (tri_num [cells] int32, tri_idx [total] int32, bad)"""
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    step = np.float32(step)
    mn = [np.float32(v) for v in min3]
    n = [int(v) for v in num3[:3]]
    cells = n[0] * n[1] * n[2]
    per_cell = [[] for _ in range(cells)]
    bad = False
    for f in range(faces.shape[0]):
        tri = faces[f]
        if (tri < 0).any() or (tri >= verts.shape[0]).any():
            bad = True
            continue
        lo, w = [], []
        for d in range(3):
            a = b = verts[tri[0], d]
            for j in (1, 2):
                x = verts[tri[j], d]
                if a > x:
                    a = x
                elif b < x:
                    b = x
            lo.append(_box_cell((a - mn[d]) / step, n[d]))
            w.append(_box_cell((b - mn[d]) / step, n[d]) + 1 - lo[d])
        for j in range(w[0] * w[1] * w[2]):
            ind, k = 0, j
            for d in range(3):
                if d > 0:
                    ind *= n[d]
                ind += lo[d] + k % w[d]
                k = int(float(k) / (float(w[d]) + 1e-8))          # the reference's double-precision quotient, truncated
            per_cell[ind].append(f + 1)
    counts = np.array([len(c) for c in per_cell], np.int64)
    tri_num = np.cumsum(counts).astype(np.int32)
    tri_idx = np.array([v for c in per_cell for v in c], np.int32).reshape(-1)
    return tri_num, tri_idx, bad


def host_search(fn, verts, faces, step, min3, num3, tri_num, tri_idx, points):
    """gnr_host.nearest / gnr_host.inside on tensors: numpy on the host, the results back where the points are"""
    step = float(step)
    if not (step > 0.0 and step < float('inf')):
        raise ValueError('the cell edge must be positive and finite')
    out = fn(verts.cpu().numpy(), faces.cpu().numpy(), step, min3, num3, tri_num.cpu().numpy(), tri_idx.cpu().numpy(),
             points.detach().cpu().numpy())
    if isinstance(out, tuple):
        return tuple(torch.from_numpy(o).to(points.device) for o in out)
    return torch.from_numpy(out).to(points.device)


class MeshGridSearcher:
    """the reference's extensions/mesh_grid/mesh_grid_searcher.py on this library"""

    def __init__(self, verts=None, faces=None):
        if verts is not None and faces is not None:
            self.set_mesh(verts, faces)

    def set_mesh(self, verts, faces):
        """Two blocking reads, where the reference has its two (`torch.zeros(self.num[-1])` and the extension's `.item()`): the mesh's
        bounding box (six floats), then the slot total together with the face-index check."""
        if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
            raise ValueError('verts must be float32 [V, 3]')
        faces = faces.reshape(-1, 3)
        if faces.dtype != torch.int32:
            raise ValueError('faces must be int32 [F, 3]')
        if verts.shape[0] == 0 or faces.shape[0] == 0:
            raise ValueError('the mesh has no vertices or no faces')
        self.verts, self.faces = verts.contiguous(), faces.contiguous()
        step_t, num_t, minmax_t = grid_geometry(self.verts)
        step, min3, num = float(step_t), minmax_t[:3].tolist(), num_t.tolist()
        if not (step > 0.0 and step < float('inf')) or not all(v == v for v in min3):
            raise ValueError('the mesh is flat or not finite: its bounding box gives no cell edge (step = %r)' % step)
        if min(num[:3]) < 1 or num[0] * num[1] * num[2] > ops.GNR_MAX_CELLS:
            raise ValueError('bad grid %r' % (num,))
        dev = self.verts.device
        self.step, self.num, self.minmax = step_t.to(dev), num_t.to(dev), minmax_t.to(dev)
        self._step, self._min3, self._num3 = step, min3, num[:3]
        if _use_kernels(self.verts):
            self.tri_num, self.tri_idx, bad = ops.gnr_grid_build(self.verts, self.faces, step, min3, num[:3])
        else:
            tn, ti, bad = host_grid_build(self.verts.cpu().numpy(), self.faces.cpu().numpy(), step, min3, num[:3])
            self.tri_num, self.tri_idx = torch.from_numpy(tn).to(verts.device), torch.from_numpy(ti).to(verts.device)
        if bad:
            raise ValueError('a face names a vertex outside [0, %d)' % verts.shape[0])

    def _grid(self):
        return self.verts, self.faces, self._step, self._min3, self._num3, self.tri_num, self.tri_idx

    def nearest(self, points):
        """-> (nearest_pts [N,3], nearest_faces [N] int32, coeff [N,3])"""
        points = points.to(self.verts.device).reshape(-1, 3)
        if not _use_kernels(points):
            f, p, c = host_search(gnr_host.nearest, *self._grid(), points)
        else:
            f, p, c = ops.gnr_nearest(*self._grid(), points)
        return p, f, c

    def nearest_points(self, points):
        p, f, _ = self.nearest(points)
        return p, f

    def inside_mesh(self, points):
        points = points.to(self.verts.device).reshape(-1, 3)
        if not _use_kernels(points):
            return host_search(gnr_host.inside, *self._grid(), points)
        return ops.gnr_inside(*self._grid(), points)

    def intersects_any(self, origins, directions):
        raise NotImplementedError('search_intersect is not ported: GNR never calls it')


def embedding_tensor_ops(pts, closest_pts, closest_idx, signs, smpl, mesh_param, width, use_nml, use_t_pose, use_smpl_sdf):
    """the embedding half of make_nerf_input as the reference's tensor ops (the host path, and the kernel's timing baseline)"""
    center, spatial_freq = mesh_param['center'], mesh_param['spatial_freq']
    out, alpha = [], None
    if use_nml:
        pts_nml = (pts - center) * spatial_freq / (width / 2)
        if use_smpl_sdf:
            pts_nml = pts_nml @ smpl['rot'][0]
        out.append(pts_nml)
    else:
        out.append(pts)
    if use_t_pose:
        closest_faces = smpl['faces'][closest_idx.long()]
        out.append(smpl['t_verts'][closest_faces.long()].sum(dim=1) / 3)
    if use_smpl_sdf:
        reg_vecs = pts - closest_pts
        if use_nml:
            reg_vecs = reg_vecs * spatial_freq / (width / 2)
            reg_vecs = reg_vecs @ smpl['rot'][0]
        alpha = (signs + 1) / 2
        norm = torch.norm(reg_vecs, dim=1, keepdim=True) + 1e-8
        sdf = norm * signs[..., None]
        out.append(reg_vecs / norm)
        out.append(torch.tanh(sdf * 20))
    return torch.cat(out, dim=-1), alpha


def embed(pts, closest_pts, closest_idx, signs, smpl, mesh_param, width, use_nml=True, use_t_pose=True, use_smpl_sdf=True):
    """the embedding from the searches' results: the kernel on device tensors, the tensor ops otherwise"""
    if not _use_kernels(pts):
        return embedding_tensor_ops(pts, closest_pts, closest_idx, signs, smpl, mesh_param, width, use_nml, use_t_pose, use_smpl_sdf)
    center3 = torch.as_tensor(mesh_param['center'], dtype=torch.float32, device=pts.device) if use_nml else None
    rot = smpl['rot'][0] if use_nml and use_smpl_sdf else None
    sf = mesh_param['spatial_freq']
    return ops.gnr_shape_embed(pts, closest_idx, closest_pts, signs, smpl['faces'], smpl.get('t_verts'), center3, rot,
                               float(sf), float(width / 2), use_nml, use_t_pose, use_smpl_sdf)


def body_shape_embedding(pts, smpl, mesh_param, width, use_nml=True, use_t_pose=True, use_smpl_sdf=True, searcher=None):
    """make_nerf_input with feats = None: pts [N,3]; smpl: verts [V,3], faces [F,3] int32, t_verts [V,3], rot [1,3,3]; mesh_param:
    center [3], spatial_freq -> (nerf_input [N, 3 + 3 use_t_pose + 4 use_smpl_sdf], alpha_smpl [N] or None).  No gradient flows: the
    reference makes pts_nml a fresh leaf and differentiates nothing upstream of it."""
    pts = pts.reshape(-1, 3)
    closest_pts = closest_idx = signs = None
    if use_smpl_sdf or use_t_pose:
        searcher = searcher if searcher is not None else MeshGridSearcher()
        searcher.set_mesh(smpl['verts'], smpl['faces'])
        closest_pts, closest_idx = searcher.nearest_points(pts)
        if use_smpl_sdf:
            signs = searcher.inside_mesh(pts)
    return embed(pts, closest_pts, closest_idx, signs, smpl, mesh_param, width, use_nml, use_t_pose, use_smpl_sdf)


# ---------------------------------------------------------------- the synthetic body
def icosphere(subdivisions):
    """-> (verts [V,3] float64 on the unit sphere, faces [F,3] int32): 12 + 30 (4^s - 1) / 3 ... vertices, 20 4^s faces"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v, np.float64), np.array(f, np.int32)


def synthetic_mesh(subdivisions, seed):
    """a closed body for tests and measurements: the icosphere stretched to (0.45, 0.9, 0.3) with smooth lobes (it stays star-shaped, so
    closed), posed by a rotation and an offset -> dict of float32 / int32 tensors: verts (posed) [V,3], t_verts (unposed) [V,3],
    faces [F,3], rot [1,3,3] (the pose's rotation: verts = t_verts rot^T + offset)"""
    v, f = icosphere(subdivisions)
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0, 2 * np.pi, 3)
    r = 1.0 + 0.15 * np.sin(3.0 * v[:, 0] + ph[0]) * np.cos(2.0 * v[:, 1] + ph[1]) + 0.1 * np.sin(4.0 * v[:, 2] + ph[2])
    t_verts = v * r[:, None] * np.array([0.45, 0.9, 0.3])
    ang = rng.uniform(-0.6, 0.6, 3)
    cx, sx, cy, sy, cz, sz = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
    rot = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ \
        np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    verts = t_verts @ rot.T + rng.uniform(-0.2, 0.2, 3)
    return {'verts': torch.from_numpy(verts.astype(np.float32)), 't_verts': torch.from_numpy(t_verts.astype(np.float32)),
            'faces': torch.from_numpy(f.copy()), 'rot': torch.from_numpy(rot.astype(np.float32))[None]}


def synthetic_queries(mesh, total, seed, grow=0.1):
    """`total` query points for a synthetic mesh -> float32 [total, 3]: first eight special points (one beyond each side of the grid,
    the grid's lower corner `minmax[:3]` itself, the box's centre), then, in a seeded random order, every vertex, every face centroid
    and points uniform in the bounding box grown by `grow`.  Any prefix of at least eight points holds all the special ones."""
    v32 = mesh['verts']
    step, num, minmax = grid_geometry(v32)
    v = v32.numpy().astype(np.float64)
    f = mesh['faces'].numpy()
    lo, hi = v.min(0), v.max(0)
    corner = minmax[:3].numpy().astype(np.float64)
    top = corner + float(step) * num[:3].numpy()
    mid = (lo + hi) / 2
    special = [corner.copy(), mid.copy()]
    for d in range(3):
        a, b = mid.copy(), mid.copy()
        a[d], b[d] = corner[d] - 0.5 * float(step), top[d] + 0.5 * float(step)
        special += [a, b]
    n_uniform = max(total - len(special) - v.shape[0] - f.shape[0], 0)
    rng = np.random.default_rng([seed, total])
    q = rng.uniform(lo - grow, hi + grow, (n_uniform, 3))
    rest = np.concatenate([v, v[f].mean(1), q])
    rest = rest[rng.permutation(rest.shape[0])]
    return torch.from_numpy(np.concatenate([np.array(special), rest])[:total].astype(np.float32))
