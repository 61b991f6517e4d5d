"""Drop-in for the reference's `mesh_grid` extension module (extensions/mesh_grid/mesh_grid.cpp): the functions its
mesh_grid_searcher.py imports, with the reference's argument order and in-place outputs, on the kernels of csrc/xr_gnr.hip --

    sys.modules['mesh_grid'] = xrnerf_amd.mesh_grid

and the reference's own MeshGridSearcher runs unmodified, the way raymarch_cuda.py serves NGPGridSampler.  `search_intersect` is
importable and raises: GNR never calls it."""
import torch

from . import gnr, ops


def _host(t):
    """the grid's scalars as host values (the extension reads them on the device; here they are launch arguments)"""
    return t.tolist() if torch.is_tensor(t) else list(t)


def insert_grid_surface(verts, faces, minmax, num, step, tri_num):
    """fills tri_num (inclusive prefix counts, in place) and returns tri_idx (face id + 1 per slot)"""
    faces = faces.reshape(-1, 3)
    min3, num3, step = _host(minmax)[:3], _host(num)[:3], float(step)
    if gnr._use_kernels(verts):
        tn, ti, bad = ops.gnr_grid_build(verts, faces, step, min3, num3)
    else:
        tn, ti, bad = gnr.host_grid_build(verts.cpu().numpy(), faces.cpu().numpy(), step, min3, num3)
        tn, ti = torch.from_numpy(tn).to(verts.device), torch.from_numpy(ti).to(verts.device)
    if bad:
        raise ValueError('a face names a vertex outside [0, %d)' % verts.shape[0])
    tri_num.copy_(tn)
    return ti


def search_nearest_point(points, verts, faces, tri_num, tri_idx, num, minmax, step, near_faces, near_pts, coeff):
    points = points.reshape(-1, 3)
    grid = (verts, faces.reshape(-1, 3), float(step), _host(minmax)[:3], _host(num)[:3], tri_num, tri_idx, points)
    f, p, c = ops.gnr_nearest(*grid) if gnr._use_kernels(points) else gnr.host_search(gnr.gnr_host.nearest, *grid)
    near_faces.copy_(f)
    near_pts.copy_(p.reshape(near_pts.shape))
    coeff.copy_(c.reshape(coeff.shape))


def search_inside_mesh(points, verts, faces, tri_num, tri_idx, num, minmax, step, signs):
    points = points.reshape(-1, 3)
    grid = (verts, faces.reshape(-1, 3), float(step), _host(minmax)[:3], _host(num)[:3], tri_num, tri_idx, points)
    signs.copy_(ops.gnr_inside(*grid) if gnr._use_kernels(points) else gnr.host_search(gnr.gnr_host.inside, *grid))


def search_intersect(origins, directions, verts, faces, tri_num, tri_idx, num, minmax, step, intersect):
    raise NotImplementedError('search_intersect is not ported: GNR never calls it')


def cumsum(input):
    input.set_(input.cumsum(0).to(input.dtype))
    return input.reshape(1, 1, -1)
