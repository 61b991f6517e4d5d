"""The inputs of the rasteriser's fixture (tests/golden/ref_gnr_raster.npz, written by tests/golden/make_golden_gnr_raster.py from the
reference's own render.h) and of the checks around it: generated here, never stored.  A case is
(name, verts [V,N,3] float32, tri [F,3] int64, h, w, persp); the reference ran every view on its own."""
import numpy as np
import torch

EPS = 1e-6


def _pv(px, py, z):
    """a vertex that lands on pixel coordinate (px, py) at depth z after the perspective division"""
    return [px * z, py * z, z]


def quads():
    """two overlapping quads at depths 2 and 3 on 16x16: occlusion; face 4 repeats face 0 (an exact-z tie, won by face 0) and face 5 is
    face 0 reversed (culled); vertex 8 lies behind the nearer quad, 9 behind it and in front of the farther one, 10 in front of both"""
    v = [_pv(2, 2, 2), _pv(10, 10, 2), _pv(10, 2, 2), _pv(2, 10, 2), _pv(6, 6, 3), _pv(14, 14, 3), _pv(14, 6, 3), _pv(6, 14, 3),
         _pv(4.5, 5.5, 2.5), _pv(8.5, 8.25, 2.5), _pv(7.5, 4.25, 1.5), _pv(12.5, 12.5, 3.5), _pv(20.0, 3.0, 2.0)]
    tri = [[0, 1, 2], [0, 3, 1], [4, 5, 6], [4, 7, 5], [0, 1, 2], [0, 2, 1]]
    return np.array(v, np.float32)[None], np.array(tri, np.int64), 16, 16


def degenerate(persp):
    """a line triangle (corners on one row, depths 2, 2.5, 3: the orthographic z takes c[2] twice) and a point triangle on 12x12, with
    a vertex under the line and one under the point"""
    pts = [(2, 5, 2.0), (9, 5, 2.5), (5, 5, 3.0), (4, 9, 2.0), (6, 5, 10.0), (4, 9, 10.0), (7, 7, 1.0)]
    v = [_pv(*p) if persp else list(p) for p in pts]
    tri = [[0, 1, 2], [3, 3, 3]]
    return np.array(v, np.float32)[None], np.array(tri, np.int64), 12, 12


def big():
    """one triangle larger than the 96x80 image, clipped on all four sides"""
    v = [_pv(-50, -40, 2.0), _pv(20, 400, 4.0), _pv(300, -30, 3.0), _pv(40.5, 30.5, 5.0)]
    return np.array(v, np.float32)[None], np.array([[0, 1, 2]], np.int64), 80, 96


def icosahedron():
    """synthetic_mesh(0) through a pinhole at distance 3 on 24x20"""
    from xrnerf_amd.gnr import synthetic_mesh
    m = synthetic_mesh(0, 0)
    p = m['verts'].numpy().astype(np.float64)
    z = p[:, 2] + 3.0
    px, py = 28.0 * p[:, 0] / z + 12.0, 28.0 * p[:, 1] / z + 10.0
    v = np.stack([px * z, py * z, z], 1).astype(np.float32)
    return v[None], m['faces'].numpy().astype(np.int64), 20, 24


def body():
    """synthetic_mesh(3) (642 vertices, 1280 faces) in two of synthetic_scene's cameras (lens distortion included) on 64x48: vertices
    fall off the image above and below, and vertex 7 of the first view is moved to z = 0"""
    from xrnerf_amd.gnr_render import _project64, synthetic_scene
    sc = synthetic_scene(seed=0)
    p = sc['smpl']['verts'].numpy().astype(np.float64)
    views = []
    for cam in (0, 2):
        pix, z = _project64(p, sc['calibs'][cam].numpy().astype(np.float64), sc['persps'][cam].numpy().astype(np.float64))
        views.append(np.stack([(pix[:, 0] - 0.5) * z, (pix[:, 1] - 8.5) * z, z], 1).astype(np.float32))
    v = np.stack(views)
    v[0, 7, 2] = 0.0
    return v, sc['smpl']['faces'].numpy().astype(np.int64), 48, 64


def cases():
    """-> list of (name, verts [V,N,3], tri [F,3], h, w, persp)"""
    out = [('quads',) + quads() + (True,), ('degenerate_persp',) + degenerate(True) + (True,), ('degenerate_ortho',) + degenerate(False) + (False,),
           ('big',) + big() + (True,), ('icosahedron',) + icosahedron() + (True,), ('body',) + body() + (True,)]
    return out


def tensors(case, device='cpu'):
    name, v, tri, h, w, persp = case
    return torch.from_numpy(v).to(device), torch.from_numpy(tri).to(device), h, w, persp
