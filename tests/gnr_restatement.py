"""A short restatement of the reference's mesh grid (extensions/mesh_grid: insert_grid_surface_kernel run serially) for meshes the fixture
does not store; tests/test_gnr_host.py pins it to tests/golden/ref_gnr.npz.  Pairs (cell, face) are listed face by face and sorted by
cell (stable): the reference's serial fill order, ascending face id with repeats adjacent."""
import numpy as np


def box_cells(x, n):
    """x < 0 ? 0 : (x >= n ? n - 1 : floor(x)) on float32 arrays"""
    with np.errstate(invalid='ignore'):
        return np.where(x < 0, 0, np.where(x >= np.float32(n), n - 1, np.floor(x))).astype(np.int64)


def grid_tables(verts, faces, step, min3, num3):
    """-> (tri_num [cells] int32 inclusive prefix counts, tri_idx [slots] int32 face id + 1)"""
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    step, mn, n = np.float32(step), np.asarray(min3, np.float32), [int(v) for v in num3[:3]]
    tri = verts[faces]                                   # [F, 3 vertices, 3 axes]
    lo = np.stack([box_cells((tri[:, :, d].min(1) - mn[d]) / step, n[d]) for d in range(3)], 1)
    hi = np.stack([box_cells((tri[:, :, d].max(1) - mn[d]) / step, n[d]) + 1 for d in range(3)], 1)
    w = hi - lo
    pairs = []
    for f in range(faces.shape[0]):
        j = np.arange(int(np.prod(w[f])))
        ind, k = np.zeros_like(j), j.copy()
        for d in range(3):
            ind = ind * (n[d] if d > 0 else 0) + lo[f, d] + k % w[f, d]
            k = (k.astype(np.float64) / (np.float64(w[f, d]) + 1e-8)).astype(np.int64)      # the quirk: truncates one too low at multiples
        pairs.append(np.stack([ind, np.full_like(j, f + 1)], 1))
    pairs = np.concatenate(pairs)
    pairs = pairs[np.argsort(pairs[:, 0], kind='stable')]
    counts = np.bincount(pairs[:, 0], minlength=n[0] * n[1] * n[2])
    return np.cumsum(counts).astype(np.int32), pairs[:, 1].astype(np.int32)
