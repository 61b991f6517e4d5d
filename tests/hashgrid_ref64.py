"""TEST INFRASTRUCTURE: the multiresolution hash-grid encoding and its table gradient restated in numpy float64, for ANY level geometry
ops.GridMeta / oracle.GridMeta can describe.  Independent of oracle/ngp_oracle.c and of the library: it reads only the level arrays
(scale, resolution, offset) of the meta it is handed.

Per level: p = fp32(fp32(x * scale) + 0.5) (the cell and the fractions are the kernels' fp32 ones), cell = floor(p), weights from
the fractions in float64.  A level is hashed iff its lattice has more points than its slice has entries, res^3 > hsize in Python
integers (no 32-bit stride: at res >= 65536 a uint32 stride res^2 wraps to 0 -- see DESIGN.md, hash grid).  Index, in uint32
arithmetic: (cx ^ cy * 2654435761 ^ cz * 805459861) mod hsize when hashed, (cx + cy res + cz res^2) mod hsize otherwise."""
import numpy as np

P1, P2, M32 = 2654435761, 805459861, 0xffffffff


def level_geometry(meta, lv):
    """-> (res, hsize, offset, hashed) of level lv as Python integers"""
    res, off = int(meta.resolution[lv]), int(meta.offset[lv])
    hsize = int(meta.offset[lv + 1]) - off
    return res, hsize, off, res ** 3 > hsize


def corners(x, meta, lv):
    """x [n, 3] fp32 -> idx int64 [n, 8] (entry inside the level's slice), w float64 [n, 8]; corner c = (c & 1, c >> 1 & 1, c >> 2)"""
    res, hsize, _, hashed = level_geometry(meta, lv)
    x = np.ascontiguousarray(x, np.float32)
    p = (x * np.float32(meta.scale[lv])).astype(np.float32) + np.float32(0.5)
    assert p.dtype == np.float32
    f = np.floor(p)
    w = (p - f).astype(np.float64)              # fp32 subtraction (exact: Sterbenz or a small integer part), widened
    g = f.astype(np.int64) & M32                # (uint32_t)(int)f
    idx = np.empty((x.shape[0], 8), np.int64)
    wt = np.empty((x.shape[0], 8), np.float64)
    for c in range(8):
        cx, cy, cz = ((g[:, d] + ((c >> d) & 1)) & M32 for d in range(3))
        if hashed:
            i = cx ^ ((cy * P1) & M32) ^ ((cz * P2) & M32)
        else:
            i = (cx + ((cy * res) & M32) + ((cz * ((res * res) & M32)) & M32)) & M32
        idx[:, c] = i % hsize
        wt[:, c] = (w[:, 0] if c & 1 else 1.0 - w[:, 0]) * (w[:, 1] if c & 2 else 1.0 - w[:, 1]) * (w[:, 2] if c & 4 else 1.0 - w[:, 2])
    return idx, wt


def encode64(table, x, meta):
    """table [n_params] (any float type), x [n, 3] fp32 -> the encoding [n, 2 L] in float64"""
    t = np.asarray(table, np.float64).reshape(-1, 2)
    y = np.zeros((np.asarray(x).shape[0], 2 * meta.n_levels))
    for lv in range(meta.n_levels):
        off = int(meta.offset[lv])
        idx, w = corners(x, meta, lv)
        y[:, 2 * lv:2 * lv + 2] = (w[:, :, None] * t[off + idx]).sum(1)
    return y


def table_grad64(x, g, meta, levels=None, init=None):
    """x [n, 3] fp32 positions, g [n, 2 L] the fp32 dL/d(encoding) handed to the scatter (rows that must not count are zero), levels
    (l0, l1) -> the dict of ref64_ngp.table_grad64: ref float64 [n_params] (= init + the levels' float64 sums; other entries = init),
    budget float64 [n_params] (|init| + sum |w g| per entry), count int64 [n_params] (contributions per entry: corners of rows with
    a non-zero gradient)"""
    g = np.asarray(g, np.float32)
    l0, l1 = (0, meta.n_levels) if levels is None else levels
    P = int(meta.offset[meta.n_levels]) * 2
    ref = np.zeros(P) if init is None else np.asarray(init, np.float64).copy()
    budget = np.abs(ref)
    count = np.zeros(P, np.int64)
    for lv in range(l0, l1):
        _, hs, off, _ = level_geometry(meta, lv)
        a, b = 2 * off, 2 * (off + hs)
        idx, w = corners(x, meta, lv)
        loc = idx.ravel()
        live = (g[:, 2 * lv] != 0) | (g[:, 2 * lv + 1] != 0)
        cnt = np.bincount(loc, weights=np.repeat(live, 8).astype(np.float64), minlength=hs).astype(np.int64)
        for f in range(2):
            c = (w * g[:, 2 * lv + f].astype(np.float64)[:, None]).ravel()
            ref[a + f:b:2] += np.bincount(loc, weights=c, minlength=hs)
            budget[a + f:b:2] += np.bincount(loc, weights=np.abs(c), minlength=hs)
            count[a + f:b:2] = cnt
    return dict(ref=ref, budget=budget, count=count)
