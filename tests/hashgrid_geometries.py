"""TEST INFRASTRUCTURE: the level geometries (n_levels, log2_hashmap_size, base_resolution, per_level_scale; None = GridMeta's
default scale) at which the hash-grid lookup and scatter are pinned beside the default one, the path xr_scatter.hip's s3_layout
gives each level there (H binned hashed, D binned dense, R run-length, A atomic; from grad_bars.level_kinds, at a row count from
min_n on), and the positions the tests use.  What each geometry reaches that the default (RRRDDHHHHHHHHHHH) does not:

A  8 levels (the forward's cost map and the atomic kernel's block map with fewer than 16), hashed levels of two partitions
B  12 levels; hashed slices below 2^13 entries have no binned layout: a mixed atomic mask (the helper-stream fork), an atomic run
   of 11 levels (not a multiple of 8: the all-XCDs block order)
C  resolutions 2, 3, 4, ... (the dense index's single-subtraction modulo at its smallest), 12 run-length levels beside 4 binned
D  no hashed level
E  run-length levels only: no binning launch, the maxima from k_scatter_rl_absmax
F  one hashed level of exactly one partition
G  one level
H  a dense level of res 128: 256 partitions of 8192 entries, the LDS capacity; a hashed level of 256 partitions
I  a hashed slice of 512 partitions: atomic, beside binned dense levels
J  per_level_scale 2.0 over 16 levels: res up to 524 288 -- res >= 8192 atomic.  Its slices (2^15 entries) are smaller than every such
   res, so a 32-bit and a 64-bit stride both hash them: J does NOT tell the two readings apart
K  the same resolutions with slices of 2^19 entries: on levels 12-15, 65536 <= res <= hsize, a 32-bit stride res^2 wraps to 0 and
   the level would be indexed as cx + cy res, unhashed and without z -- the geometry that pins the 64-bit rule"""
import numpy as np

import grad_bars as B
import hashgrid_ref64 as H64

GEOMETRIES = {
    'A': (8, 14, 4, 1.5),
    'B': (12, 12, 16, 1.5),
    'C': (16, 15, 2, 1.26),
    'D': (5, 19, 16, None),
    'E': (3, 19, 16, None),
    'F': (4, 13, 3, 2.0),
    'G': (1, 19, 16, None),
    'H': (5, 21, 16, 2.0),
    'I': (5, 22, 16, 2.0),
    'J': (16, 15, 16, 2.0),
    'K': (16, 19, 16, 2.0),
    'default': (),
}
PATHS = {'A': 'RRRRRHHH', 'B': 'RAAAAAAAAAAA', 'C': 'RRRRRRRRRRRRHHHH', 'D': 'RRRDD', 'E': 'RRR', 'F': 'RRRH', 'G': 'R', 'H': 'RRDDH',
         'I': 'RRDDA', 'J': 'RRHHHHHHHAAAAAAA', 'K': 'RRDHHHHHHAAAAAAA', 'default': 'RRRDDHHHHHHHHHHH'}
ENTRIES = {'A': 62176, 'B': 49152, 'C': 167896, 'D': 330952, 'E': 46056, 'F': 10168, 'G': 4096, 'H': 4493312, 'I': 6590464,
           'J': 495616, 'K': 7114752}


def paths(meta, n):
    """one letter per level: level_kinds with the binned levels told apart by hashed / dense"""
    kinds = B.level_kinds(meta, n)
    return ''.join({'atomic': 'A', 'rl': 'R'}.get(k) or ('H' if H64.level_geometry(meta, lv)[3] else 'D') for lv, k in enumerate(kinds))


def positions(n, rng, layout='faces'):
    """[n, 3] fp32 in the unit cube.  'faces': uniform, a fifth of the rows on the x = 1 face, a tenth also on y = 1 (the dense
    index leaves its lattice row there), rows [0, 1, .5] and [1, 1, 1] (the index wraps at the upper corner).  'rays': 20 consecutive
    samples per ray, sqrt(3)/1024 apart (runs inside one coarse cell), the same two corner rows."""
    x = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    if layout == 'rays':
        nr = n // 20
        o3 = rng.uniform(0.2, 0.8, (nr, 3)).astype(np.float32)
        d3 = rng.normal(0, 1, (nr, 3)).astype(np.float32)
        d3 /= np.linalg.norm(d3, axis=1, keepdims=True)
        k = np.arange(nr * 20)
        x[:nr * 20] = np.clip(o3[k // 20] + (np.float32(0.0017) * (k % 20).astype(np.float32))[:, None] * d3[k // 20], 0, 1)
    else:
        x[: n // 5, 0] = 1.0
        x[: n // 10, 1] = 1.0
    x[0] = [1.0, 1.0, 1.0]
    if n > 1:
        x[1] = [0.0, 1.0, 0.5]
    return x
