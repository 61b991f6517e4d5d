// GNR's mesh reconstruction (GnrRenderer.reconstruct / octree_reconstruct, the reference's gnr_render.py:643-815) for gfx950: the
// occupancy volume is made, refined and turned into a welded triangle mesh without leaving the device.
//   k_gc_hull      thread = grid point: the point (np.linspace, / spatial_freq + center, evaluated in double and rounded once to fp32),
//                  its projection into every source view by the hull's own device functions (xr_gnr_project.h) and the nearest sample
//                  of the dilated masks -> one state byte: 1 = still to be evaluated, 0 = processed
//   k_gc_sel_count / scan / k_gc_sel_write   a level's test set -- indices multiples of reso, state 1 -- compacted in C order:
//                  per-workgroup counts, a two-level exclusive scan (xr_scan.h's xr_scan_two_level), ranked write of (flat, point,
//                  normalised projections)
//   k_gc_scatter   the level's occupancies into the fp32 volume at `flat`, the state byte cleared
//   k_gc_cells / k_gc_fill   the fold: per coarse cell min, max, the centre's state -> skip decision (in double) and fill value; then
//                  per fine point the lexicographically LAST skipped cell among the (up to 8) cells whose closed block covers it
//   k_mc_count / scan / k_mc_verts / k_mc_tris   the iso-surface: a voxel owns the three edges that leave its lowest corner; owned
//                  crossed edges and triangles are counted per workgroup, scanned, and written in voxel C order (vertices: then axis
//                  order; triangles: then table order) -- 4 bytes of workspace per grid point (the voxel's rank inside its workgroup)
//   k_gc_world     index coordinates -> the reference's world coordinates (its N-for-N-1 included), in double
//   k_gc_point_rows  per vertex the normalised projections and make_att_input's directions (query direction = the normal)
//   k_lap_step / k_vol_partial / k_vol_final / k_lap_scale   trimesh's filter_laplacian defaults in double: the neighbour mean in CSR
//                  order, the signed volume as a fixed-order sum, the rescale about the origin
// No floating-point atomics and no atomic cursor anywhere: the same input gives the same bits.
#include "xr_common.h"
#define XR_SCAN_TWO_LEVEL
#include "xr_scan.h"
#include "../../include/xrnerf_mi355_gnr.h"
#include "../../include/xrnerf_mi355_gnr_recon.h"
#include "xr_gnr_project.h"

#define GC_BLOCK 256
static_assert(GC_BLOCK == XR_SCAN_BLOCK, "the shared workgroup routines are written for 256 threads");
#define GC_MAX_N XR_GNR_RECON_MAX_N

struct GcGrid {
    uint32_t N;
    double start[3], stop[3], step[3], sf;      // np.linspace per axis; spatial_freq
    const float* center;                        // [3] device
    const float* coords;                        // [N^3, 3] or null: the caller's points instead
};

// grid / spatial_freq + center in double (center is fp32), rounded once: the reference's point, bit for bit
static __device__ inline void gc_point(const GcGrid& g, const uint32_t* ijk, uint64_t flat, float* p) {
    if (g.coords) { p[0] = g.coords[3 * flat]; p[1] = g.coords[3 * flat + 1]; p[2] = g.coords[3 * flat + 2]; return; }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double lin = ijk[a] == g.N - 1 ? g.stop[a] : (double)ijk[a] * g.step[a] + g.start[a];
        p[a] = (float)(lin / g.sf + (double)g.center[a]);
    }
}

static __device__ inline bool gc_in_hull(const GrHull& a, const float* p) {
    for (uint32_t v = 0; v < a.V; ++v) {
        float xy[2], z;
        int px, py;
        gr_project(a, v, p, xy, &z);
        if (!gr_nearest_pixel(xy[0], xy[1], a.H, a.W, &px, &py)) return false;
        if (!(a.masks[((uint64_t)v * a.H + py) * a.W + px] > 0.f)) return false;
    }
    return true;
}

// ------------------------------------------------------------------------------------------ grid hull
__global__ void __launch_bounds__(GC_BLOCK) k_gc_hull(GcGrid g, GrHull a, uint8_t* __restrict__ state) {
    const uint64_t id = (uint64_t)blockIdx.x * GC_BLOCK + threadIdx.x, N = g.N;
    if (id >= N * N * N) return;
    const uint32_t ijk[3] = {(uint32_t)(id / (N * N)), (uint32_t)(id / N % N), (uint32_t)(id % N)};
    float p[3];
    gc_point(g, ijk, id, p);
    const bool open = ijk[0] + 1 < g.N && ijk[1] + 1 < g.N && ijk[2] + 1 < g.N;       // notprocessed[:-1, :-1, :-1]
    state[id] = (open && gc_in_hull(a, p)) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------ level select
struct GcLevel { uint32_t N, reso, L; };       // L lattice points per axis: the multiples of reso below N

static __device__ inline bool gc_lattice(const GcLevel& l, uint64_t id, uint32_t* ijk, uint64_t* flat) {
    const uint64_t L = l.L;
    if (id >= L * L * L) return false;
    ijk[0] = (uint32_t)(id / (L * L)) * l.reso; ijk[1] = (uint32_t)(id / L % L) * l.reso; ijk[2] = (uint32_t)(id % L) * l.reso;
    *flat = ((uint64_t)ijk[0] * l.N + ijk[1]) * l.N + ijk[2];
    return true;
}

__global__ void __launch_bounds__(GC_BLOCK) k_gc_sel_count(GcLevel l, const uint8_t* __restrict__ state, uint32_t* __restrict__ bcount) {
    uint32_t ijk[3], sum;
    uint64_t flat;
    const bool on = gc_lattice(l, (uint64_t)blockIdx.x * GC_BLOCK + threadIdx.x, ijk, &flat) && state[flat] == 1;
    xr_block_excl_flag(on, &sum);
    if (threadIdx.x == 0) bcount[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(GC_BLOCK) k_gc_sel_write(GcLevel l, GcGrid g, GrHull a, const uint8_t* __restrict__ state,
                                                          const uint32_t* __restrict__ bbase, uint32_t M, int32_t* __restrict__ flat_out,
                                                          float* __restrict__ pts, float* __restrict__ xy) {
    uint32_t ijk[3], sum;
    uint64_t flat;
    const bool on = gc_lattice(l, (uint64_t)blockIdx.x * GC_BLOCK + threadIdx.x, ijk, &flat) && state[flat] == 1;
    const uint64_t m = (uint64_t)bbase[blockIdx.x] + xr_block_excl_flag(on, &sum);
    if (!on || m >= M) return;                                     // (M is the scan's total: the second test never holds)
    float p[3];
    gc_point(g, ijk, flat, p);
    flat_out[m] = (int32_t)flat;
    pts[3 * m] = p[0]; pts[3 * m + 1] = p[1]; pts[3 * m + 2] = p[2];
    for (uint32_t v = 0; v < a.V; ++v) {
        float q[2], z;
        gr_project(a, v, p, q, &z);
        xy[(m * a.V + v) * 2] = q[0]; xy[(m * a.V + v) * 2 + 1] = q[1];
    }
}

// ------------------------------------------------------------------------------------------ scatter, fold
__global__ void __launch_bounds__(GC_BLOCK) k_gc_scatter(const int32_t* __restrict__ flat, const float* __restrict__ val, uint32_t M, int sigmoid,
                                                        float gamma, uint64_t points, float* __restrict__ vol, uint8_t* __restrict__ state) {
    const uint32_t m = blockIdx.x * GC_BLOCK + threadIdx.x;
    if (m >= M) return;
    const uint64_t f = (uint64_t)(uint32_t)flat[m];
    if (flat[m] < 0 || f >= points) return;
    vol[f] = sigmoid ? 1.f / (1.f + expf(-(val[m] * gamma))) : val[m];
    state[f] = 0;
}

struct GcFold { uint32_t N, reso, G; };        // G coarse cells per axis

__global__ void __launch_bounds__(GC_BLOCK) k_gc_cells(GcFold f, const float* __restrict__ vol, const uint8_t* __restrict__ state,
                                                      float* __restrict__ fill, uint8_t* __restrict__ skip) {
    const uint64_t id = (uint64_t)blockIdx.x * GC_BLOCK + threadIdx.x, G = f.G, N = f.N;
    if (id >= G * G * G) return;
    const uint64_t x = id / (G * G) * f.reso, y = id / G % G * f.reso, z = id % G * f.reso;
    float lo = vol[(x * N + y) * N + z], hi = lo;
#pragma unroll
    for (int c = 1; c < 8; ++c) {
        const float v = vol[((x + (c >> 2) * f.reso) * N + y + ((c >> 1) & 1) * f.reso) * N + z + (c & 1) * f.reso];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    const uint32_t h = f.reso / 2;
    const bool open = state[((x + h) * N + y + h) * N + z + h] == 1;
    skip[id] = (open && (double)hi - (double)lo < 0.01) ? 1 : 0;
    fill[id] = (float)(0.5 * ((double)lo + (double)hi));
}

__global__ void __launch_bounds__(GC_BLOCK) k_gc_fill(GcFold f, const float* __restrict__ fill, const uint8_t* __restrict__ skip,
                                                     float* __restrict__ vol, uint8_t* __restrict__ state) {
    const uint64_t P = (uint64_t)f.G * f.reso + 1, id = (uint64_t)blockIdx.x * GC_BLOCK + threadIdx.x, N = f.N, G = f.G;
    if (id >= P * P * P) return;
    const uint32_t p[3] = {(uint32_t)(id / (P * P)), (uint32_t)(id / P % P), (uint32_t)(id % P)};
    uint32_t hi[3], lo[3];                                          // the cells whose closed block [c reso, c reso + reso] holds p: lo .. hi
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        hi[a] = p[a] / f.reso;
        lo[a] = (p[a] % f.reso == 0 && hi[a] > 0) ? hi[a] - 1 : hi[a];
        if (hi[a] > f.G - 1) hi[a] = f.G - 1;
    }
    // the serial loop applies the cells in C order, so the last one in that order is what remains: walk the candidates downwards
    for (uint32_t cx = hi[0] + 1; cx-- > lo[0];)
        for (uint32_t cy = hi[1] + 1; cy-- > lo[1];)
            for (uint32_t cz = hi[2] + 1; cz-- > lo[2];) {
                const uint64_t c = ((uint64_t)cx * G + cy) * G + cz;
                if (skip[c]) {
                    const uint64_t at = ((uint64_t)p[0] * N + p[1]) * N + p[2];
                    vol[at] = fill[c];
                    state[at] = 0;
                    return;
                }
            }
}

// ------------------------------------------------------------------------------------------ iso-surface
// Corner c of a cell sits at offset (c & 1, c >> 1 & 1, c >> 2 & 1) along the volume's axes 0, 1, 2; edge e = 4 axis + (u + 2 v) runs
// along `axis` from the corner whose other two offsets (ascending axis order) are (u, v), so it is the edge the voxel at that corner
// owns along `axis`.  A case is the sum of 1 << c over the corners with value > level.  256 rows without complement symmetry: every
// cube face is cut by its own four corner values alone (two inside corners on a diagonal are each cut off by themselves), so both cubes
// at a face draw the same segments; no triangle side inside a cube lies in a cube face.  tests/gnr_recon_restatement.py derives the
// same table from these rules and tests/test_gnr_recon_host.py compares the two row by row.
static __device__ const int8_t GC_TRI[256][16] = {
    {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 4,  8,  5,  8,  9,  5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1, 10,  4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  8,  1, 10,  8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  5,  1, 10,  4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1, 10,  5, 10,  8,  5,  8,  9,  5, -1, -1, -1, -1, -1, -1, -1},
    { 1,  5, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  8,  1,  5, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  1,  9, 11,  1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  4, 11,  4,  8, 11,  8,  9, 11, -1, -1, -1, -1, -1, -1, -1},
    { 4,  5, 10,  5, 11, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  5,  8,  5, 11,  8, 11, 10,  8, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  4,  9, 11,  4, 11, 10,  4, -1, -1, -1, -1, -1, -1, -1},
    { 8,  9, 10,  9, 11, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 2,  8,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  2,  4,  6,  2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  5,  2,  8,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 2,  9,  6,  9,  5,  6,  5,  4,  6, -1, -1, -1, -1, -1, -1, -1},
    { 1, 10,  4,  2,  8,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  2,  1, 10,  2, 10,  6,  2, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  5,  1, 10,  4,  2,  8,  6, -1, -1, -1, -1, -1, -1, -1},
    { 1, 10,  5, 10,  6,  5,  6,  2,  5,  2,  9,  5, -1, -1, -1, -1},
    { 1,  5, 11,  2,  8,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  2,  4,  6,  2,  1,  5, 11, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  1,  9, 11,  1,  2,  8,  6, -1, -1, -1, -1, -1, -1, -1},
    { 1,  4, 11,  4,  6, 11,  6,  2, 11,  2,  9, 11, -1, -1, -1, -1},
    { 2,  8,  6,  4,  5, 10,  5, 11, 10, -1, -1, -1, -1, -1, -1, -1},
    { 0,  5,  2,  5, 11,  2, 11, 10,  2, 10,  6,  2, -1, -1, -1, -1},
    { 0,  9,  4,  9, 11,  4, 11, 10,  4,  2,  8,  6, -1, -1, -1, -1},
    { 2,  9,  6,  9, 11,  6, 11, 10,  6, -1, -1, -1, -1, -1, -1, -1},
    { 2,  7,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  8,  2,  7,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  2,  5,  2,  7,  5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 2,  7,  8,  7,  5,  8,  5,  4,  8, -1, -1, -1, -1, -1, -1, -1},
    { 1, 10,  4,  2,  7,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  8,  1, 10,  8,  2,  7,  9, -1, -1, -1, -1, -1, -1, -1},
    { 0,  2,  5,  2,  7,  5,  1, 10,  4, -1, -1, -1, -1, -1, -1, -1},
    { 1, 10,  5, 10,  8,  5,  8,  2,  5,  2,  7,  5, -1, -1, -1, -1},
    { 1,  5, 11,  2,  7,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  8,  1,  5, 11,  2,  7,  9, -1, -1, -1, -1, -1, -1, -1},
    { 0,  2,  1,  2,  7,  1,  7, 11,  1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  4, 11,  4,  8, 11,  8,  2, 11,  2,  7, 11, -1, -1, -1, -1},
    { 2,  7,  9,  4,  5, 10,  5, 11, 10, -1, -1, -1, -1, -1, -1, -1},
    { 0,  5,  8,  5, 11,  8, 11, 10,  8,  2,  7,  9, -1, -1, -1, -1},
    { 0,  2,  4,  2,  7,  4,  7, 11,  4, 11, 10,  4, -1, -1, -1, -1},
    { 2,  7,  8,  7, 11,  8, 11, 10,  8, -1, -1, -1, -1, -1, -1, -1},
    { 6,  7,  8,  7,  9,  8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  9,  4,  6,  9,  6,  7,  9, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  5,  8,  6,  5,  6,  7,  5, -1, -1, -1, -1, -1, -1, -1},
    { 4,  6,  5,  6,  7,  5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1, 10,  4,  6,  7,  8,  7,  9,  8, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  9,  1, 10,  9, 10,  6,  9,  6,  7,  9, -1, -1, -1, -1},
    { 0,  8,  5,  8,  6,  5,  6,  7,  5,  1, 10,  4, -1, -1, -1, -1},
    { 1, 10,  5, 10,  6,  5,  6,  7,  5, -1, -1, -1, -1, -1, -1, -1},
    { 1,  5, 11,  6,  7,  8,  7,  9,  8, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  9,  4,  6,  9,  6,  7,  9,  1,  5, 11, -1, -1, -1, -1},
    { 0,  8,  1,  8,  6,  1,  6,  7,  1,  7, 11,  1, -1, -1, -1, -1},
    { 1,  4, 11,  4,  6, 11,  6,  7, 11, -1, -1, -1, -1, -1, -1, -1},
    { 4,  5, 10,  5, 11, 10,  6,  7,  8,  7,  9,  8, -1, -1, -1, -1},
    { 0,  5, 10,  5, 11, 10,  0, 10,  9, 10,  6,  9,  6,  7,  9, -1},
    { 0,  8,  7,  8,  6,  7,  0,  7,  4,  7, 11,  4, 11, 10,  4, -1},
    { 6,  7, 10,  7, 11, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 3,  6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  8,  3,  6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  5,  3,  6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 3,  6, 10,  4,  8,  5,  8,  9,  5, -1, -1, -1, -1, -1, -1, -1},
    { 1,  3,  4,  3,  6,  4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  8,  1,  3,  8,  3,  6,  8, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  5,  1,  3,  4,  3,  6,  4, -1, -1, -1, -1, -1, -1, -1},
    { 1,  3,  5,  3,  6,  5,  6,  8,  5,  8,  9,  5, -1, -1, -1, -1},
    { 1,  5, 11,  3,  6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  8,  1,  5, 11,  3,  6, 10, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  1,  9, 11,  1,  3,  6, 10, -1, -1, -1, -1, -1, -1, -1},
    { 1,  4, 11,  4,  8, 11,  8,  9, 11,  3,  6, 10, -1, -1, -1, -1},
    { 3,  6, 11,  6,  4, 11,  4,  5, 11, -1, -1, -1, -1, -1, -1, -1},
    { 0,  5,  8,  5, 11,  8, 11,  3,  8,  3,  6,  8, -1, -1, -1, -1},
    { 0,  9,  4,  9, 11,  4, 11,  3,  4,  3,  6,  4, -1, -1, -1, -1},
    { 3,  6, 11,  6,  8, 11,  8,  9, 11, -1, -1, -1, -1, -1, -1, -1},
    { 2,  8,  3,  8, 10,  3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  2,  4, 10,  2, 10,  3,  2, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  5,  2,  8,  3,  8, 10,  3, -1, -1, -1, -1, -1, -1, -1},
    { 2,  9,  3,  9,  5,  3,  5,  4,  3,  4, 10,  3, -1, -1, -1, -1},
    { 1,  3,  4,  3,  2,  4,  2,  8,  4, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  2,  1,  3,  2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  5,  1,  3,  4,  3,  2,  4,  2,  8,  4, -1, -1, -1, -1},
    { 1,  3,  5,  3,  2,  5,  2,  9,  5, -1, -1, -1, -1, -1, -1, -1},
    { 1,  5, 11,  2,  8,  3,  8, 10,  3, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  2,  4, 10,  2, 10,  3,  2,  1,  5, 11, -1, -1, -1, -1},
    { 0,  9,  1,  9, 11,  1,  2,  8,  3,  8, 10,  3, -1, -1, -1, -1},
    { 1,  4, 11,  4, 10,  2, 10,  3,  2,  4,  2, 11,  2,  9, 11, -1},
    { 2,  8,  3,  8,  4,  3,  4,  5,  3,  5, 11,  3, -1, -1, -1, -1},
    { 0,  5,  2,  5, 11,  2, 11,  3,  2, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  4,  9, 11,  4, 11,  3,  4,  3,  2,  4,  2,  8,  4, -1},
    { 2,  9,  3,  9, 11,  3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 2,  7,  9,  3,  6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  8,  2,  7,  9,  3,  6, 10, -1, -1, -1, -1, -1, -1, -1},
    { 0,  2,  5,  2,  7,  5,  3,  6, 10, -1, -1, -1, -1, -1, -1, -1},
    { 2,  7,  8,  7,  5,  8,  5,  4,  8,  3,  6, 10, -1, -1, -1, -1},
    { 1,  3,  4,  3,  6,  4,  2,  7,  9, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  8,  1,  3,  8,  3,  6,  8,  2,  7,  9, -1, -1, -1, -1},
    { 0,  2,  5,  2,  7,  5,  1,  3,  4,  3,  6,  4, -1, -1, -1, -1},
    { 1,  3,  5,  3,  6,  5,  6,  8,  5,  8,  2,  5,  2,  7,  5, -1},
    { 1,  5, 11,  2,  7,  9,  3,  6, 10, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  8,  1,  5, 11,  2,  7,  9,  3,  6, 10, -1, -1, -1, -1},
    { 0,  2,  1,  2,  7,  1,  7, 11,  1,  3,  6, 10, -1, -1, -1, -1},
    { 1,  4, 11,  4,  8, 11,  8,  2, 11,  2,  7, 11,  3,  6, 10, -1},
    { 2,  7,  9,  3,  6, 11,  6,  4, 11,  4,  5, 11, -1, -1, -1, -1},
    { 0,  5,  8,  5, 11,  8, 11,  3,  8,  3,  6,  8,  2,  7,  9, -1},
    { 0,  2,  4,  2,  7,  4,  7, 11,  4, 11,  3,  4,  3,  6,  4, -1},
    { 2,  7,  8,  7, 11,  8, 11,  3,  8,  3,  6,  8, -1, -1, -1, -1},
    { 3,  7, 10,  7,  9, 10,  9,  8, 10, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  9,  4, 10,  9, 10,  3,  9,  3,  7,  9, -1, -1, -1, -1},
    { 0,  8,  5,  8, 10,  5, 10,  3,  5,  3,  7,  5, -1, -1, -1, -1},
    { 3,  7, 10,  7,  5, 10,  5,  4, 10, -1, -1, -1, -1, -1, -1, -1},
    { 1,  3,  4,  3,  7,  4,  7,  9,  4,  9,  8,  4, -1, -1, -1, -1},
    { 0,  1,  9,  1,  3,  9,  3,  7,  9, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  5,  8,  4,  3,  4,  1,  3,  8,  3,  5,  3,  7,  5, -1},
    { 1,  3,  5,  3,  7,  5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  5, 11,  3,  7, 10,  7,  9, 10,  9,  8, 10, -1, -1, -1, -1},
    { 0,  4,  9,  4, 10,  9, 10,  3,  9,  3,  7,  9,  1,  5, 11, -1},
    { 0,  8,  1,  8, 10,  7, 10,  3,  7,  8,  7,  1,  7, 11,  1, -1},
    { 1,  4, 11,  4, 10,  7, 10,  3,  7,  4,  7, 11, -1, -1, -1, -1},
    { 3,  7,  8,  7,  9,  8,  3,  8, 11,  8,  4, 11,  4,  5, 11, -1},
    { 0,  5,  3,  5, 11,  3,  0,  3,  9,  3,  7,  9, -1, -1, -1, -1},
    { 0,  8,  4,  3,  7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 3,  7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 3, 11,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  8,  3, 11,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  5,  3, 11,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 3, 11,  7,  4,  8,  5,  8,  9,  5, -1, -1, -1, -1, -1, -1, -1},
    { 1, 10,  4,  3, 11,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  8,  1, 10,  8,  3, 11,  7, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  5,  1, 10,  4,  3, 11,  7, -1, -1, -1, -1, -1, -1, -1},
    { 1, 10,  5, 10,  8,  5,  8,  9,  5,  3, 11,  7, -1, -1, -1, -1},
    { 1,  5,  3,  5,  7,  3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  8,  1,  5,  3,  5,  7,  3, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  1,  9,  7,  1,  7,  3,  1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  4,  3,  4,  8,  3,  8,  9,  3,  9,  7,  3, -1, -1, -1, -1},
    { 3, 10,  7, 10,  4,  7,  4,  5,  7, -1, -1, -1, -1, -1, -1, -1},
    { 0,  5,  8,  5,  7,  8,  7,  3,  8,  3, 10,  8, -1, -1, -1, -1},
    { 0,  9,  4,  9,  7,  4,  7,  3,  4,  3, 10,  4, -1, -1, -1, -1},
    { 3, 10,  7, 10,  8,  7,  8,  9,  7, -1, -1, -1, -1, -1, -1, -1},
    { 2,  8,  6,  3, 11,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  2,  4,  6,  2,  3, 11,  7, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  5,  2,  8,  6,  3, 11,  7, -1, -1, -1, -1, -1, -1, -1},
    { 2,  9,  6,  9,  5,  6,  5,  4,  6,  3, 11,  7, -1, -1, -1, -1},
    { 1, 10,  4,  2,  8,  6,  3, 11,  7, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  2,  1, 10,  2, 10,  6,  2,  3, 11,  7, -1, -1, -1, -1},
    { 0,  9,  5,  1, 10,  4,  2,  8,  6,  3, 11,  7, -1, -1, -1, -1},
    { 1, 10,  5, 10,  6,  5,  6,  2,  5,  2,  9,  5,  3, 11,  7, -1},
    { 1,  5,  3,  5,  7,  3,  2,  8,  6, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  2,  4,  6,  2,  1,  5,  3,  5,  7,  3, -1, -1, -1, -1},
    { 0,  9,  1,  9,  7,  1,  7,  3,  1,  2,  8,  6, -1, -1, -1, -1},
    { 1,  4,  3,  4,  6,  9,  6,  2,  9,  4,  9,  3,  9,  7,  3, -1},
    { 2,  8,  6,  3, 10,  7, 10,  4,  7,  4,  5,  7, -1, -1, -1, -1},
    { 0,  5,  2,  5,  7, 10,  7,  3, 10,  5, 10,  2, 10,  6,  2, -1},
    { 0,  9,  4,  9,  7,  4,  7,  3,  4,  3, 10,  4,  2,  8,  6, -1},
    { 2,  9,  6,  9,  7, 10,  7,  3, 10,  9, 10,  6, -1, -1, -1, -1},
    { 2,  3,  9,  3, 11,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  8,  2,  3,  9,  3, 11,  9, -1, -1, -1, -1, -1, -1, -1},
    { 0,  2,  5,  2,  3,  5,  3, 11,  5, -1, -1, -1, -1, -1, -1, -1},
    { 2,  3,  8,  3, 11,  8, 11,  5,  8,  5,  4,  8, -1, -1, -1, -1},
    { 1, 10,  4,  2,  3,  9,  3, 11,  9, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  8,  1, 10,  8,  2,  3,  9,  3, 11,  9, -1, -1, -1, -1},
    { 0,  2,  5,  2,  3,  5,  3, 11,  5,  1, 10,  4, -1, -1, -1, -1},
    { 1, 10,  5, 10,  8,  5,  8,  2,  5,  2,  3,  5,  3, 11,  5, -1},
    { 1,  5,  3,  5,  9,  3,  9,  2,  3, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  8,  1,  5,  3,  5,  9,  3,  9,  2,  3, -1, -1, -1, -1},
    { 0,  2,  1,  2,  3,  1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  4,  3,  4,  8,  3,  8,  2,  3, -1, -1, -1, -1, -1, -1, -1},
    { 2,  3,  9,  3, 10,  9, 10,  4,  9,  4,  5,  9, -1, -1, -1, -1},
    { 0,  5,  8,  5,  9,  3,  9,  2,  3,  5,  3,  8,  3, 10,  8, -1},
    { 0,  2,  4,  2,  3,  4,  3, 10,  4, -1, -1, -1, -1, -1, -1, -1},
    { 2,  3,  8,  3, 10,  8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 3, 11,  6, 11,  9,  6,  9,  8,  6, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  9,  4,  6,  9,  6,  3,  9,  3, 11,  9, -1, -1, -1, -1},
    { 0,  8,  5,  8,  6,  5,  6,  3,  5,  3, 11,  5, -1, -1, -1, -1},
    { 3, 11,  6, 11,  5,  6,  5,  4,  6, -1, -1, -1, -1, -1, -1, -1},
    { 1, 10,  4,  3, 11,  6, 11,  9,  6,  9,  8,  6, -1, -1, -1, -1},
    { 0,  1,  9,  1, 10,  9, 10,  6,  9,  6,  3,  9,  3, 11,  9, -1},
    { 0,  8,  5,  8,  6,  5,  6,  3,  5,  3, 11,  5,  1, 10,  4, -1},
    { 1, 10,  5, 10,  6,  5,  6,  3,  5,  3, 11,  5, -1, -1, -1, -1},
    { 1,  5,  3,  5,  9,  3,  9,  8,  3,  8,  6,  3, -1, -1, -1, -1},
    { 0,  4,  9,  4,  6,  9,  6,  3,  9,  3,  1,  9,  1,  5,  9, -1},
    { 0,  8,  1,  8,  6,  1,  6,  3,  1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  4,  3,  4,  6,  3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 3, 10,  5, 10,  4,  5,  3,  5,  6,  5,  9,  6,  9,  8,  6, -1},
    { 0,  5,  9,  3, 10,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  3,  8,  6,  3,  0,  3,  4,  3, 10,  4, -1, -1, -1, -1},
    { 3, 10,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 6, 10,  7, 10, 11,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  8,  6, 10,  7, 10, 11,  7, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  5,  6, 10,  7, 10, 11,  7, -1, -1, -1, -1, -1, -1, -1},
    { 4,  8,  5,  8,  9,  5,  6, 10,  7, 10, 11,  7, -1, -1, -1, -1},
    { 1, 11,  4, 11,  7,  4,  7,  6,  4, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  8,  1, 11,  8, 11,  7,  8,  7,  6,  8, -1, -1, -1, -1},
    { 0,  9,  5,  1, 11,  4, 11,  7,  4,  7,  6,  4, -1, -1, -1, -1},
    { 1, 11,  6, 11,  7,  6,  1,  6,  5,  6,  8,  5,  8,  9,  5, -1},
    { 1,  5, 10,  5,  7, 10,  7,  6, 10, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  8,  1,  5, 10,  5,  7, 10,  7,  6, 10, -1, -1, -1, -1},
    { 0,  9,  1,  9,  7,  1,  7,  6,  1,  6, 10,  1, -1, -1, -1, -1},
    { 1,  4,  9,  4,  8,  9,  1,  9, 10,  9,  7, 10,  7,  6, 10, -1},
    { 4,  5,  6,  5,  7,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  5,  8,  5,  7,  8,  7,  6,  8, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  4,  9,  7,  4,  7,  6,  4, -1, -1, -1, -1, -1, -1, -1},
    { 6,  8,  7,  8,  9,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 2,  8,  7,  8, 10,  7, 10, 11,  7, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  2,  4, 10,  2, 10, 11,  2, 11,  7,  2, -1, -1, -1, -1},
    { 0,  9,  5,  2,  8,  7,  8, 10,  7, 10, 11,  7, -1, -1, -1, -1},
    { 2,  9,  4,  9,  5,  4,  2,  4,  7,  4, 10,  7, 10, 11,  7, -1},
    { 1, 11,  4, 11,  7,  4,  7,  2,  4,  2,  8,  4, -1, -1, -1, -1},
    { 0,  1,  2,  1, 11,  2, 11,  7,  2, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  5,  1, 11,  4, 11,  7,  4,  7,  2,  4,  2,  8,  4, -1},
    { 1, 11,  2, 11,  7,  2,  1,  2,  5,  2,  9,  5, -1, -1, -1, -1},
    { 1,  5, 10,  5,  7, 10,  7,  2, 10,  2,  8, 10, -1, -1, -1, -1},
    { 0,  4,  2,  4, 10,  2, 10,  1,  2,  1,  5,  2,  5,  7,  2, -1},
    { 0,  9,  1,  9,  7,  1,  7,  2,  1,  2,  8,  1,  8, 10,  1, -1},
    { 1,  4, 10,  2,  9,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 2,  8,  7,  8,  4,  7,  4,  5,  7, -1, -1, -1, -1, -1, -1, -1},
    { 0,  5,  2,  5,  7,  2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  4,  9,  7,  4,  7,  2,  4,  2,  8,  4, -1, -1, -1, -1},
    { 2,  9,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 2,  6,  9,  6, 10,  9, 10, 11,  9, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  8,  2,  6,  9,  6, 10,  9, 10, 11,  9, -1, -1, -1, -1},
    { 0,  2,  5,  2,  6,  5,  6, 10,  5, 10, 11,  5, -1, -1, -1, -1},
    { 2,  6, 11,  6, 10, 11,  2, 11,  8, 11,  5,  8,  5,  4,  8, -1},
    { 1, 11,  4, 11,  9,  4,  9,  2,  4,  2,  6,  4, -1, -1, -1, -1},
    { 0,  1,  8,  1, 11,  8, 11,  9,  6,  9,  2,  6, 11,  6,  8, -1},
    { 0,  2,  5,  2,  6,  5,  6,  4, 11,  4,  1, 11,  6, 11,  5, -1},
    { 1, 11,  5,  2,  6,  8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  5, 10,  5,  9, 10,  9,  2, 10,  2,  6, 10, -1, -1, -1, -1},
    { 0,  4,  8,  1,  5, 10,  5,  9, 10,  9,  2, 10,  2,  6, 10, -1},
    { 0,  2,  1,  2,  6,  1,  6, 10,  1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  4,  2,  4,  8,  2,  1,  2, 10,  2,  6, 10, -1, -1, -1, -1},
    { 2,  6,  9,  6,  4,  9,  4,  5,  9, -1, -1, -1, -1, -1, -1, -1},
    { 0,  5,  8,  5,  9,  6,  9,  2,  6,  5,  6,  8, -1, -1, -1, -1},
    { 0,  2,  4,  2,  6,  4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 2,  6,  8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 8, 10,  9, 10, 11,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  9,  4, 10,  9, 10, 11,  9, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  5,  8, 10,  5, 10, 11,  5, -1, -1, -1, -1, -1, -1, -1},
    { 4, 10,  5, 10, 11,  5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1, 11,  4, 11,  9,  4,  9,  8,  4, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  9,  1, 11,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  5,  8,  4, 11,  4,  1, 11,  8, 11,  5, -1, -1, -1, -1},
    { 1, 11,  5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  5, 10,  5,  9, 10,  9,  8, 10, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  9,  4, 10,  9, 10,  1,  9,  1,  5,  9, -1, -1, -1, -1},
    { 0,  8,  1,  8, 10,  1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  4, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 4,  5,  8,  5,  9,  8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  5,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
};

struct McVol { uint32_t N; const float* vol; float level; };

static __device__ inline void mc_ijk(const McVol& m, uint64_t id, uint32_t* ijk) {
    const uint64_t N = m.N;
    ijk[0] = (uint32_t)(id / (N * N)); ijk[1] = (uint32_t)(id / N % N); ijk[2] = (uint32_t)(id % N);
}
static __device__ inline uint64_t mc_stride(const McVol& m, int a) { return a == 0 ? (uint64_t)m.N * m.N : (a == 1 ? m.N : 1); }
// does the voxel at flat index q own a crossed edge along axis a?
static __device__ inline bool mc_cross(const McVol& m, uint64_t q, const uint32_t* ijk, int a) {
    if (ijk[a] + 1 >= m.N) return false;
    return (m.vol[q] > m.level) != (m.vol[q + mc_stride(m, a)] > m.level);
}
// the cell's case, or 0 where the voxel is no cell's lowest corner
static __device__ inline uint32_t mc_case(const McVol& m, uint64_t q, const uint32_t* ijk) {
    if (ijk[0] + 1 >= m.N || ijk[1] + 1 >= m.N || ijk[2] + 1 >= m.N) return 0;
    uint32_t k = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if (m.vol[q + (c & 1) * mc_stride(m, 0) + ((c >> 1) & 1) * mc_stride(m, 1) + (c >> 2) * mc_stride(m, 2)] > m.level) k |= 1u << c;
    return k;
}
static __device__ inline uint32_t mc_triangles(uint32_t k) {
    uint32_t n = 0;
    while (n < 5 && GC_TRI[k][3 * n] >= 0) ++n;
    return n;
}

// rank [N^3]: the voxel's first vertex inside its workgroup; bsum_v / bsum_t [workgroups]: the workgroup's vertices and triangles
__global__ void __launch_bounds__(GC_BLOCK) k_mc_count(McVol m, uint32_t* __restrict__ rank, uint32_t* __restrict__ bsum_v, uint32_t* __restrict__ bsum_t) {
    const uint64_t id = (uint64_t)blockIdx.x * GC_BLOCK + threadIdx.x, total = (uint64_t)m.N * m.N * m.N;
    uint32_t nv = 0, nt = 0, ijk[3];
    if (id < total) {
        mc_ijk(m, id, ijk);
#pragma unroll
        for (int a = 0; a < 3; ++a) nv += mc_cross(m, id, ijk, a) ? 1u : 0u;
        nt = mc_triangles(mc_case(m, id, ijk));
    }
    uint32_t sum;
    const uint32_t ex = xr_block_excl(nv | (nt << 16), &sum);      // at most 3 and 5 per thread: both fit 16 bits over 256 threads
    if (id < total) rank[id] = ex & 0xffffu;
    if (threadIdx.x == 0) { bsum_v[blockIdx.x] = sum & 0xffffu; bsum_t[blockIdx.x] = sum >> 16; }
}

static __device__ inline void mc_gradient(const McVol& m, uint64_t q, const uint32_t* ijk, float* g) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const uint64_t s = mc_stride(m, a);
        if (ijk[a] == 0) g[a] = m.vol[q + s] - m.vol[q];
        else if (ijk[a] + 1 >= m.N) g[a] = m.vol[q] - m.vol[q - s];
        else g[a] = (m.vol[q + s] - m.vol[q - s]) * 0.5f;
    }
}

__global__ void __launch_bounds__(GC_BLOCK) k_mc_verts(McVol m, const uint32_t* __restrict__ rank, const uint32_t* __restrict__ bbase_v, uint32_t Nv,
                                                      float* __restrict__ verts, float* __restrict__ normals) {
    const uint64_t id = (uint64_t)blockIdx.x * GC_BLOCK + threadIdx.x;
    if (id >= (uint64_t)m.N * m.N * m.N) return;
    uint32_t ijk[3];
    mc_ijk(m, id, ijk);
    uint64_t vid = (uint64_t)bbase_v[blockIdx.x] + rank[id];
    for (int a = 0; a < 3; ++a) {
        if (!mc_cross(m, id, ijk, a)) continue;
        if (vid >= Nv) return;                                     // (Nv is the scan's total: never taken)
        const uint64_t q = id + mc_stride(m, a);
        uint32_t ijk_b[3] = {ijk[0], ijk[1], ijk[2]};
        ijk_b[a] += 1;
        const float va = m.vol[id], vb = m.vol[q];
        const float t = (m.level - va) / (vb - va);
        float ga[3], gb[3], n[3];
        mc_gradient(m, id, ijk, ga);
        mc_gradient(m, q, ijk_b, gb);
#pragma unroll
        for (int c = 0; c < 3; ++c) n[c] = ga[c] + t * (gb[c] - ga[c]);
        float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
        if (len < 1e-9f) len = 1e-9f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            verts[3 * vid + c] = (float)ijk[c] + (c == a ? t : 0.f);
            normals[3 * vid + c] = -n[c] / len;                    // towards lower occupancy: out of the body
        }
        ++vid;
    }
}

__global__ void __launch_bounds__(GC_BLOCK) k_mc_tris(McVol m, const uint32_t* __restrict__ rank, const uint32_t* __restrict__ bbase_v,
                                                     const uint32_t* __restrict__ bbase_t, uint32_t T, int32_t* __restrict__ faces) {
    const uint64_t id = (uint64_t)blockIdx.x * GC_BLOCK + threadIdx.x, total = (uint64_t)m.N * m.N * m.N;
    uint32_t k = 0, ijk[3] = {0, 0, 0};
    if (id < total) { mc_ijk(m, id, ijk); k = mc_case(m, id, ijk); }
    const uint32_t nt = mc_triangles(k);
    uint32_t sum;
    uint64_t tri = (uint64_t)xr_block_excl(nt, &sum);
    if (nt == 0) return;
    tri += bbase_t[blockIdx.x];
    for (uint32_t t = 0; t < nt; ++t, ++tri) {
        if (tri >= T) return;                                      // (T is the scan's total: never taken)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int e = GC_TRI[k][3 * t + c], axis = e >> 2, u = e & 1, v = (e >> 1) & 1;
            uint32_t o[3];
            o[axis] = ijk[axis];
            o[axis == 0 ? 1 : 0] = ijk[axis == 0 ? 1 : 0] + u;
            o[axis == 2 ? 1 : 2] = ijk[axis == 2 ? 1 : 2] + v;
            const uint64_t q = ((uint64_t)o[0] * m.N + o[1]) * m.N + o[2];
            uint32_t vid = bbase_v[q / GC_BLOCK] + rank[q];
            for (int b = 0; b < axis; ++b) vid += mc_cross(m, q, o, b) ? 1u : 0u;     // the owner's vertices come in axis order
            faces[3 * tri + c] = (int32_t)vid;
        }
    }
}

// (v - N / 2) / N ext, / spatial_freq + center: N, not N - 1, is the reference's
__global__ void __launch_bounds__(GC_BLOCK) k_gc_world(const float* __restrict__ verts, uint32_t Nv, double n, double e0, double e1, double e2, double sf,
                                                      const float* __restrict__ center, double* __restrict__ world, float* __restrict__ pts) {
    const uint32_t i = blockIdx.x * GC_BLOCK + threadIdx.x;
    if (i >= Nv) return;
    const double ext[3] = {e0, e1, e2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double w = (((double)verts[3ull * i + c] - n / 2.0) / n * ext[c]) / sf + (double)center[c];
        world[3ull * i + c] = w;
        pts[3ull * i + c] = (float)w;
    }
}

__global__ void __launch_bounds__(GC_BLOCK) k_gc_point_rows(GrHull a, const float* __restrict__ pts, const float* __restrict__ dirs, uint32_t n,
                                                           float* __restrict__ xy, float* __restrict__ attdirs) {
    const uint64_t i = (uint64_t)blockIdx.x * GC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]}, q[3] = {dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]};
    for (uint32_t v = 0; v < a.V; ++v) {
        float s[2], z;
        gr_project(a, v, p, s, &z);
        xy[(i * a.V + v) * 2] = s[0]; xy[(i * a.V + v) * 2 + 1] = s[1];
    }
    gr_att_directions(a, p, q, attdirs + i * (a.V + 1) * 3);
}

// ------------------------------------------------------------------------------------------ Laplacian filter (double)
__global__ void __launch_bounds__(GC_BLOCK) k_lap_step(const double* __restrict__ v, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                      uint32_t Nv, uint32_t nnz, double lamb, double* __restrict__ out) {
    const uint32_t i = blockIdx.x * GC_BLOCK + threadIdx.x;
    if (i >= Nv) return;
    uint32_t b = (uint32_t)rowptr[i], e = (uint32_t)rowptr[i + 1];
    if (e > nnz) e = nnz;
    double s[3] = {0.0, 0.0, 0.0};
    uint32_t deg = 0;
    for (uint32_t k = b; k < e; ++k) {
        const uint32_t j = (uint32_t)cols[k];
        if (j >= Nv) continue;
        s[0] += v[3ull * j]; s[1] += v[3ull * j + 1]; s[2] += v[3ull * j + 2];
        ++deg;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double x = v[3ull * i + c];
        out[3ull * i + c] = deg ? x + lamb * (s[c] / (double)deg - x) : x;
    }
}

// a fixed tree over the workgroup's 256 values: the same order of additions on every launch
static __device__ inline double gc_block_sum(double x) {
    __shared__ double s_x[GC_BLOCK];
    __syncthreads();
    s_x[threadIdx.x] = x;
    __syncthreads();
    for (uint32_t h = GC_BLOCK / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h) s_x[threadIdx.x] += s_x[threadIdx.x + h];
        __syncthreads();
    }
    return s_x[0];
}

__global__ void __launch_bounds__(GC_BLOCK) k_vol_partial(const double* __restrict__ v, const int32_t* __restrict__ faces, uint32_t T, uint32_t Nv,
                                                         double* __restrict__ partial) {
    const uint32_t t = blockIdx.x * GC_BLOCK + threadIdx.x;
    double d = 0.0;
    if (t < T) {
        const uint32_t i = (uint32_t)faces[3ull * t], j = (uint32_t)faces[3ull * t + 1], k = (uint32_t)faces[3ull * t + 2];
        if (i < Nv && j < Nv && k < Nv) {
            const double* a = v + 3ull * i; const double* b = v + 3ull * j; const double* c = v + 3ull * k;
            d = (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2])) + a[2] * (b[0] * c[1] - b[1] * c[0]);
        }
    }
    const double s = gc_block_sum(d);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void __launch_bounds__(GC_BLOCK) k_vol_final(const double* __restrict__ partial, uint32_t n, double* __restrict__ out) {
    double s = 0.0;
    for (uint32_t k = threadIdx.x; k < n; k += GC_BLOCK) s += partial[k];
    s = gc_block_sum(s);
    if (threadIdx.x == 0) out[0] = s / 6.0;
}

__global__ void __launch_bounds__(GC_BLOCK) k_lap_scale(double* __restrict__ v, uint64_t n, const double* __restrict__ vols) {
    const uint64_t i = (uint64_t)blockIdx.x * GC_BLOCK + threadIdx.x;
    if (i >= n) return;
    v[i] = v[i] * cbrt(vols[0] / vols[1]);
}

// ------------------------------------------------------------------------------------------ entry points
static int gc_views(GrHull* a, const char* fn, const float* w2c, const float* cams, uint32_t cam_cols, uint32_t V, const float* masks, int H, int W,
                    float width, float height) {
    if (!w2c || !cams) { xr_set_error("%s: null pointer", fn); return XR_EINVAL; }
    if (V < 1 || V > XR_GNR_MAX_VIEWS) { xr_set_error("%s: 1 .. XR_GNR_MAX_VIEWS source views", fn); return XR_EINVAL; }
    if (cam_cols < 4 || (cam_cols > 6 && cam_cols < 9)) { xr_set_error("%s: a camera row has 4 .. 6 entries, or at least 9 with distortion", fn); return XR_EINVAL; }
    if (masks && (H < 1 || W < 1 || H > (1 << 14) || W > (1 << 14))) { xr_set_error("%s: bad mask size", fn); return XR_EINVAL; }
    if (!(width > 0.f) || !(height > 0.f)) { xr_set_error("%s: the image size must be positive", fn); return XR_EINVAL; }
    memset(a, 0, sizeof(*a));
    a->V = V; a->w2c = w2c; a->cams = cams; a->cam_cols = cam_cols; a->masks = masks; a->H = H; a->W = W; a->width = width; a->height = height;
    return 0;
}

static int gc_grid(GcGrid* g, const char* fn, uint32_t N, const double* lin9, double sf, const float* center3, const float* coords) {
    if (N < 2 || N > GC_MAX_N) { xr_set_error("%s: 2 .. XR_GNR_RECON_MAX_N points per axis", fn); return XR_EINVAL; }
    if (!coords && (!lin9 || !center3 || !(sf == sf) || sf == 0.0)) { xr_set_error("%s: the grid needs its linspaces, centre and a non-zero spatial_freq", fn); return XR_EINVAL; }
    memset(g, 0, sizeof(*g));
    g->N = N; g->sf = sf; g->center = center3; g->coords = coords;
    if (lin9) for (int a = 0; a < 3; ++a) { g->start[a] = lin9[3 * a]; g->stop[a] = lin9[3 * a + 1]; g->step[a] = lin9[3 * a + 2]; }
    return 0;
}

static int gc_level(GcLevel* l, const char* fn, uint32_t N, uint32_t reso) {
    if (N < 2 || N > GC_MAX_N || reso < 1 || reso >= N) { xr_set_error("%s: bad grid size or level", fn); return XR_EINVAL; }
    l->N = N; l->reso = reso; l->L = (N - 1) / reso + 1;
    return 0;
}

extern "C" int xr_gnr_recon_hull(uint32_t N, const double* lin9, double spatial_freq, const float* center3, const float* coords, const float* w2c,
                                 const float* cams, uint32_t cam_cols, uint32_t V, const float* masks, int H, int W, float width, float height,
                                 uint8_t* state, void* stream) {
    GcGrid g; GrHull a;
    int rc = gc_grid(&g, __func__, N, lin9, spatial_freq, center3, coords);
    if (rc == 0) rc = gc_views(&a, __func__, w2c, cams, cam_cols, V, masks, H, W, width, height);
    if (rc != 0) return rc;
    XR_REQUIRE(masks && state, "null pointer");
    hipLaunchKernelGGL(k_gc_hull, dim3(xr_div_up((uint64_t)N * N * N, GC_BLOCK)), dim3(GC_BLOCK), 0, (hipStream_t)stream, g, a, state);
    XR_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t xr_gnr_recon_select_workspace_bytes(uint32_t N, uint32_t reso) {
    GcLevel l;
    if (N < 2 || N > GC_MAX_N || reso < 1 || reso >= N) return 0;
    l.L = (N - 1) / reso + 1;
    const uint32_t nb = xr_div_up((uint64_t)l.L * l.L * l.L, GC_BLOCK);
    return (size_t)(nb + xr_div_up(nb, GC_BLOCK)) * sizeof(uint32_t);
}

extern "C" int xr_gnr_recon_select_count(uint32_t N, uint32_t reso, const uint8_t* state, void* workspace, size_t workspace_bytes, int32_t* total,
                                         void* stream) {
    GcLevel l;
    const int rc = gc_level(&l, __func__, N, reso);
    if (rc != 0) return rc;
    XR_REQUIRE(state && workspace && total, "null pointer");
    if (workspace_bytes < xr_gnr_recon_select_workspace_bytes(N, reso)) { xr_set_error("%s: workspace too small", __func__); return XR_ENOMEM; }
    const uint32_t nb = xr_div_up((uint64_t)l.L * l.L * l.L, GC_BLOCK);
    hipLaunchKernelGGL(k_gc_sel_count, dim3(nb), dim3(GC_BLOCK), 0, (hipStream_t)stream, l, state, (uint32_t*)workspace);
    xr_scan_two_level((hipStream_t)stream, nb, (uint32_t*)workspace, (uint32_t*)workspace + nb, total);
    XR_LAUNCH_CHECK();
    return 0;
}

extern "C" int xr_gnr_recon_select_write(uint32_t N, uint32_t reso, const double* lin9, double spatial_freq, const float* center3, const float* coords,
                                         const float* w2c, const float* cams, uint32_t cam_cols, uint32_t V, float width, float height,
                                         const uint8_t* state, const void* workspace, uint32_t M, int32_t* flat, float* pts, float* xy, void* stream) {
    if (M == 0) return 0;
    GcLevel l; GcGrid g; GrHull a;
    int rc = gc_level(&l, __func__, N, reso);
    if (rc == 0) rc = gc_grid(&g, __func__, N, lin9, spatial_freq, center3, coords);
    if (rc == 0) rc = gc_views(&a, __func__, w2c, cams, cam_cols, V, nullptr, 0, 0, width, height);
    if (rc != 0) return rc;
    XR_REQUIRE(state && workspace && flat && pts && xy, "null pointer");
    XR_REQUIRE((uint64_t)M <= (uint64_t)l.L * l.L * l.L, "more selected points than lattice points");
    hipLaunchKernelGGL(k_gc_sel_write, dim3(xr_div_up((uint64_t)l.L * l.L * l.L, GC_BLOCK)), dim3(GC_BLOCK), 0, (hipStream_t)stream, l, g, a, state,
                       (const uint32_t*)workspace, M, flat, pts, xy);
    XR_LAUNCH_CHECK();
    return 0;
}

extern "C" int xr_gnr_recon_scatter(const int32_t* flat, const float* values, uint32_t M, int apply_sigmoid, float gamma, uint32_t N, float* volume,
                                    uint8_t* state, void* stream) {
    if (M == 0) return 0;
    XR_REQUIRE(N >= 2 && N <= GC_MAX_N, "2 .. XR_GNR_RECON_MAX_N points per axis");
    XR_REQUIRE(flat && values && volume && state, "null pointer");
    hipLaunchKernelGGL(k_gc_scatter, dim3(xr_div_up(M, GC_BLOCK)), dim3(GC_BLOCK), 0, (hipStream_t)stream, flat, values, M, apply_sigmoid ? 1 : 0, gamma,
                       (uint64_t)N * N * N, volume, state);
    XR_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t xr_gnr_recon_fold_workspace_bytes(uint32_t N, uint32_t reso) {
    if (N < 2 || N > GC_MAX_N || reso < 2 || reso >= N) return 0;
    const uint64_t G = (N - 1) / reso;
    return (size_t)(G * G * G * 5);
}

extern "C" int xr_gnr_recon_fold(uint32_t N, uint32_t reso, float* volume, uint8_t* state, void* workspace, size_t workspace_bytes, void* stream) {
    XR_REQUIRE(N >= 2 && N <= GC_MAX_N && reso >= 2 && reso < N, "bad grid size or level");
    XR_REQUIRE(volume && state && workspace, "null pointer");
    XR_REQUIRE(((uintptr_t)workspace & 3u) == 0, "the workspace must be 4-byte aligned");
    if (workspace_bytes < xr_gnr_recon_fold_workspace_bytes(N, reso)) { xr_set_error("%s: workspace too small", __func__); return XR_ENOMEM; }
    GcFold f;
    f.N = N; f.reso = reso; f.G = (N - 1) / reso;
    const uint64_t cells = (uint64_t)f.G * f.G * f.G, P = (uint64_t)f.G * reso + 1;
    float* fill = (float*)workspace;
    uint8_t* skip = (uint8_t*)workspace + cells * 4;
    hipLaunchKernelGGL(k_gc_cells, dim3(xr_div_up(cells, GC_BLOCK)), dim3(GC_BLOCK), 0, (hipStream_t)stream, f, (const float*)volume, (const uint8_t*)state, fill, skip);
    hipLaunchKernelGGL(k_gc_fill, dim3(xr_div_up(P * P * P, GC_BLOCK)), dim3(GC_BLOCK), 0, (hipStream_t)stream, f, (const float*)fill, (const uint8_t*)skip, volume, state);
    XR_LAUNCH_CHECK();
    return 0;
}

// workspace: rank [N^3] | bsum_v [nb] | bsum_t [nb] | the scans' sums [2 nb / 256], uint32 each
extern "C" size_t xr_gnr_recon_surface_workspace_bytes(uint32_t N) {
    if (N < 2 || N > GC_MAX_N) return 0;
    const uint64_t total = (uint64_t)N * N * N;
    const uint32_t nb = xr_div_up(total, GC_BLOCK);
    return (size_t)((total + 2ull * nb + 2ull * xr_div_up(nb, GC_BLOCK)) * sizeof(uint32_t));
}

extern "C" int xr_gnr_recon_surface_count(const float* volume, uint32_t N, float level, void* workspace, size_t workspace_bytes, int32_t* totals2,
                                          void* stream) {
    XR_REQUIRE(N >= 2 && N <= GC_MAX_N, "2 .. XR_GNR_RECON_MAX_N points per axis");
    XR_REQUIRE(volume && workspace && totals2, "null pointer");
    XR_REQUIRE(((uintptr_t)workspace & 3u) == 0, "the workspace must be 4-byte aligned");
    if (workspace_bytes < xr_gnr_recon_surface_workspace_bytes(N)) { xr_set_error("%s: workspace too small", __func__); return XR_ENOMEM; }
    const uint64_t total = (uint64_t)N * N * N;
    const uint32_t nb = xr_div_up(total, GC_BLOCK);
    uint32_t* rank = (uint32_t*)workspace;
    uint32_t* bv = rank + total;
    uint32_t* bt = bv + nb;
    McVol m;
    m.N = N; m.vol = volume; m.level = level;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mc_count, dim3(nb), dim3(GC_BLOCK), 0, st, m, rank, bv, bt);
    xr_scan_two_level(st, nb, bv, bt + nb, totals2);
    xr_scan_two_level(st, nb, bt, bt + nb + xr_div_up(nb, GC_BLOCK), totals2 + 1);
    XR_LAUNCH_CHECK();
    return 0;
}

extern "C" int xr_gnr_recon_surface_write(const float* volume, uint32_t N, float level, const void* workspace, uint32_t Nv, uint32_t T, float* verts,
                                          float* normals, int32_t* faces, void* stream) {
    if (Nv == 0 && T == 0) return 0;
    XR_REQUIRE(N >= 2 && N <= GC_MAX_N, "2 .. XR_GNR_RECON_MAX_N points per axis");
    XR_REQUIRE(volume && workspace && verts && normals && (T == 0 || faces), "null pointer");
    const uint64_t total = (uint64_t)N * N * N;
    const uint32_t nb = xr_div_up(total, GC_BLOCK);
    const uint32_t* rank = (const uint32_t*)workspace;
    const uint32_t* bv = rank + total;
    const uint32_t* bt = bv + nb;
    McVol m;
    m.N = N; m.vol = volume; m.level = level;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mc_verts, dim3(nb), dim3(GC_BLOCK), 0, st, m, rank, bv, Nv, verts, normals);
    if (T > 0) hipLaunchKernelGGL(k_mc_tris, dim3(nb), dim3(GC_BLOCK), 0, st, m, rank, bv, bt, T, faces);
    XR_LAUNCH_CHECK();
    return 0;
}

extern "C" int xr_gnr_recon_world(const float* verts_idx, uint32_t Nv, uint32_t N, const double* extent3, double spatial_freq, const float* center3,
                                  double* verts, float* pts, void* stream) {
    if (Nv == 0) return 0;
    XR_REQUIRE(verts_idx && extent3 && center3 && verts && pts, "null pointer");
    XR_REQUIRE(N >= 1 && spatial_freq != 0.0, "bad grid size or spatial_freq");
    hipLaunchKernelGGL(k_gc_world, dim3(xr_div_up(Nv, GC_BLOCK)), dim3(GC_BLOCK), 0, (hipStream_t)stream, verts_idx, Nv, (double)N, extent3[0], extent3[1],
                       extent3[2], spatial_freq, center3, verts, pts);
    XR_LAUNCH_CHECK();
    return 0;
}

extern "C" int xr_gnr_recon_point_rows(const float* pts, const float* dirs, uint32_t n, const float* w2c, const float* cams, uint32_t cam_cols, uint32_t V,
                                       float width, float height, const float* cam_c, const float* rot9, float* xy, float* attdirs, void* stream) {
    if (n == 0) return 0;
    GrHull a;
    const int rc = gc_views(&a, __func__, w2c, cams, cam_cols, V, nullptr, 0, 0, width, height);
    if (rc != 0) return rc;
    XR_REQUIRE(pts && dirs && cam_c && xy && attdirs, "null pointer");
    a.cam_c = cam_c; a.rot = rot9;
    hipLaunchKernelGGL(k_gc_point_rows, dim3(xr_div_up(n, GC_BLOCK)), dim3(GC_BLOCK), 0, (hipStream_t)stream, a, pts, dirs, n, xy, attdirs);
    XR_LAUNCH_CHECK();
    return 0;
}

// workspace: the second vertex buffer [Nv, 3] | vols [2] | partial sums [workgroups over T], doubles
extern "C" size_t xr_gnr_recon_smooth_workspace_bytes(uint32_t Nv, uint32_t T) {
    return (size_t)((3ull * Nv + 2 + xr_div_up(T, GC_BLOCK) + 1) * sizeof(double));
}

extern "C" int xr_gnr_recon_smooth(double* verts, uint32_t Nv, const int32_t* faces, uint32_t T, const int32_t* rowptr, const int32_t* cols, uint32_t nnz,
                                   int iterations, double lamb, void* workspace, size_t workspace_bytes, void* stream) {
    if (Nv == 0 || T == 0 || iterations <= 0) return 0;
    XR_REQUIRE(verts && faces && rowptr && workspace && (nnz == 0 || cols), "null pointer");
    XR_REQUIRE(((uintptr_t)workspace & 7u) == 0, "the workspace must be 8-byte aligned");
    XR_REQUIRE(iterations <= 1024, "at most 1024 iterations");
    if (workspace_bytes < xr_gnr_recon_smooth_workspace_bytes(Nv, T)) { xr_set_error("%s: workspace too small", __func__); return XR_ENOMEM; }
    hipStream_t st = (hipStream_t)stream;
    double* other = (double*)workspace;
    double* vols = other + 3ull * Nv;
    double* partial = vols + 2;
    const uint32_t nbt = xr_div_up(T, GC_BLOCK), nbv = xr_div_up(Nv, GC_BLOCK);
    double* cur = verts;
    double* nxt = other;
    hipLaunchKernelGGL(k_vol_partial, dim3(nbt), dim3(GC_BLOCK), 0, st, (const double*)cur, faces, T, Nv, partial);
    hipLaunchKernelGGL(k_vol_final, dim3(1), dim3(GC_BLOCK), 0, st, (const double*)partial, nbt, vols);
    for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(k_lap_step, dim3(nbv), dim3(GC_BLOCK), 0, st, (const double*)cur, rowptr, cols, Nv, nnz, lamb, nxt);
        hipLaunchKernelGGL(k_vol_partial, dim3(nbt), dim3(GC_BLOCK), 0, st, (const double*)nxt, faces, T, Nv, partial);
        hipLaunchKernelGGL(k_vol_final, dim3(1), dim3(GC_BLOCK), 0, st, (const double*)partial, nbt, vols + 1);
        hipLaunchKernelGGL(k_lap_scale, dim3(xr_div_up(3ull * Nv, GC_BLOCK)), dim3(GC_BLOCK), 0, st, nxt, 3ull * Nv, (const double*)vols);
        double* t = cur; cur = nxt; nxt = t;
    }
    if (cur != verts) XR_HIP(hipMemcpyAsync(verts, cur, 3ull * Nv * sizeof(double), hipMemcpyDeviceToDevice, st));
    XR_LAUNCH_CHECK();
    return 0;
}
