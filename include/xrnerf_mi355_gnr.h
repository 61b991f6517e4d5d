/* GNR body-shape entry points of libxrnerf_mi355.so (xrnerf_amd/csrc/xr_gnr.hip): what the reference's `extensions/mesh_grid`
 * extension (MeshGridSearcher) is to configs/gnr/gnr_genebody.py -- a uniform grid over a triangle mesh with per-cell face lists, the
 * nearest-point and inside queries GnrRenderer.make_nerf_input makes through it, and the embedding half of make_nerf_input itself.
 * A header of their own, bound by their own ctypes table (xrnerf_amd/_lib.py GNR_SIGNATURES), like xrnerf_mi355_neuralbody.h.
 * Conventions of xrnerf_mi355.h: 0 or a negative XR_E* code (message: xr_last_error()); never throws, syncs or allocates; raw device
 * pointers, fp32, indices int32, contiguous; the launch goes to `stream`.  The same input gives the same bits.
 *
 * The grid.  `num3` = cells per axis (HOST ints), `min3` = the grid's lower corner (HOST floats), `step` = the cell edge; cell
 * (x, y, z) has the linear index (x num3[1] + y) num3[2] + z.  tri_num [cells] holds INCLUSIVE prefix counts, tri_idx [total] the
 * face id + 1 of every slot, a cell's slots ascending.  The reference's kernels are the specification, quirks included (DESIGN.md
 * section 14): the cell enumeration of a face's box divides in double precision by (width + 1e-8) and truncates, so some cells get a
 * face twice and others not at all; the closest point is a Lagrange-multiplier solve with fallbacks; the inside test counts
 * crossings in a 15-entry buffer.  A query whose result would read outside a table reads nothing: segment bounds are clamped to
 * [0, total], face ids to [0, F), vertex ids to [0, V), and every loop bound comes from num3.
 * XR_EINVAL (nothing launched): step <= 0 or not finite, a num3 entry < 1, more than XR_GNR_MAX_CELLS cells, V or F = 0 with work
 * to do.  N = 0 (and F = 0 for the grid build) is a no-op that returns 0. */
#ifndef XRNERF_MI355_GNR_H
#define XRNERF_MI355_GNR_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define XR_GNR_MAX_CELLS (1u << 28)
#define XR_GNR_VISITED 16            /* the inside test's buffer: entry 0 unused, 15 face ids */
#define XR_GNR_EMBED_COLS 10         /* 3 normalised point + 3 T-pose + 3 SDF direction + 1 SDF */

/* first pass: tri_num [cells] = the number of slots of every cell (cleared here), one thread per face, integer atomic adds.
 * status [2] (cleared here): status[1] becomes 1 when a face names a vertex outside [0, V); such a face is left out of both passes.
 * The caller scans tri_num inclusively (int32), copies its last entry to status[0] and reads status ONCE. */
int xr_gnr_grid_count(const float* verts, const int32_t* faces, uint32_t V, uint32_t F, float step, const float* min3, const int32_t* num3,
                      int32_t* tri_num, int32_t* status, void* stream);
/* second pass: tri_idx [total] from the scanned tri_num.  A face claims its slot in a cell with an atomic add on the cell's cursor
 * (cursor [cells], cleared here), then one thread per cell sorts its segment ascending: the reference's serial result.  Three launches. */
int xr_gnr_grid_fill(const float* verts, const int32_t* faces, uint32_t V, uint32_t F, float step, const float* min3, const int32_t* num3,
                     const int32_t* tri_num, int32_t total, int32_t* tri_idx, int32_t* cursor, void* stream);
/* nearest point of the mesh for pts [N,3], one thread per point, the reference's shell order and strict `<`:
 * near_faces [N] (the face id; `total` when no face was met; -1 for a point with a non-finite coordinate), near_pts [N,3], coeff [N,3]
 * (barycentric; both zero when no face was met, NaN for a non-finite point). */
int xr_gnr_nearest(const float* verts, const int32_t* faces, uint32_t V, uint32_t F, float step, const float* min3, const int32_t* num3,
                   const int32_t* tri_num, const int32_t* tri_idx, int32_t total, const float* pts, uint32_t N, int32_t* near_faces,
                   float* near_pts, float* coeff, void* stream);
/* signs [N]: +1 inside, -1 outside (and outside the grid, and for a non-finite point): parity of the distinct faces crossed on the way
 * to the nearest grid face along one axis. */
int xr_gnr_inside(const float* verts, const int32_t* faces, uint32_t V, uint32_t F, float step, const float* min3, const int32_t* num3,
                  const int32_t* tri_num, const int32_t* tri_idx, int32_t total, const float* pts, uint32_t N, float* signs, void* stream);
/* the embedding half of make_nerf_input with feats = None, one thread per point.  out row i = out + i ld, columns in the reference's
 * concatenation order: [pts_nml | pts (3)] [T-pose (3), use_t_pose] [reg_vecs / norm (3), tanh(20 norm sign) (1), use_smpl_sdf];
 * alpha [N] = (sign + 1) / 2 (use_smpl_sdf; may be null otherwise).  center3 / rot9 (row-major smpl['rot'][0]) are DEVICE floats
 * (per-frame data: no host read per call); scale = spatial_freq, half = width / 2.  Products with rot are sum_k ascending, un-fused.  A near face outside [0, F) gives NaN
 * T-pose columns. */
int xr_gnr_shape_embed(const float* pts, uint32_t N, const int32_t* near_faces, const float* near_pts, const float* signs,
                       const int32_t* faces, uint32_t F, const float* t_verts, uint32_t V, const float* center3, const float* rot9,
                       float scale, float half, int use_nml, int use_t_pose, int use_smpl_sdf, float* out, uint32_t ld, float* alpha,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
