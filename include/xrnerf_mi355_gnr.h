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
#define XR_GNR_MAX_VIEWS 8           /* source views of the renderer's stages */

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

/* ---- the renderer's stages (xrnerf_amd/csrc/xr_gnr_render.hip): what GnrRenderer.render_rays does around the network ----
 * R rays of S samples, V <= XR_GNR_MAX_VIEWS source views.  rays [R,6] = (start, end); t_vals [R,S]; the sample point is
 * end t + (1 - t) start.  w2c [V,4,4] row-major; cams [V,cam_cols] = fx, fy, cx, cy, then (cam_cols > 6) k1, k2, p1, p2, k3 at
 * entries 4 .. 8; masks [V,H,W]; width / height = what the pixel coordinates are divided by (loadSize).  A point is inside when, in
 * every view, torch's grid_sample(mode='nearest', align_corners=False, zero padding) of the mask at its projection is > 0; a point
 * with a non-finite projected coordinate is outside (torch leaves that case unspecified). */

/* count / scan: rank [R S] (workspace: a survivor's rank inside its ray, -1 otherwise), table [R,2] = (count, base) per ray,
 * total [1] = M.  Three launches; the caller reads total ONCE to size the next call's outputs.  R = 0 clears total. */
int xr_gnr_hull_count(const float* rays, const float* t_vals, uint32_t R, uint32_t S, const float* w2c, const float* cams,
                      uint32_t cam_cols, uint32_t V, const float* masks, int H, int W, float width, float height, int32_t* rank,
                      int32_t* table, int32_t* total, void* stream);
/* ranked write, survivors in ascending flat index (the order of torch.nonzero): pts [M,3], idx [M] (flat index r S + s), xy [M,V,2]
 * (normalised), z [M,V] (camera depth); with depth [V,H,W] (smpl['depth'], nearest sample d): vis [M,V] bytes = (z - d <= 0) & (d > 0);
 * with attdirs [M,V+1,3]: make_att_input's perspective branch -- [start - end | cam_c [V,3] - point], each times rot9 (row vector
 * times the row-major matrix; may be null), over clamp(norm, 1e-9).  depth, vis, attdirs, cam_c, rot9 may be null.  M = 0: no-op. */
int xr_gnr_hull_write(const float* rays, const float* t_vals, uint32_t R, uint32_t S, const float* w2c, const float* cams,
                      uint32_t cam_cols, uint32_t V, const float* masks, const float* depth, int H, int W, float width, float height,
                      const float* cam_c, const float* rot9, const int32_t* rank, const int32_t* table, uint32_t M, float* pts,
                      int32_t* idx, float* xy, float* z, uint8_t* vis, float* attdirs, void* stream);
/* pixel-aligned gather (the `feats is not None` half of make_nerf_input): bilinear samples, torch's grid_sample defaults
 * (align_corners=False, zero padding), its corner order and weight products.  feats [V,fh,fw,C] CHANNEL-LAST, C a multiple of 4,
 * 16-byte aligned; images [V,3,ih,iw], or [V,ih,iw,3] with images_channel_last.  Row (m V + v) of out starts at out + (m V + v) ld:
 * columns col0 .. col0 + C hold the features, the next 3 the sampled colour, the rest up to ld exact zeros; columns below col0 are
 * left alone.  source_rgb [M,V,3] holds the sampled colours again. */
int xr_gnr_gather(const float* xy, uint32_t M, uint32_t V, const float* feats, int fh, int fw, uint32_t C, const float* images, int ih,
                  int iw, int images_channel_last, float* out, uint32_t ld, uint32_t col0, float* source_rgb, void* stream);
/* the gather's gradient in the feature maps (needed when the encoder is trained): d_feats [V,fh,fw,C] channel-last, every element
 * written, from grad rows laid out like xr_gnr_gather's out (columns col0 .. col0 + C are read; the colour columns have no trained
 * source).  64-bit fixed point: the largest |grad|, one scale for the call, integer atomic adds, one conversion -- two runs give the
 * same bits; a NaN or infinite entry contributes nothing.  Four launches and a clear of the workspace (8-byte aligned, at least
 * xr_gnr_gather_backward_workspace_bytes). */
size_t xr_gnr_gather_backward_workspace_bytes(uint32_t V, int fh, int fw, uint32_t C);
int xr_gnr_gather_backward(const float* xy, uint32_t M, uint32_t V, const float* grad, uint32_t ld, uint32_t col0, int fh, int fw,
                           uint32_t C, float* d_feats, void* workspace, size_t workspace_bytes, void* stream);
/* blend compositor (make_nerf_output and the lines around it), one wave per ray, the ray's survivors in its lanes in sample order.  net [M,ld]:
 * columns 0 .. 2 colour, 3 density, 4 .. 4 + V attention over [own colour | V source colours]; source_rgb [M,V,3]; idx / table as
 * written by the hull; noise [R,S] is added to the density (null: inference).  alpha = 1 - exp(-relu(.)) uses no distances, the
 * transmittance is the running product of (1 - alpha) + 1e-10.  rgb_map [R,6], depth [R] over z = t z_near + (1 - t) z_far (have_z)
 * or 2 t - 1, acc [R], weights [R,S] (cleared here: zeros outside the hull), trans [M] (kept for the backward).  white: rgb_map + (1 - acc). */
int xr_gnr_composite_forward(const float* net, uint32_t ld, const float* source_rgb, const int32_t* idx, const int32_t* table,
                             const float* t_vals, const float* noise, uint32_t R, uint32_t S, uint32_t V, uint32_t M, int have_z,
                             float z_near, float z_far, int white, float* rgb_map, float* depth, float* acc, float* weights,
                             float* trans, void* stream);
/* d_net [M, 4 + V + 1] (every entry written) from d_rgb_map [R,6]; fixed summation order, no atomics */
int xr_gnr_composite_backward(const float* net, uint32_t ld, const float* source_rgb, const int32_t* idx, const int32_t* table,
                              const float* t_vals, const float* noise, uint32_t R, uint32_t S, uint32_t V, uint32_t M, int white,
                              const float* d_rgb_map, const float* trans, float* d_net, void* stream);

#ifdef __cplusplus
}
#endif
#endif
