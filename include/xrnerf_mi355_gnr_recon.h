/* GNR mesh-reconstruction entry points of libxrnerf_mi355.so (xrnerf_amd/csrc/xr_gnr_recon.hip): what GnrRenderer.reconstruct and
 * octree_reconstruct do around the network -- the grid's visual hull, the coarse-to-fine octree bookkeeping, the iso-surface with
 * welded vertices, the reference's vertex transform, trimesh's Laplacian filter and the inputs of the colour pass.  A header of its
 * own, bound by its own ctypes table (xrnerf_amd/_lib.py GNR_RECON_SIGNATURES).
 * Conventions of xrnerf_mi355_gnr.h: 0 or a negative XR_E* code (message: xr_last_error()); never throws, syncs or allocates; raw
 * device pointers, contiguous; the launch goes to `stream`.  The same input gives the same bits: no floating-point atomics, no atomic
 * cursor -- every compaction is count / scan / ranked write.
 *
 * The grid has N points per axis, C order: flat = (i N + j) N + k.  `volume` is fp32 [N^3]; `state` one byte per point, 1 = still to
 * be evaluated (the reference's `notprocessed`), 0 = processed.  `lin9` (HOST doubles) holds per axis (start, stop, step) of
 * np.linspace(start, stop, N), step = (stop - start) / (N - 1); a point is ((i step + start) / spatial_freq + center) evaluated in
 * double (the last point of an axis is `stop` itself, as in numpy) and rounded once to fp32.  With `coords` [N^3, 3] (fp32) the points
 * are read from it instead.  Views: w2c [V,4,4], cams [V,cam_cols], V <= XR_GNR_MAX_VIEWS, projected with the hull's arithmetic
 * (xr_gnr_hull_count).  XR_EINVAL launches nothing and leaves every output untouched. */
#ifndef XRNERF_MI355_GNR_RECON_H
#define XRNERF_MI355_GNR_RECON_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define XR_GNR_RECON_MAX_N 1024u     /* points per axis: flat indices fit int32 */

/* state [N^3] = 1 where all three indices are below N - 1 and every view's (dilated) mask [V,H,W] is > 0 at the nearest pixel of the
 * point's projection, else 0.  One launch; no coordinate array is written. */
int xr_gnr_recon_hull(uint32_t N, const double* lin9, double spatial_freq, const float* center3, const float* coords, const float* w2c,
                      const float* cams, uint32_t cam_cols, uint32_t V, const float* masks, int H, int W, float width, float height,
                      uint8_t* state, void* stream);

/* a level's test set: the points whose indices are multiples of `reso` and whose state is 1, in C order.  _count leaves per-workgroup
 * bases in `workspace` and the number M in total[0] (four launches: count, two-level scan); the caller reads M and sizes flat [M] (int32), pts [M,3] and
 * xy [M,V,2] (normalised projections, the layout xr_gnr_gather reads) for _write (one launch), which needs the same state bytes. */
size_t xr_gnr_recon_select_workspace_bytes(uint32_t N, uint32_t reso);
int xr_gnr_recon_select_count(uint32_t N, uint32_t reso, const uint8_t* state, void* workspace, size_t workspace_bytes, int32_t* total,
                              void* stream);
int xr_gnr_recon_select_write(uint32_t N, uint32_t reso, const double* lin9, double spatial_freq, const float* center3, const float* coords,
                              const float* w2c, const float* cams, uint32_t cam_cols, uint32_t V, float width, float height,
                              const uint8_t* state, const void* workspace, uint32_t M, int32_t* flat, float* pts, float* xy, void* stream);

/* volume[flat[m]] = apply_sigmoid ? 1 / (1 + exp(-(values[m] gamma))) : values[m]; state[flat[m]] = 0.  An index outside the grid
 * writes nothing. */
int xr_gnr_recon_scatter(const int32_t* flat, const float* values, uint32_t M, int apply_sigmoid, float gamma, uint32_t N, float* volume,
                         uint8_t* state, void* stream);

/* the fold after a level with reso >= 2, two launches.  First per coarse cell (corners at multiples of reso, (N - 1) / reso cells per
 * axis): min and max of the 8 corners; the cell is skipped when (double)max - (double)min < 0.01 and the state of its centre
 * (corner + reso / 2) is 1; its fill value is 0.5 (min + max) in double, rounded once.  Then per fine point: among the (up to 8) cells
 * whose closed block [corner, corner + reso]^3 holds it, the skipped one that is last in C order gives the point its value and
 * clears its state -- what the reference's serial loop over the skipped cells leaves behind.  workspace: 5 bytes per coarse cell. */
size_t xr_gnr_recon_fold_workspace_bytes(uint32_t N, uint32_t reso);
int xr_gnr_recon_fold(uint32_t N, uint32_t reso, float* volume, uint8_t* state, void* workspace, size_t workspace_bytes, void* stream);

/* the iso-surface of `volume` at `level`; a corner is inside when its value is > level.  Every voxel owns the three edges that leave
 * it along +0, +1, +2.  _count (seven launches: count, two two-level scans) leaves ranks in `workspace` (4 bytes per grid point + a
 * little over 8 per workgroup) and
 * totals2 = (vertices Nv, triangles T), -1 for a count that does not fit int32 (a dense noisy volume near XR_GNR_RECON_MAX_N: the
 * caller must then not call _write); the caller reads them and sizes verts [Nv,3], normals [Nv,3], faces [T,3] (int32) for _write
 * (two launches).  Vertices: owner-voxel C order, then axis order; position = a + (level - v_a) / (v_b - v_a) in index coordinates;
 * normal = minus the central-difference gradient (one-sided at the borders) interpolated with the same weight, over
 * clamp(norm, 1e-9): it points to lower values.  Triangles: cell C order, then table order, welded vertex ids, wound so that the face
 * normals agree with the vertex normals. */
size_t xr_gnr_recon_surface_workspace_bytes(uint32_t N);
int xr_gnr_recon_surface_count(const float* volume, uint32_t N, float level, void* workspace, size_t workspace_bytes, int32_t* totals2,
                               void* stream);
int xr_gnr_recon_surface_write(const float* volume, uint32_t N, float level, const void* workspace, uint32_t Nv, uint32_t T, float* verts,
                               float* normals, int32_t* faces, void* stream);

/* verts [Nv,3] (double) = ((verts_idx - N / 2) / N extent3) / spatial_freq + center3, in double (extent3: HOST doubles; N, not N - 1,
 * is the reference's); pts [Nv,3] = its fp32 rounding. */
int xr_gnr_recon_world(const float* verts_idx, uint32_t Nv, uint32_t N, const double* extent3, double spatial_freq, const float* center3,
                       double* verts, float* pts, void* stream);

/* per point the colour pass's inputs: xy [n,V,2] and make_att_input's directions attdirs [n,V+1,3] with the query direction dirs [n,3]
 * (cam_c [V,3]: the camera centres; rot9: row-major smpl['rot'][0] or null), by the hull's device functions. */
int xr_gnr_recon_point_rows(const float* pts, const float* dirs, uint32_t n, const float* w2c, const float* cams, uint32_t cam_cols, uint32_t V,
                            float width, float height, const float* cam_c, const float* rot9, float* xy, float* attdirs, void* stream);

/* `iterations` rounds of v <- v + lamb (mean of the edge neighbours - v), each followed by a scale of all vertices about the origin
 * by (vol0 / vol)^(1/3), vol = sum of det / 6 over the faces, in double and in place.  rowptr [Nv+1] / cols [nnz]: the neighbour lists
 * (CSR, each neighbour once); sums run in list order and the volume is a fixed-order sum. */
size_t xr_gnr_recon_smooth_workspace_bytes(uint32_t Nv, uint32_t T);
int xr_gnr_recon_smooth(double* verts, uint32_t Nv, const int32_t* faces, uint32_t T, const int32_t* rowptr, const int32_t* cols, uint32_t nnz,
                        int iterations, double lamb, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
