/* GNR body depth maps: the z-buffer rasteriser entry points of libxrnerf_mi355.so (xrnerf_amd/csrc/xr_gnr_raster.hip) -- the
 * reference's extensions/mesh_grid render.h (zbuffer_forward, process_one_tri, normalize_coeff) restated for gfx950 with its arithmetic
 * order and its quirks.  A header of its own, bound by its own ctypes table (xrnerf_amd/_lib.py
 * GNR_RASTER_SIGNATURES).
 * Conventions of xrnerf_mi355_gnr.h: 0 or a negative XR_E* code (message: xr_last_error()); never throws, syncs or allocates; raw
 * device pointers, contiguous; the launch goes to `stream`.  The same input gives the same bits: the only atomics are integer adds
 * (per-pixel vertex counts) and a 64-bit integer min (the z-buffer), and `visual` is only ever cleared.  XR_EINVAL launches nothing
 * and leaves every output untouched. */
#ifndef XRNERF_MI355_GNR_RASTER_H
#define XRNERF_MI355_GNR_RASTER_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define XR_GNR_RASTER_MAX_SIDE 32768u     /* image height / width */

/* bytes of `workspace` for one call (0 for sizes the call refuses) */
size_t xr_gnr_raster_workspace_bytes(uint32_t V, uint32_t N, uint32_t H, uint32_t W);

/* V views of one mesh per call: verts [V,N,3] fp32 as the reference takes them (with `persp` x and y are divided by z in the kernel; a
 * vertex or a face with z <= eps is dropped), faces [F,3] int32 shared by the views (a face with an index outside 0 .. N-1 is
 * dropped).  A face with det > eps is culled unless `double_face`.  The sample point of pixel (x, y) is the integer (x, y).
 *   index  [V,H,W]   int64  the winning face, -1 where empty: strict z order, the lowest face index wins a tie
 *   coeff  [V,H,W,3] fp32   its barycentric coefficients at the pixel, 0 where empty
 *   visual [V,N]     1 byte 1 = the vertex lies in the image and no face (of which it is no corner) covers it at z_face <= z_vertex
 *   depth  [V,H,W]   fp32   the z-buffer (the array the reference frees without returning), 0 where empty
 * Refused: eps < 0 (or NaN), H or W of 0 or above XR_GNR_RASTER_MAX_SIDE, V H W or V N beyond int32, F >= 2^32 - 1, a workspace that
 * is too small or not 8-byte aligned.  Eight launches (init, vertex pass, three of the scan, list fill, face pass, resolve). */
int xr_gnr_raster_forward(const float* verts, uint32_t V, uint32_t N, const int32_t* faces, uint32_t F, uint32_t H, uint32_t W, int persp,
                          int double_face, float eps, int64_t* index, float* coeff, uint8_t* visual, float* depth, void* workspace,
                          size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
