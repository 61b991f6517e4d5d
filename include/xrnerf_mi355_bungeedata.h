/* BungeeNeRF data: a training item and a validation frame of libxrnerf_mi355.so (xrnerf_amd/csrc/xr_bungeedata.hip) -- what the
 * reference's load_rays_bungee + BungeeBatchSample + GetViewdirs + BungeeGetBounds + BungeeGetZvals + PerturbZvals, and GetRays(include_radius)
 * + FlattenRays + GetViewdirs + BungeeGetBounds + BungeeGetZvals (datasets/load_data/get_rays.py, datasets/pipelines/create.py, augment.py)
 * compute on the host, for the rays of one item only.  A header of its own, bound by its own ctypes table
 * (xrnerf_amd/_lib.py BUNGEEDATA_SIGNATURES).
 * Conventions of xrnerf_mi355_pipeline.h: 0 or a negative XR_E* code (message: xr_last_error()); never throws, syncs or allocates; raw
 * device pointers; the launch goes to `stream`.  XR_EINVAL launches nothing and leaves every output untouched.  No atomics: the same
 * input gives the same bits. */
#ifndef XRNERF_MI355_BUNGEEDATA_H
#define XRNERF_MI355_BUNGEEDATA_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define XR_BGD_CAM_DOUBLES 12u     /* one camera row: cam2world rows 0..2, row-major */
#define XR_BGD_MAX_SAMPLES 1024u   /* z_vals per ray: a ray's row is sorted in LDS */

/* The bounds and z-values both entry points end with, fp32, the arithmetic of xr_bungee_zvals (xrnerf_mi355_bungee.h) on the fp32 rays_o
 * and viewdirs they write: bounds_mode 1 (sphere; globe_center = host float[3], r2_top, r2_earth) or 2 (flat; scaling), S edges per ray
 * (the first floor(2S/3) linear in disparity, the rest linear in depth), sorted ascending with NaN last.  t_rand (device [R,S] or NULL):
 * z = lower + (upper - lower) t_rand between the mid-points of the sorted row, closed by its first / last edge (PerturbZvals).
 * S may be 0 when near_out, far_out, z_vals and t_rand are NULL; otherwise 2 <= S <= XR_BGD_MAX_SAMPLES. */

/* R rays of a training split: ray r is flat index f = perm[start + r] of the [n_train, H, W] rays of the train images, image slot
 * t = f / (H W), image i = i_train[t], pixel (row, col) of f % (H W).
 *   cams     device [n_images, 12] doubles, cam2world rows 0..2        codes   device [n_images] int64 scale codes
 *   images   device [n_images, H, W, 3] floats                          i_train device [n_train] int32, each in [0, n_images)
 *   perm     device int64, at least start + R entries
 * Per ray, in double, un-fused, in this order (get_rays.py:156-189 with an fp32 meshgrid and a double focal):
 *   x = double(float(col) - half_w) / focal;  y = double(-(float(row) - half_h)) / focal;  z = -1
 *   n = sqrt((x x + y y) + z z);  u = (x, y, z) / n;  d_r = (u_0 C[r][0] + u_1 C[r][1]) + u_2 C[r][2];  rays_o = C[:, 3]
 *   radii = (|d(row', col) - d(row' + 1, col)| 2) / sqrt(12.0), row' = row below the last row and H - 3 on it
 *   viewdirs = d / sqrt(fma(d_2, d_2, fma(d_1, d_1, d_0 d_0)))
 * every output rounded to fp32 once; target_s = the pixel; scale_code [R,1] int64 = codes[i].
 * An f outside [0, n_train H W), or an i_train entry outside [0, n_images), gives that ray NaN outputs (scale_code -1) and reads nothing.
 * Every output pointer may be NULL.  R == 0 launches nothing.
 * Refused: cams, i_train or perm NULL; target_s without images; scale_code without codes; n_images, n_train of 0; H < 3; W of 0;
 * n_train H W beyond 2^62; focal not finite or 0; a bounds_mode outside 1 .. 2 or S outside the range above when a bound or z output is
 * asked for; sphere bounds without globe_center; more than 2^31 - 1 workgroups. */
int xr_bgd_item(const double* cams, const int64_t* codes, const float* images, const int32_t* i_train, uint32_t n_images, uint32_t n_train,
                uint32_t H, uint32_t W, double focal, float half_w, float half_h, const int64_t* perm, uint64_t start, uint64_t R, uint32_t S,
                int bounds_mode, const float* globe_center, float r2_top, float r2_earth, float scaling, const float* t_rand, float* rays_o,
                float* rays_d, float* target_s, float* radii, int64_t* scale_code, float* viewdirs, float* near_out, float* far_out,
                float* z_vals, void* stream);

/* The H W rays of one posed frame, row-major, fp32 (create.py:211-245 GetRays(include_radius=True), FlattenRays, GetViewdirs):
 *   c2w  device 12 floats, cam2world rows 0..2
 *   i = torch.linspace(0, W - 1, W)[col], j = torch.linspace(0, H - 1, H)[row];  dirs = ((i - cx) / fx, -(j - cy) / fy, -1)
 *   rays_d_r = (dirs_0 c2w[r][0] + dirs_1 c2w[r][1]) + dirs_2 c2w[r][2]  (NOT normalised);  rays_o = c2w[:, 3]
 *   radii = (|d(row', col) - d(row' + 1, col)| 2) / sqrt(12.f), row' as above;  viewdirs = d / sqrt(fma(d_2, d_2, fma(d_1, d_1, d_0 d_0)))
 * Every output pointer may be NULL.  Refused: c2w NULL; H < 3; W of 0; the bounds / S rules above; more than 2^31 - 1 workgroups. */
int xr_bgd_frame(const float* c2w, uint32_t H, uint32_t W, float fx, float fy, float cx, float cy, uint32_t S, int bounds_mode,
                 const float* globe_center, float r2_top, float r2_earth, float scaling, float* rays_o, float* rays_d, float* radii,
                 float* viewdirs, float* near_out, float* far_out, float* z_vals, void* stream);

#ifdef __cplusplus
}
#endif
#endif
