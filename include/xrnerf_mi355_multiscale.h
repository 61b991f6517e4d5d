/* Mip-NeRF multiscale data: the ray sampler and the image pyramid of libxrnerf_mi355.so (xrnerf_amd/csrc/xr_multiscale.hip) -- what the
 * reference's load_rays_multiscale + flatten + MipMultiScaleSample + GetZvals (datasets/load_data/get_rays.py, datasets/utils/flatten.py,
 * datasets/pipelines/create.py) and tools/convert_blender_data.py + load_multiscale_data compute on the host, for the drawn pixels only
 * (DESIGN.md section 21).  A header of its own, bound by its own ctypes table (xrnerf_amd/_lib.py MULTISCALE_SIGNATURES).
 * Conventions of xrnerf_mi355_pipeline.h: 0 or a negative XR_E* code (message: xr_last_error()); never throws, syncs or allocates; raw
 * device pointers; the launch goes to `stream`.  XR_EINVAL launches nothing and leaves every output untouched.  No atomics: the same
 * input gives the same bits. */
#ifndef XRNERF_MI355_MULTISCALE_H
#define XRNERF_MI355_MULTISCALE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define XR_MS_CAM_DOUBLES 24u      /* one camera row: pix2cam[3][3], cam2world[3][4], lossmult, near, far */
#define XR_MS_MAX_DOWN 8u          /* pyramid levels */
#define XR_MS_MAX_IMAGES (1u << 20)

/* R rays of a set of n_images posed images of different sizes, S samples per ray.
 *   cams    device [n_images, 24] doubles: P = pix2cam row-major (9), C = cam2world rows 0..2 row-major (12), lossmult, near, far
 *   hw      device [n_images, 2] int32 (H, W)
 *   prefix  device [n_images + 1] int64, the exclusive prefix of H W; total = prefix[n_images] is passed by the host as well
 *   images  device [total, 3] floats (the images packed in table order) or NULL; target_s[R,3] is gathered from it
 * The selection -- idx non-NULL: R device int64 flat ray indices into the concatenation (duplicates are legal); the image is found by
 * binary search of prefix.  idx NULL: the R consecutive pixels of image `image` from `first_pixel` on, row-major.  An index outside
 * [0, total), or a pixel past its image's H W, gives that ray NaN outputs and reads nothing out of bounds.
 * Per ray, pixel (row, col) of an H x W image, in double, un-fused, in this order:
 *   x = col + 0.5, y = row + 0.5;   cam_r = (x P[r][0] + y P[r][1]) + P[r][2];   d_r = (cam_0 C[r][0] + cam_1 C[r][1]) + cam_2 C[r][2]
 *   rays_o = C[:, 3];   viewdirs = d / sqrt((d_0^2 + d_1^2) + d_2^2)
 *   radii = (|d(row', col) - d(row' + 1, col)| 2) / sqrt(12.0), row' = row below the last row and H - 3 on it (the reference appends
 *   dx[-2:-1]); an image with H < 3 gives NaN radii (the Python layer refuses it)
 * every output rounded to fp32 once.  lossmult, near, far [R,1]: the image's scalars.
 * z_vals [R,S], fp32, as xr_pipe_ray_front: t = torch.linspace(0, 1, S)[k]; z = near (1 - t) + far t, or 1 / (1 / near (1 - t) + 1 / far t)
 * with lindisp; t_rand (device [R,S] or NULL): z = lower + (upper - lower) t_rand between the mid-points closed by z[0] / z[S-1].
 * Every output pointer may be NULL.  S may be 0 when z_vals and t_rand are NULL.  R == 0 launches nothing.
 * Refused: cams, hw or prefix NULL; n_images of 0 or above XR_MS_MAX_IMAGES; total of 0 or beyond 2^62; target_s without images; without idx:
 * image >= n_images or first_pixel + R > total; z_vals or t_rand at S == 0; more than 2^31 - 1 workgroups. */
int xr_ms_rays(const double* cams, const int32_t* hw, const int64_t* prefix, uint32_t n_images, uint64_t total, const float* images,
               const int64_t* idx, uint32_t image, uint64_t first_pixel, uint64_t R, uint32_t S, int lindisp, const float* t_rand, float* rays_o,
               float* rays_d, float* viewdirs, float* radii, float* lossmult, float* near_out, float* far_out, float* z_vals, float* target_s,
               void* stream);

/* The converter's image side: base [N,H,W,C] uint8 (C = 3 or 4) -> n_down levels per view, packed view-major with a view's levels
 * consecutive (000_d0, 000_d1, ...): level j is (H >> j) x (W >> j), a view takes per_view = sum_j (H >> j)(W >> j) pixels.
 *   level 0 float = byte / 255 (fp32);  level j float = down2 of level j-1's FLOAT: (((a + b) + c) + d) / 4 with a = (2r, 2c),
 *   b = (2r, 2c+1), c = (2r+1, 2c), d = (2r+1, 2c+1)
 *   bytes_out  [N per_view, C] uint8 or NULL: the saved byte trunc(float 255)
 *   pixels_out [N per_view, 3] floats or NULL: the loaded pixel byte / 255, with white_bkgd rgb a + (1 - a) (un-fused), a = the LAST channel
 * Refused: base NULL; N, H or W of 0; C not 3 or 4; n_down outside 1 .. XR_MS_MAX_DOWN; H or W not divisible by 2^(n_down-1); N per_view
 * beyond 2^40; both outputs NULL. */
int xr_ms_pyramid(const uint8_t* base, uint32_t N, uint32_t H, uint32_t W, uint32_t C, uint32_t n_down, int white_bkgd, uint8_t* bytes_out,
                  float* pixels_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
