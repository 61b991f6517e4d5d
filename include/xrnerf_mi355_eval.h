/* Test-set evaluation: the image-metric entry points of libxrnerf_mi355.so (xrnerf_amd/csrc/xr_eval.hip) -- the windowed moments, the
 * SSIM map and the squared error of skimage's structural_similarity as the reference's hooks call it (core/hooks/utils.py), and the
 * 8-bit side-by-side image ValidateHook saves.  A header of its own, bound by its own ctypes table
 * (xrnerf_amd/_lib.py EVAL_SIGNATURES).
 * Conventions of xrnerf_mi355_gnr.h: 0 or a negative XR_E* code (message: xr_last_error()); never throws, syncs or allocates; raw
 * device pointers; the launches go to `stream`.  The same input gives the same bits: no atomics at all -- every workgroup writes its
 * own partial sums and a second launch adds them in a fixed order.  XR_EINVAL launches nothing and leaves every output untouched. */
#ifndef XRNERF_MI355_EVAL_H
#define XRNERF_MI355_EVAL_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define XR_EVAL_MAX_RADIUS 5u       /* window of at most 11 x 11 (skimage's Gaussian window: sigma 1.5, truncate 3.5) */
#define XR_EVAL_MAX_CHANNELS 4u
#define XR_EVAL_TILE_W 32u          /* one workgroup: 8 rows of 32 pixels, every channel */
#define XR_EVAL_TILE_H 8u

/* bytes of `workspace` for one xr_eval_ssim call: two doubles per (image, tile); 0 for sizes the call refuses */
size_t xr_eval_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t C);

/* B image pairs x, y [B,H,W,C] fp32 with element strides (batch, row, pixel, channel) shared by x and y, all >= 0 -- a slice of a wider
 * buffer or a channel-first view is such a layout.  taps: 2 r + 1 HOST doubles, the window is their outer product; out-of-image indices
 * reflect about the edge (-1 -> 0, -2 -> 1, n -> n-1: scipy's mode='reflect').  Inputs are read as fp32, every operation is in double:
 *   ux, uy, uxx, uyy, uxy   the weighted moments, rows first, then columns, taps in ascending order
 *   vx = cov_norm (uxx - ux ux), vy, vxy likewise
 *   S  = ((2 ux uy + C1) (2 vxy + C2)) / ((ux ux + uy uy + C1) (vx + vy + C2))
 *   ssim_sum [B] double     the sum of S over the WHOLE map of image b, borders included
 *   sq_sum   [B] double     the sum of (double)(x - y)^2, the difference rounded to fp32 first
 *   map      [B,H,W,C] double, contiguous, or NULL: S itself
 * Refused: a null x, y, taps, ssim_sum, sq_sum or workspace; r > XR_EVAL_MAX_RADIUS; H or W below 2 r + 1; C outside
 * 1 .. XR_EVAL_MAX_CHANNELS; B of 0; a negative stride; B H W C beyond int32; a workspace that is too small (XR_ENOMEM) or not 8-byte
 * aligned.  Two launches (tiles, fold). */
int xr_eval_ssim(const float* x, const float* y, uint32_t B, uint32_t H, uint32_t W, uint32_t C, int64_t batch_stride, int64_t row_stride,
                 int64_t pixel_stride, int64_t channel_stride, const double* taps, uint32_t r, double cov_norm, double C1, double C2,
                 double* ssim_sum, double* sq_sum, double* map, void* workspace, size_t workspace_bytes, void* stream);

/* out [H, 2 W, C] bytes = to8b(hstack(rgb, gt)), to8b(v) = (uint8)(255.f * clip(v, 0, 1)): the fp32 product, truncated; NaN -> 0.  With a
 * NULL gt out is [H, W, C], the single image TestHook saves.  rgb and gt [H,W,C] fp32 share the element strides (row, pixel, channel).
 * Refused: a null rgb or out, H or W of 0, C outside 1 .. XR_EVAL_MAX_CHANNELS, a negative stride, 2 H W C beyond int32. */
int xr_eval_to8b_pair(const float* rgb, const float* gt, uint32_t H, uint32_t W, uint32_t C, int64_t row_stride, int64_t pixel_stride,
                      int64_t channel_stride, uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
