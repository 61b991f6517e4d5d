/* Scene data pipelines: the fused ray front end of libxrnerf_mi355.so (xrnerf_amd/csrc/xr_pipeline.hip) -- what the reference's
 * per-item transforms GetRays, SelectRays / FlattenRays / BatchSample, GetViewdirs, ToNDC, GetBounds, GetZvals, PerturbZvals and GetPts
 * (datasets/pipelines/create.py, augment.py, transforms.py) compute on the host, for the selected pixels only, in one launch
 * (DESIGN.md section 20).  A header of its own, bound by its own ctypes table (xrnerf_amd/_lib.py PIPELINE_SIGNATURES).
 * Conventions of xrnerf_mi355_eval.h: 0 or a negative XR_E* code (message: xr_last_error()); never throws, syncs or allocates; raw
 * device pointers; the launch goes to `stream`.  XR_EINVAL launches nothing and leaves every output untouched.  No atomics: the same
 * input gives the same bits. */
#ifndef XRNERF_MI355_PIPELINE_H
#define XRNERF_MI355_PIPELINE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define XR_PIPE_MAX_CHANNELS 4u     /* RGB or RGBA targets */

/* R rays, S samples per ray; every expression is un-fused fp32 in the reference's operation order, divisions and square roots
 * correctly rounded.
 * Source of the rays -- exactly one of c2w / table is non-null:
 *   c2w    12 device floats, row-major [3,4].  Pixel (h, w), i = (float)w, j = (float)h (torch.linspace(0, W-1, W) has step 1):
 *            dirs   = ((i - cx) / fx, -(j - cy) / fy, -1)
 *            rays_d[r] = (dirs[0] c2w[r][0] + dirs[1] c2w[r][1]) + dirs[2] c2w[r][2],   rays_o[r] = c2w[r][3]
 *          sel: R device int32 flat pixel indices h W + w (the SelectRays gather), or NULL: the R consecutive pixels from pix0 on in
 *          row-major order (FlattenRays; pix0 lets a frame be made in pieces; pix0 + R <= H W).  A sel entry outside [0, H W) makes that
 *          ray's outputs NaN and reads nothing.
 *          image: device [H,W,C] floats or NULL; target_s[R,C] is gathered from it.
 *          with_radii: h' = h below the last row and H - 3 on it (the reference appends dx[-2:-1], the row BEFORE the last difference),
 *            dx = sqrt(sum_c (d(h', w)[c] - d(h' + 1, w)[c])^2), radii = dx * 2 / sqrtf(12)  (needs H >= 3)
 *   table  device [R,3,3] rows (o, d, rgb) of a BatchSample slice: rays_o, rays_d and target_s[R,3] are its columns.  H, W and the
 *          intrinsics are only read for ndc; sel, image and with_radii must be off.
 * with_viewdirs: viewdirs = d / sqrt(fma(d2, d2, fma(d1, d1, d0 d0))) -- torch.norm's accumulation on the host, the one fused
 *          operation of the chain --, of the direction BEFORE ndc.
 * ndc (ToNDC, ndc_rays): t = -(ndc_near + o2) / d2; o += t d; then
 *            o' = (ndc_w o0 / o2, ndc_h o1 / o2, 1 + 2 ndc_near / o2),  d' = (ndc_w (d0/d2 - o0/o2), ndc_h (d1/d2 - o1/o2), -2 ndc_near / o2)
 *          ndc_w = -1 / (W / (2 f)), ndc_h = -1 / (H / (2 f)): evaluated by the host in double and rounded to fp32 once; ndc_near = 1.
 * near / far: the constants GetBounds broadcasts; near_out / far_out [R,1].
 * z_vals [R,S]: t = torch.linspace(0, 1, S)[k]; z = near (1 - t) + far t, or 1 / (1 / near (1 - t) + 1 / far t) with lindisp.
 *          t_rand: device [R,S] floats or NULL; z = lower + (upper - lower) t_rand, lower / upper the mid-points .5 (z[k+1] + z[k]) closed
 *          by z[0] / z[S-1]  (PerturbZvals and GetZvals(randomized=True): the same formula).
 * pts [R,S,3] = o + d z, of the rays AFTER ndc.
 * Every output pointer may be NULL (not computed).  S may be 0 when z_vals, pts and t_rand are NULL.  R == 0 launches nothing.
 * Refused: both or neither of c2w / table; with c2w: H or W of 0, H W beyond int32, fx or fy of 0 or not finite, pix0 + R > H W without
 * sel, with_radii at H < 3 or without radii; with table: sel, image, with_radii or radii; image with C outside 1 .. XR_PIPE_MAX_CHANNELS;
 * with_viewdirs without viewdirs; ndc at H or W of 0; z_vals, pts or t_rand at S == 0; more than 2^31 - 1 workgroups. */
int xr_pipe_ray_front(const float* c2w, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W, const int32_t* sel, uint64_t pix0,
                      uint64_t R, const float* image, uint32_t C, const float* table, int with_viewdirs, int ndc, int with_radii, float ndc_w,
                      float ndc_h, float ndc_near, float near, float far, uint32_t S, int lindisp, const float* t_rand, float* rays_o,
                      float* rays_d, float* viewdirs, float* radii, float* near_out, float* far_out, float* z_vals, float* pts,
                      float* target_s, void* stream);

#ifdef __cplusplus
}
#endif
#endif
