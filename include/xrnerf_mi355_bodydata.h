/* ZJU-MoCap / H36M human data: the frame store and the body-box ray sampler of libxrnerf_mi355.so (xrnerf_amd/csrc/xr_bodydata.hip) --
 * what the reference's LoadImageAndCamera, NBGetRays and NBSelectRays (datasets/pipelines/create.py, augment.py) compute on the host for
 * every item, split into what depends on the image alone (made once, kept on the device) and what depends on the draw (DESIGN.md
 * section 22).  A header of its own, bound by its own ctypes table (xrnerf_amd/_lib.py BODYDATA_SIGNATURES).
 * Conventions of xrnerf_mi355_pipeline.h: 0 or a negative XR_E* code (message: xr_last_error()); never throws, syncs or allocates; raw
 * device pointers unless a parameter says "host"; the launches go to `stream`.  XR_EINVAL launches nothing and leaves every output
 * untouched.  No atomics: the same input gives the same bits. */
#ifndef XRNERF_MI355_BODYDATA_H
#define XRNERF_MI355_BODYDATA_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define XR_BODY_CAM_DOUBLES 30u    /* inv(K)[3][3], R[3][3], T[3], rays_o[3], bounds min[3], bounds max[3] */
#define XR_BODY_ROUNDS 8u          /* rounds of the rejection loop inside xr_body_sample */
#define XR_BODY_MAX_SEL 65536u     /* rays per training item */
#define XR_BODY_MAX_SHRINK 16u     /* 1 / ratio */

/* The prepared image and mask of one picture.
 *   img8   device [Hs, Ws, 3] uint8;  msk8 device [Hm, Wm] uint8 (any size: it is resized to the image by nearest)
 *   kd     HOST, 14 doubles: K row-major (9), then D = k1 k2 p1 p2 k3
 *   s      the shrink 1 / ratio, 1 .. XR_BODY_MAX_SHRINK; Hs and Ws must be multiples of it.  H = Hs / s, W = Ws / s
 *   img    device [H, W, 3] floats;  msk device [H, W] uint8 (0 / 1)
 * Source pixel: byte / 255 in fp32.  Mask source at (y, x) of the image grid: msk8[(y Hm) / Hs][(x Wm) / Ws] != 0 (integer division).
 * Undistortion of destination (v, u), in double, un-fused: x = (u - cx) / fx, y = (v - cy) / fy, r2 = x x + y y,
 *   kr = 1 + ((k3 r2 + k2) r2 + k1) r2, xd = (x kr + p1 (2 x y)) + p2 (r2 + 2 x x), yd = (y kr + p1 (r2 + 2 y y)) + p2 (2 x y),
 *   us = fx xd + cx, vs = fy yd + cy; the image takes the bilinear sample at (vs, us) with a zero border -- weights
 *   ax = (float)(us - floor(us)), fp32: top = p00 (1 - ax) + p01 ax, bottom likewise, top (1 - ay) + bottom ay -- the mask the nearest
 *   sample at (floor(vs + 0.5), floor(us + 0.5)), zero outside.  D all zero: the source pixel itself (a copy of its bits).
 * Shrink: the s x s block's mean, summed in row-major order in fp32 and divided by s s; the mask takes the block's first pixel.
 * Background: where the mask is 0 the pixel is 0, or 1 with white_bkgd.
 * Refused: a null pointer; a size of 0; Hs Ws beyond int32; s out of range or not dividing Hs and Ws; fx or fy of 0 or not finite. */
int xr_body_prepare(const uint8_t* img8, const uint8_t* msk8, uint32_t Hs, uint32_t Ws, uint32_t Hm, uint32_t Wm, const double* kd, uint32_t s,
                    int white_bkgd, float* img, uint8_t* msk, void* stream);

size_t xr_body_masks_workspace_bytes(uint32_t H, uint32_t W);

/* The two candidate lists of one prepared picture, flat pixel indices (row W + col) in row-major (argwhere) order:
 *   bound_list  the pixels of the box silhouette: the union of six closed polygons over corners8 (HOST, 16 int32: x, y of the box's
 *               eight projected corners), vertex lists {0,1,3,2,0} {4,5,7,6,5} {0,1,5,4,0} {2,3,7,6,2} {0,2,6,4,0} {1,3,7,5,1}, each
 *               closed by an edge from its last vertex to its first; a pixel belongs to a polygon when it lies on an edge or is
 *               interior by the even-odd rule, decided by int64 cross products (exact)
 *   body_list   those of them where msk != 0
 * Both lists need room for H W entries; totals (device, 2 int32) receives their lengths, or -1 for one that does not fit int32.
 * Count, xr_scan.h's two-level scan over the workgroups' counts, ranked write.  workspace: xr_body_masks_workspace_bytes(H, W), 4-byte aligned.
 * Refused: a null pointer; H or W of 0; H W beyond int32; a corner beyond +-2^30; a workspace too small (XR_ENOMEM). */
int xr_body_masks(const uint8_t* msk, uint32_t H, uint32_t W, const int32_t* corners8, int32_t* bound_list, int32_t* body_list, int32_t* totals,
                  void* workspace, size_t workspace_bytes, void* stream);

/* One training item: sel_n rays of one prepared picture, ONE workgroup, the reference's rejection rounds inside the kernel.
 *   cam     device, XR_BODY_CAM_DOUBLES doubles (layout above; bounds are the fp32 values widened)
 *   img     device [H, W, 3] floats (the prepared image) or NULL with target_s NULL
 *   draws   device int64 [XR_BODY_ROUNDS, sel_n]
 * Round r with rem rays missing: n_body = rem / 2; slot j < n_body takes body_list[draws[r][j] mod len_body], slot n_body <= j < rem
 * takes bound_list[draws[r][j] mod len_bound].  The pixel's ray, in double, un-fused: pc_r = ((col Ki[r][0] + row Ki[r][1]) + Ki[r][2]) - T[r];
 * pw_c = (pc_0 R[0][c] + pc_1 R[1][c]) + pc_2 R[2][c]; d = pw - rays_o; d = d / sqrt((d_0^2 + d_1^2) + d_2^2).  The box: n = |d| again,
 * v = d / n; v in (-1e-10, 1e-5) becomes 1e-5, then v in (-1e-5, 1e-10) becomes -1e-5; t = (bounds - rays_o) / v; near = max of the
 * three smaller, far = min of the three larger; the ray survives when near < far; near / n, far / n.  Survivors are appended in slot
 * order; rays_o, rays_d [sel_n,3], near, far [sel_n,1], target_s [sel_n,3] are each rounded to fp32 once.  After XR_BODY_ROUNDS rounds
 * the missing rays are NaN and short_items[0] (device uint32) is incremented (one lane, a plain store: launches on one stream are ordered).
 * With S >= 1: z_vals [sel_n,S] and pts [sel_n,S,3] as xr_body_points makes them, written by this workgroup (either may be NULL).
 * Refused: a null pointer among cam, the lists, draws, rays_o, rays_d, near, far, short_items; len_body or len_bound of 0 or beyond
 * H W; sel_n of 0 or above XR_BODY_MAX_SEL; H W of 0 or beyond int32; target_s without img; z_vals, pts or t_rand at S == 0. */
int xr_body_sample(const double* cam, uint32_t H, uint32_t W, const float* img, const int32_t* body_list, uint32_t len_body, const int32_t* bound_list,
                   uint32_t len_bound, const int64_t* draws, uint32_t sel_n, uint32_t S, const float* t_rand, float* rays_o, float* rays_d,
                   float* near_out, float* far_out, float* target_s, float* z_vals, float* pts, uint32_t* short_items, void* stream);

/* z_vals [R,S] and pts [R,S,3] of R rays with per-ray near / far [R,1], one thread per (ray, sample), un-fused fp32:
 * t = torch.linspace(0, 1, S)[k]; z = near (1 - t) + far t; t_rand (device [R,S] or NULL): z = lower + (upper - lower) t_rand between
 * the mid-points closed by z[0] / z[S-1]; pts = o + d z.  Either output may be NULL.  R == 0 launches nothing.
 * Refused: a null input; S of 0; both outputs NULL; more than 2^31 - 1 workgroups. */
int xr_body_points(const float* rays_o, const float* rays_d, const float* near_in, const float* far_in, uint64_t R, uint32_t S, const float* t_rand,
                   float* z_vals, float* pts, void* stream);

size_t xr_body_frame_workspace_bytes(uint32_t H, uint32_t W);

/* A whole frame (NBSelectRays(sel_all=True)): every pixel's ray is made in double as above and rounded to fp32; the box test then runs
 * on the ROUNDED rays in fp32 (the reference casts before it calls get_near_far), with the fp32 values of the four thresholds.
 * xr_body_frame_count writes mask_at_box [H W] (0 / 1) and total (device int32: the number of survivors M, -1 beyond int32);
 * xr_body_frame_write, given the same workspace, writes the M survivors in row-major (nonzero) order: rays_o, rays_d [M,3], near, far
 * [M,1], target_s [M,3] (NULL: not written; needs img).  workspace: xr_body_frame_workspace_bytes(H, W), 4-byte aligned.
 * Refused: a null pointer; H W of 0 or beyond int32; a workspace too small (XR_ENOMEM); target_s without img. */
int xr_body_frame_count(const double* cam, uint32_t H, uint32_t W, uint8_t* mask_at_box, int32_t* total, void* workspace, size_t workspace_bytes,
                        void* stream);
int xr_body_frame_write(const double* cam, uint32_t H, uint32_t W, const float* img, const uint8_t* mask_at_box, const void* workspace,
                        size_t workspace_bytes, uint32_t M, float* rays_o, float* rays_d, float* near_out, float* far_out, float* target_s,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
