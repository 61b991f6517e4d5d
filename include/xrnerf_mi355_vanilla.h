/* Vanilla-NeRF entry points of libxrnerf_mi355.so (xrnerf_amd/csrc/xr_vanilla.hip): the training stages of
 * configs/nerf/nerf_blender_base01.py around its 8 x 256 MLP.  A header of their own, bound by their own ctypes table
 * (xrnerf_amd/_lib.py VANILLA_SIGNATURES), like xrnerf_mi355_bungee.h: the host emulation of the original kernel sources
 * (tests/hip_emu) binds xrnerf_mi355.h's own declarations one to one, and these come from a separate source file.
 * Conventions of xrnerf_mi355.h: 0 or a negative XR_E* code (message: xr_last_error()); never throws, syncs or allocates; raw device
 * pointers, fp32, contiguous unless a row stride is given; the launch goes to `stream`.  The same input gives the same bits. */
#ifndef XRNERF_MI355_VANILLA_H
#define XRNERF_MI355_VANILLA_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* BaseEmbedder.forward (xrnerf/models/embedders/base.py): out row r (stride ld floats) =
 *   [p, sin(2^0 p), cos(2^0 p), .., sin(2^(L-1) p), cos(2^(L-1) p) | d, sin(2^0 d), cos(2^0 d), ..]   (L = multires, multires_dirs)
 * with p = pts[r] and d = viewdirs[r / rows_per_dir]; accurate sinf / cosf.  channels = 6 + 6 multires + 6 multires_dirs;
 * ld >= channels rounded up to a multiple of 4, and columns [channels, ld) are WRITTEN as zeros.  multires, multires_dirs in [0, 16]. */
int xr_nerf_encode(const float* pts, const float* viewdirs, uint64_t n_rows, uint32_t rows_per_dir, int multires, int multires_dirs,
                   float* out, uint32_t ld, void* stream);
/* NerfRender.forward (xrnerf/models/renders/nerf_render.py) for relu density, sigmoid colours, rgb_padding = 0, density_bias = 0:
 * raw [n_rays,n_samples,4] (16-byte aligned), z_vals [n_rays,n_samples] sample positions (last interval 1e10, distances times
 * |rays_d|), noise [n_rays,n_samples] or NULL (added to raw's density before the relu); w = alpha cumprod(1 - alpha + 1e-10);
 * white_bkgd adds 1 - acc.  -> rgb [n_rays,3], disp [n_rays], acc [n_rays], weights [n_rays,n_samples].  n_samples in [1, 4096]. */
int xr_nerf_render_train_forward(const float* raw, const float* z_vals, const float* rays_d, const float* noise, uint32_t n_rays,
                                 uint32_t n_samples, int white_bkgd, float* rgb, float* disp, float* acc, float* weights, void* stream);
/* dL/draw [n_rays,n_samples,4] (16-byte aligned) given dL/drgb [n_rays,3], recomputed from the forward's inputs; relu' is 0 at 0 */
int xr_nerf_render_backward(const float* raw, const float* z_vals, const float* rays_d, const float* noise, uint32_t n_rays,
                            uint32_t n_samples, int white_bkgd, const float* grad_rgb, float* grad_raw, void* stream);
/* sample_pdf (xrnerf/models/networks/utils/hierarchical_sample.py): n_new samples per ray from the pdf (weights[1:-1] + 1e-5) over the
 * midpoints of z_vals [n_rays,n_coarse] by inverting its cdf at u [n_rays,n_new] (NULL: linspace(0, 1, n_new)), with the reference's
 * searchsorted(right=True) and `denom < 1e-5 -> 1` rule; merged with z_vals and sorted -> z_out [n_rays,n_coarse+n_new],
 * pts_out [n_rays,n_coarse+n_new,3] = rays_o + rays_d z_out.  z_samples_out [n_rays,n_new] (nullable): the new samples before the
 * merge.  3 <= n_coarse <= 1024, 1 <= n_new <= 1024, else XR_EINVAL. */
int xr_nerf_sample_pdf(const float* z_vals, const float* weights, const float* u, const float* rays_o, const float* rays_d,
                       uint32_t n_rays, uint32_t n_coarse, uint32_t n_new, float* z_out, float* pts_out, float* z_samples_out,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
