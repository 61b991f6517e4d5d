/* BungeeNeRF entry points of libxrnerf_mi355.so (xrnerf_amd/csrc/xr_bungee.hip), included by xrnerf_mi355.h.
 * A header of their own, bound by their own ctypes table (xrnerf_amd/_lib.py BUNGEE_SIGNATURES): the host emulation of the original
 * kernel sources (tests/hip_emu) binds xrnerf_mi355.h's own declarations one to one, and these come from a separate source file. */
#ifndef XRNERF_MI355_BUNGEE_H
#define XRNERF_MI355_BUNGEE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * BungeeNeRF (configs/bungeenerf/bungeenerf_multiscale_google.py): the stages either side of the growing residual MLP,
 * one launch each (xrnerf_amd/csrc/xr_bungee.hip).  fp32, contiguous unless a row stride is given; n_z = interval EDGES.
 *
 * BungeeGetBounds + BungeeGetZvals (xrnerf/datasets/pipelines/create.py): bounds_mode 0 = near/far [n_rays] are inputs;
 * 1 = 'sphere' (building-top sphere of radius^2 r2_top and earth sphere of radius^2 r2_earth around globe_center, a HOST array of
 * 3 = float32(scene_origin * scaling); near x0.9, far x1.1); 2 = 'flat' (planes z = 250 scaling and z = 0, near clamped to >= 1e-6).
 * With a mode, near/far are written.  z_out [n_rays,n_z]: floor(2 n_z/3) edges linear in disparity, the rest linear in depth
 * to far, sorted.  fp32 like the reference: the sphere test's cancellation is documented in xr_bungee.hip. */
int xr_bungee_zvals(const float* rays_o, const float* viewdirs, float* near, float* far, uint32_t n_rays, uint32_t n_z,
                    int bounds_mode, const float* globe_center, float r2_top, float r2_earth, float scaling, float* z_out,
                    void* stream);
/* cast_rays (mip.py; ray_shape 0 = cone, 1 = cylinder; diagonal covariances) + BungeeEmbedder.forward
 * (xrnerf/models/embedders/bungee_embedder.py), from the frustum (rays_o, rays_d [n_rays,3], radii [n_rays], z_vals
 * [n_rays,n_samples+1]) OR from materialised (means, covs) [n_rays*n_samples,3]: exactly one set is non-NULL.
 * out_pts rows (stride ld_pts): [mean, (sin(mean 2^l) e_l, cos(mean 2^l) e_l)_{l<multires}], e_l = exp(-0.5 4^l cov), 3 + 6 multires
 * columns; out_dir rows (stride ld_dir): [d, sin(d 2^l), cos(d 2^l)]_{l<multires_dirs} of the ray's viewdirs, 3 + 6 multires_dirs. */
int xr_bungee_encode(const float* rays_o, const float* rays_d, const float* radii, const float* z_vals, const float* means,
                     const float* covs, const float* viewdirs, uint32_t n_rays, uint32_t n_samples, int multires, int multires_dirs,
                     int ray_shape, float* out_pts, uint32_t ld_pts, float* out_dir, uint32_t ld_dir, void* stream);
/* BungeeNerfRender.forward (xrnerf/models/renders/bungeenerf_render.py): raw [n_rays,n_z-1,n_heads,4] (16-byte aligned), heads
 * 0..stage summed; distances between interval MIDPOINTS (1e10 appended) times |viewdirs|; noise [n_rays,n_z-1] or NULL;
 * density_activation 0 = softplus, 1 = relu.  -> rgb [n_rays,3], disp [n_rays], acc [n_rays], weights [n_rays,n_z-1]. */
int xr_bungee_render_forward(const float* raw, const float* z_vals, const float* viewdirs, const float* noise, uint32_t n_rays,
                             uint32_t n_z, uint32_t n_heads, int stage, float density_bias, float rgb_padding, int white_bkgd,
                             int density_activation, float* rgb, float* disp, float* acc, float* weights, void* stream);
/* dL/draw [n_rays,n_z-1,n_heads,4] given dL/drgb [n_rays,3]: every head <= stage gets the same gradient, heads above are written 0 */
int xr_bungee_render_backward(const float* raw, const float* z_vals, const float* viewdirs, const float* noise, const float* grad_rgb,
                              uint32_t n_rays, uint32_t n_z, uint32_t n_heads, int stage, float density_bias, float rgb_padding,
                              int white_bkgd, int density_activation, float* grad_raw, void* stream);

#ifdef __cplusplus
}
#endif
#endif
