/* GNR image-encoder entry points of libxrnerf_mi355.so (xrnerf_amd/csrc/xr_gnr_encoder.hip): the layers of the stacked-hourglass
 * filter (`HGFilter` of configs/gnr/gnr_genebody.py: ConvBlock, HourGlass) on channel-last activations.
 * A header of their own, bound by their own ctypes table (xrnerf_amd/_lib.py GNR_ENCODER_SIGNATURES), like xrnerf_mi355_gnr.h.
 * Conventions of xrnerf_mi355.h: 0 or a negative XR_E* code (message: xr_last_error()); never throws, syncs or allocates; raw device
 * pointers, fp32; the launch goes to `stream`.  No float atomics: the same input gives the same bits.
 *
 * Activations.  A map is [N, H, W, C] with C contiguous and a ROW STRIDE ld >= C floats between two pixels; the pointer handed over is
 * the address of channel 0 of the slice, so a layer reads or writes a column range of a wider buffer (pointer = buffer + first
 * column).  Pointers are 16-byte aligned and ld, C are multiples of 4 (16-byte vector access) -- except the input of a convolution
 * whose Cin is no multiple of 16 (the 3-channel stem), which is read element by element and needs neither.
 * XR_EINVAL (nothing launched): a null pointer, a row stride below the slice, a size of 0 where work remains, an unsupported shape.
 * N = 0 is a no-op that returns 0. */
#ifndef XRNERF_MI355_GNR_ENCODER_H
#define XRNERF_MI355_GNR_ENCODER_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define XR_HG_STATS_PIXELS 128       /* pixels per workgroup of the statistics' first pass */

/* k x k convolution, k in {1, 3, 7}, stride in {1, 2}, zero padding k / 2: y [N, Ho, Wo, Cout] with Ho = (H + 2 (k / 2) - k) / stride + 1.
 * An implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32): rows = output pixels, contraction over (tap, Cin) in that order.
 * w_kc [k k Cin, Cout]: the weight re-laid ONCE by the caller, row (ky k + kx) Cin + c, column = output channel
 * (torch: weight.permute(2, 3, 1, 0).reshape(-1, Cout)).  Cout is a multiple of 4.
 * gn_mean / gn_rstd [N, gn_groups] and gn_gamma / gn_beta [Cin] (all four or none): the input is relu(group_norm(x)) computed as it
 * is loaded; Cin / gn_groups is a power of two.  A tap outside the image contributes exactly 0 (the padding follows the norm).
 * bias [Cout] nullable; relu != 0: max(., 0) on the output; accumulate != 0: y = y + (result) instead of y = result. */
int xr_hg_conv2d(const float* x, uint32_t ldx, uint32_t N, uint32_t H, uint32_t W, uint32_t Cin, const float* w_kc, uint32_t Cout, int ksize,
                 int stride, const float* gn_mean, const float* gn_rstd, const float* gn_gamma, const float* gn_beta, uint32_t gn_groups,
                 const float* bias, int relu, int accumulate, float* y, uint32_t ldy, void* stream);
/* per (image, group) mean and 1 / sqrt(biased variance + eps) of x [N, HW, C] -> mean, rstd [N, groups].  C is a power of two in
 * 4 .. 1024 and C / groups a power of two.  Two launches: per-workgroup partial sums (fp64) over XR_HG_STATS_PIXELS pixels into
 * `workspace`, then one workgroup per image adds them in a fixed order.  At most 256 groups. */
size_t xr_hg_gn_stats_workspace_bytes(uint32_t N, uint32_t HW, uint32_t groups);
int xr_hg_gn_stats(const float* x, uint32_t ldx, uint32_t N, uint32_t HW, uint32_t C, uint32_t groups, float eps, float* mean, float* rstd,
                   void* workspace, size_t workspace_bytes, void* stream);
/* y = relu(group_norm(x)) from the statistics above (y may be x) */
int xr_hg_gn_relu(const float* x, uint32_t ldx, uint32_t N, uint32_t HW, uint32_t C, uint32_t groups, const float* mean, const float* rstd,
                  const float* gamma, const float* beta, float* y, uint32_t ldy, void* stream);
/* F.avg_pool2d(x, 2, stride=2): y [N, H / 2, W / 2, C] (floor on odd sizes) */
int xr_hg_avgpool2(const float* x, uint32_t ldx, uint32_t N, uint32_t H, uint32_t W, uint32_t C, float* y, uint32_t ldy, void* stream);
/* F.interpolate(x, scale_factor=2, mode='bicubic', align_corners=True): y [N, 2 H, 2 W, C] (+ addend [N, 2 H, 2 W, C] when given;
 * y may be addend).  A = -0.75, clamped taps, source coordinate dst (in - 1) / (out - 1). */
int xr_hg_bicubic_up2(const float* x, uint32_t ldx, uint32_t N, uint32_t H, uint32_t W, uint32_t C, const float* addend, uint32_t ldadd,
                      float* y, uint32_t ldy, void* stream);
/* y [rows, C] = y + x */
int xr_hg_add(const float* x, uint32_t ldx, uint64_t rows, uint32_t C, float* y, uint32_t ldy, void* stream);
/* one ConvBlock (conv1 | conv2 | conv3 into the column ranges [0, Cout/2), [Cout/2, 3 Cout/4), [3 Cout/4, Cout) of y, each reading
 * relu(group_norm(.)) of its input, then the residual) as the entry points above in sequence: ten launches, one call.  w1, w2, w3 and
 * w_down are re-laid weights (xr_hg_conv2d); w_down = NULL: the residual is x itself (Cin == Cout), else the 1x1 convolution of
 * relu(group_norm(x; gamma4, beta4)).  x and y must not overlap.  Cout is a multiple of 16. */
size_t xr_hg_conv_block_workspace_bytes(uint32_t N, uint32_t HW, uint32_t groups);
int xr_hg_conv_block(const float* x, uint32_t ldx, uint32_t N, uint32_t H, uint32_t W, uint32_t Cin, uint32_t Cout, const float* w1,
                     const float* w2, const float* w3, const float* w_down, const float* gamma1, const float* beta1, const float* gamma2,
                     const float* beta2, const float* gamma3, const float* beta3, const float* gamma4, const float* beta4, uint32_t groups,
                     float eps, float* y, uint32_t ldy, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
