/* Animatable-NeRF entry points of libxrnerf_mi355.so (xrnerf_amd/csrc/xr_aninerf.hip): what stands around the 256-wide MLPs in a step of
 * configs/animatable_nerf/an_h36m_s9_train_pose.py -- the nearest-SMPL-vertex query, the "near the body" compaction, the blend-weight
 * head, linear blend skinning with its backward, and the input gradient of the positional encoding.  A header of their own, bound by
 * their own ctypes table (xrnerf_amd/_lib.py ANINERF_SIGNATURES), like xrnerf_mi355_vanilla.h.
 * Conventions of xrnerf_mi355.h: 0 or a negative XR_E* code (message: xr_last_error()); never throws, syncs or allocates; raw device
 * pointers, fp32 (indices, flags and counts: int32), contiguous unless a row stride is given; the launch goes to `stream`.  No atomics,
 * every reduction has a fixed order: the same input gives the same bits.  A count of 0 points is a no-op that returns 0. */
#ifndef XRNERF_MI355_ANINERF_H
#define XRNERF_MI355_ANINERF_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define XR_ANI_JOINTS 24          /* blend-weight channels (SMPL joints) */
#define XR_ANI_CLOSEST_TILE 1024  /* vertices staged in LDS at a time by xr_ani_closest */

/* sample_closest_points (xrnerf/models/networks/utils/aninerf.py; knn_points with K = 1) for pts [n,3] against verts [n_verts,3].
 * With R [3,3] and T [3] (both or neither) points and vertices first go to the pose space, q_j = sum_k (p_k - T_k) R_kj with k ascending;
 * without them q = p.  d2 = (dx dx + dy dy) + dz dz in un-fused fp32; the smallest d2 wins, the lowest index on an exact tie.
 * -> q_out [n,3] (nullable), idx_out [n] int32, d2_out [n] (nullable), dist_out [n] = sqrtf(d2), flag_out [n] int32 = dist < th.
 * n_verts >= 1. */
int xr_ani_closest(const float* pts, const float* verts, const float* R, const float* T, uint32_t n, uint32_t n_verts, float th,
                   float* q_out, int32_t* idx_out, float* d2_out, float* dist_out, int32_t* flag_out, void* stream);
/* bytes of workspace xr_ani_select needs for n points */
size_t xr_ani_select_workspace_bytes(uint32_t n);
/* pind = flags; pind[argmin(dist)] = True (lowest index on a tie); list = nonzero(pind) in ascending order, count [1] = its length.
 * Three launches (per-block counts and minima, one block that orders them, the ranked write); n = 0 writes count = 0. */
int xr_ani_select(const int32_t* flags, const float* dist, uint32_t n, int32_t* list, int32_t* count, void* workspace,
                  size_t workspace_bytes, void* stream);
/* bw[i,:] = softmax_j(logf(smpl_bw[idx[i], j] + 1e-9) + logits[i, j]) over 24 channels (max subtracted); smpl_bw [n_verts,24],
 * idx [n] in [0, n_verts) (not checked), logits / bw [n,24]; all three matrices 16-byte aligned. */
int xr_ani_blend_forward(const float* smpl_bw, const int32_t* idx, const float* logits, uint32_t n, float* bw, void* stream);
/* dlogits = bw * (g - sum_j g_j bw_j), evaluated as bw_j sum_k bw_k (g_j - g_k) (no cancellation on a peaked row);
 * bw / grad_bw / grad_logits [n,24], 16-byte aligned */
int xr_ani_blend_backward(const float* bw, const float* grad_bw, uint32_t n, float* grad_logits, void* stream);
/* linear blend skinning there and back: A = sum_j bw_j a_from[j], B = sum_j bw_j a_to[j] (24 row-major 4x4 matrices each),
 *   p' = A_R^-1 (p - A_t), p'' = B_R p' + B_t -> pts_out [n,3];   d'' = B_R A_R^-1 d -> dirs_out [n,3] (dirs may be NULL).
 * The 3x3 inverse is adjugate / determinant in fp32.  bw [n,24] 16-byte aligned. */
int xr_ani_skin_forward(const float* pts, const float* dirs, const float* bw, const float* a_from, const float* a_to, uint32_t n,
                        float* pts_out, float* dirs_out, void* stream);
/* dL/dbw [n,24] (16-byte aligned) given dL/dp'' (grad_pts, nullable) and dL/dd'' (grad_dirs, nullable; needs dirs), recomputed from the
 * forward's inputs.  pts and dirs get no gradient (they carry none in the reference's step). */
int xr_ani_skin_backward(const float* pts, const float* dirs, const float* bw, const float* a_from, const float* a_to, uint32_t n,
                         const float* grad_pts, const float* grad_dirs, float* grad_bw, void* stream);
/* input gradient of BaseEmbedder's encoding [p, sin(2^0 p), cos(2^0 p), .., sin(2^(L-1) p), cos(2^(L-1) p)]: grad row i = grad + i ld
 * (3 + 6 L columns read), dL/dp = g_p + sum_l 2^l (g_sin,l cos(2^l p) - g_cos,l sin(2^l p)) with l ascending -> grad_pts [n,3].
 * multires in [0, 16], ld >= 3 + 6 multires. */
int xr_ani_encode_backward(const float* pts, const float* grad, uint32_t ld, uint32_t n, int multires, float* grad_pts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
