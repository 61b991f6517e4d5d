/* KiloNeRF distillation, the discovery loop's validation numbers: the entry point of libxrnerf_mi355.so that turns one validation pass of a
 * batch of student networks into the per-network table SaveDistillResultsHook decides on (xrnerf_amd/csrc/xr_kilotree.hip, DESIGN.md
 * section 25).  A header of its own, bound by its own ctypes table (xrnerf_amd/_lib.py KILOTREE_SIGNATURES).
 * Conventions of xrnerf_mi355_eval.h: 0 or a negative XR_E* code (message: xr_last_error()); never throws, syncs or allocates; raw
 * device pointers; the launch goes to `stream`.  The same input gives the same bits: every floating-point sum is taken in a fixed order,
 * every atomic adds integers.  XR_EINVAL launches nothing and leaves every output untouched. */
#ifndef XRNERF_MI355_KILOTREE_H
#define XRNERF_MI355_KILOTREE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define XR_KILOTREE_BLOCK 256u           /* one workgroup of 256 threads owns one network's P points */
#define XR_KILOTREE_MAX_POINTS (1u << 24) /* P beyond this is refused: the 64-bit fixed-point running sum keeps 61 - 24 bits per weight */
#define XR_KILOTREE_COLS 16u             /* floats per network in `table` */
/* columns of `table` */
#define XR_KT_MSE 0u                     /* mse: all four channels, colour (0..2), density (3) */
#define XR_KT_MAE 3u                     /* mae: likewise */
#define XR_KT_MAPE 6u                    /* mape: likewise */
#define XR_KT_QUANTILE 9u                /* quantile_se: total, colour, density */
#define XR_KT_SATURATION 12u             /* 1.f or 0.f */
#define XR_KT_THRESHOLD 13u              /* the equal-error split threshold, or NaN */
#define XR_KT_METRIC_MAX 14u             /* the largest finite per-point split metric (what fixes the fixed-point unit), 0.f without a split */
/* column 15 is written as 0.f */
#define XR_KT_METRIC_MSE 0
#define XR_KT_METRIC_MAE 1
#define XR_KT_METRIC_MAPE 2

/* out [N,P,4] fp32 contiguous, 16-byte aligned.  targets: N x P rows of 4 floats, points: N x P rows of 3 floats, each row contiguous, with
 * element strides (network, row) -- columns 6:10 and 0:3 of the example rows are such views.  Per element, in fp32 exactly as the tensor ops
 * form them: d = out - target, se = d d, ae = |d|, ape = ae / (|target| + 0.1f).  Per network n:
 *   table[n][XR_KT_MSE + {0,1,2}] (MAE, MAPE likewise)   the double sum of the fp32 errors over {all four, the first three, the last}
 *        channel(s) and all P points -- per channel over the points in a fixed order, then ((c0 + c1) + c2) + c3 -- divided once by the
 *        element count and rounded to fp32 once
 *   table[n][XR_KT_QUANTILE + {0,1,2}]   the order statistic of rank quantile_index (0-based, ascending, NaN last) of the per-point
 *        squared error: total (float)((((se0 + se1) + se2) + se3) / 4.0), colour (float)(((se0 + se1) + se2) / 3.0), sums in double;
 *        density se3 itself.  A NaN comes back as the canonical quiet NaN
 *   table[n][XR_KT_SATURATION]   any colour channel c with all_p(|out_c| < 1e-3f) and not all_p(|target_c| < 1e-3f), or the same with
 *        |out_c - 1.f|, |target_c - 1.f|
 *   table[n][XR_KT_THRESHOLD]   with split_axis non-null and 0 <= split_axis[n] <= 2: over the per-point metric m_p =
 *        (float)((((x0 + x1) + x2) + x3) / 4.0), x the channel errors `split_metric` names, and the coordinate c_p = points[n][p][axis] + 0.f:
 *        the smallest coordinate c with 2 W(c) > W(+inf), W(c) the sum over the points with c_p <= c of w_p = llrint(m_p scale),
 *        scale = 2^(61 - b - e), max_p m_p < 2^e, P <= 2^b.  A function of the multiset of (c_p, m_p) pairs: integer sums, any order.
 *        NaN when every m_p is 0 or one of them is not finite, when split_axis is null or split_axis[n] is outside 0 .. 2
 *   point_metric [N,P] (may be null)   m_p
 * Refused (XR_EINVAL): a null out, targets or table; points null while split_axis is not; N or P of 0; P beyond XR_KILOTREE_MAX_POINTS;
 * quantile_index outside [0, P); a split_metric outside 0 .. 2; out not 16-byte aligned.  One launch of N workgroups. */
int xr_kilotree_val_metrics(const float* out, const float* targets, int64_t target_net_stride, int64_t target_row_stride, const float* points,
                            int64_t point_net_stride, int64_t point_row_stride, uint32_t N, uint32_t P, int32_t quantile_index,
                            const int32_t* split_axis, int split_metric, float* table, float* point_metric, void* stream);

#ifdef __cplusplus
}
#endif
#endif
