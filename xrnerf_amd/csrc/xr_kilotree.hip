// KiloNeRF distillation, the discovery loop's validation numbers (include/xrnerf_mi355_kilotree.h): what
// calculate_error_metrics and get_equal_error_split_threshold of the reference's save_distill_results_hook.py give per network, in one
// launch.  One workgroup owns one network's P points and walks them five times; nothing of size [N, P] is kept between the walks (the
// per-element errors are formed again from out and targets: 8 floats a point, which stay in the L2):
//   walk 0   the nine double sums, the saturation tests, the largest per-point split metric, the top digit of the three quantile keys
//   walk s   (s = 1 .. 3) digit s of the quantile keys still matching their prefix, digit s - 1 of the split's coordinate key
//   walk 4   the last digit of the coordinate key
// Quantiles: a radix select over the bit pattern of the non-negative fp32 value (it orders like the value; every NaN becomes the largest
// key), 8 bits a walk, counts in LDS.  Split threshold: the same select over the coordinate's ordered bit pattern with 64-bit fixed-point
// weights in place of counts (the scale is xr_fixed.h's: 2^(61 - b - e)), so the running sum is an integer and no order of the points
// can change it.  Un-fused fp32 (-ffp-contract=off): d d, |d| and |d| / (|t| + 0.1f) round like the tensor ops.
#include "xr_common.h"
#include "../../include/xrnerf_mi355_kilotree.h"

#define KT_BLOCK XR_KILOTREE_BLOCK
#define KT_WAVES (KT_BLOCK / XR_WAVE)
#define KT_NAN_KEY 0xffffffffu

static __device__ inline uint32_t kt_bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static __device__ inline float kt_float(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }
// the key of a non-negative float or a NaN (squared errors are never -0)
static __device__ inline uint32_t kt_value_key(float v) { return v != v ? KT_NAN_KEY : kt_bits(v); }
// the key of any float, ascending like the float; -0 was folded into +0 before
static __device__ inline uint32_t kt_coord_key(float v) { const uint32_t u = kt_bits(v); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
static __device__ inline float kt_coord_of(uint32_t k) { return kt_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

static __device__ inline float kt_mean4(const float* x) { return (float)(((((double)x[0] + (double)x[1]) + (double)x[2]) + (double)x[3]) / 4.0); }
static __device__ inline float kt_mean3(const float* x) { return (float)((((double)x[0] + (double)x[1]) + (double)x[2]) / 3.0); }

// the sum of v over the wave in a fixed order, valid in lane 0
static __device__ inline double kt_wave_sum(double v) {
    for (int off = XR_WAVE / 2; off; off >>= 1) v += __shfl_down(v, off);
    return v;
}

struct KtArgs {
    const float* out; const float* targets; const float* points;
    long long t_net, t_row, p_net, p_row;
    uint32_t P; uint32_t rank; const int32_t* axis; int metric; float* table; float* point_metric;
};

struct KtShared {
    uint32_t cnt[3][256];                // quantile digit counts
    unsigned long long w[256];           // split digit weights
    double part[12][KT_WAVES];           // per-wave sums, [metric * 4 + channel]
    float wmax[KT_WAVES];
    uint32_t wflag[KT_WAVES];
    uint32_t prefix[3], rank[3];         // the quantile selects
    uint32_t sprefix; int split;         // the split select: key prefix, still running
    unsigned long long carry, total;
    double scale;
};

// the errors of point p: se, ae (and ape when asked for)
static __device__ inline void kt_point(const KtArgs& a, const float* __restrict__ o, const float* __restrict__ t, uint32_t p, bool want_ape, float* se,
                                       float* ae, float* ape) {
    const float4 ov = *(const float4*)(o + (size_t)p * 4);
    const float* tp = t + (long long)p * a.t_row;
    const float oc[4] = {ov.x, ov.y, ov.z, ov.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float tc = tp[c];
        const float d = oc[c] - tc;
        se[c] = d * d;
        ae[c] = fabsf(d);
        ape[c] = want_ape ? ae[c] / (fabsf(tc) + 0.1f) : 0.f;
    }
}

static __global__ void __launch_bounds__(KT_BLOCK) k_kilotree(KtArgs a) {
    __shared__ KtShared s;
    const uint32_t n = blockIdx.x, tid = threadIdx.x, lane = tid % XR_WAVE, wave = tid / XR_WAVE, P = a.P;
    const float* __restrict__ o = a.out + (size_t)n * P * 4;
    const float* __restrict__ t = a.targets + (long long)n * a.t_net;
    int axis = a.axis ? a.axis[n] : -1;
    if (axis > 2) axis = -1;
    const float* __restrict__ x = axis >= 0 ? a.points + (long long)n * a.p_net + axis : nullptr;
    const int metric = a.metric;

    for (uint32_t e = tid; e < 256; e += KT_BLOCK) { s.cnt[0][e] = s.cnt[1][e] = s.cnt[2][e] = 0; s.w[e] = 0; }
    __syncthreads();

    // ---- walk 0
    {
        double acc[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) acc[k] = 0.0;
        float mmax = 0.f;
        uint32_t flag = 0;              // bits 0..11: a point broke all_p of {out ~ 0, target ~ 0, out ~ 1, target ~ 1} x channel; bit 12: a metric not finite
        for (uint32_t p = tid; p < P; p += KT_BLOCK) {
            float se[4], ae[4], ape[4];
            kt_point(a, o, t, p, true, se, ae, ape);
            const float4 ov = *(const float4*)(o + (size_t)p * 4);
            const float* tp = t + (long long)p * a.t_row;
            const float oc[3] = {ov.x, ov.y, ov.z};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float tc = tp[c];
                if (!(fabsf(oc[c]) < 0.001f)) flag |= 1u << c;
                if (!(fabsf(tc) < 0.001f)) flag |= 1u << (3 + c);
                if (!(fabsf(oc[c] - 1.f) < 0.001f)) flag |= 1u << (6 + c);
                if (!(fabsf(tc - 1.f) < 0.001f)) flag |= 1u << (9 + c);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) { acc[c] += (double)se[c]; acc[4 + c] += (double)ae[c]; acc[8 + c] += (double)ape[c]; }
            atomicAdd(&s.cnt[0][kt_value_key(kt_mean4(se)) >> 24], 1u);
            atomicAdd(&s.cnt[1][kt_value_key(kt_mean3(se)) >> 24], 1u);
            atomicAdd(&s.cnt[2][kt_value_key(se[3]) >> 24], 1u);
            const float m = kt_mean4(metric == XR_KT_METRIC_MSE ? se : metric == XR_KT_METRIC_MAE ? ae : ape);
            if (!(m <= 3.4028235e38f)) flag |= 1u << 12;
            else mmax = fmaxf(mmax, m);
            if (a.point_metric) a.point_metric[(size_t)n * P + p] = m;
        }
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const double v = kt_wave_sum(acc[k]);
            if (lane == 0) s.part[k][wave] = v;
        }
        for (int off = XR_WAVE / 2; off; off >>= 1) { mmax = fmaxf(mmax, __shfl_down(mmax, off)); flag |= __shfl_down(flag, off); }
        if (lane == 0) { s.wmax[wave] = mmax; s.wflag[wave] = flag; }
    }
    __syncthreads();
    if (tid < 3) {                       // the means of metric tid
        double c[4];
        for (int k = 0; k < 4; ++k) {
            double v = s.part[tid * 4 + k][0];
            for (uint32_t w = 1; w < KT_WAVES; ++w) v += s.part[tid * 4 + k][w];
            c[k] = v;
        }
        const double colour = (c[0] + c[1]) + c[2];
        float* row = a.table + (size_t)n * XR_KILOTREE_COLS + tid * 3;
        row[0] = (float)((colour + c[3]) / (4.0 * (double)P));
        row[1] = (float)(colour / (3.0 * (double)P));
        row[2] = (float)(c[3] / (double)P);
    }
    if (tid == 3) {                      // saturation, and the split's scale
        uint32_t flag = 0;
        float mmax = 0.f;
        for (uint32_t w = 0; w < KT_WAVES; ++w) { flag |= s.wflag[w]; mmax = fmaxf(mmax, s.wmax[w]); }
        bool sat = false;
        for (int c = 0; c < 3; ++c) {
            const bool o0 = !(flag >> c & 1u), t0 = !(flag >> (3 + c) & 1u), o1 = !(flag >> (6 + c) & 1u), t1 = !(flag >> (9 + c) & 1u);
            sat = sat || (o0 && !t0) || (o1 && !t1);
        }
        float* row = a.table + (size_t)n * XR_KILOTREE_COLS;
        row[XR_KT_SATURATION] = sat ? 1.f : 0.f;
        row[XR_KT_METRIC_MAX] = axis >= 0 ? mmax : 0.f;
        row[15] = 0.f;
        const bool split = axis >= 0 && !(flag >> 12 & 1u) && mmax > 0.f;
        s.split = split ? 1 : 0;
        if (split) {
            int ex = 0, b = 0;
            frexpf(mmax, &ex);
            while (b < 31 && (1u << b) < P) ++b;
            s.scale = ldexp(1.0, 61 - b - ex);
        } else {
            s.scale = 0.0;
            row[XR_KT_THRESHOLD] = kt_float(0x7fc00000u);
        }
        s.sprefix = 0; s.carry = 0; s.total = 0;
    }
    if (tid >= XR_WAVE && tid < XR_WAVE + 3) {   // the top digit of quantile tid - 64
        const uint32_t q = tid - XR_WAVE;
        uint32_t r = a.rank, b = 0;
        for (; b < 255; ++b) { const uint32_t c = s.cnt[q][b]; if (r < c) break; r -= c; }
        s.prefix[q] = b << 24; s.rank[q] = r;
    }
    __syncthreads();

    // ---- walks 1 .. 4
    for (int walk = 1; walk <= 4; ++walk) {
        const bool quant = walk <= 3, split = s.split != 0;
        const int qshift = 24 - 8 * walk, sshift = 32 - 8 * walk;
        const uint32_t pq0 = s.prefix[0], pq1 = s.prefix[1], pq2 = s.prefix[2], ps = s.sprefix;
        const double scale = s.scale;
        __syncthreads();
        for (uint32_t e = tid; e < 256; e += KT_BLOCK) { s.cnt[0][e] = s.cnt[1][e] = s.cnt[2][e] = 0; s.w[e] = 0; }
        __syncthreads();
        if (quant || split) {
            for (uint32_t p = tid; p < P; p += KT_BLOCK) {
                float se[4], ae[4], ape[4];
                kt_point(a, o, t, p, split && metric == XR_KT_METRIC_MAPE, se, ae, ape);
                if (quant) {
                    const uint32_t k0 = kt_value_key(kt_mean4(se)), k1 = kt_value_key(kt_mean3(se)), k2 = kt_value_key(se[3]);
                    if (((k0 ^ pq0) >> (qshift + 8)) == 0) atomicAdd(&s.cnt[0][(k0 >> qshift) & 255u], 1u);
                    if (((k1 ^ pq1) >> (qshift + 8)) == 0) atomicAdd(&s.cnt[1][(k1 >> qshift) & 255u], 1u);
                    if (((k2 ^ pq2) >> (qshift + 8)) == 0) atomicAdd(&s.cnt[2][(k2 >> qshift) & 255u], 1u);
                }
                if (split) {
                    const uint32_t k = kt_coord_key(x[(long long)p * a.p_row] + 0.f);
                    if (walk == 1 || ((k ^ ps) >> (sshift + 8)) == 0) {
                        const float m = kt_mean4(metric == XR_KT_METRIC_MSE ? se : metric == XR_KT_METRIC_MAE ? ae : ape);
                        const unsigned long long w = (unsigned long long)llrint((double)m * scale);
                        if (w) atomicAdd(&s.w[(k >> sshift) & 255u], w);
                    }
                }
            }
        }
        __syncthreads();
        if (quant && tid < 3) {
            uint32_t r = s.rank[tid], b = 0;
            for (; b < 255; ++b) { const uint32_t c = s.cnt[tid][b]; if (r < c) break; r -= c; }
            s.prefix[tid] |= b << qshift; s.rank[tid] = r;
            if (walk == 3) {
                const uint32_t k = s.prefix[tid];
                a.table[(size_t)n * XR_KILOTREE_COLS + XR_KT_QUANTILE + tid] = kt_float(k == KT_NAN_KEY ? 0x7fc00000u : k);
            }
        }
        if (split && tid == XR_WAVE) {
            unsigned long long total = s.total, carry = s.carry;
            if (walk == 1) {
                total = 0;
                for (uint32_t b = 0; b < 256; ++b) total += s.w[b];
                s.total = total;
            }
            uint32_t b = 0;
            for (; b < 255; ++b) { const unsigned long long w = s.w[b]; if (2 * (carry + w) > total) break; carry += w; }
            s.carry = carry;
            s.sprefix |= b << sshift;
            if (walk == 4) a.table[(size_t)n * XR_KILOTREE_COLS + XR_KT_THRESHOLD] = kt_coord_of(s.sprefix);
        }
        __syncthreads();
    }
}

extern "C" int xr_kilotree_val_metrics(const float* out, const float* targets, int64_t target_net_stride, int64_t target_row_stride,
                                       const float* points, int64_t point_net_stride, int64_t point_row_stride, uint32_t N, uint32_t P,
                                       int32_t quantile_index, const int32_t* split_axis, int split_metric, float* table, float* point_metric,
                                       void* stream) {
    XR_REQUIRE(out && targets && table, "out, targets and table must not be null");
    XR_REQUIRE(!split_axis || points, "split_axis without points");
    XR_REQUIRE(N >= 1 && P >= 1, "N and P must be at least 1");
    XR_REQUIRE(P <= XR_KILOTREE_MAX_POINTS, "P beyond XR_KILOTREE_MAX_POINTS");
    XR_REQUIRE(quantile_index >= 0 && (uint32_t)quantile_index < P, "quantile_index outside [0, P)");
    XR_REQUIRE(split_metric >= XR_KT_METRIC_MSE && split_metric <= XR_KT_METRIC_MAPE, "split_metric is 0 (mse), 1 (mae) or 2 (mape)");
    XR_REQUIRE(((uintptr_t)out & 15) == 0, "out must be 16-byte aligned");
    XR_REQUIRE(target_net_stride >= 0 && target_row_stride >= 0 && point_net_stride >= 0 && point_row_stride >= 0, "strides must not be negative");
    KtArgs a;
    a.out = out; a.targets = targets; a.points = points;
    a.t_net = target_net_stride; a.t_row = target_row_stride; a.p_net = point_net_stride; a.p_row = point_row_stride;
    a.P = P; a.rank = (uint32_t)quantile_index; a.axis = split_axis; a.metric = split_metric; a.table = table; a.point_metric = point_metric;
    hipLaunchKernelGGL(k_kilotree, dim3(N), dim3(KT_BLOCK), 0, (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return XR_OK;
}
