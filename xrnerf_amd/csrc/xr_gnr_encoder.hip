// GNR's image encoder (configs/gnr/gnr_genebody.py: image_filter = HGFilter, the stacked hourglass of xrnerf/models/embedders/
// gnr_embedder.py) on channel-last activations: the reference hands these layers to the vendor convolution library in NCHW; here
//   xr_hg_conv2d       k x k convolution as an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32, an fmaf chain per output): rows =
//                      output pixels, contraction over (tap, Cin).  The panel / accumulator scheme is k_gemm_f32's (xr_gemm.hip):
//                      operands staged through LDS as [k][row] panels of 32 k, two buffers, the next panel's global loads in flight while
//                      the current one is multiplied.  The A panel is gathered from the input map -- a tap outside the image is a panel
//                      of zeros -- with GroupNorm + ReLU applied on the way in; bias, ReLU and "add to the output" in the epilogue.
//   xr_hg_gn_stats     GroupNorm's per-(image, group) mean and rstd, two launches with a fixed summation order
//   xr_hg_gn_relu, xr_hg_avgpool2, xr_hg_bicubic_up2, xr_hg_add   the elementwise layers between the convolutions
// A map is [N, H, W, C] with a row stride ld >= C, so ConvBlock's three convolutions write the column ranges of one buffer (no cat) and
// the filter's output is the buffer the renderer's pixel gather reads.  No float atomics, no workspace beyond the statistics' partials.
#include "xr_common.h"
#include "../../include/xrnerf_mi355_gnr_encoder.h"

typedef float hg_f32x16 __attribute__((ext_vector_type(16)));
#define HG_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
#define HG_BK 32                                 // contraction entries per panel: every Cin but the stem's is a multiple, so a panel is one tap
#define HG_FLUSH 2                               // panels per partial sum: the MFMA chain is folded into a second accumulator every 64 entries

struct HgConv {
    const float* x; const float* w; float* y;
    const float* mean; const float* rstd; const float* gamma; const float* beta;     // all four or none
    const float* bias;
    uint32_t H, W, Cin, Ho, Wo, Cout, ldx, ldy;
    uint32_t M, K;                               // output pixels N Ho Wo; contraction length ks ks Cin
    int ks, stride, pad;
    uint32_t groups, cg_shift;                   // channels per group = 1 << cg_shift
    int relu, accumulate;
    int flat;                                    // Cin is no multiple of HG_BK: a panel crosses taps, the input is read element by element
};

__device__ __forceinline__ float hg_norm_relu(const HgConv& g, float v, uint32_t n, uint32_t c) {
    const uint32_t s = n * g.groups + (c >> g.cg_shift);
    const float a = g.rstd[s] * g.gamma[c];
    return fmaxf(fmaf(v, a, g.beta[c] - g.mean[s] * a), 0.f);
}

// Workgroup = (32 WMT WGM) x (32 WNT WGN) outputs, 4 waves in WGM x WGN, each WMT x WNT accumulators of 32 x 32:
//   <2, 2, 2, 2>  128 x 128   the wide layers at the large maps
//   <1, 2, 4, 1>  128 x 64    Cout <= 64 at the large maps: no column of the tile is idle
//   <1, 1, 2, 2>   64 x 64    the small maps (32 x 32 and below), where 128-row tiles leave most of the chip without a workgroup
template <int WMT, int WNT, int WGM, int WGN>
__global__ void __launch_bounds__(256, 2) k_hg_conv(HgConv g) {
    static_assert(WGM * WGN == 4, "four waves");
    constexpr int BM = 32 * WMT * WGM, BN = 32 * WNT * WGN;
    constexpr int CPT = HG_BK * BM / 256;         // A: contraction entries per thread (threads t, t + BM, .. share a row)
    constexpr int F4 = BN / 4, RPP = 256 / F4, NB = HG_BK / RPP;      // B: float4 per k-row, k-rows per pass, passes
    __shared__ float sA[2][HG_BK * BM];
    __shared__ __attribute__((aligned(16))) float sB[2][HG_BK * BN];
    const uint32_t t = threadIdx.x;
    const uint32_t m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int lane = t & 63, col = lane & 31, hi = lane >> 5;
    const int wave = t >> 6, wm = wave / WGN, wn = wave % WGN;
    // this thread's row of the A panel = one output pixel
    const uint32_t arow = t % BM, acoff = (t / BM) * CPT;
    const uint32_t row = m0 + arow;
    const bool rvalid = row < g.M;
    const uint32_t pn = row / (g.Ho * g.Wo), prem = row - pn * (g.Ho * g.Wo);
    const int iy0 = (int)(prem / g.Wo) * g.stride - g.pad, ix0 = (int)(prem % g.Wo) * g.stride - g.pad;
    const bool norm = g.mean != nullptr;
    // a single fmaf chain over (tap, Cin) -- up to 2304 terms -- loses more than the blocked sums of a CPU convolution, which the bars are
    // taken from: the chain restarts every HG_FLUSH panels and its partial sums are added in order (fixed, so the bits repeat)
    hg_f32x16 acc[WMT][WNT], total[WMT][WNT];
#pragma unroll
    for (int i = 0; i < WMT; ++i)
#pragma unroll
        for (int j = 0; j < WNT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; total[i][j][r] = 0.f; }
    float ra[CPT];
    float4 rb[NB];
    auto load = [&](uint32_t k0) {
#pragma unroll
        for (int e = 0; e < CPT; ++e) ra[e] = 0.f;
        if (!g.flat) {                            // one tap per panel (uniform), CPT consecutive channels per thread
            const uint32_t tap = k0 / g.Cin, c = k0 - tap * g.Cin + acoff;
            const int iy = iy0 + (int)(tap / g.ks), ix = ix0 + (int)(tap % g.ks);
            if (rvalid && iy >= 0 && iy < (int)g.H && ix >= 0 && ix < (int)g.W) {
                const float* p = g.x + ((size_t)(pn * g.H + iy) * g.W + ix) * g.ldx + c;
#pragma unroll
                for (int q = 0; q < CPT / 4; ++q) {
                    const float4 v = *reinterpret_cast<const float4*>(p + 4 * q);
                    ra[4 * q] = v.x; ra[4 * q + 1] = v.y; ra[4 * q + 2] = v.z; ra[4 * q + 3] = v.w;
                }
                if (norm) {
#pragma unroll
                    for (int e = 0; e < CPT; ++e) ra[e] = hg_norm_relu(g, ra[e], pn, c + e);
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < CPT; ++e) {
                const uint32_t kk = k0 + acoff + e;
                if (!rvalid || kk >= g.K) continue;
                const uint32_t tap = kk / g.Cin, c = kk - tap * g.Cin;
                const int iy = iy0 + (int)(tap / g.ks), ix = ix0 + (int)(tap % g.ks);
                if (iy < 0 || iy >= (int)g.H || ix < 0 || ix >= (int)g.W) continue;
                const float v = g.x[((size_t)(pn * g.H + iy) * g.W + ix) * g.ldx + c];
                ra[e] = norm ? hg_norm_relu(g, v, pn, c) : v;
            }
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const uint32_t k = k0 + t / F4 + RPP * j, n = n0 + (t % F4) * 4;
            rb[j] = (k < g.K && n < g.Cout) ? *reinterpret_cast<const float4*>(g.w + (size_t)k * g.Cout + n) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    load(0);
    int buf = 0, chained = 0;
    for (uint32_t k0 = 0; k0 < g.K; k0 += HG_BK) {
#pragma unroll
        for (int e = 0; e < CPT; ++e) sA[buf][(acoff + e) * BM + arow] = ra[e];
#pragma unroll
        for (int j = 0; j < NB; ++j) *reinterpret_cast<float4*>(&sB[buf][(t / F4 + RPP * j) * BN + (t % F4) * 4]) = rb[j];
        __syncthreads();                                   // panel `buf` complete; the other buffer was consumed one step ago
        if (k0 + HG_BK < g.K) load(k0 + HG_BK);
        const float* pa = sA[buf] + hi * BM + wm * 32 * WMT + col;
        const float* pb = sB[buf] + hi * BN + wn * 32 * WNT + col;
#pragma unroll
        for (int s = 0; s < HG_BK / 2; ++s) {
            float a[WMT], b[WNT];
#pragma unroll
            for (int i = 0; i < WMT; ++i) a[i] = pa[2 * s * BM + 32 * i];
#pragma unroll
            for (int j = 0; j < WNT; ++j) b[j] = pb[2 * s * BN + 32 * j];
#pragma unroll
            for (int i = 0; i < WMT; ++i)
#pragma unroll
                for (int j = 0; j < WNT; ++j) acc[i][j] = HG_MFMA(a[i], b[j], acc[i][j]);
        }
        buf ^= 1;
        if (++chained == HG_FLUSH || k0 + HG_BK >= g.K) {
            chained = 0;
#pragma unroll
            for (int i = 0; i < WMT; ++i)
#pragma unroll
                for (int j = 0; j < WNT; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) { total[i][j][r] += acc[i][j][r]; acc[i][j][r] = 0.f; }
        }
    }
    // epilogue: lane l, register r of a 32x32 accumulator holds row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
#pragma unroll
    for (int i = 0; i < WMT; ++i)
#pragma unroll
        for (int j = 0; j < WNT; ++j) {
            const uint32_t n = n0 + wn * 32 * WNT + j * 32 + col;
            if (n >= g.Cout) continue;
            const float b = g.bias != nullptr ? g.bias[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t m = m0 + wm * 32 * WMT + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (m < g.M) {
                    float v = total[i][j][r] + b;
                    if (g.relu) v = fmaxf(v, 0.f);
                    float* o = g.y + (size_t)m * g.ldy + n;
                    if (g.accumulate) v = *o + v;
                    *o = v;
                }
            }
        }
}

static inline bool hg_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline int hg_log2(uint32_t v) { int s = 0; while ((1u << s) < v) ++s; return (1u << s) == v ? s : -1; }

extern "C" int xr_hg_conv2d(const float* x, uint32_t ldx, uint32_t N, uint32_t H, uint32_t W, uint32_t Cin, const float* w_kc, uint32_t Cout,
                            int ksize, int stride, const float* gn_mean, const float* gn_rstd, const float* gn_gamma, const float* gn_beta,
                            uint32_t gn_groups, const float* bias, int relu, int accumulate, float* y, uint32_t ldy, void* stream) {
    XR_REQUIRE(ksize == 1 || ksize == 3 || ksize == 7, "the kernel size must be 1, 3 or 7");
    XR_REQUIRE(stride == 1 || stride == 2, "the stride must be 1 or 2");
    if (N == 0) return XR_OK;
    XR_REQUIRE(x && w_kc && y, "null pointer");
    XR_REQUIRE(H >= 1 && W >= 1 && Cin >= 1 && Cout >= 4 && Cout % 4 == 0, "bad shape (Cout must be a multiple of 4)");
    XR_REQUIRE(ldx >= Cin && ldy >= Cout, "a row stride is smaller than its slice");
    XR_REQUIRE(hg_aligned(w_kc) && hg_aligned(y) && ldy % 4 == 0, "the weight, the output and its row stride must allow 16-byte access");
    const int flat = Cin % HG_BK != 0;
    XR_REQUIRE(flat || (hg_aligned(x) && ldx % 4 == 0), "the input and its row stride must allow 16-byte access");
    const bool any = gn_mean || gn_rstd || gn_gamma || gn_beta, all = gn_mean && gn_rstd && gn_gamma && gn_beta;
    XR_REQUIRE(any == all, "the norm prologue takes mean, rstd, gamma and beta together");
    int cg_shift = 0;
    if (all) {
        XR_REQUIRE(gn_groups >= 1 && Cin % gn_groups == 0, "the groups must divide Cin");
        cg_shift = hg_log2(Cin / gn_groups);
        XR_REQUIRE(cg_shift >= 0, "the channels of a group must be a power of two");
    }
    const int pad = ksize / 2;
    const uint32_t Ho = (H + 2 * pad - ksize) / stride + 1, Wo = (W + 2 * pad - ksize) / stride + 1;
    const uint64_t M = (uint64_t)N * Ho * Wo;
    XR_REQUIRE(M <= (1ull << 31) && (uint64_t)N * H * W <= (1ull << 31), "more than 2^31 pixels in one call");
    HgConv g{x, w_kc, y, gn_mean, gn_rstd, gn_gamma, gn_beta, bias, H, W, Cin, Ho, Wo, Cout, ldx, ldy, (uint32_t)M,
             (uint32_t)(ksize * ksize) * Cin, ksize, stride, pad, gn_groups, (uint32_t)cg_shift, relu, accumulate, flat};
    const uint64_t wide = (uint64_t)xr_div_up(M, 128) * xr_div_up(Cout, 128);
    if (Cout >= 128 && wide >= 256) {
        XR_REQUIRE(xr_div_up(M, 128) <= 65535, "too many row tiles");
        hipLaunchKernelGGL((k_hg_conv<2, 2, 2, 2>), dim3(xr_div_up(Cout, 128), xr_div_up(M, 128)), dim3(256), 0, (hipStream_t)stream, g);
    } else if (Cout <= 64 && xr_div_up(M, 128) >= 256) {
        XR_REQUIRE(xr_div_up(M, 128) <= 65535, "too many row tiles");
        hipLaunchKernelGGL((k_hg_conv<1, 2, 4, 1>), dim3(1, xr_div_up(M, 128)), dim3(256), 0, (hipStream_t)stream, g);
    } else {
        XR_REQUIRE(xr_div_up(M, 64) <= 65535, "too many row tiles");
        hipLaunchKernelGGL((k_hg_conv<1, 1, 2, 2>), dim3(xr_div_up(Cout, 64), xr_div_up(M, 64)), dim3(256), 0, (hipStream_t)stream, g);
    }
    XR_LAUNCH_CHECK();
    return XR_OK;
}

// ---------------------------------------------------------------- GroupNorm statistics
// first pass: workgroup (chunk, image) sums XR_HG_STATS_PIXELS pixels of every channel of the slice.  Thread = one float4 of channels
// (t % (C / 4)) and one pixel phase (t / (C / 4)); its fp64 sums go to LDS, and thread g < groups adds group g's channels and phases
// in ascending order.  part [N, chunks, groups] x (sum, sum of squares).
__global__ void __launch_bounds__(256) k_hg_stats_partial(const float* __restrict__ x, uint32_t ldx, uint32_t HW, uint32_t C, uint32_t groups,
                                                          double2* __restrict__ part) {
    __shared__ double s_sum[1024], s_sq[1024];
    const uint32_t t = threadIdx.x, Q = C / 4, P = 256 / Q;
    const uint32_t q = t % Q, ph = t / Q;
    const uint32_t n = blockIdx.y, p0 = blockIdx.x * XR_HG_STATS_PIXELS;
    const uint32_t p1 = p0 + XR_HG_STATS_PIXELS < HW ? p0 + XR_HG_STATS_PIXELS : HW;
    double s[4] = {0., 0., 0., 0.}, ss[4] = {0., 0., 0., 0.};
#pragma unroll 4
    for (uint32_t p = p0 + ph; p < p1; p += P) {
        const float4 v = *reinterpret_cast<const float4*>(x + ((size_t)n * HW + p) * ldx + q * 4);
        const double d[4] = {(double)v.x, (double)v.y, (double)v.z, (double)v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) { s[e] += d[e]; ss[e] += d[e] * d[e]; }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { s_sum[ph * C + q * 4 + e] = s[e]; s_sq[ph * C + q * 4 + e] = ss[e]; }
    __syncthreads();
    for (uint32_t gi = t; gi < groups; gi += 256) {
        const uint32_t cg = C / groups;
        double a = 0., b = 0.;
        for (uint32_t c = gi * cg; c < (gi + 1) * cg; ++c)
            for (uint32_t f = 0; f < P; ++f) { a += s_sum[f * C + c]; b += s_sq[f * C + c]; }
        part[((size_t)n * gridDim.x + blockIdx.x) * groups + gi] = make_double2(a, b);
    }
}

// second pass: workgroup = image.  Thread (phase, group) adds the chunks phase, phase + phases, .. of its group in ascending order,
// thread `group` then adds the phases in ascending order.
__global__ void __launch_bounds__(256) k_hg_stats_final(const double2* __restrict__ part, uint32_t chunks, uint32_t groups, double count,
                                                        float eps, float* __restrict__ mean, float* __restrict__ rstd) {
    __shared__ double2 s_part[256];
    const uint32_t n = blockIdx.x, t = threadIdx.x, phases = 256 / groups;
    const uint32_t gi = t % groups, ph = t / groups;
    double a = 0., b = 0.;
    if (ph < phases) {
#pragma unroll 4
        for (uint32_t c = ph; c < chunks; c += phases) { const double2 v = part[((size_t)n * chunks + c) * groups + gi]; a += v.x; b += v.y; }
    }
    s_part[t] = make_double2(a, b);
    __syncthreads();
    if (t >= groups) return;
    a = 0.; b = 0.;
    for (uint32_t f = 0; f < phases; ++f) { a += s_part[f * groups + t].x; b += s_part[f * groups + t].y; }
    const double m = a / count;
    double var = b / count - m * m;
    if (!(var > 0.)) var = 0.;
    mean[n * groups + t] = (float)m;
    rstd[n * groups + t] = (float)(1. / sqrt(var + (double)eps));
}

extern "C" size_t xr_hg_gn_stats_workspace_bytes(uint32_t N, uint32_t HW, uint32_t groups) {
    return (size_t)N * xr_div_up(HW, XR_HG_STATS_PIXELS) * groups * sizeof(double2);
}

static int hg_slice_ok(const char* fn, const void* p, uint32_t ld, uint32_t C) {
    if (!p) { xr_set_error("%s: null pointer", fn); return XR_EINVAL; }
    if (C < 4 || C % 4 != 0 || ld < C || ld % 4 != 0 || !hg_aligned(p)) {
        xr_set_error("%s: a slice must be 16-byte aligned, C and ld multiples of 4, ld >= C", fn);
        return XR_EINVAL;
    }
    return XR_OK;
}
#define HG_SLICE(p, ld, C) do { const int rc_ = hg_slice_ok(__func__, (p), (ld), (C)); if (rc_ != XR_OK) return rc_; } while (0)

extern "C" int xr_hg_gn_stats(const float* x, uint32_t ldx, uint32_t N, uint32_t HW, uint32_t C, uint32_t groups, float eps, float* mean,
                              float* rstd, void* workspace, size_t workspace_bytes, void* stream) {
    if (N == 0) return XR_OK;
    HG_SLICE(x, ldx, C);
    XR_REQUIRE(mean && rstd && workspace, "null pointer");
    XR_REQUIRE(HW >= 1 && (uint64_t)N * HW <= (1ull << 31), "bad pixel count");
    XR_REQUIRE(C <= 1024 && hg_log2(C) >= 0, "C must be a power of two in 4 .. 1024");
    XR_REQUIRE(groups >= 1 && groups <= 256 && C % groups == 0 && hg_log2(C / groups) >= 0, "at most 256 groups, C / groups a power of two");
    XR_REQUIRE(N <= 65535, "more than 65535 images");
    XR_REQUIRE(((uintptr_t)workspace & 15) == 0, "the workspace must be 16-byte aligned");
    if (workspace_bytes < xr_hg_gn_stats_workspace_bytes(N, HW, groups)) { xr_set_error("%s: workspace too small", __func__); return XR_ENOMEM; }
    const uint32_t chunks = xr_div_up(HW, XR_HG_STATS_PIXELS);
    hipLaunchKernelGGL(k_hg_stats_partial, dim3(chunks, N), dim3(256), 0, (hipStream_t)stream, x, ldx, HW, C, groups, (double2*)workspace);
    XR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_hg_stats_final, dim3(N), dim3(256), 0, (hipStream_t)stream, (const double2*)workspace, chunks, groups,
                       (double)HW * (double)(C / groups), eps, mean, rstd);
    XR_LAUNCH_CHECK();
    return XR_OK;
}

// ---------------------------------------------------------------- elementwise layers: one thread per float4 of the output
__global__ void __launch_bounds__(256) k_hg_gn_relu(const float* x, uint32_t ldx, uint64_t total, uint32_t HW, uint32_t C, uint32_t groups,
                                                    uint32_t cg_shift, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta, float* y, uint32_t ldy) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const uint32_t Q = C / 4, c = (uint32_t)(i % Q) * 4;
    const uint64_t p = i / Q;
    const uint32_t n = (uint32_t)(p / HW);
    const float4 v = *reinterpret_cast<const float4*>(x + p * ldx + c);
    const float in[4] = {v.x, v.y, v.z, v.w};
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t s = n * groups + ((c + e) >> cg_shift);
        const float a = rstd[s] * gamma[c + e];
        o[e] = fmaxf(fmaf(in[e], a, beta[c + e] - mean[s] * a), 0.f);
    }
    *reinterpret_cast<float4*>(y + p * ldy + c) = make_float4(o[0], o[1], o[2], o[3]);
}

extern "C" int xr_hg_gn_relu(const float* x, uint32_t ldx, uint32_t N, uint32_t HW, uint32_t C, uint32_t groups, const float* mean,
                             const float* rstd, const float* gamma, const float* beta, float* y, uint32_t ldy, void* stream) {
    if (N == 0 || HW == 0) return XR_OK;
    HG_SLICE(x, ldx, C);
    HG_SLICE(y, ldy, C);
    XR_REQUIRE(mean && rstd && gamma && beta, "null pointer");
    XR_REQUIRE(groups >= 1 && C % groups == 0 && hg_log2(C / groups) >= 0, "C / groups must be a power of two");
    const uint64_t total = (uint64_t)N * HW * (C / 4);
    XR_REQUIRE(total <= (1ull << 38), "too large");
    hipLaunchKernelGGL(k_hg_gn_relu, dim3(xr_div_up(total, 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, total, HW, C, groups,
                       (uint32_t)hg_log2(C / groups), mean, rstd, gamma, beta, y, ldy);
    XR_LAUNCH_CHECK();
    return XR_OK;
}

__global__ void __launch_bounds__(256) k_hg_avgpool2(const float* __restrict__ x, uint32_t ldx, uint64_t total, uint32_t H, uint32_t W, uint32_t C,
                                                     float* __restrict__ y, uint32_t ldy) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const uint32_t Q = C / 4, c = (uint32_t)(i % Q) * 4, Ho = H / 2, Wo = W / 2;
    const uint64_t p = i / Q;
    const uint32_t ox = (uint32_t)(p % Wo), oy = (uint32_t)((p / Wo) % Ho);
    const uint64_t n = p / ((uint64_t)Wo * Ho);
    const float* s = x + ((n * H + 2 * oy) * W + 2 * ox) * ldx + c;
    const float4 a = *reinterpret_cast<const float4*>(s), b = *reinterpret_cast<const float4*>(s + ldx);
    const float4 d = *reinterpret_cast<const float4*>(s + (size_t)W * ldx), e = *reinterpret_cast<const float4*>(s + (size_t)(W + 1) * ldx);
    *reinterpret_cast<float4*>(y + p * ldy + c) = make_float4((((a.x + b.x) + d.x) + e.x) * 0.25f, (((a.y + b.y) + d.y) + e.y) * 0.25f,
                                                              (((a.z + b.z) + d.z) + e.z) * 0.25f, (((a.w + b.w) + d.w) + e.w) * 0.25f);
}

extern "C" int xr_hg_avgpool2(const float* x, uint32_t ldx, uint32_t N, uint32_t H, uint32_t W, uint32_t C, float* y, uint32_t ldy, void* stream) {
    if (N == 0 || H < 2 || W < 2) return XR_OK;
    HG_SLICE(x, ldx, C);
    HG_SLICE(y, ldy, C);
    const uint64_t total = (uint64_t)N * (H / 2) * (W / 2) * (C / 4);
    XR_REQUIRE(total <= (1ull << 38), "too large");
    hipLaunchKernelGGL(k_hg_avgpool2, dim3(xr_div_up(total, 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, total, H, W, C, y, ldy);
    XR_LAUNCH_CHECK();
    return XR_OK;
}

// torch's bicubic coefficients (A = -0.75) for the fraction t
__device__ __forceinline__ void hg_cubic(float t, float (&w)[4]) {
    const float A = -0.75f;
    const float x0 = t + 1.f, x1 = t, x2 = 1.f - t, x3 = 2.f - t;
    w[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
    w[1] = ((A + 2.f) * x1 - (A + 3.f)) * x1 * x1 + 1.f;
    w[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
    w[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

__global__ void __launch_bounds__(256) k_hg_bicubic_up2(const float* __restrict__ x, uint32_t ldx, uint64_t total, uint32_t H, uint32_t W, uint32_t C,
                                                        const float* addend, uint32_t ldadd, float* y, uint32_t ldy) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const uint32_t Q = C / 4, c = (uint32_t)(i % Q) * 4, Ho = 2 * H, Wo = 2 * W;
    const uint64_t p = i / Q;
    const uint32_t ox = (uint32_t)(p % Wo), oy = (uint32_t)((p / Wo) % Ho);
    const uint64_t n = p / ((uint64_t)Wo * Ho);
    // align_corners: source = dst (in - 1) / (out - 1), the scale rounded to fp32 first like torch's
    const float sy = (float)(H - 1) / (float)(Ho - 1), sx = (float)(W - 1) / (float)(Wo - 1);
    const float fy = sy * (float)oy, fx = sx * (float)ox;
    const float flo_y = floorf(fy), flo_x = floorf(fx);
    float wy[4], wx[4];
    hg_cubic(fy - flo_y, wy);
    hg_cubic(fx - flo_x, wx);
    const int by = (int)flo_y - 1, bx = (int)flo_x - 1;
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int iy = min(max(by + a, 0), (int)H - 1);
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int ix = min(max(bx + b, 0), (int)W - 1);
            const float4 v = *reinterpret_cast<const float4*>(x + ((n * H + iy) * W + ix) * ldx + c);
            if (b == 0) { r.x = wx[0] * v.x; r.y = wx[0] * v.y; r.z = wx[0] * v.z; r.w = wx[0] * v.w; }
            else { r.x += wx[b] * v.x; r.y += wx[b] * v.y; r.z += wx[b] * v.z; r.w += wx[b] * v.w; }
        }
        if (a == 0) { out.x = wy[0] * r.x; out.y = wy[0] * r.y; out.z = wy[0] * r.z; out.w = wy[0] * r.w; }
        else { out.x += wy[a] * r.x; out.y += wy[a] * r.y; out.z += wy[a] * r.z; out.w += wy[a] * r.w; }
    }
    if (addend != nullptr) {
        const float4 u = *reinterpret_cast<const float4*>(addend + p * ldadd + c);
        out.x = u.x + out.x; out.y = u.y + out.y; out.z = u.z + out.z; out.w = u.w + out.w;
    }
    *reinterpret_cast<float4*>(y + p * ldy + c) = out;
}

extern "C" int xr_hg_bicubic_up2(const float* x, uint32_t ldx, uint32_t N, uint32_t H, uint32_t W, uint32_t C, const float* addend, uint32_t ldadd,
                                 float* y, uint32_t ldy, void* stream) {
    if (N == 0) return XR_OK;
    XR_REQUIRE(H >= 1 && W >= 1 && H <= (1u << 14) && W <= (1u << 14), "bad map size");
    HG_SLICE(x, ldx, C);
    HG_SLICE(y, ldy, C);
    if (addend != nullptr) HG_SLICE(addend, ldadd, C);
    const uint64_t total = (uint64_t)N * (2 * H) * (2 * W) * (C / 4);
    XR_REQUIRE(total <= (1ull << 38), "too large");
    hipLaunchKernelGGL(k_hg_bicubic_up2, dim3(xr_div_up(total, 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, total, H, W, C, addend, ldadd, y, ldy);
    XR_LAUNCH_CHECK();
    return XR_OK;
}

__global__ void __launch_bounds__(256) k_hg_add(const float* __restrict__ x, uint32_t ldx, uint64_t total, uint32_t C, float* __restrict__ y, uint32_t ldy) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const uint32_t Q = C / 4, c = (uint32_t)(i % Q) * 4;
    const uint64_t p = i / Q;
    const float4 a = *reinterpret_cast<const float4*>(x + p * ldx + c);
    float4* o = reinterpret_cast<float4*>(y + p * ldy + c);
    const float4 b = *o;
    *o = make_float4(b.x + a.x, b.y + a.y, b.z + a.z, b.w + a.w);
}

extern "C" int xr_hg_add(const float* x, uint32_t ldx, uint64_t rows, uint32_t C, float* y, uint32_t ldy, void* stream) {
    if (rows == 0) return XR_OK;
    HG_SLICE(x, ldx, C);
    HG_SLICE(y, ldy, C);
    const uint64_t total = rows * (C / 4);
    XR_REQUIRE(rows <= (1ull << 31) && total <= (1ull << 38), "too large");
    hipLaunchKernelGGL(k_hg_add, dim3(xr_div_up(total, 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, total, C, y, ldy);
    XR_LAUNCH_CHECK();
    return XR_OK;
}

// ---------------------------------------------------------------- one ConvBlock per call
// gnr_embedder.py:57-79 as the entry points above in sequence (ten launches, one call from the host): statistics of x -> conv1 into
// columns [0, Cout/2) -> statistics of those -> conv2 into [Cout/2, 3 Cout/4) -> statistics -> conv3 into the rest; then the residual,
// after conv2 and conv3 have read out1 and out2 as they were: the 1x1 downsample convolution adding to all columns (w_down given; bn4
// shares bn1's statistics, both normalise x), or out += x.
// workspace: the statistics' partial sums (reused by the three passes, in stream order), then three (mean, rstd) pairs of [N, groups]
extern "C" size_t xr_hg_conv_block_workspace_bytes(uint32_t N, uint32_t HW, uint32_t groups) {
    return (xr_hg_gn_stats_workspace_bytes(N, HW, groups) + 15) / 16 * 16 + 6 * (size_t)N * groups * sizeof(float);
}

extern "C" int xr_hg_conv_block(const float* x, uint32_t ldx, uint32_t N, uint32_t H, uint32_t W, uint32_t Cin, uint32_t Cout, const float* w1,
                                const float* w2, const float* w3, const float* w_down, const float* gamma1, const float* beta1, const float* gamma2,
                                const float* beta2, const float* gamma3, const float* beta3, const float* gamma4, const float* beta4, uint32_t groups,
                                float eps, float* y, uint32_t ldy, void* workspace, size_t workspace_bytes, void* stream) {
    if (N == 0) return XR_OK;
    XR_REQUIRE(x && y && w1 && w2 && w3 && gamma1 && beta1 && gamma2 && beta2 && gamma3 && beta3 && workspace, "null pointer");
    XR_REQUIRE(Cout % 16 == 0 && Cout >= 16 && ldy >= Cout, "Cout must be a multiple of 16 within the output's row stride");
    XR_REQUIRE(w_down ? (gamma4 && beta4) : Cin == Cout, "without a downsample convolution the residual is the input: Cin must equal Cout");
    XR_REQUIRE(((uintptr_t)workspace & 15) == 0, "the workspace must be 16-byte aligned");
    if (workspace_bytes < xr_hg_conv_block_workspace_bytes(N, H * W, groups)) { xr_set_error("%s: workspace too small", __func__); return XR_ENOMEM; }
    const size_t part = (xr_hg_gn_stats_workspace_bytes(N, H * W, groups) + 15) / 16 * 16, ng = (size_t)N * groups;
    float* st = reinterpret_cast<float*>(static_cast<char*>(workspace) + part);
    const uint32_t a = Cout / 2, b = Cout / 4, HW = H * W;
    int rc;
#define HG_STEP(call) do { rc = (call); if (rc != XR_OK) return rc; } while (0)
    HG_STEP(xr_hg_gn_stats(x, ldx, N, HW, Cin, groups, eps, st, st + ng, workspace, part, stream));
    HG_STEP(xr_hg_conv2d(x, ldx, N, H, W, Cin, w1, a, 3, 1, st, st + ng, gamma1, beta1, groups, nullptr, 0, 0, y, ldy, stream));
    HG_STEP(xr_hg_gn_stats(y, ldy, N, HW, a, groups, eps, st + 2 * ng, st + 3 * ng, workspace, part, stream));
    HG_STEP(xr_hg_conv2d(y, ldy, N, H, W, a, w2, b, 3, 1, st + 2 * ng, st + 3 * ng, gamma2, beta2, groups, nullptr, 0, 0, y + a, ldy, stream));
    HG_STEP(xr_hg_gn_stats(y + a, ldy, N, HW, b, groups, eps, st + 4 * ng, st + 5 * ng, workspace, part, stream));
    HG_STEP(xr_hg_conv2d(y + a, ldy, N, H, W, b, w3, b, 3, 1, st + 4 * ng, st + 5 * ng, gamma3, beta3, groups, nullptr, 0, 0, y + a + b, ldy, stream));
    if (w_down) HG_STEP(xr_hg_conv2d(x, ldx, N, H, W, Cin, w_down, Cout, 1, 1, st, st + ng, gamma4, beta4, groups, nullptr, 0, 1, y, ldy, stream));
    else HG_STEP(xr_hg_add(x, ldx, (uint64_t)N * HW, Cout, y, ldy, stream));
#undef HG_STEP
    return XR_OK;
}
