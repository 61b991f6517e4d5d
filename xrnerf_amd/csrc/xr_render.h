// The wave-per-ray volume renderers, once: wave = ray, lane = sample, 64 samples per sweep.  A sweep loads one sample per lane, scans
// the transmittance across the wave and carries it into the next sweep, accumulates weight, depth and colour per lane; butterflies fold
// them at the end and lane 0 writes the ray.  What differs between the renderers is a policy struct in their own source:
//   xr_vanilla.hip  VnRender      cumprod transmittance, sample positions, sigmoid colours, disparity
//   xr_bungee.hip   BungeeRender  cumprod transmittance, interval midpoints, summed heads, padded colours, disparity
//   xr_mip.hip      MipRender     cumsum transmittance, interval midpoints, padded colours, clamped distance
// A policy has: the argument struct `a` (with n_rays, n_s, white_bkgd), `Sample`, `Step` (one of the two steppers below), and
//   ray(r)                     per-ray state (the direction's norm)
//   load(r, i)                 sample i of ray r
//   step_in(s)                 what the stepper scans (the factor 1 - alpha + 1e-10, or density_delta)
//   weight(s, t)               w from the sample and the stepper's output
//   colours(s, c) / depth(s)   the three colours and the depth coordinate that w multiplies
//   ray_scalar(r, depth, acc)  the second output of the ray (disparity or distance)
// k_mip_render_bwd and k_bungee_render_bwd are one two-pass algorithm (total = sum w gc, then suffix = total - prefix) and share its
// pass body, xr_render_term, which both passes of both kernels call.  The kernels themselves stay apart: with the last block (the
// density gradient from (T, gc, suffix) and the store) handed in as a policy function or a lambda, the compiler schedules
// k_mip_render_bwd into 66 VGPRs instead of 62 and it drops from 8 to 7 waves per SIMD; written in the kernel it keeps its registers.
// k_nerf_render (xr_kilo.hip) takes only the stepper: its span bounds, the ballot that skips sweeps without density, the nullable
// weights, the net_of rows and the lattice positions would each be a branch of this sweep, and it sits in the frame that bench.py times.
// k_gr_comp_fwd / _bwd (xr_gnr_render.hip) keep their loops as well (survivor lists, eight sums, a stored fp32 transmittance).
// Two backward algorithms exist on purpose: the two-pass one restates autograd (Bungee's with autograd's division by the factor),
// k_nerf_render_bwd (xr_vanilla.hip) is the division-free reverse scan.  They compute the same gradient by different arithmetic and
// each test's bar was set against its own, so they stay two.
// Device code only, and only for sources compiled with -ffp-contract=off: every expression is fp32 in the reference's operation order.
#pragma once
#include "xr_wave.h"

// ------------------------------------------------------------------------------------------ transmittance steppers
// "scan this sweep, combine with the carry of the sweeps before, advance the carry" in one call.  All lanes call together; a lane
// without a sample passes `identity`.  The scans and the carry are fp64 (torch's CPU cumprod / cumsum of fp32), the result is rounded
// to fp32 like torch's output.
struct XrCumprodStep {                           // prod_{j < i} f_j
    static constexpr double identity = 1.0;
    double carry = 1.0;
    __device__ inline double step64(double f) {
        const double incl = xr_wave_incl_prod(f);
        const double t = carry * xr_wave_excl_of_prod(incl);
        carry *= __shfl(incl, 63, 64);
        return t;
    }
    __device__ inline float step(double f) { return (float)step64(f); }
};
struct XrCumsumStep {                            // sum_{j < i} v_j
    static constexpr double identity = 0.0;
    double carry = 0.0;
    __device__ inline float step(double v) {
        const double incl = xr_wave_incl_sum(v);
        const float before = (float)(carry + (incl - v));
        carry += __shfl(incl, 63, 64);
        return before;
    }
};

// 1 / max(1e-10, depth / acc): torch.max propagates the NaN of 0 / 0
static __device__ inline float xr_render_disp(float depth, float acc) {
    const float q = depth / acc;
    return 1.f / (q != q ? q : fmaxf(1e-10f, q));
}

// ------------------------------------------------------------------------------------------ forward
template <class P>
static __device__ inline void xr_render_fwd(P p, uint32_t r, float* __restrict__ rgb_out, float* __restrict__ scalar_out,
                                            float* __restrict__ acc_out, float* __restrict__ weights_out) {
    const uint32_t lane = threadIdx.x & 63, n_s = p.a.n_s;
    if (r >= p.a.n_rays) return;               // whole waves leave together
    p.ray(r);
    typename P::Step st;
    float a_c[3] = {0.f, 0.f, 0.f}, a_w = 0.f, a_z = 0.f;
    for (uint32_t base = 0; base < n_s; base += 64) {
        const uint32_t i = base + lane;
        const bool live = i < n_s;
        typename P::Sample s;
        double x = P::Step::identity;
        if (live) { s = p.load(r, i); x = p.step_in(s); }
        const float t = st.step(x);            // all lanes take part in the shuffles
        if (live) {
            const float w = p.weight(s, t);
            float c[3];
            p.colours(s, c);
            weights_out[(uint64_t)r * n_s + i] = w;
            a_w += w;
            a_z += w * p.depth(s);
            for (int k = 0; k < 3; ++k) a_c[k] += w * c[k];
        }
    }
    const float acc = xr_wave_sum(a_w), depth = xr_wave_sum(a_z);
    float col[3];
    for (int k = 0; k < 3; ++k) col[k] = xr_wave_sum(a_c[k]);
    if (lane == 0) {
        scalar_out[r] = p.ray_scalar(r, depth, acc);
        acc_out[r] = acc;
        for (int k = 0; k < 3; ++k) rgb_out[r * 3ull + k] = p.a.white_bkgd ? col[k] + (1.f - acc) : col[k];
    }
}

// ------------------------------------------------------------------------------------------ two-pass backward: the pass body
// dL/draw given dL/drgb.  With gc_i = sum_ch g_ch (rgb_i,ch - [white]) and w_i the forward's weight, pass 1 computes
// total = sum_i w_i gc_i and pass 2 gives every sample suffix = sum_{i > k} w_i gc_i = total - inclusive prefix (both in fp64).
template <class P> struct XrRenderTerm { typename P::Sample s; float t, w, gc; double wg; };

// sample i of both passes: the stepper's output t, w, gc and wg = w gc (0 for a lane without a sample).  All lanes call together.
template <class P>
static __device__ inline XrRenderTerm<P> xr_render_term(const P& p, typename P::Step& st, uint32_t r, uint32_t i, const float* g,
                                                        float white) {
    XrRenderTerm<P> q;
    const bool live = i < p.a.n_s;
    double x = P::Step::identity;
    q.w = 0.f; q.gc = 0.f; q.wg = 0.0;
    if (live) { q.s = p.load(r, i); x = p.step_in(q.s); }
    q.t = st.step(x);
    if (live) {
        q.w = p.weight(q.s, q.t);
        float c[3];
        p.colours(q.s, c);
        for (int k = 0; k < 3; ++k) q.gc += g[k] * (c[k] - white);
        q.wg = (double)q.w * (double)q.gc;
    }
    return q;
}
