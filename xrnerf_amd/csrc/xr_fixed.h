// Order-independent scatter in 64-bit fixed point: the ONE copy of the accumulator under NeuralBody's sampling backward
// (xr_neuralbody.hip) and GNR's gather backward (xr_gnr_render.hip).  The largest |gradient| gives a power-of-two scale, every
// contribution w g is rounded once to a multiple of 1 / scale and added as an integer (integer adds commute: the same bits on every
// launch), a last kernel converts the sums back to float.  Four launches around the family's own walk:
//   absmax (the family's)   reads the gradient in the family's layout; xr_fix_block_max leaves one maximum per workgroup
//   k_xr_fix_scale          ONE workgroup folds the maxima into the scale
//   scatter (the family's)  xr_fix_add per (destination, weight, gradient element)
//   convert (the family's)  xr_fix_to_float per accumulator
// The absmax loops differ in more than layout, and that is behaviour: GNR leaves an entry above 3.0e38f (an infinity, a NaN) out of the
// maximum, so finite entries keep the scale they would have had alone; NeuralBody lets an infinity through and k_xr_fix_scale clamps
// it, so the scale becomes the smallest there is.  Either way xr_fix_add drops the non-finite products.  Do not unify the two.
#pragma once
#include "xr_common.h"

#define XR_FIX_BLOCK 256
// workspace: block maxima [XR_FIX_MAX_BMAX] floats | the scale (one double) | the 64-bit accumulators
#define XR_FIX_MAX_BMAX 1024u
#define XR_FIX_HEAD (XR_FIX_MAX_BMAX * sizeof(float) + sizeof(double))
struct XrFixWs { float* bmax; double* scale; unsigned long long* acc; };
static inline XrFixWs xr_fix_ws(void* ws) {
    return {(float*)ws, (double*)((char*)ws + XR_FIX_MAX_BMAX * sizeof(float)), (unsigned long long*)((char*)ws + XR_FIX_HEAD)};
}

// the maximum of m over the workgroup's 256 threads, valid in thread 0; EVERY thread of the workgroup calls it, once per kernel
static __device__ inline float xr_fix_block_fold(float m) {
    __shared__ float s_m[XR_FIX_BLOCK];
    s_m[threadIdx.x] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < XR_FIX_BLOCK; ++k) m = fmaxf(m, s_m[k]);
    return m;
}
static __device__ inline void xr_fix_block_max(float m, float* __restrict__ bmax) {
    m = xr_fix_block_fold(m);
    if (threadIdx.x == 0) bmax[blockIdx.x] = m;
}

// 2^(61 - b - e) with max |grad| < 2^e and n <= 2^b, n a bound on the contributions one accumulator receives, each |w g| <= |g|: the sum
// stays below 2^61 in magnitude.  A maximum that is not below 3.0e38f (an infinity) counts as 3.0e38f
static __global__ void __launch_bounds__(XR_FIX_BLOCK) k_xr_fix_scale(const float* __restrict__ bmax, uint32_t n_bmax, uint32_t n,
                                                                      double* __restrict__ scale) {
    float m = 0.f;
    for (uint32_t e = threadIdx.x; e < n_bmax; e += XR_FIX_BLOCK) m = fmaxf(m, bmax[e]);
    m = xr_fix_block_fold(m);
    if (threadIdx.x == 0) {
        if (!(m < 3.0e38f)) m = 3.0e38f;
        int ex = 0, b = 0;
        if (m > 0.f) frexpf(m, &ex);
        while (b < 31 && (1u << b) < n) ++b;
        scale[0] = ldexp(1.0, 61 - b - ex);
    }
}

// *d += round(w g scale).  A NaN or an infinite gradient contributes nothing: |v| < 2^61 for every finite one, and llrint is undefined
// beyond 2^63
static __device__ inline void xr_fix_add(unsigned long long* d, double w, float g, double scale) {
    const double v = (w * (double)g) * scale;
    if (v != 0.0 && fabs(v) < 4.0e18) atomicAdd(d, (unsigned long long)(long long)llrint(v));
}
static __device__ inline float xr_fix_to_float(unsigned long long acc, double scale) { return (float)((double)(long long)acc / scale); }
