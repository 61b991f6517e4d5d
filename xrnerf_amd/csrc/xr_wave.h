// wave64 collectives of the wave-per-ray kernels (xr_mip.hip, xr_bungee.hip, xr_vanilla.hip, xr_kilo.hip): the ONE copy of the few lines
// the renderers' determinism rests on.  Every scan is a Hillis-Steele sweep over the offsets 1, 2, 4, .. 32 and every sum a butterfly over
// 32, 16, .. 1, so the order of the additions / products is fixed by the lane number alone: the same input gives the same bits on every
// launch.  The fp64 scans restate torch's CPU cumsum / cumprod of fp32 values, which accumulate in double.
// All lanes of the wave must call these together (the shuffles read every lane).  static: each translation unit inlines its own copy.
#pragma once
#include <hip/hip_runtime.h>

// inclusive prefix product over the wave's 64 lanes
static __device__ inline double xr_wave_incl_prod(double v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        double o = __shfl_up(v, off, 64);
        if (lane >= off) v *= o;
    }
    return v;
}
// exclusive prefix of an inclusive product scan, without dividing (a factor can be 1e-10): the value of the lane below (1 for lane 0)
static __device__ inline double xr_wave_excl_of_prod(double incl) {
    const double o = __shfl_up(incl, 1, 64);
    return (threadIdx.x & 63) ? o : 1.0;
}
// inclusive prefix sum over the wave's 64 lanes
static __device__ inline double xr_wave_incl_sum(double v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        double o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}
// sum over the wave's 64 lanes, the same value in every lane
static __device__ inline double xr_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
static __device__ inline float xr_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
