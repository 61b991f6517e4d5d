// wave64 collectives of the wave-per-ray kernels (xr_render.h, xr_mip.hip, xr_bungee.hip, xr_vanilla.hip, xr_kilo.hip,
// xr_gnr_render.hip) and of the workgroup scans of the count / scan / rank kernels (xr_scan.h, under xr_neuralbody.hip, xr_aninerf.hip,
// xr_gnr_render.hip and xr_gnr_recon.hip): the ONE copy of the few lines the renderers' determinism rests on.  Every scan is a Hillis-Steele sweep over the offsets 1, 2, 4, .. 32 and every sum a butterfly over
// 32, 16, .. 1, so the order of the additions / products is fixed by the lane number alone: the same input gives the same bits on every
// launch.  Each computes in the type of its argument: double restates torch's CPU cumsum / cumprod of fp32 values, which accumulate in
// double; float is GNR's compositor; uint32_t the counts of the scan kernels.
// All lanes of the wave must call these together (the shuffles read every lane).  static: each translation unit inlines its own copy.
#pragma once
#include <hip/hip_runtime.h>

// inclusive prefix product over the wave's 64 lanes
template <class T> static __device__ inline T xr_wave_incl_prod(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        T o = __shfl_up(v, off, 64);
        if (lane >= off) v *= o;
    }
    return v;
}
// exclusive prefix of an inclusive product scan, without dividing (a factor can be 1e-10): the value of the lane below (1 for lane 0)
template <class T> static __device__ inline T xr_wave_excl_of_prod(T incl) {
    const T o = __shfl_up(incl, 1, 64);
    return (threadIdx.x & 63) ? o : (T)1;
}
// inclusive prefix sum over the wave's 64 lanes
template <class T> static __device__ inline T xr_wave_incl_sum(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        T o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}
// sum over the wave's 64 lanes, the same value in every lane
template <class T> static __device__ inline T xr_wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// reverse inclusive scan of the affine maps x -> A + F x: (F, A) of lane k becomes the composition of the maps of the lanes k .. 63,
// lane k's applied last.  No division, so a factor may be 0 or 1e-10
template <class T> struct XrAffine { T F, A; };
template <class T> static __device__ inline XrAffine<T> xr_wave_affine_rscan(T F, T A) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T Fo = __shfl_down(F, off, 64), Ao = __shfl_down(A, off, 64);
        if (lane + off < 64) { A = A + F * Ao; F = F * Fo; }
    }
    return {F, A};
}
