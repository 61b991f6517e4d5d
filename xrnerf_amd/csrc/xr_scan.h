// Stream compaction -- count, exclusive scan, ranked write -- for workgroups of 256 threads (four wave64): the ONE copy of the
// workgroup-level scans under xr_neuralbody.hip, xr_aninerf.hip, xr_gnr_render.hip and xr_gnr_recon.hip.  Built on xr_wave.h: a wave's
// prefix has a fixed order, the four wave sums pass through LDS and are added in wave order, so counts, bases and ranks are the same
// integers on every launch.
// (xr_raymarch.hip's block_excl_scan / k_scan_blocks, with its crossing limit, and xr_scatter.hip's LDS accumulators stay where they
// are: they sit on the path bench.py times and were tuned against measurements.)
#pragma once
#include "xr_common.h"
#include "xr_wave.h"

#define XR_SCAN_BLOCK 256
#define XR_SCAN_WAVES (XR_SCAN_BLOCK / 64)

// exclusive prefix of c over the workgroup's threads and the workgroup's sum; EVERY thread of the workgroup calls it
static __device__ inline uint32_t xr_block_excl(uint32_t c, uint32_t* sum) {
    __shared__ uint32_t s_w[XR_SCAN_WAVES];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t incl = xr_wave_incl_sum(c);
    __syncthreads();                                               // s_w of an earlier call has been read
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < XR_SCAN_WAVES; ++w) { if (w < wave) before += s_w[w]; all += s_w[w]; }
    *sum = (uint32_t)__builtin_amdgcn_readfirstlane((int)all);       // (the same in every thread: callers keep it in a scalar register)
    return before + incl - c;
}

// the same for one flag per thread (its rank among the set flags): one ballot and two popcounts, no shuffles
static __device__ inline uint32_t xr_block_excl_flag(bool f, uint32_t* sum) {
    __shared__ uint32_t s_w[XR_SCAN_WAVES];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(f);
    __syncthreads();                                               // s_w of an earlier call has been read
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < XR_SCAN_WAVES; ++w) { if (w < wave) before += s_w[w]; all += s_w[w]; }
    *sum = (uint32_t)__builtin_amdgcn_readfirstlane((int)all);       // (the same in every thread: callers keep it in a scalar register)
    return before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// ONE workgroup: the exclusive scan of n counts, 256 per sweep.  load(b) yields count b, store(b, base) receives its exclusive base
// (modulo 2^32); returns the total.  The total is carried in 64 bits, so that a sum beyond int32 is seen (xr_scan_total)
template <class Load, class Store> static __device__ inline uint64_t xr_scan_sweeps(uint32_t n, Load load, Store store) {
    uint64_t carry = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += XR_SCAN_BLOCK) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t c = b < n ? load(b) : 0u;
        uint32_t sum;
        const uint32_t ex = xr_block_excl(c, &sum);
        if (b < n) store(b, (uint32_t)carry + ex);
        carry += sum;
    }
    return carry;
}
// what a scan reports as its total: one that does not fit int32 is -1 (the bases are then meaningless and the caller must not use them)
static __device__ inline int32_t xr_scan_total(uint64_t total) { return total > 0x7fffffffull ? -1 : (int32_t)total; }

// ---- the scan of n counts in two levels, in place: every workgroup scans its 256 counts and leaves their sum, one workgroup scans the
// sums (n / 256 of them: 2059 at 513^3 grid points), every workgroup adds its base.  sums: xr_div_up(n, 256) words of workspace.
// (A kernel is emitted into every translation unit that sees it: the source that calls xr_scan_two_level defines XR_SCAN_TWO_LEVEL
// before it includes this header.)
#ifdef XR_SCAN_TWO_LEVEL
static __global__ void __launch_bounds__(XR_SCAN_BLOCK) k_xr_scan_part(uint32_t n, uint32_t* __restrict__ counts,
                                                                                      uint32_t* __restrict__ sums) {
    const uint32_t b = blockIdx.x * XR_SCAN_BLOCK + threadIdx.x;
    uint32_t sum;
    const uint32_t ex = xr_block_excl(b < n ? counts[b] : 0u, &sum);
    if (b < n) counts[b] = ex;
    if (threadIdx.x == 0) sums[blockIdx.x] = sum;
}

static __global__ void __launch_bounds__(XR_SCAN_BLOCK) k_xr_scan_sums(uint32_t n, uint32_t* __restrict__ counts,
                                                                                      int32_t* __restrict__ total) {
    const uint64_t sum = xr_scan_sweeps(n, [&](uint32_t b) { return counts[b]; }, [&](uint32_t b, uint32_t base) { counts[b] = base; });
    if (threadIdx.x == 0) total[0] = xr_scan_total(sum);
}

static __global__ void __launch_bounds__(XR_SCAN_BLOCK) k_xr_scan_add(uint32_t n, uint32_t* __restrict__ counts,
                                                                                     const uint32_t* __restrict__ sums) {
    const uint32_t b = blockIdx.x * XR_SCAN_BLOCK + threadIdx.x;
    if (b < n) counts[b] += sums[blockIdx.x];
}

static void xr_scan_two_level(hipStream_t st, uint32_t n, uint32_t* counts, uint32_t* sums, int32_t* total) {
    const uint32_t n2 = xr_div_up(n, XR_SCAN_BLOCK);
    hipLaunchKernelGGL(k_xr_scan_part, dim3(n2), dim3(XR_SCAN_BLOCK), 0, st, n, counts, sums);
    hipLaunchKernelGGL(k_xr_scan_sums, dim3(1), dim3(XR_SCAN_BLOCK), 0, st, n2, sums, total);
    hipLaunchKernelGGL(k_xr_scan_add, dim3(n2), dim3(XR_SCAN_BLOCK), 0, st, n, counts, (const uint32_t*)sums);
}
#endif
