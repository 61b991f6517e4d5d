// The optimiser step for any number of tensors and the device-side log window (include/xrnerf_mi355_optim.h): what a
// training runner does once per iteration besides the family's own step.
//   k_adam_list        xr_adam_step_multi's update over a work list of up to XR_ADAM_LIST_CAPACITY tensors passed BY VALUE in the kernel
//                      arguments (gradient pointers change whenever zero_grad(set_to_none=True) ran: a by-value table needs no upload and
//                      no synchronisation).  The unit of work is a segment -- XR_ADAM_LIST_SEGMENT floats of one tensor -- and a workgroup
//                      walks XR_ADAM_LIST_SEGMENTS_PER_GROUP consecutive segments: the ~50 tensors of a NerfNetwork (mostly 256-float
//                      biases) share workgroups, a hash table spreads over thousands.  The tensor of a segment is found by a binary search
//                      over the prefix of segment counts; the segment index depends on blockIdx and the loop counter alone, so the search
//                      and everything it selects (pointers, length) is wave-uniform and stays in scalar registers.
//   k_log_window_add   one iteration's log scalars times num_samples, added into double sums on the device: the text logger reads the
//                      window once per interval instead of three scalars per iteration.
// The per-element arithmetic is adam1 / ema1 of xr_adam.h and this file is compiled without fused multiply-adds like xr_misc.hip, so a tensor
// updated here is bit for bit what k_adam_multi makes of it; g, m, v and ema go through the same non-temporal accesses.
#include "xr_common.h"
#include "xr_adam.h"
#include "../../include/xrnerf_mi355_optim.h"

#define AL_CAP XR_ADAM_LIST_CAPACITY
#define AL_SEG XR_ADAM_LIST_SEGMENT
#define AL_PER_GROUP XR_ADAM_LIST_SEGMENTS_PER_GROUP
#define AL_BLOCK (AL_SEG / 4u)

// first[k] = segments of the tensors before k (first[nt] = all of them); bit k of `narrow`: tensor k is not 16-byte aligned
struct AdamList {
    float* p[AL_CAP]; const float* g[AL_CAP]; float* m[AL_CAP]; float* v[AL_CAP]; float* ema[AL_CAP];
    uint32_t n[AL_CAP]; uint32_t first[AL_CAP + 1]; uint32_t narrow[AL_CAP / 32];
};
static_assert(sizeof(AdamList) + 64 <= 4096, "the work list and the constants must fit HIP's 4-KiB kernel-argument block");

static __device__ __forceinline__ void al_one(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                              float* __restrict__ ema, size_t i, float b1, float b2, float step_size, float bc2s, float eps,
                                              float wd, float mom, float gs) {
    float pp = p[i], mm = m[i], vv = v[i];
    adam1(pp, g[i], mm, vv, b1, b2, step_size, bc2s, eps, wd, gs);
    p[i] = pp; m[i] = mm; v[i] = vv;
    if (ema) ema[i] = ema1(ema[i], pp, mom);
}

template <bool NT>
static __global__ __launch_bounds__(AL_BLOCK) void k_adam_list(AdamList t, int nt, float b1, float b2, float step_size, float bc2s, float eps,
                                                               float wd, float mom, float gs) {
    const uint32_t total = t.first[nt];
    for (uint32_t j = 0; j < AL_PER_GROUP; ++j) {
        const uint32_t s = blockIdx.x * AL_PER_GROUP + j;
        if (s >= total) break;
        int lo = 0, hi = nt;                                   // first[lo] <= s < first[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (t.first[mid] <= s) lo = mid; else hi = mid;
        }
        const int k = lo;
        float* __restrict__ p = t.p[k]; const float* __restrict__ g = t.g[k];
        float* __restrict__ m = t.m[k]; float* __restrict__ v = t.v[k]; float* __restrict__ ema = t.ema[k];
        const size_t n = t.n[k], off = (size_t)(s - t.first[k]) * AL_SEG;
        if ((t.narrow[k >> 5] >> (k & 31)) & 1u) {
            // 4-byte accesses, a wave on consecutive floats
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const size_t i = off + q * AL_BLOCK + threadIdx.x;
                if (i < n) al_one(p, g, m, v, ema, i, b1, b2, step_size, bc2s, eps, wd, mom, gs);
            }
            continue;
        }
        const size_t e = off + threadIdx.x * 4u;
        if (e + 4 <= n) {
            const size_t i = e / 4;
            float4 pp = ((float4*)p)[i], mm = am_ld<NT>(m, i), vv = am_ld<NT>(v, i);
            const float4 gg = am_ld<NT>(g, i);
            adam1(pp.x, gg.x, mm.x, vv.x, b1, b2, step_size, bc2s, eps, wd, gs);
            adam1(pp.y, gg.y, mm.y, vv.y, b1, b2, step_size, bc2s, eps, wd, gs);
            adam1(pp.z, gg.z, mm.z, vv.z, b1, b2, step_size, bc2s, eps, wd, gs);
            adam1(pp.w, gg.w, mm.w, vv.w, b1, b2, step_size, bc2s, eps, wd, gs);
            ((float4*)p)[i] = pp; am_st<NT>(m, i, mm); am_st<NT>(v, i, vv);
            if (ema) {
                float4 ee = am_ld<NT>(ema, i);
                ee.x = ema1(ee.x, pp.x, mom); ee.y = ema1(ee.y, pp.y, mom); ee.z = ema1(ee.z, pp.z, mom); ee.w = ema1(ee.w, pp.w, mom);
                am_st<NT>(ema, i, ee);
            }
        } else {
            // the tensor's last 1 .. 3 floats (e < n holds for one thread of its last segment at the most)
            for (size_t i = e; i < n; ++i) al_one(p, g, m, v, ema, i, b1, b2, step_size, bc2s, eps, wd, mom, gs);
        }
    }
}

extern "C" int xr_adam_list_capacity(void) { return (int)AL_CAP; }

extern "C" int xr_adam_step_list(int n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v, float* const* ema,
                                 const size_t* n, int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                                 float ema_momentum, float grad_scale, void* stream_) {
    XR_REQUIRE(n_tensors >= 1 && p && g && m && v && n && step >= 1, "bad argument");
    for (int k = 0; k < n_tensors; ++k) {
        XR_REQUIRE(p[k] && g[k] && m[k] && v[k], "null tensor");
        XR_REQUIRE(n[k] > 0 && n[k] <= 0xffffffffull, "a tensor holds 1 .. 2^32 - 1 floats");
        XR_REQUIRE((((uintptr_t)p[k] | (uintptr_t)g[k] | (uintptr_t)m[k] | (uintptr_t)v[k] | (uintptr_t)(ema ? ema[k] : nullptr)) & 3) == 0,
                   "buffers must be 4-byte aligned");
    }
    const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
#ifndef XR_ADAM_NT
#define XR_ADAM_NT 1
#endif
    for (int base = 0; base < n_tensors; base += (int)AL_CAP) {
        const int nt = min(n_tensors - base, (int)AL_CAP);
        AdamList t; memset(&t, 0, sizeof(t));
        uint64_t segments = 0;
        for (int k = 0; k < nt; ++k) {
            const int s = base + k;
            float* const e = ema ? ema[s] : nullptr;
            t.p[k] = p[s]; t.g[k] = g[s]; t.m[k] = m[s]; t.v[k] = v[s]; t.ema[k] = e; t.n[k] = (uint32_t)n[s];
            if (((uintptr_t)p[s] | (uintptr_t)g[s] | (uintptr_t)m[s] | (uintptr_t)v[s] | (uintptr_t)e) & 15) t.narrow[k >> 5] |= 1u << (k & 31);
            t.first[k] = (uint32_t)segments;
            segments += xr_div_up(n[s], AL_SEG);
        }
        XR_REQUIRE(segments <= 0xffffffffull, "too many segments for one launch");
        for (int k = nt; k <= (int)AL_CAP; ++k) t.first[k] = (uint32_t)segments;
        hipLaunchKernelGGL(k_adam_list<XR_ADAM_NT != 0>, dim3(xr_div_up(segments, AL_PER_GROUP)), dim3(AL_BLOCK), 0, (hipStream_t)stream_, t, nt,
                           beta1, beta2, lr / bc1, sqrtf(bc2), eps, weight_decay, ema_momentum, grad_scale);
        XR_LAUNCH_CHECK();
    }
    return XR_OK;
}

// ------------------------------------------------------------------ the log window
struct LogValues { const float* v[XR_LOG_WINDOW_SLOTS]; };
static __global__ __launch_bounds__(XR_WAVE) void k_log_window_add(LogValues a, int nv, uint32_t num_samples, double* __restrict__ window) {
    const int i = threadIdx.x;
    if (i < nv) {
        const double ns = (double)num_samples;
        window[i] += (double)*a.v[i] * ns;                     // exact product: 24 + 29 bits
        window[XR_LOG_WINDOW_SLOTS + i] += ns;
    }
}

extern "C" int xr_log_window_add(int n_values, const float* const* values, uint32_t num_samples, double* window, void* stream_) {
    XR_REQUIRE(n_values >= 1 && n_values <= (int)XR_LOG_WINDOW_SLOTS && values && window, "bad argument");
    XR_REQUIRE(num_samples >= 1 && num_samples < (1u << 29), "num_samples is 1 .. 2^29 - 1");
    LogValues a; memset(&a, 0, sizeof(a));
    for (int i = 0; i < n_values; ++i) {
        XR_REQUIRE(values[i] && ((uintptr_t)values[i] & 3) == 0, "null or misaligned value");
        a.v[i] = values[i];
    }
    XR_REQUIRE(((uintptr_t)window & 7) == 0, "window must be 8-byte aligned");
    hipLaunchKernelGGL(k_log_window_add, dim3(1), dim3(XR_WAVE), 0, (hipStream_t)stream_, a, n_values, num_samples, window);
    XR_LAUNCH_CHECK();
    return XR_OK;
}
