// Vanilla NeRF (configs/nerf/nerf_blender_base01.py) training stages for gfx950: what stands around the 8 x 256 MLP in a step.
// The reference runs each as a chain of small PyTorch launches (models/embedders/base.py BaseEmbedder, models/renders/nerf_render.py
// NerfRender, models/networks/utils/hierarchical_sample.py sample_pdf); here each is ONE launch:
//   k_nerf_encode        workgroup = 64 consecutive rows.  The lanes sweep (row, frequency, axis) items -- one exact scaling, one sinf and
//                        one cosf each -- into an LDS tile; the direction features are computed once per direction of the tile; the tile
//                        (padding columns as zeros) then leaves as one contiguous, coalesced block of ld floats per row
//   k_nerf_render_fwd    wave = ray, 64 samples per sweep: the forward sweep of xr_render.h with the policy VnRender; transmittance as an
//                        fp64 prefix PRODUCT of (1 - alpha + 1e-10) (the arithmetic of the inference kernel k_nerf_render, xr_kilo.hip)
//   k_nerf_render_bwd    wave = ray; dL/draw from dL/drgb without a division: with G_k = sum_c g_c rgb_kc - [white] sum_c g_c and the
//                        reverse recurrence S_{k-1} = alpha_k G_k + f_k S_k (S_last = 0, f = 1 - alpha + 1e-10),
//                        dL/dalpha_k = T_k (G_k - S_k).  The recurrence is an affine map per sample; the wave composes them with a reverse
//                        Hillis-Steele scan in fp64, sweeps taken from the last to the first (kept apart from the two-pass backward of
//                        xr_mip.hip / xr_bungee.hip: xr_render.h says why)
//   k_nerf_sample_pdf    wave = ray; cdf over the bin midpoints (fp64 scan) in LDS, one binary search per draw, then a bitonic sort of
//                        [z_vals | z_samples] in LDS and pts = o + d z
// No atomics anywhere, every reduction / scan has a fixed order: the same input gives the same bits on every launch.
// Compiled with -ffp-contract=off: every expression is fp32 in the reference's operation order.
#include "xr_common.h"
#include "xr_mip_math.h"
#include "xr_render.h"
#include "../../include/xrnerf_mi355_vanilla.h"

#define VN_BLOCK 256
#define VN_WAVES (VN_BLOCK / 64)
#define VN_TILE 64
#define VN_MAX_FREQS 16                    /* multires, multires_dirs <= 16: at most 99 columns per part */
#define VN_MAX_S 4096u                     /* renderer: at most 64 sweeps (one carry per lane in the backward) */
#define VN_PDF_MAX 1024u                   /* sample_pdf: S and N each */

// ------------------------------------------------------------------------------------------ BaseEmbedder.forward
struct VnEncArgs {
    const float* pts; const float* dirs;
    uint64_t n_rows; uint32_t rows_per_dir;
    int L, Ld;
    float* out; uint32_t ld;
};

__global__ void __launch_bounds__(VN_BLOCK) k_nerf_encode(VnEncArgs a) {
    extern __shared__ float vn_tile[];                     // [VN_TILE][cp] point features, then [VN_TILE][cd] direction features
    const uint32_t cp = 3u + 6u * (uint32_t)a.L, cd = 3u + 6u * (uint32_t)a.Ld, ch = cp + cd;
    float* s_dir = vn_tile + (size_t)VN_TILE * cp;         // one row per direction of the tile
    const uint64_t g0 = (uint64_t)blockIdx.x * VN_TILE;
    const uint32_t tile = (uint32_t)(a.n_rows - g0 < VN_TILE ? a.n_rows - g0 : VN_TILE);
    const uint64_t d0 = g0 / a.rows_per_dir;
    const uint32_t n_dirs = (uint32_t)((g0 + tile - 1) / a.rows_per_dir - d0) + 1;      // <= tile
    // item q of a row / direction: identity column q (q < 3), else (l, axis) = ((q-3)/3, (q-3)%3) -> columns 3+6l+axis (sin), 6+6l+axis (cos)
    const uint32_t per = 3u + 3u * (uint32_t)a.L;
    for (uint32_t e = threadIdx.x; e < tile * per; e += VN_BLOCK) {
        const uint32_t sl = e / per, q = e - sl * per;
        float* row = vn_tile + (size_t)sl * cp;
        if (q < 3) { row[q] = a.pts[(g0 + sl) * 3 + q]; continue; }
        const uint32_t l = (q - 3) / 3u, ax = (q - 3) % 3u;
        const float y = ldexpf(a.pts[(g0 + sl) * 3 + ax], (int)l);          // p * 2^l: exact
        row[3 + 6 * l + ax] = sinf(y);
        row[6 + 6 * l + ax] = cosf(y);
    }
    const uint32_t per_d = 3u + 3u * (uint32_t)a.Ld;
    for (uint32_t e = threadIdx.x; e < n_dirs * per_d; e += VN_BLOCK) {
        const uint32_t t = e / per_d, q = e - t * per_d;
        if (q < 3) { s_dir[t * cd + q] = a.dirs[(d0 + t) * 3 + q]; continue; }
        const uint32_t l = (q - 3) / 3u, ax = (q - 3) % 3u;
        const float y = ldexpf(a.dirs[(d0 + t) * 3 + ax], (int)l);
        s_dir[t * cd + 3 + 6 * l + ax] = sinf(y);
        s_dir[t * cd + 6 + 6 * l + ax] = cosf(y);
    }
    __syncthreads();
    // the tile's rows are one contiguous block of tile * ld floats: consecutive lanes write consecutive addresses
    float* out = a.out + g0 * a.ld;
    for (uint32_t e = threadIdx.x; e < tile * a.ld; e += VN_BLOCK) {
        const uint32_t sl = e / a.ld, c = e - sl * a.ld;
        float v = 0.f;                                                       // columns [ch, ld) are written as zeros
        if (c < cp) v = vn_tile[(size_t)sl * cp + c];
        else if (c < ch) v = s_dir[(uint32_t)((g0 + sl) / a.rows_per_dir - d0) * cd + (c - cp)];
        out[e] = v;
    }
}

// ------------------------------------------------------------------------------------------ NerfRender.forward (training)
struct VnRenderArgs {
    const float4* raw;                       // [R, S] of (r, g, b, sigma)
    const float* z_vals;                     // [R, S] sample positions
    const float* rays_d;                     // [R, 3]
    const float* noise;                      // [R, S] or null (raw_noise_std * randn, drawn by the caller)
    uint32_t n_rays, n_s;
    int white_bkgd;
};

struct VnSample { float4 v; float z, dist, x, ed, alpha, f; };

// nerf_render.py:60-88 for one sample: last interval 1e10, distances times |rays_d|, sigma = relu(raw_3 + noise)
static __device__ inline VnSample vn_load(const VnRenderArgs& a, uint32_t r, uint32_t i, float dnorm) {
    VnSample s;
    const uint64_t g = (uint64_t)r * a.n_s + i;
    s.v = a.raw[g];
    s.z = a.z_vals[g];
    s.dist = (i + 1 < a.n_s ? a.z_vals[g + 1] - s.z : 1e10f) * dnorm;
    s.x = a.noise != nullptr ? s.v.w + a.noise[g] : s.v.w;
    s.ed = expf(-(fmaxf(s.x, 0.f) * s.dist));
    s.alpha = 1.f - s.ed;
    s.f = 1.f - s.alpha + 1e-10f;
    return s;
}
static __device__ inline float vn_dnorm(const VnRenderArgs& a, uint32_t r) {
    const float dx = a.rays_d[r * 3ull], dy = a.rays_d[r * 3ull + 1], dz = a.rays_d[r * 3ull + 2];
    return sqrtf(dx * dx + dy * dy + dz * dz);
}

// the forward sweep's policy (xr_render.h)
struct VnRender {
    typedef VnSample Sample;
    typedef XrCumprodStep Step;
    VnRenderArgs a;
    float dnorm;
    __device__ void ray(uint32_t r) { dnorm = vn_dnorm(a, r); }
    __device__ VnSample load(uint32_t r, uint32_t i) const { return vn_load(a, r, i, dnorm); }
    __device__ double step_in(const VnSample& s) const { return (double)s.f; }
    __device__ float weight(const VnSample& s, float t) const { return s.alpha * t; }
    __device__ void colours(const VnSample& s, float* c) const {
        c[0] = xr_mip_sigmoid(s.v.x); c[1] = xr_mip_sigmoid(s.v.y); c[2] = xr_mip_sigmoid(s.v.z);
    }
    __device__ float depth(const VnSample& s) const { return s.z; }
    __device__ float ray_scalar(uint32_t, float depth, float acc) const { return xr_render_disp(depth, acc); }
};

__global__ void __launch_bounds__(VN_BLOCK) k_nerf_render_fwd(VnRenderArgs a, float* __restrict__ rgb_out, float* __restrict__ disp_out,
                                                              float* __restrict__ acc_out, float* __restrict__ weights_out) {
    xr_render_fwd(VnRender{a, 0.f}, blockIdx.x * VN_WAVES + (threadIdx.x >> 6), rgb_out, disp_out, acc_out, weights_out);
}

__global__ void __launch_bounds__(VN_BLOCK) k_nerf_render_bwd(VnRenderArgs a, const float* __restrict__ grad_rgb,
                                                              float4* __restrict__ grad_raw) {
    const uint32_t r = blockIdx.x * VN_WAVES + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (r >= a.n_rays) return;
    const float dnorm = vn_dnorm(a, r);
    const float g[3] = {grad_rgb[r * 3ull], grad_rgb[r * 3ull + 1], grad_rgb[r * 3ull + 2]};
    const float gw = a.white_bkgd ? (g[0] + g[1]) + g[2] : 0.f;
    const uint32_t n_sweeps = (a.n_s + 63) / 64;
    // pass 1 (only with more than one sweep): lane b keeps the transmittance in front of sweep b
    double my_carry = 1.0;
    if (n_sweeps > 1) {
        XrCumprodStep st;
        for (uint32_t b = 0; b + 1 < n_sweeps; ++b) {
            if (lane == b) my_carry = st.carry;
            const uint32_t i = b * 64 + lane;                                // a full sweep: every lane is live
            st.step64((double)vn_load(a, r, i, dnorm).f);
        }
        if (lane == n_sweeps - 1) my_carry = st.carry;
    }
    // pass 2, last sweep first: S_carry is S at the last sample of the sweep
    double s_carry = 0.0;
    for (uint32_t b = n_sweeps; b-- > 0;) {
        const uint32_t i = b * 64 + lane;
        const bool live = i < a.n_s;
        VnSample s;
        double f = 1.0, ag = 0.0;
        float G = 0.f, sg[3] = {0.f, 0.f, 0.f};
        if (live) {
            s = vn_load(a, r, i, dnorm);
            f = (double)s.f;
            sg[0] = xr_mip_sigmoid(s.v.x); sg[1] = xr_mip_sigmoid(s.v.y); sg[2] = xr_mip_sigmoid(s.v.z);
            G = ((g[0] * sg[0] + g[1] * sg[1]) + g[2] * sg[2]) - gw;
            ag = (double)s.alpha * (double)G;
        }
        XrCumprodStep st;
        st.carry = __shfl(my_carry, (int)b, 64);                             // the transmittance in front of this sweep, from pass 1
        const double T = st.step64(f);
        // reverse inclusive scan of the maps x -> ag + f x: (F, A) of lane k covers samples k .. 63
        const XrAffine<double> m = xr_wave_affine_rscan(f, ag);
        const double F = m.F, A = m.A;
        // S_k = the map of samples k+1 .. 63 applied to the carry
        const double Fn = __shfl_down(F, 1, 64), An = __shfl_down(A, 1, 64);
        const double S = lane == 63 ? s_carry : An + Fn * s_carry;
        if (live) {
            const float Tf = (float)T;
            const float w = s.alpha * Tf;
            const float d_alpha = (float)(T * ((double)G - S));
            float4 o;
            o.x = g[0] * w * (sg[0] * (1.f - sg[0]));
            o.y = g[1] * w * (sg[1] * (1.f - sg[1]));
            o.z = g[2] * w * (sg[2] * (1.f - sg[2]));
            o.w = s.x > 0.f ? d_alpha * s.ed * s.dist : 0.f;                 // relu' is 0 at 0, as in torch
            grad_raw[(uint64_t)r * a.n_s + i] = o;
        }
        s_carry = __shfl(A, 0, 64) + __shfl(F, 0, 64) * s_carry;
    }
}

// ------------------------------------------------------------------------------------------ sample_pdf
// hierarchical_sample.py:6-53.  LDS per wave: cdf [S-1] and the sort buffer [P], P = the power of two >= S + N.
__global__ void __launch_bounds__(VN_BLOCK) k_nerf_sample_pdf(const float* __restrict__ z_vals, const float* __restrict__ weights,
                                                              const float* __restrict__ u_in, const float* __restrict__ rays_o,
                                                              const float* __restrict__ rays_d, uint32_t n_rays, uint32_t S, uint32_t N,
                                                              uint32_t P, float* __restrict__ z_out, float* __restrict__ pts_out,
                                                              float* __restrict__ z_samples_out) {
    extern __shared__ float vn_mem[];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t r = blockIdx.x * VN_WAVES + wave;
    if (r >= n_rays) return;                   // no block-wide barrier below: waves are independent
    const uint32_t n = S - 2;                  // pdf entries; the cdf has n + 1 = S - 1 entries, one per bin midpoint
    float* cdf = vn_mem + (size_t)wave * (S - 1 + P);
    float* buf = cdf + (S - 1);
    const float* w = weights + (uint64_t)r * S + 1;          // weights[1:-1]
    const float* z = z_vals + (uint64_t)r * S;
    for (uint32_t i = lane; i < P; i += 64) buf[i] = i < S ? z[i] : __uint_as_float(0x7f800000u);       // +inf behind the data
    double part = 0.0;
    for (uint32_t i = lane; i < n; i += 64) part += (double)(w[i] + 1e-5f);
    const float wsum = (float)xr_wave_sum(part);
    double carry = 0.0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t i = base + lane;
        double p = 0.0;
        if (i < n) p = (double)((w[i] + 1e-5f) / wsum);
        const double incl = xr_wave_incl_sum(p);
        if (i < n) cdf[i + 1] = (float)(carry + incl);
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) cdf[0] = 0.f;
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    for (uint32_t j = lane; j < N; j += 64) {
        const float u = u_in != nullptr ? u_in[(uint64_t)r * N + j] : xr_torch_linspace(0.f, 1.f, N, j);
        // searchsorted(right=True) - 1: the last index with cdf <= u (cdf[0] = 0; a NaN draw stays at 0)
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (cdf[mid] <= u) lo = mid; else hi = mid - 1;
        }
        const uint32_t above = lo + 1 < n ? lo + 1 : n;
        const float c0 = cdf[lo], c1 = cdf[above];
        const float b0 = .5f * (buf[lo + 1] + buf[lo]), b1 = .5f * (buf[above + 1] + buf[above]);
        float denom = c1 - c0;
        if (denom < 1e-5f) denom = 1.f;
        const float t = (u - c0) / denom;
        const float zs = b0 + t * (b1 - b0);
        buf[S + j] = zs;           // (the bins read buf[0 .. S-1] only)
        if (z_samples_out != nullptr) z_samples_out[(uint64_t)r * N + j] = zs;
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    // torch.sort of [z_vals | z_samples]: bitonic network over P slots
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = lane; t < P / 2; t += 64) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const float x = buf[i], y = buf[p];
                const bool up = (i & k) == 0;
                if (up ? (x > y) : (x < y)) { buf[i] = y; buf[p] = x; }
            }
            __builtin_amdgcn_wave_barrier();
            __threadfence_block();
        }
    }
    const uint32_t M = S + N;
    for (uint32_t i = lane; i < M; i += 64) z_out[(uint64_t)r * M + i] = buf[i];
    const float o[3] = {rays_o[r * 3ull], rays_o[r * 3ull + 1], rays_o[r * 3ull + 2]};
    const float d[3] = {rays_d[r * 3ull], rays_d[r * 3ull + 1], rays_d[r * 3ull + 2]};
    for (uint32_t e = lane; e < 3 * M; e += 64) {
        const uint32_t i = e / 3u, c = e - 3u * i;
        pts_out[(uint64_t)r * 3 * M + e] = o[c] + d[c] * buf[i];
    }
}

// ------------------------------------------------------------------------------------------ C-ABI
extern "C" int xr_nerf_encode(const float* pts, const float* viewdirs, uint64_t n_rows, uint32_t rows_per_dir, int multires,
                              int multires_dirs, float* out, uint32_t ld, void* stream) {
    XR_REQUIRE(multires >= 0 && multires <= VN_MAX_FREQS && multires_dirs >= 0 && multires_dirs <= VN_MAX_FREQS,
               "multires and multires_dirs must be in [0, 16]");
    XR_REQUIRE(rows_per_dir >= 1, "rows_per_dir must be >= 1");
    const uint32_t cp = 3u + 6u * (uint32_t)multires, ch = cp + 3u + 6u * (uint32_t)multires_dirs;
    XR_REQUIRE(ld >= (ch + 3u) / 4u * 4u, "ld must be >= the channel count rounded up to a multiple of 4");
    if (n_rows == 0) return XR_OK;
    XR_REQUIRE(pts && viewdirs && out, "null pointer");
    XR_REQUIRE(n_rows <= 0x7fffffffull * VN_TILE, "too many rows");
    VnEncArgs a{pts, viewdirs, n_rows, rows_per_dir, multires, multires_dirs, out, ld};
    hipLaunchKernelGGL(k_nerf_encode, dim3(xr_div_up(n_rows, VN_TILE)), dim3(VN_BLOCK), (size_t)VN_TILE * ch * sizeof(float),
                       (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return XR_OK;
}

static int vn_render_args(VnRenderArgs& a, const float* raw, const float* z_vals, const float* rays_d, const float* noise, uint32_t n_rays,
                          uint32_t n_samples, int white_bkgd) {
    XR_REQUIRE(n_samples >= 1 && n_samples <= VN_MAX_S, "n_samples must be in [1, 4096]");
    XR_REQUIRE(n_rays == 0 || (raw && z_vals && rays_d), "null pointer");
    XR_REQUIRE(((uintptr_t)raw & 15) == 0, "raw must be 16-byte aligned");
    a = VnRenderArgs{reinterpret_cast<const float4*>(raw), z_vals, rays_d, noise, n_rays, n_samples, white_bkgd};
    return XR_OK;
}

extern "C" int xr_nerf_render_train_forward(const float* raw, const float* z_vals, const float* rays_d, const float* noise, uint32_t n_rays,
                                            uint32_t n_samples, int white_bkgd, float* rgb, float* disp, float* acc, float* weights,
                                            void* stream) {
    VnRenderArgs a;
    int rc = vn_render_args(a, raw, z_vals, rays_d, noise, n_rays, n_samples, white_bkgd);
    if (rc) return rc;
    if (n_rays == 0) return XR_OK;
    XR_REQUIRE(rgb && disp && acc && weights, "null pointer");
    hipLaunchKernelGGL(k_nerf_render_fwd, dim3(xr_div_up(n_rays, VN_WAVES)), dim3(VN_BLOCK), 0, (hipStream_t)stream, a, rgb, disp, acc,
                       weights);
    XR_LAUNCH_CHECK();
    return XR_OK;
}

extern "C" int xr_nerf_render_backward(const float* raw, const float* z_vals, const float* rays_d, const float* noise, uint32_t n_rays,
                                       uint32_t n_samples, int white_bkgd, const float* grad_rgb, float* grad_raw, void* stream) {
    VnRenderArgs a;
    int rc = vn_render_args(a, raw, z_vals, rays_d, noise, n_rays, n_samples, white_bkgd);
    if (rc) return rc;
    if (n_rays == 0) return XR_OK;
    XR_REQUIRE(grad_rgb && grad_raw, "null pointer");
    XR_REQUIRE(((uintptr_t)grad_raw & 15) == 0, "grad_raw must be 16-byte aligned");
    hipLaunchKernelGGL(k_nerf_render_bwd, dim3(xr_div_up(n_rays, VN_WAVES)), dim3(VN_BLOCK), 0, (hipStream_t)stream, a, grad_rgb,
                       reinterpret_cast<float4*>(grad_raw));
    XR_LAUNCH_CHECK();
    return XR_OK;
}

extern "C" int xr_nerf_sample_pdf(const float* z_vals, const float* weights, const float* u, const float* rays_o, const float* rays_d,
                                  uint32_t n_rays, uint32_t n_coarse, uint32_t n_new, float* z_out, float* pts_out, float* z_samples_out,
                                  void* stream) {
    XR_REQUIRE(n_coarse >= 3 && n_coarse <= VN_PDF_MAX, "the coarse sample count must be in [3, 1024]");
    XR_REQUIRE(n_new >= 1 && n_new <= VN_PDF_MAX, "the new sample count must be in [1, 1024]");
    if (n_rays == 0) return XR_OK;
    XR_REQUIRE(z_vals && weights && rays_o && rays_d && z_out && pts_out, "null pointer");
    XR_REQUIRE(z_out != z_vals, "in-place resampling is not supported");
    uint32_t P = 4;
    while (P < n_coarse + n_new) P <<= 1;                                    // <= 2048
    const size_t lds = (size_t)VN_WAVES * (n_coarse - 1 + P) * sizeof(float);   // <= 4 * 3071 * 4 = 49136 bytes
    hipLaunchKernelGGL(k_nerf_sample_pdf, dim3(xr_div_up(n_rays, VN_WAVES)), dim3(VN_BLOCK), lds, (hipStream_t)stream, z_vals, weights, u,
                       rays_o, rays_d, n_rays, n_coarse, n_new, P, z_out, pts_out, z_samples_out);
    XR_LAUNCH_CHECK();
    return XR_OK;
}
