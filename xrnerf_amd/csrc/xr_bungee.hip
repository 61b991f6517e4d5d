// BungeeNeRF (configs/bungeenerf/bungeenerf_multiscale_google.py) for gfx950: bounds + z-values, cast_rays + BungeeEmbedder, and the
// multi-head renderer.  The reference runs each of these as a chain of small PyTorch elementwise launches
// (datasets/pipelines/create.py BungeeGetBounds / BungeeGetZvals, models/networks/utils/mip.py cast_rays,
// models/embedders/bungee_embedder.py, models/renders/bungeenerf_render.py); here each is ONE launch:
//   k_bungee_zvals     thread = ray: sphere / flat bounds, disparity-then-depth edges, the reference's sort
//   k_bungee_encode    workgroup = 64 consecutive samples; gaussians in LDS, the per-ray direction features once per ray of the tile,
//                      then the lanes sweep (sample, frequency, axis) items, one exp factor shared by the sin and the cos column
//   k_bungee_render_*  wave = ray; 64 intervals per sweep: the forward sweep and the backward's pass body of xr_render.h with the policy
//                      BungeeRender; transmittance as an fp64 prefix PRODUCT of (1 - alpha + 1e-10) (torch's CPU cumprod
//                      accumulates fp32 in double), fixed-order butterflies for the sums
// Compiled with -ffp-contract=off: every expression is fp32 in the reference's operation order.
//
// Bounds precision.  The sphere mode intersects spheres of earth radius (6371011 m times the scene scaling): |o - c|^2 - r^2 subtracts
// two fp32 numbers of ~4e13 s^2 whose difference is ~2 r h s^2 (h = camera height above the 250 m building sphere), so the fp32
// rounding of the squares (~6e-8 relative) leaves a relative error of ~6e-8 r / (2 h), i.e. ~2e-4 at h = 1 km and ~2e-5 at h = 10 km,
// in both the reference and here.  fp64 would bring it to ~1e-12; this kernel reproduces the reference's fp32 arithmetic instead (its
// trained networks expect its bounds), so the sphere bounds agree with the reference to the extent that both round the same
// expressions the same way, not to the precision fp64 would give.
#include "xr_common.h"
#include "xr_mip_math.h"
#include "xr_bungee_zvals.h"
#include "xr_render.h"

#define BG_TILE 64
#define BG_BLOCK 256
#define BG_MAX_DIR_CH 64                 /* 3 + 6 multires_dirs <= 64: multires_dirs <= 10 */

// ------------------------------------------------------------------------------------------ BungeeGetBounds + BungeeGetZvals
struct BungeeZArgs {
    const float* rays_o; const float* viewdirs;
    float* near; float* far;                 // inputs (mode 0) or outputs (modes 1, 2)
    uint32_t n_rays, n_z;
    BgBounds b;
    float* z_out;
};

// the bounds, the edges and the reference's sort: xr_bungee_zvals.h (shared with xr_bungeedata.hip)
__global__ void k_bungee_zvals(BungeeZArgs a) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_rays) return;
    float nr, fr;
    if (a.b.mode == 0) {
        nr = a.near[r]; fr = a.far[r];
    } else {
        const float o[3] = {a.rays_o[r * 3ull], a.rays_o[r * 3ull + 1], a.rays_o[r * 3ull + 2]};
        const float v[3] = {a.viewdirs[r * 3ull], a.viewdirs[r * 3ull + 1], a.viewdirs[r * 3ull + 2]};
        bg_bounds(a.b, o, v, &nr, &fr);
        a.near[r] = nr; a.far[r] = fr;
    }
    bg_zvals_row(nr, fr, a.n_z, a.z_out + (uint64_t)r * a.n_z);
}

// ------------------------------------------------------------------------------------------ cast_rays + BungeeEmbedder
struct BungeeEncArgs {
    const float* rays_o; const float* rays_d; const float* radii; const float* z_vals;   // frustum description, or
    const float* means; const float* covs;                                               // materialised gaussians [R*S, 3] each
    const float* viewdirs;
    uint32_t n_rays, n_s;
    int multires, multires_dirs, cylinder;
    float* out_pts; uint32_t ld_pts;         // [R*S rows] x (3 + 6 multires) columns from the row start
    float* out_dir; uint32_t ld_dir;         // [R*S rows] x (3 + 6 multires_dirs)
};

__global__ void __launch_bounds__(BG_BLOCK) k_bungee_encode(BungeeEncArgs a) {
    __shared__ float s_g[6][BG_TILE];                    // mean3, cov3 per sample of the tile
    __shared__ float s_dir[BG_TILE][BG_MAX_DIR_CH];      // direction features per ray of the tile
    const uint64_t n_total = (uint64_t)a.n_rays * a.n_s;
    const uint64_t g0 = (uint64_t)blockIdx.x * BG_TILE;
    const uint32_t tile = (uint32_t)(n_total - g0 < BG_TILE ? n_total - g0 : BG_TILE);
    const uint32_t r0 = (uint32_t)(g0 / a.n_s);
    const uint32_t n_tile_rays = (uint32_t)((g0 + tile - 1) / a.n_s) - r0 + 1;       // <= 64
    const uint32_t dch = 3u + 6u * (uint32_t)a.multires_dirs;
    if (threadIdx.x < tile) {
        const uint64_t g = g0 + threadIdx.x;
        const uint32_t r = (uint32_t)(g / a.n_s), s = (uint32_t)(g % a.n_s);
        float mean[3], cov[3];
        if (a.means != nullptr) {
            for (int k = 0; k < 3; ++k) { mean[k] = a.means[g * 3 + k]; cov[k] = a.covs[g * 3 + k]; }
        } else {
            const float o[3] = {a.rays_o[r * 3ull], a.rays_o[r * 3ull + 1], a.rays_o[r * 3ull + 2]};
            const float d[3] = {a.rays_d[r * 3ull], a.rays_d[r * 3ull + 1], a.rays_d[r * 3ull + 2]};
            const float* z = a.z_vals + (uint64_t)r * (a.n_s + 1) + s;
            xr_mip_gaussian(o, d, a.radii[r], z[0], z[1], a.cylinder, mean, cov);
        }
        for (int k = 0; k < 3; ++k) { s_g[k][threadIdx.x] = mean[k]; s_g[3 + k][threadIdx.x] = cov[k]; }
    } else if (threadIdx.x >= BG_TILE && threadIdx.x - BG_TILE < n_tile_rays) {
        // the direction part depends on the ray only: [d, sin(d 2^l), cos(d 2^l)]_{l < multires_dirs}
        const uint32_t t = threadIdx.x - BG_TILE, r = r0 + t;
        float* o = s_dir[t];
        for (int k = 0; k < 3; ++k) {
            const float v = a.viewdirs[r * 3ull + k];
            o[k] = v;
            for (int l = 0; l < a.multires_dirs; ++l) {
                const float y = ldexpf(v, l);                            // x * 2^l: exact
                o[3 + 6 * l + k] = sinf(y);
                o[6 + 6 * l + k] = cosf(y);
            }
        }
    }
    __syncthreads();
    // point part: item q of a sample = identity column q (q < 3) or (l, axis) = ((q-3)/3, (q-3)%3) -> columns 3+6l+axis, 6+6l+axis
    const uint32_t per = 3u + 3u * (uint32_t)a.multires;
    for (uint32_t e = threadIdx.x; e < tile * per; e += BG_BLOCK) {
        const uint32_t sl = e / per, q = e - sl * per;
        float* row = a.out_pts + (g0 + sl) * a.ld_pts;
        if (q < 3) { row[q] = s_g[q][sl]; continue; }
        const uint32_t l = (q - 3) / 3u, ax = (q - 3) % 3u;
        const float y = ldexpf(s_g[ax][sl], (int)l);                     // mean * 2^l: exact
        const float w = expf(ldexpf(s_g[3 + ax][sl], 2 * (int)l) * -0.5f);   // (-0.5 * 4^l) * cov: exact scalings, one exp
        row[3 + 6 * l + ax] = sinf(y) * w;
        row[6 + 6 * l + ax] = cosf(y) * w;
    }
    for (uint32_t e = threadIdx.x; e < tile * dch; e += BG_BLOCK) {
        const uint32_t sl = e / dch, c = e - sl * dch;
        const uint32_t t = (uint32_t)((g0 + sl) / a.n_s) - r0;
        a.out_dir[(g0 + sl) * a.ld_dir + c] = s_dir[t][c];
    }
}

// ------------------------------------------------------------------------------------------ BungeeNerfRender
struct BungeeRenderArgs {
    const float* raw;                        // [R, S, H, 4]
    const float* z_vals;                     // [R, S+1] interval edges
    const float* viewdirs;                   // [R, 3]
    const float* noise;                      // [R, S] or null (raw_noise_std * randn, drawn by the caller)
    uint32_t n_rays, n_s, n_heads, n_used;   // n_used = min(stage + 1, H) heads are summed
    float density_bias, rgb_k, rgb_padding;  // rgb_k = float32(1 + 2 rgb_padding)
    int white_bkgd, relu;
};

struct BungeeSample { float a_rgb[3], x, dist, zmid, dd, f; };

// per-interval quantities in the reference's order: head sums, midpoint distances, density_delta, 1 - alpha + 1e-10
static __device__ inline BungeeSample bg_load(const BungeeRenderArgs& a, uint32_t r, uint32_t i, float vnorm) {
    BungeeSample s;
    const float4* p = reinterpret_cast<const float4*>(a.raw) + ((uint64_t)r * a.n_s + i) * a.n_heads;
    float4 acc = p[0];
    for (uint32_t h = 1; h < a.n_used; ++h) {
        const float4 v = p[h];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    s.a_rgb[0] = acc.x; s.a_rgb[1] = acc.y; s.a_rgb[2] = acc.z;
    const float* z = a.z_vals + (uint64_t)r * (a.n_s + 1) + i;
    s.zmid = .5f * (z[1] + z[0]);
    float d = 1e10f;
    if (i + 1 < a.n_s) d = .5f * (z[2] + z[1]) - s.zmid;
    s.dist = d * vnorm;
    float x = acc.w;
    if (a.noise != nullptr) x = x + a.noise[(uint64_t)r * a.n_s + i];
    s.x = x + a.density_bias;
    s.dd = -xr_mip_density_act(s.x, a.relu) * s.dist;
    s.f = (1.f - (1.f - expf(s.dd))) + 1e-10f;
    return s;
}
static __device__ inline float bg_rgb(const BungeeRenderArgs& a, float x) { return a.rgb_k / (1.f + expf(-x)) - a.rgb_padding; }

// the policy of xr_render.h: the forward sweep, and the pass body of the two-pass backward
struct BungeeRender {
    typedef BungeeSample Sample;
    typedef XrCumprodStep Step;
    BungeeRenderArgs a;
    float vnorm;
    __device__ void ray(uint32_t r) { vnorm = bg_norm3(a.viewdirs[r * 3ull], a.viewdirs[r * 3ull + 1], a.viewdirs[r * 3ull + 2]); }
    __device__ BungeeSample load(uint32_t r, uint32_t i) const { return bg_load(a, r, i, vnorm); }
    __device__ double step_in(const BungeeSample& s) const { return (double)s.f; }
    __device__ float weight(const BungeeSample& s, float T) const { return (1.f - expf(s.dd)) * T; }
    __device__ void colours(const BungeeSample& s, float* c) const {
        for (int k = 0; k < 3; ++k) c[k] = bg_rgb(a, s.a_rgb[k]);
    }
    __device__ float depth(const BungeeSample& s) const { return s.zmid; }
    __device__ float ray_scalar(uint32_t, float depth, float acc) const { return xr_render_disp(depth, acc); }
};

__global__ void __launch_bounds__(BG_BLOCK) k_bungee_render_fwd(BungeeRenderArgs a, float* __restrict__ rgb_out,
                                                                float* __restrict__ disp_out, float* __restrict__ acc_out,
                                                                float* __restrict__ weights_out) {
    xr_render_fwd(BungeeRender{a, 0.f}, blockIdx.x * (BG_BLOCK / 64) + (threadIdx.x >> 6), rgb_out, disp_out, acc_out, weights_out);
}

// dL/draw given dL/drgb.  With gc_i = sum_ch g_ch (rgb_i,ch - [white]), w_i = alpha_i T_i, T_i = prod_{j<i} f_j, f_j = 1 - alpha_j + 1e-10:
//   dL/dalpha_k = T_k gc_k - (sum_{i>k} w_i gc_i) / f_k          (autograd's cumprod backward divides by the factor as well)
//   dL/dx_k     = dL/dalpha_k * exp(dd_k) * act'(x_k) * dist_k
// Every head h <= stage receives the same gradient; heads above the stage are written as exact zeros.
__global__ void __launch_bounds__(BG_BLOCK) k_bungee_render_bwd(BungeeRenderArgs a, const float* __restrict__ grad_rgb,
                                                                float* __restrict__ grad_raw) {
    const uint32_t r = blockIdx.x * (BG_BLOCK / 64) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (r >= a.n_rays) return;
    BungeeRender p{a, 0.f};
    p.ray(r);
    const float g[3] = {grad_rgb[r * 3ull], grad_rgb[r * 3ull + 1], grad_rgb[r * 3ull + 2]};
    const float white = a.white_bkgd ? 1.f : 0.f;
    // pass 1: total = sum_i w_i gc_i
    double total = 0.0;
    XrCumprodStep st;
    for (uint32_t base = 0; base < a.n_s; base += 64) total += xr_wave_sum(xr_render_term(p, st, r, base + lane, g, white).wg);
    // pass 2: gradients
    st = XrCumprodStep();
    double carry_wg = 0.0;
    for (uint32_t base = 0; base < a.n_s; base += 64) {
        const uint32_t i = base + lane;
        const XrRenderTerm<BungeeRender> q = xr_render_term(p, st, r, i, g, white);
        const BungeeSample& s = q.s;
        const double incl_wg = xr_wave_incl_sum(q.wg);
        if (i < a.n_s) {
            const double suffix = total - (carry_wg + incl_wg);
            const float d_alpha = (float)((double)(q.t * q.gc) - suffix / (double)s.f);
            const float ed = expf(s.dd);
            float4 o;
            float* oc = &o.x;
            for (int c = 0; c < 3; ++c) {
                const float e = expf(-s.a_rgb[c]), den = 1.f + e;
                oc[c] = g[c] * q.w * (a.rgb_k * e / (den * den));
            }
            o.w = d_alpha * ed * xr_mip_density_dact(s.x, a.relu) * s.dist;
            float4* out = reinterpret_cast<float4*>(grad_raw) + ((uint64_t)r * a.n_s + i) * a.n_heads;
            for (uint32_t h = 0; h < a.n_heads; ++h) out[h] = h < a.n_used ? o : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        carry_wg += __shfl(incl_wg, 63, 64);
    }
}

// ------------------------------------------------------------------------------------------ C-ABI
extern "C" int xr_bungee_zvals(const float* rays_o, const float* viewdirs, float* near, float* far, uint32_t n_rays, uint32_t n_z,
                               int bounds_mode, const float* globe_center, float r2_top, float r2_earth, float scaling, float* z_out,
                               void* stream) {
    XR_REQUIRE(n_z >= 2, "n_z must be >= 2");
    XR_REQUIRE(bounds_mode >= 0 && bounds_mode <= 2, "bounds_mode: 0 = none, 1 = sphere, 2 = flat");
    if (n_rays == 0) return XR_OK;
    XR_REQUIRE(near && far && z_out, "null pointer");
    XR_REQUIRE(bounds_mode == 0 || (rays_o && viewdirs), "null pointer");
    XR_REQUIRE(bounds_mode != 1 || globe_center, "sphere bounds need the globe centre");
    BungeeZArgs a{rays_o, viewdirs, near, far, n_rays, n_z, BgBounds{bounds_mode, 0.f, 0.f, 0.f, r2_top, r2_earth, scaling}, z_out};
    if (bounds_mode == 1) { a.b.cx = globe_center[0]; a.b.cy = globe_center[1]; a.b.cz = globe_center[2]; }
    hipLaunchKernelGGL(k_bungee_zvals, dim3(xr_div_up(n_rays, 128)), dim3(128), 0, (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return XR_OK;
}

extern "C" int xr_bungee_encode(const float* rays_o, const float* rays_d, const float* radii, const float* z_vals, const float* means,
                                const float* covs, const float* viewdirs, uint32_t n_rays, uint32_t n_samples, int multires,
                                int multires_dirs, int ray_shape, float* out_pts, uint32_t ld_pts, float* out_dir, uint32_t ld_dir,
                                void* stream) {
    XR_REQUIRE(multires >= 0 && multires <= 30, "multires must be in [0, 30]");
    XR_REQUIRE(multires_dirs >= 0 && 3 + 6 * multires_dirs <= BG_MAX_DIR_CH, "multires_dirs must be in [0, 10]");
    XR_REQUIRE(ray_shape == 0 || ray_shape == 1, "ray_shape: 0 = cone, 1 = cylinder");
    XR_REQUIRE(ld_pts >= 3u + 6u * (uint32_t)multires && ld_dir >= 3u + 6u * (uint32_t)multires_dirs, "row stride smaller than the row");
    const uint64_t n = (uint64_t)n_rays * n_samples;
    if (n == 0) return XR_OK;
    const bool frustum = rays_o || rays_d || radii || z_vals, gauss = means || covs;
    XR_REQUIRE(frustum != gauss, "give exactly one of (rays_o, rays_d, radii, z_vals) and (means, covs)");
    XR_REQUIRE(frustum ? (rays_o && rays_d && radii && z_vals) : (means && covs), "null pointer");
    XR_REQUIRE(viewdirs && out_pts && out_dir, "null pointer");
    XR_REQUIRE(n <= 0xffffffffull * BG_TILE, "too many samples");
    BungeeEncArgs a{rays_o, rays_d, radii, z_vals, means, covs, viewdirs, n_rays, n_samples, multires, multires_dirs, ray_shape,
                    out_pts, ld_pts, out_dir, ld_dir};
    hipLaunchKernelGGL(k_bungee_encode, dim3(xr_div_up(n, BG_TILE)), dim3(BG_BLOCK), 0, (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return XR_OK;
}

static int bungee_render_args(BungeeRenderArgs& a, const float* raw, const float* z_vals, const float* viewdirs, const float* noise,
                              uint32_t n_rays, uint32_t n_z, uint32_t n_heads, int stage, float density_bias, float rgb_padding,
                              int white_bkgd, int density_activation) {
    XR_REQUIRE(n_rays == 0 || (raw && z_vals && viewdirs), "null pointer");
    XR_REQUIRE(n_z >= 2, "n_z must be >= 2");
    XR_REQUIRE(n_heads >= 1 && stage >= 0, "need >= 1 head and stage >= 0");
    XR_REQUIRE(density_activation == 0 || density_activation == 1, "density_activation: 0 = softplus, 1 = relu");
    XR_REQUIRE(((uintptr_t)raw & 15) == 0, "raw must be 16-byte aligned");
    const uint32_t used = (uint32_t)stage + 1 < n_heads ? (uint32_t)stage + 1 : n_heads;
    a = BungeeRenderArgs{raw, z_vals, viewdirs, noise, n_rays, n_z - 1, n_heads, used, density_bias,
                         (float)(1.0 + 2.0 * (double)rgb_padding), rgb_padding, white_bkgd, density_activation};
    return XR_OK;
}

extern "C" int xr_bungee_render_forward(const float* raw, const float* z_vals, const float* viewdirs, const float* noise, uint32_t n_rays,
                                        uint32_t n_z, uint32_t n_heads, int stage, float density_bias, float rgb_padding, int white_bkgd,
                                        int density_activation, float* rgb, float* disp, float* acc, float* weights, void* stream) {
    BungeeRenderArgs a;
    int rc = bungee_render_args(a, raw, z_vals, viewdirs, noise, n_rays, n_z, n_heads, stage, density_bias, rgb_padding, white_bkgd,
                                density_activation);
    if (rc) return rc;
    if (n_rays == 0) return XR_OK;
    XR_REQUIRE(rgb && disp && acc && weights, "null pointer");
    hipLaunchKernelGGL(k_bungee_render_fwd, dim3(xr_div_up(n_rays, BG_BLOCK / 64)), dim3(BG_BLOCK), 0, (hipStream_t)stream, a, rgb, disp,
                       acc, weights);
    XR_LAUNCH_CHECK();
    return XR_OK;
}

extern "C" int xr_bungee_render_backward(const float* raw, const float* z_vals, const float* viewdirs, const float* noise,
                                         const float* grad_rgb, uint32_t n_rays, uint32_t n_z, uint32_t n_heads, int stage,
                                         float density_bias, float rgb_padding, int white_bkgd, int density_activation, float* grad_raw,
                                         void* stream) {
    BungeeRenderArgs a;
    int rc = bungee_render_args(a, raw, z_vals, viewdirs, noise, n_rays, n_z, n_heads, stage, density_bias, rgb_padding, white_bkgd,
                                density_activation);
    if (rc) return rc;
    if (n_rays == 0) return XR_OK;
    XR_REQUIRE(grad_rgb && grad_raw, "null pointer");
    XR_REQUIRE(((uintptr_t)grad_raw & 15) == 0, "grad_raw must be 16-byte aligned");
    hipLaunchKernelGGL(k_bungee_render_bwd, dim3(xr_div_up(n_rays, BG_BLOCK / 64)), dim3(BG_BLOCK), 0, (hipStream_t)stream, a, grad_rgb,
                       grad_raw);
    XR_LAUNCH_CHECK();
    return XR_OK;
}
