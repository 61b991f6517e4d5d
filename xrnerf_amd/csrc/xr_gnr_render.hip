// GNR's renderer stages (configs/gnr/gnr_genebody.py) for gfx950: what GnrRenderer.render_rays does around the network, as kernels.
// The reference's tensor lines are the specification, quirks included; every expression below is fp32 in the
// reference's order, compiled with -ffp-contract=off.
// (The projection's device functions -- GrHull, gr_project, gr_nearest_pixel, gr_att_directions -- live in xr_gnr_project.h, which
// xr_gnr_recon.hip includes as well.)
//   k_gr_flag      thread = (ray, sample): the sample point, its projection into every source view (w2c, division by clamp(z, 1e-9),
//                  five-coefficient distortion, intrinsics, normalisation) and the nearest mask sample of torch's grid_sample
//   k_gr_ray       thread = ray: the ray's flags become ranks inside the ray, their number the ray's count
//   k_gr_scan      one workgroup: exclusive scan of the counts -> (count, base) per ray and the total (xr_scan.h)
//   k_gr_write     thread = (ray, sample): a survivor writes its row at base + rank -- ascending flat index, the order of
//                  torch.nonzero -- with what the later stages need, so nothing is projected a second time
//   k_gr_gather    thread = (survivor, view, float4 of channels): bilinear samples of the channel-last feature maps and of the
//                  images, written at a row stride into the network's input
//   k_gr_gather_bwd  the same walk, adding w g to the feature maps in 64-bit fixed point (xr_fixed.h; k_gr_absmax and k_gr_gather_cvt
//                  around it)
//   k_gr_comp_fwd  wave = ray, lane = survivor, 64 at a time in sample order (outside the hull the reference's -1e4 gives alpha = 0
//                  and a factor of exactly 1.0f, so leaving those samples out changes no factor of the running product); the
//                  transmittance is a product scan over the lanes, the sums a butterfly: a fixed order, the same bits every run
//   k_gr_comp_bwd  wave = ray, the chunks backwards with a suffix scan of B <- G alpha + (1 - alpha + 1e-10) B; no division by a
//                  transmittance, no atomics
#include "xr_common.h"
#include "xr_wave.h"
#include "xr_scan.h"
#include "xr_fixed.h"
#include "../../include/xrnerf_mi355_gnr.h"
#include "xr_gnr_project.h"

#define GR_BLOCK 256
static_assert(GR_BLOCK == XR_SCAN_BLOCK && GR_BLOCK == XR_FIX_BLOCK, "the shared workgroup routines are written for 256 threads");
#define GR_WAVES (GR_BLOCK / 64)
#define GR_V XR_GNR_MAX_VIEWS

static __device__ inline void gr_point(const GrHull& a, uint32_t r, uint32_t s, float* p) {
    const float t = a.t_vals[(uint64_t)r * a.S + s];
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = a.rays[6ull * r + 3 + c] * t + (1.f - t) * a.rays[6ull * r + c];
}

__global__ void __launch_bounds__(GR_BLOCK) k_gr_flag(GrHull a, int32_t* __restrict__ rank) {
    const uint64_t id = (uint64_t)blockIdx.x * GR_BLOCK + threadIdx.x;
    if (id >= (uint64_t)a.R * a.S) return;
    const uint32_t r = (uint32_t)(id / a.S), s = (uint32_t)(id - (uint64_t)r * a.S);
    float p[3];
    gr_point(a, r, s, p);
    bool in = true;
    for (uint32_t v = 0; v < a.V; ++v) {
        float xy[2], z;
        int px, py;
        gr_project(a, v, p, xy, &z);
        if (!gr_nearest_pixel(xy[0], xy[1], a.H, a.W, &px, &py)) { in = false; break; }
        if (!(a.masks[((uint64_t)v * a.H + py) * a.W + px] > 0.f)) { in = false; break; }
    }
    rank[id] = in ? 1 : 0;
}

__global__ void __launch_bounds__(GR_BLOCK) k_gr_ray(uint32_t R, uint32_t S, int32_t* __restrict__ rank, int32_t* __restrict__ table) {
    const uint32_t r = blockIdx.x * GR_BLOCK + threadIdx.x;
    if (r >= R) return;
    int32_t* row = rank + (uint64_t)r * S;
    int32_t n = 0;
    for (uint32_t s = 0; s < S; ++s) {
        const int32_t f = row[s];
        row[s] = f ? n : -1;
        n += f;
    }
    table[2ull * r] = n;
}

// exclusive scan of table[r][0] -> table[r][1], the total -> total[0]; one workgroup
__global__ void __launch_bounds__(GR_BLOCK) k_gr_scan(uint32_t R, int32_t* __restrict__ table, int32_t* __restrict__ total) {
    const uint64_t sum = xr_scan_sweeps(R, [&](uint32_t b) { return (uint32_t)table[2ull * b]; },
                                        [&](uint32_t b, uint32_t base) { table[2ull * b + 1] = (int32_t)base; });
    if (threadIdx.x == 0) total[0] = xr_scan_total(sum);
}

struct GrRows {
    uint32_t M;
    float* pts; int32_t* idx; float* xy; float* z; uint8_t* vis; float* attdirs;
};

__global__ void __launch_bounds__(GR_BLOCK) k_gr_write(GrHull a, const int32_t* __restrict__ rank, const int32_t* __restrict__ table, GrRows o) {
    const uint64_t id = (uint64_t)blockIdx.x * GR_BLOCK + threadIdx.x;
    if (id >= (uint64_t)a.R * a.S) return;
    const int32_t k = rank[id];
    if (k < 0) return;
    const uint32_t r = (uint32_t)(id / a.S), s = (uint32_t)(id - (uint64_t)r * a.S);
    const uint64_t m = (uint64_t)(uint32_t)table[2ull * r + 1] + (uint32_t)k;
    if (m >= o.M) return;                                          // (the caller's M is the scan's total: never taken)
    float p[3];
    gr_point(a, r, s, p);
    o.pts[3 * m] = p[0]; o.pts[3 * m + 1] = p[1]; o.pts[3 * m + 2] = p[2];
    o.idx[m] = (int32_t)id;
    for (uint32_t v = 0; v < a.V; ++v) {
        float xy[2], z;
        gr_project(a, v, p, xy, &z);
        o.xy[(m * a.V + v) * 2] = xy[0]; o.xy[(m * a.V + v) * 2 + 1] = xy[1];
        o.z[m * a.V + v] = z;
        if (a.depth) {
            int px, py;
            float d = 0.f;
            if (gr_nearest_pixel(xy[0], xy[1], a.H, a.W, &px, &py)) d = a.depth[((uint64_t)v * a.H + py) * a.W + px];
            o.vis[m * a.V + v] = (z - d <= 0.f && d > 0.f) ? 1 : 0;
        }
    }
    if (o.attdirs) {
        const float q[3] = {a.rays[6ull * r] - a.rays[6ull * r + 3], a.rays[6ull * r + 1] - a.rays[6ull * r + 4], a.rays[6ull * r + 2] - a.rays[6ull * r + 5]};
        gr_att_directions(a, p, q, o.attdirs + m * (a.V + 1) * 3);
    }
}

static int gr_hull_args(GrHull* a, const char* fn, const float* rays, const float* t_vals, uint32_t R, uint32_t S, const float* w2c,
                        const float* cams, uint32_t cam_cols, uint32_t V, const float* masks, int H, int W, float width, float height) {
    if (!rays || !t_vals || !w2c || !cams || !masks) { xr_set_error("%s: null pointer", fn); return XR_EINVAL; }
    if (V < 1 || V > GR_V) { xr_set_error("%s: 1 .. XR_GNR_MAX_VIEWS source views", fn); return XR_EINVAL; }
    if (cam_cols < 4 || (cam_cols > 6 && cam_cols < 9)) { xr_set_error("%s: a camera row has 4 .. 6 entries, or at least 9 with distortion", fn); return XR_EINVAL; }
    if (H < 1 || W < 1 || H > (1 << 14) || W > (1 << 14)) { xr_set_error("%s: bad mask size", fn); return XR_EINVAL; }
    if (!(width > 0.f) || !(height > 0.f)) { xr_set_error("%s: the image size must be positive", fn); return XR_EINVAL; }
    if (S < 1 || (uint64_t)R * S > (1ull << 30)) { xr_set_error("%s: bad ray or sample count", fn); return XR_EINVAL; }
    memset(a, 0, sizeof(*a));
    a->rays = rays; a->t_vals = t_vals; a->R = R; a->S = S; a->V = V; a->w2c = w2c; a->cams = cams; a->cam_cols = cam_cols;
    a->masks = masks; a->H = H; a->W = W; a->width = width; a->height = height;
    return 0;
}

extern "C" int xr_gnr_hull_count(const float* rays, const float* t_vals, uint32_t R, uint32_t S, const float* w2c, const float* cams,
                                 uint32_t cam_cols, uint32_t V, const float* masks, int H, int W, float width, float height, int32_t* rank,
                                 int32_t* table, int32_t* total, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    XR_REQUIRE(total != nullptr, "null pointer");
    if (R == 0) { XR_HIP(hipMemsetAsync(total, 0, sizeof(int32_t), st)); return 0; }
    GrHull a;
    const int rc = gr_hull_args(&a, __func__, rays, t_vals, R, S, w2c, cams, cam_cols, V, masks, H, W, width, height);
    if (rc != 0) return rc;
    XR_REQUIRE(rank && table, "null pointer");
    hipLaunchKernelGGL(k_gr_flag, dim3(xr_div_up((uint64_t)R * S, GR_BLOCK)), dim3(GR_BLOCK), 0, st, a, rank);
    hipLaunchKernelGGL(k_gr_ray, dim3(xr_div_up(R, GR_BLOCK)), dim3(GR_BLOCK), 0, st, R, S, rank, table);
    hipLaunchKernelGGL(k_gr_scan, dim3(1), dim3(GR_BLOCK), 0, st, R, table, total);
    XR_LAUNCH_CHECK();
    return 0;
}

extern "C" int xr_gnr_hull_write(const float* rays, const float* t_vals, uint32_t R, uint32_t S, const float* w2c, const float* cams,
                                 uint32_t cam_cols, uint32_t V, const float* masks, const float* depth, int H, int W, float width, float height,
                                 const float* cam_c, const float* rot9, const int32_t* rank, const int32_t* table, uint32_t M, float* pts,
                                 int32_t* idx, float* xy, float* z, uint8_t* vis, float* attdirs, void* stream) {
    if (R == 0 || M == 0) return 0;
    GrHull a;
    const int rc = gr_hull_args(&a, __func__, rays, t_vals, R, S, w2c, cams, cam_cols, V, masks, H, W, width, height);
    if (rc != 0) return rc;
    XR_REQUIRE(rank && table && pts && idx && xy && z, "null pointer");
    XR_REQUIRE((uint64_t)M <= (uint64_t)R * S, "more survivors than points");
    XR_REQUIRE(!depth || vis, "the depth maps need the visibility output");
    XR_REQUIRE(!attdirs || cam_c, "the attention directions need the camera centres");
    a.depth = depth; a.cam_c = cam_c; a.rot = rot9;
    GrRows o;
    o.M = M; o.pts = pts; o.idx = idx; o.xy = xy; o.z = z; o.vis = vis; o.attdirs = attdirs;
    hipLaunchKernelGGL(k_gr_write, dim3(xr_div_up((uint64_t)R * S, GR_BLOCK)), dim3(GR_BLOCK), 0, (hipStream_t)stream, a, rank, table, o);
    XR_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------ pixel-aligned gather
struct GrGather {
    const float* xy; uint32_t M, V;
    const float* feats; int fh, fw; uint32_t C;          // [V, fh, fw, C] channel-last, C a multiple of 4
    const float* images; int ih, iw; int images_last;    // [V, 3, ih, iw], or [V, ih, iw, 3]
    float* out; uint32_t ld, col0;                       // row (m V + v) of out, columns col0 .. col0 + C + 3
    float* source_rgb;                                   // [M, V, 3]
};

// torch's grid_sampler_compute_source_index + the four corners (nw, ne, sw, se) and their weight products
struct GrCorners { int x0, y0; float w[4]; };
static __device__ inline void gr_corners(float nx, float ny, int H, int W, GrCorners* c) {
    const float ix = ((nx + 1.f) * (float)W - 1.f) / 2.f, iy = ((ny + 1.f) * (float)H - 1.f) / 2.f;
    const float fx = floorf(ix), fy = floorf(iy);
    // a coordinate beyond the map by more than a pixel (or not finite) has no corner inside: park it so the int conversion is defined
    const bool far = !(fx >= -2.f && fx <= (float)W && fy >= -2.f && fy <= (float)H);
    c->x0 = far ? -2 : (int)fx; c->y0 = far ? -2 : (int)fy;
    const float x1 = fx + 1.f, y1 = fy + 1.f;
    c->w[0] = (x1 - ix) * (y1 - iy);
    c->w[1] = (ix - fx) * (y1 - iy);
    c->w[2] = (x1 - ix) * (iy - fy);
    c->w[3] = (ix - fx) * (iy - fy);
}

__global__ void __launch_bounds__(GR_BLOCK) k_gr_gather(GrGather a) {
    const uint32_t q4 = a.C / 4, per = q4 + 1;                    // the last slot of a (survivor, view) samples the image
    const uint64_t id = (uint64_t)blockIdx.x * GR_BLOCK + threadIdx.x;
    if (id >= (uint64_t)a.M * a.V * per) return;
    const uint64_t mv = id / per;
    const uint32_t q = (uint32_t)(id - mv * per), v = (uint32_t)(mv % a.V);
    const float nx = a.xy[2 * mv], ny = a.xy[2 * mv + 1];
    float* row = a.out + mv * a.ld + a.col0;
    GrCorners c;
    if (q < q4) {
        gr_corners(nx, ny, a.fh, a.fw, &c);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = c.x0 + (k & 1), y = c.y0 + (k >> 1);
            if (x >= 0 && x < a.fw && y >= 0 && y < a.fh) {
                const float4 f = *reinterpret_cast<const float4*>(a.feats + (((uint64_t)v * a.fh + y) * a.fw + x) * a.C + 4ull * q);
                acc.x += f.x * c.w[k]; acc.y += f.y * c.w[k]; acc.z += f.z * c.w[k]; acc.w += f.w * c.w[k];
            }
        }
        row[4 * q] = acc.x; row[4 * q + 1] = acc.y; row[4 * q + 2] = acc.z; row[4 * q + 3] = acc.w;
    } else {
        gr_corners(nx, ny, a.ih, a.iw, &c);
        float rgb[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = c.x0 + (k & 1), y = c.y0 + (k >> 1);
            if (x >= 0 && x < a.iw && y >= 0 && y < a.ih) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const uint64_t at = a.images_last ? (((uint64_t)v * a.ih + y) * a.iw + x) * 3 + ch
                                                      : (((uint64_t)v * 3 + ch) * a.ih + y) * a.iw + x;
                    rgb[ch] += a.images[at] * c.w[k];
                }
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) { row[a.C + ch] = rgb[ch]; a.source_rgb[3 * mv + ch] = rgb[ch]; }
        for (uint32_t p = a.col0 + a.C + 3; p < a.ld; ++p) a.out[mv * a.ld + p] = 0.f;           // the padding columns
    }
}

extern "C" int xr_gnr_gather(const float* xy, uint32_t M, uint32_t V, const float* feats, int fh, int fw, uint32_t C, const float* images,
                             int ih, int iw, int images_channel_last, float* out, uint32_t ld, uint32_t col0, float* source_rgb, void* stream) {
    if (M == 0) return 0;
    XR_REQUIRE(xy && feats && images && out && source_rgb, "null pointer");
    XR_REQUIRE(V >= 1 && V <= GR_V, "1 .. XR_GNR_MAX_VIEWS source views");
    XR_REQUIRE(M <= (1u << 28), "too many points");
    XR_REQUIRE(C >= 4 && C % 4 == 0 && C <= 4096, "the feature channels must be a multiple of 4");
    XR_REQUIRE(fh >= 1 && fw >= 1 && ih >= 1 && iw >= 1 && fh <= (1 << 14) && fw <= (1 << 14) && ih <= (1 << 14) && iw <= (1 << 14), "bad map size");
    XR_REQUIRE((uint64_t)col0 + C + 3 <= ld, "the row stride is smaller than the row");
    XR_REQUIRE(((uintptr_t)feats & 15) == 0, "the feature maps must be 16-byte aligned");
    GrGather a;
    a.xy = xy; a.M = M; a.V = V; a.feats = feats; a.fh = fh; a.fw = fw; a.C = C; a.images = images; a.ih = ih; a.iw = iw;
    a.images_last = images_channel_last ? 1 : 0; a.out = out; a.ld = ld; a.col0 = col0; a.source_rgb = source_rgb;
    const uint64_t n = (uint64_t)M * V * (C / 4 + 1);
    hipLaunchKernelGGL(k_gr_gather, dim3(xr_div_up(n, GR_BLOCK)), dim3(GR_BLOCK), 0, (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return 0;
}

// ---- backward: the gradient in the feature maps, 64-bit fixed point (xr_fixed.h: integer adds commute, so two runs give the same
// bits).  The scale's n is M: a map element receives at most one corner of every (point, view) of its view
struct GrGatherBwd {
    const float* xy; uint32_t M, V;
    const float* grad; uint32_t ld, col0;                // row (m V + v) of grad, columns col0 .. col0 + C
    int fh, fw; uint32_t C;
    const double* scale; unsigned long long* acc;        // [V, fh, fw, C]
};

__global__ void __launch_bounds__(GR_BLOCK) k_gr_absmax(GrGatherBwd a, float* __restrict__ bmax) {
    float m = 0.f;
    const uint64_t total = (uint64_t)a.M * a.V * a.C;
    for (uint64_t e = (uint64_t)blockIdx.x * GR_BLOCK + threadIdx.x; e < total; e += (uint64_t)gridDim.x * GR_BLOCK) {
        const uint64_t mv = e / a.C;
        const float g = fabsf(a.grad[mv * a.ld + a.col0 + (uint32_t)(e - mv * a.C)]);
        if (g <= 3.0e38f) m = fmaxf(m, g);                          // (a NaN or an infinite entry contributes nothing, here either)
    }
    xr_fix_block_max(m, bmax);
}

__global__ void __launch_bounds__(GR_BLOCK) k_gr_gather_bwd(GrGatherBwd a) {
    const uint32_t q4 = a.C / 4;
    const uint64_t id = (uint64_t)blockIdx.x * GR_BLOCK + threadIdx.x;
    if (id >= (uint64_t)a.M * a.V * q4) return;
    const uint64_t mv = id / q4;
    const uint32_t q = (uint32_t)(id - mv * q4), v = (uint32_t)(mv % a.V);
    const double scale = a.scale[0];
    GrCorners c;
    gr_corners(a.xy[2 * mv], a.xy[2 * mv + 1], a.fh, a.fw, &c);
    const float* g = a.grad + mv * a.ld + a.col0 + 4u * q;
    const float ge[4] = {g[0], g[1], g[2], g[3]};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = c.x0 + (k & 1), y = c.y0 + (k >> 1);
        if (!(x >= 0 && x < a.fw && y >= 0 && y < a.fh)) continue;
        unsigned long long* d = a.acc + (((uint64_t)v * a.fh + y) * a.fw + x) * a.C + 4ull * q;
        const double w = (double)c.w[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) xr_fix_add(d + j, w, ge[j], scale);
    }
}

__global__ void __launch_bounds__(GR_BLOCK) k_gr_gather_cvt(const double* __restrict__ scale, const unsigned long long* __restrict__ acc,
                                                            uint64_t n, float* __restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * GR_BLOCK + threadIdx.x;
    if (e >= n) return;
    out[e] = xr_fix_to_float(acc[e], scale[0]);
}

extern "C" size_t xr_gnr_gather_backward_workspace_bytes(uint32_t V, int fh, int fw, uint32_t C) {
    if (fh < 1 || fw < 1) return 0;
    return (size_t)(XR_FIX_HEAD + (uint64_t)V * (uint32_t)fh * (uint32_t)fw * C * sizeof(unsigned long long));
}

extern "C" int xr_gnr_gather_backward(const float* xy, uint32_t M, uint32_t V, const float* grad, uint32_t ld, uint32_t col0, int fh, int fw,
                                      uint32_t C, float* d_feats, void* workspace, size_t workspace_bytes, void* stream) {
    XR_REQUIRE(d_feats != nullptr, "null pointer");
    XR_REQUIRE(V >= 1 && V <= GR_V, "1 .. XR_GNR_MAX_VIEWS source views");
    XR_REQUIRE(M <= (1u << 28), "too many points");
    XR_REQUIRE(C >= 4 && C % 4 == 0 && C <= 4096, "the feature channels must be a multiple of 4");
    XR_REQUIRE(fh >= 1 && fw >= 1 && fh <= (1 << 14) && fw <= (1 << 14), "bad map size");
    XR_REQUIRE(workspace != nullptr && ((uintptr_t)workspace & 7u) == 0, "the workspace must be 8-byte aligned");
    if (workspace_bytes < xr_gnr_gather_backward_workspace_bytes(V, fh, fw, C)) { xr_set_error("%s: workspace too small", __func__); return XR_ENOMEM; }
    const uint64_t el = (uint64_t)V * (uint32_t)fh * (uint32_t)fw * C;
    hipStream_t st = (hipStream_t)stream;
    const XrFixWs ws = xr_fix_ws(workspace);
    XR_HIP(hipMemsetAsync(workspace, 0, XR_FIX_HEAD + (size_t)el * sizeof(unsigned long long), st));
    GrGatherBwd a;
    a.xy = xy; a.M = M; a.V = V; a.grad = grad; a.ld = ld; a.col0 = col0; a.fh = fh; a.fw = fw; a.C = C; a.scale = ws.scale; a.acc = ws.acc;
    uint32_t nbm = 1;
    if (M != 0) {
        XR_REQUIRE(xy && grad, "null pointer");
        XR_REQUIRE((uint64_t)col0 + C <= ld, "the row stride is smaller than the row");
        nbm = xr_div_up((uint64_t)M * V * C, GR_BLOCK);
        if (nbm > XR_FIX_MAX_BMAX) nbm = XR_FIX_MAX_BMAX;
        hipLaunchKernelGGL(k_gr_absmax, dim3(nbm), dim3(GR_BLOCK), 0, st, a, ws.bmax);
    }
    hipLaunchKernelGGL(k_xr_fix_scale, dim3(1), dim3(XR_FIX_BLOCK), 0, st, (const float*)ws.bmax, nbm, M, ws.scale);
    if (M != 0) hipLaunchKernelGGL(k_gr_gather_bwd, dim3(xr_div_up((uint64_t)M * V * (C / 4), GR_BLOCK)), dim3(GR_BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_gr_gather_cvt, dim3(xr_div_up(el, GR_BLOCK)), dim3(GR_BLOCK), 0, st, (const double*)ws.scale, (const unsigned long long*)ws.acc, el, d_feats);
    XR_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------ blend compositor
struct GrComp {
    const float* net; uint32_t ld;                     // [M, ld]: rgb (3), density (1), attention (V + 1)
    const float* source_rgb;                           // [M, V, 3]
    const int32_t* idx; const int32_t* table;          // flat index per survivor; (count, base) per ray
    const float* t_vals; const float* noise;           // [R, S]; noise may be null (inference)
    uint32_t R, S, V, M;
    int have_z; float z_near, z_far; int white;
};

// one survivor: colours [own rgb | attention blend], alpha, and (backward) the pieces the chain rule needs
struct GrSample { float c[3]; float col[6]; float alpha; float raw; float z; uint32_t s; };

static __device__ inline void gr_sample(const GrComp& a, uint32_t r, uint64_t m, GrSample* o) {
    const float* n = a.net + m * a.ld;
    uint32_t s = (uint32_t)a.idx[m] - r * a.S;
    if (s >= a.S) s = a.S - 1;                                     // (an index of another ray: never taken with the hull's table)
    o->s = s;
#pragma unroll
    for (int k = 0; k < 3; ++k) o->c[k] = 1.f / (1.f + expf(-n[k]));
    o->raw = n[3] + (a.noise ? a.noise[(uint64_t)r * a.S + s] : 0.f);
    o->alpha = 1.f - expf(-(o->raw > 0.f ? o->raw : 0.f));
    const float* att = n + 4;
    const float* src = a.source_rgb + m * a.V * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o->col[k] = o->c[k];
        float b = o->c[k] * att[0];
        for (uint32_t v = 0; v < a.V; ++v) b += src[3 * v + k] * att[1 + v];
        o->col[3 + k] = b;
    }
    const float t = a.t_vals[(uint64_t)r * a.S + s];
    o->z = a.have_z ? t * a.z_near + (1.f - t) * a.z_far : 2.f * t - 1.f;
}

// the ray of this wave and its survivors [base, base + n)
static __device__ inline bool gr_ray(const GrComp& a, uint32_t* r, uint32_t* n, uint64_t* base) {
    *r = blockIdx.x * GR_WAVES + (threadIdx.x >> 6);
    if (*r >= a.R) return false;                                   // (the whole wave)
    *n = (uint32_t)a.table[2ull * *r];
    *base = (uint64_t)(uint32_t)a.table[2ull * *r + 1];
    if (*n > a.S) *n = a.S;
    if (*base + *n > a.M) *n = *base < a.M ? (uint32_t)(a.M - *base) : 0u;
    return true;
}

// wave = ray, lane = survivor, 64 at a time in sample order.  The transmittance in front of a lane is the carry of the chunks before
// times an exclusive product scan over the lanes (a fixed tree: the same bits every run; the factors of a ray are associated
// otherwise than by a serial cumprod, which the bars allow for).  weights was cleared by the entry point.
__global__ void __launch_bounds__(GR_BLOCK) k_gr_comp_fwd(GrComp a, float* __restrict__ rgb_map, float* __restrict__ depth,
                                                         float* __restrict__ acc, float* __restrict__ weights, float* __restrict__ trans) {
    uint32_t r, n; uint64_t base;
    if (!gr_ray(a, &r, &n, &base)) return;
    const uint32_t lane = threadIdx.x & 63;
    float carry = 1.f, sum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // 6 colours, depth, acc: per lane, folded at the end
    for (uint32_t c0 = 0; c0 < n; c0 += 64) {
        const uint32_t i = c0 + lane;
        const bool on = i < n;
        GrSample q;
        float f = 1.f;
        if (on) { gr_sample(a, r, base + i, &q); f = (1.f - q.alpha) + 1e-10f; }
        const float incl = xr_wave_incl_prod(f);
        const float T = carry * xr_wave_excl_of_prod(incl);
        if (on) {
            const float w = q.alpha * T;
            trans[base + i] = T;
            weights[(uint64_t)r * a.S + q.s] = w;
#pragma unroll
            for (int k = 0; k < 6; ++k) sum[k] += w * q.col[k];
            sum[6] += w * q.z;
            sum[7] += w;
        }
        carry = carry * __shfl(incl, 63, 64);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) sum[k] = xr_wave_sum(sum[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) rgb_map[6ull * r + k] = a.white ? sum[k] + (1.f - sum[7]) : sum[k];
        depth[r] = sum[6];
        acc[r] = sum[7];
    }
}

// the chunks from the last to the first; inside a chunk an inclusive suffix scan of the maps x -> g + f x (g = G alpha), so that
// C_i = g_i + f_i C_(i+1) and B_i = C_(i+1): d alpha_i = T_i (G_i - B_i), no division by a transmittance, no atomics
__global__ void __launch_bounds__(GR_BLOCK) k_gr_comp_bwd(GrComp a, const float* __restrict__ d_rgb, const float* __restrict__ trans,
                                                         float* __restrict__ d_net) {
    uint32_t r, n; uint64_t base;
    if (!gr_ray(a, &r, &n, &base)) return;
    if (n == 0) return;
    const uint32_t lane = threadIdx.x & 63;
    float g[6], g_all = 0.f;
#pragma unroll
    for (int k = 0; k < 6; ++k) { g[k] = d_rgb[6ull * r + k]; g_all += g[k]; }
    const uint32_t cols = 4 + a.V + 1;
    float carry = 0.f;
    for (uint32_t c0 = ((n - 1) / 64) * 64 + 64; c0 >= 64; c0 -= 64) {
        const uint32_t i = c0 - 64 + lane;
        const bool on = i < n;
        const uint64_t m = base + i;
        GrSample q;
        float G = 0.f, F = 1.f, Cv = 0.f, T = 0.f;
        if (on) {
            gr_sample(a, r, m, &q);
            T = trans[m];
#pragma unroll
            for (int k = 0; k < 6; ++k) G += g[k] * q.col[k];
            if (a.white) G -= g_all;
            F = (1.f - q.alpha) + 1e-10f;
            Cv = G * q.alpha;
        }
        const XrAffine<float> sc = xr_wave_affine_rscan(F, Cv);
        F = sc.F; Cv = sc.A;
        const float full = Cv + F * carry;
        float B = __shfl_down(full, 1, 64);
        if (lane == 63) B = carry;
        carry = __shfl(full, 0, 64);
        if (on) {
            const float w = q.alpha * T;
            float* o = d_net + m * cols;
            const float* att = a.net + m * a.ld + 4;
            const float* src = a.source_rgb + m * a.V * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = (w * (g[k] + att[0] * g[3 + k])) * (q.c[k] * (1.f - q.c[k]));
            const float d_alpha = T * (G - B);
            o[3] = q.raw > 0.f ? d_alpha * (1.f - q.alpha) : 0.f;
            o[4] = w * ((g[3] * q.c[0] + g[4] * q.c[1]) + g[5] * q.c[2]);
            for (uint32_t v = 0; v < a.V; ++v) o[5 + v] = w * ((g[3] * src[3 * v] + g[4] * src[3 * v + 1]) + g[5] * src[3 * v + 2]);
        }
    }
}

static int gr_comp_args(GrComp* a, const char* fn, const float* net, uint32_t ld, const float* source_rgb, const int32_t* idx,
                        const int32_t* table, const float* t_vals, const float* noise, uint32_t R, uint32_t S, uint32_t V, uint32_t M,
                        int have_z, float z_near, float z_far, int white) {
    if (!table || !t_vals || (M > 0 && (!net || !source_rgb || !idx))) { xr_set_error("%s: null pointer", fn); return XR_EINVAL; }
    if (V < 1 || V > GR_V) { xr_set_error("%s: 1 .. XR_GNR_MAX_VIEWS source views", fn); return XR_EINVAL; }
    if (ld < 4 + V + 1) { xr_set_error("%s: the row stride is smaller than rgb, density and attention", fn); return XR_EINVAL; }
    if (S < 1 || (uint64_t)R * S > (1ull << 30) || (uint64_t)M > (uint64_t)R * S) { xr_set_error("%s: bad ray, sample or survivor count", fn); return XR_EINVAL; }
    a->net = net; a->ld = ld; a->source_rgb = source_rgb; a->idx = idx; a->table = table; a->t_vals = t_vals; a->noise = noise;
    a->R = R; a->S = S; a->V = V; a->M = M; a->have_z = have_z ? 1 : 0; a->z_near = z_near; a->z_far = z_far; a->white = white ? 1 : 0;
    return 0;
}

extern "C" int xr_gnr_composite_forward(const float* net, uint32_t ld, const float* source_rgb, const int32_t* idx, const int32_t* table,
                                        const float* t_vals, const float* noise, uint32_t R, uint32_t S, uint32_t V, uint32_t M, int have_z,
                                        float z_near, float z_far, int white, float* rgb_map, float* depth, float* acc, float* weights,
                                        float* trans, void* stream) {
    if (R == 0) return 0;
    GrComp a;
    const int rc = gr_comp_args(&a, __func__, net, ld, source_rgb, idx, table, t_vals, noise, R, S, V, M, have_z, z_near, z_far, white);
    if (rc != 0) return rc;
    XR_REQUIRE(rgb_map && depth && acc && weights && (M == 0 || trans), "null pointer");
    XR_HIP(hipMemsetAsync(weights, 0, (size_t)R * S * sizeof(float), (hipStream_t)stream));
    hipLaunchKernelGGL(k_gr_comp_fwd, dim3(xr_div_up(R, GR_WAVES)), dim3(GR_BLOCK), 0, (hipStream_t)stream, a, rgb_map, depth, acc, weights, trans);
    XR_LAUNCH_CHECK();
    return 0;
}

extern "C" int xr_gnr_composite_backward(const float* net, uint32_t ld, const float* source_rgb, const int32_t* idx, const int32_t* table,
                                         const float* t_vals, const float* noise, uint32_t R, uint32_t S, uint32_t V, uint32_t M, int white,
                                         const float* d_rgb_map, const float* trans, float* d_net, void* stream) {
    if (R == 0 || M == 0) return 0;
    GrComp a;
    const int rc = gr_comp_args(&a, __func__, net, ld, source_rgb, idx, table, t_vals, noise, R, S, V, M, 0, 0.f, 0.f, white);
    if (rc != 0) return rc;
    XR_REQUIRE(d_rgb_map && trans && d_net, "null pointer");
    hipLaunchKernelGGL(k_gr_comp_bwd, dim3(xr_div_up(R, GR_WAVES)), dim3(GR_BLOCK), 0, (hipStream_t)stream, a, d_rgb_map, trans, d_net);
    XR_LAUNCH_CHECK();
    return 0;
}
