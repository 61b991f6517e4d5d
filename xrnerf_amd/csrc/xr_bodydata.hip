// ZJU-MoCap / H36M human data for gfx950: the frame store and the body-box ray sampler.  The reference reads,
// undistorts and resizes a picture and its mask, makes float64 rays for every pixel, fills six polygons, runs two argwheres and draws
// its rays in a rejection loop -- on the host, for every item.  Everything but the draw is a function of the picture alone:
//   k_body_prepare   thread = one output pixel: bytes / 255, undistortion (map in double, bilinear in fp32, zero border), the s x s block
//                    mean, the mask (nearest throughout) and the background.  Made once per picture
//   k_body_flags / k_body_lists   thread = one pixel: the box silhouette by exact int64 cross products over the reference's six vertex
//                    lists (even-odd interior plus on-edge), the two candidate lists by per-workgroup counts, xr_scan.h's two-level
//                    scan and a ranked write -- row-major order, the same integers on every launch.  Made once per picture
//   k_body_sample    ONE workgroup of 256 threads per training item, the rejection rounds inside: a slot's pixel from the draw table, its
//                    ray and box test in double in the reference's operation order, survivors appended in slot order
//                    (xr_block_excl_flag), outputs rounded to fp32 once.  Optionally z_vals and pts by the same workgroup
//   k_body_points    thread = one (ray, sample): z_vals, the perturbation and pts in un-fused fp32 with per-ray near / far
//   k_body_frame_count / k_body_frame_write   thread = one pixel of a test frame: ray in double rounded to fp32, box test in fp32 (the
//                    reference casts first), survivors compacted in row-major order
// No atomics, no scratch.  Reference lines:
//   xrnerf/datasets/pipelines/create.py:308-352,660-722   NBGetRays, LoadImageAndCamera
//   xrnerf/datasets/pipelines/augment.py:84-253           NBSelectRays (get_bound_2d_mask, get_near_far, sample_rays, select_all_rays)
//   create.py:502-531,586-600, augment.py:261-286         GetZvals, GetPts, PerturbZvals
// Built with -ffp-contract=off: nothing is fused, and the host build of this file (tests/hip_emu) produces the same bits.
#include "xr_common.h"
#define XR_SCAN_TWO_LEVEL
#include "xr_scan.h"
#include "xr_mip_math.h"      // xr_mip_zval: GetZvals' t and z, as xr_pipe_ray_front makes them
#include "../../include/xrnerf_mi355_bodydata.h"

#define BD_BLOCK 256
static_assert(BD_BLOCK == XR_SCAN_BLOCK, "the shared workgroup routines are written for 256 threads");

// ---------------------------------------------------------------------------------------------- the prepared picture
struct BdPrepArgs {
    const uint8_t *img8, *msk8;
    uint32_t Hs, Ws, Hm, Wm, s, H, W;
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
    int identity, white_bkgd;
    float* img;
    uint8_t* msk;
};

static __device__ inline bool bd_mask_src(const BdPrepArgs& a, uint32_t y, uint32_t x) {
    const uint32_t ym = (uint32_t)(((uint64_t)y * a.Hm) / a.Hs), xm = (uint32_t)(((uint64_t)x * a.Wm) / a.Ws);   // < Hm, < Wm
    return a.msk8[(size_t)ym * a.Wm + xm] != 0;
}

static __device__ inline float bd_src(const BdPrepArgs& a, long y, long x, uint32_t ch) {
    if (y < 0 || x < 0 || y >= (long)a.Hs || x >= (long)a.Ws) return 0.f;
    return (float)a.img8[((size_t)y * a.Ws + (size_t)x) * 3 + ch] / 255.f;
}

// the source position of destination (v, u): OpenCV's documented distortion model
static __device__ inline void bd_map(const BdPrepArgs& a, uint32_t v, uint32_t u, double* us, double* vs) {
    const double x = ((double)u - a.cx) / a.fx, y = ((double)v - a.cy) / a.fy;
    const double r2 = x * x + y * y;
    const double kr = 1.0 + ((a.k3 * r2 + a.k2) * r2 + a.k1) * r2;
    const double xd = (x * kr + a.p1 * (2.0 * x * y)) + a.p2 * (r2 + 2.0 * x * x);
    const double yd = (y * kr + a.p1 * (r2 + 2.0 * y * y)) + a.p2 * (2.0 * x * y);
    *us = a.fx * xd + a.cx;
    *vs = a.fy * yd + a.cy;
}

static __global__ void __launch_bounds__(BD_BLOCK) k_body_prepare(BdPrepArgs a) {
    const size_t pix = (size_t)blockIdx.x * BD_BLOCK + threadIdx.x;
    if (pix >= (size_t)a.H * a.W) return;
    const uint32_t Y = (uint32_t)(pix / a.W), X = (uint32_t)(pix - (size_t)Y * a.W);
    float acc[3] = {0.f, 0.f, 0.f};
    bool m = false;
    for (uint32_t dy = 0; dy < a.s; ++dy)
        for (uint32_t dx = 0; dx < a.s; ++dx) {
            const uint32_t v = Y * a.s + dy, u = X * a.s + dx;               // < Hs, < Ws
            float p[3];
            bool mk;
            if (a.identity) {
                for (uint32_t ch = 0; ch < 3; ++ch) p[ch] = bd_src(a, v, u, ch);
                mk = bd_mask_src(a, v, u);
            } else {
                double us, vs;
                bd_map(a, v, u, &us, &vs);
                // a position outside (-2, size + 1) samples the border only; the test also catches NaN before any conversion to integer
                const bool near_image = us > -2.0 && us < (double)a.Ws + 1.0 && vs > -2.0 && vs < (double)a.Hs + 1.0;
                if (near_image) {
                    const double fx0 = floor(us), fy0 = floor(vs);
                    const long x0 = (long)fx0, y0 = (long)fy0;
                    const float ax = (float)(us - fx0), ay = (float)(vs - fy0);
                    for (uint32_t ch = 0; ch < 3; ++ch) {
                        const float top = bd_src(a, y0, x0, ch) * (1.f - ax) + bd_src(a, y0, x0 + 1, ch) * ax;
                        const float bot = bd_src(a, y0 + 1, x0, ch) * (1.f - ax) + bd_src(a, y0 + 1, x0 + 1, ch) * ax;
                        p[ch] = top * (1.f - ay) + bot * ay;
                    }
                    const long xn = (long)floor(us + 0.5), yn = (long)floor(vs + 0.5);
                    mk = xn >= 0 && yn >= 0 && xn < (long)a.Ws && yn < (long)a.Hs && bd_mask_src(a, (uint32_t)yn, (uint32_t)xn);
                } else {
                    p[0] = p[1] = p[2] = 0.f;
                    mk = false;
                }
            }
            const bool first = dy == 0 && dx == 0;
            for (uint32_t ch = 0; ch < 3; ++ch) acc[ch] = first ? p[ch] : acc[ch] + p[ch];
            if (first) m = mk;
        }
    const float div = (float)(a.s * a.s), bg = a.white_bkgd ? 1.f : 0.f;
    for (uint32_t ch = 0; ch < 3; ++ch) a.img[pix * 3 + ch] = m ? (a.s == 1 ? acc[ch] : acc[ch] / div) : bg;
    a.msk[pix] = m ? 1 : 0;
}

extern "C" int xr_body_prepare(const uint8_t* img8, const uint8_t* msk8, uint32_t Hs, uint32_t Ws, uint32_t Hm, uint32_t Wm, const double* kd, uint32_t s,
                               int white_bkgd, float* img, uint8_t* msk, void* stream) {
    XR_REQUIRE(img8 && msk8 && kd && img && msk, "null pointer");
    XR_REQUIRE(Hs >= 1 && Ws >= 1 && Hm >= 1 && Wm >= 1 && (uint64_t)Hs * Ws <= 0x7fffffffull && (uint64_t)Hm * Wm <= 0x7fffffffull, "sizes of 0 or beyond int32");
    XR_REQUIRE(s >= 1 && s <= XR_BODY_MAX_SHRINK && Hs % s == 0 && Ws % s == 0, "the shrink must be 1 .. XR_BODY_MAX_SHRINK and divide Hs and Ws");
    XR_REQUIRE(kd[0] != 0.0 && kd[4] != 0.0 && kd[0] - kd[0] == 0.0 && kd[4] - kd[4] == 0.0, "fx and fy must be finite and not 0");
    BdPrepArgs a;
    a.img8 = img8; a.msk8 = msk8; a.Hs = Hs; a.Ws = Ws; a.Hm = Hm; a.Wm = Wm; a.s = s; a.H = Hs / s; a.W = Ws / s;
    a.fx = kd[0]; a.fy = kd[4]; a.cx = kd[2]; a.cy = kd[5];
    a.k1 = kd[9]; a.k2 = kd[10]; a.p1 = kd[11]; a.p2 = kd[12]; a.k3 = kd[13];
    a.identity = a.k1 == 0.0 && a.k2 == 0.0 && a.p1 == 0.0 && a.p2 == 0.0 && a.k3 == 0.0;
    a.white_bkgd = white_bkgd; a.img = img; a.msk = msk;
    const uint32_t blocks = xr_div_up((uint64_t)a.H * a.W, BD_BLOCK);
    hipLaunchKernelGGL(k_body_prepare, dim3(blocks), dim3(BD_BLOCK), 0, (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- the silhouette and the candidate lists
struct BdPoly { int32_t cx[8], cy[8]; };
// augment.py:126-131, verbatim: the second list closes on 5, not on 4 (under even-odd that face is the triangle 5 7 6 plus the segment 4 5).
// Three bits per vertex, so that every corner index is a constant after inlining (the corners stay in the kernel's argument registers)
#define BD_FACE(a, b, c, d, e) ((uint32_t)(a) | ((uint32_t)(b) << 3) | ((uint32_t)(c) << 6) | ((uint32_t)(d) << 9) | ((uint32_t)(e) << 12))

// (x, y) belongs to the closed polygon v[0..4] (five edges, the last from v[4] back to v[0]): on an edge, or interior by even-odd
static __device__ __forceinline__ bool bd_in_polygon(const BdPoly& c, const uint32_t face, int64_t x, int64_t y) {
    bool inside = false, on_edge = false;
#pragma unroll
    for (int e = 0; e < 5; ++e) {
        const uint32_t i = (face >> (3 * e)) & 7u, j = (face >> (3 * (e == 4 ? 0 : e + 1))) & 7u;
        const int64_t ax = c.cx[i], ay = c.cy[i], bx = c.cx[j], by = c.cy[j];
        const int64_t cross = (bx - ax) * (y - ay) - (x - ax) * (by - ay);
        if (cross == 0 && x >= (ax < bx ? ax : bx) && x <= (ax < bx ? bx : ax) && y >= (ay < by ? ay : by) && y <= (ay < by ? by : ay)) on_edge = true;
        if ((ay > y) != (by > y) && ((cross > 0) == (by > ay))) inside = !inside;       // the edge crosses the pixel's row right of it
    }
    return inside || on_edge;
}

static __device__ inline bool bd_in_bound(const BdPoly& c, int64_t x, int64_t y) {
    return bd_in_polygon(c, BD_FACE(0, 1, 3, 2, 0), x, y) || bd_in_polygon(c, BD_FACE(4, 5, 7, 6, 5), x, y) || bd_in_polygon(c, BD_FACE(0, 1, 5, 4, 0), x, y) ||
           bd_in_polygon(c, BD_FACE(2, 3, 7, 6, 2), x, y) || bd_in_polygon(c, BD_FACE(0, 2, 6, 4, 0), x, y) || bd_in_polygon(c, BD_FACE(1, 3, 7, 5, 1), x, y);
}

// flags[pix]: bit 0 = bound mask, bit 1 = body (bound and msk); the workgroup's two counts
static __global__ void __launch_bounds__(BD_BLOCK) k_body_flags(BdPoly c, const uint8_t* __restrict__ msk, uint32_t W, uint32_t n, uint8_t* __restrict__ flags,
                                                                uint32_t* __restrict__ cnt_bound, uint32_t* __restrict__ cnt_body) {
    const uint32_t pix = blockIdx.x * BD_BLOCK + threadIdx.x;
    bool fb = false, fh = false;
    if (pix < n) {
        const uint32_t row = pix / W, col = pix - row * W;
        fb = bd_in_bound(c, (int64_t)col, (int64_t)row);
        fh = fb && msk[pix] != 0;
        flags[pix] = (uint8_t)((fb ? 1 : 0) | (fh ? 2 : 0));
    }
    uint32_t sb, sh;
    xr_block_excl_flag(fb, &sb);
    xr_block_excl_flag(fh, &sh);
    if (threadIdx.x == 0) { cnt_bound[blockIdx.x] = sb; cnt_body[blockIdx.x] = sh; }
}

static __global__ void __launch_bounds__(BD_BLOCK) k_body_lists(const uint8_t* __restrict__ flags, uint32_t n, const uint32_t* __restrict__ base_bound,
                                                                const uint32_t* __restrict__ base_body, const int32_t* __restrict__ totals,
                                                                int32_t* __restrict__ bound_list, int32_t* __restrict__ body_list) {
    const uint32_t pix = blockIdx.x * BD_BLOCK + threadIdx.x;
    const uint8_t f = pix < n ? flags[pix] : 0;
    uint32_t sum;
    const uint32_t rb = xr_block_excl_flag((f & 1) != 0, &sum);
    const uint32_t rh = xr_block_excl_flag((f & 2) != 0, &sum);
    // a rank is below its list's total, and a total within int32 is at most n: the write stays inside the n entries of the list
    if ((f & 1) && totals[0] >= 0) bound_list[base_bound[blockIdx.x] + rb] = (int32_t)pix;
    if ((f & 2) && totals[1] >= 0) body_list[base_body[blockIdx.x] + rh] = (int32_t)pix;
}

// workspace: flags [n] bytes padded to 4, then per list: counts [nb], sums [div_up(nb, 256)]
static size_t bd_masks_ws(uint64_t n, uint32_t* nb_out, uint32_t* n2_out, size_t* flag_bytes) {
    const uint32_t nb = xr_div_up(n, BD_BLOCK), n2 = xr_div_up(nb, BD_BLOCK);
    *nb_out = nb; *n2_out = n2; *flag_bytes = (size_t)((n + 3) & ~3ull);
    return *flag_bytes + 2 * (size_t)(nb + n2) * sizeof(uint32_t);
}

extern "C" size_t xr_body_masks_workspace_bytes(uint32_t H, uint32_t W) {
    uint32_t nb, n2; size_t fbytes;
    return bd_masks_ws((uint64_t)H * W, &nb, &n2, &fbytes);
}

extern "C" int xr_body_masks(const uint8_t* msk, uint32_t H, uint32_t W, const int32_t* corners8, int32_t* bound_list, int32_t* body_list, int32_t* totals,
                             void* workspace, size_t workspace_bytes, void* stream) {
    XR_REQUIRE(msk && corners8 && bound_list && body_list && totals && workspace, "null pointer");
    XR_REQUIRE(H >= 1 && W >= 1 && (uint64_t)H * W <= 0x7fffffffull, "H, W >= 1 and H W within int32");
    XR_REQUIRE(((uintptr_t)workspace & 3u) == 0, "the workspace must be 4-byte aligned");
    BdPoly c;
    for (int i = 0; i < 8; ++i) {
        c.cx[i] = corners8[2 * i]; c.cy[i] = corners8[2 * i + 1];
        XR_REQUIRE(c.cx[i] >= -(1 << 30) && c.cx[i] <= (1 << 30) && c.cy[i] >= -(1 << 30) && c.cy[i] <= (1 << 30), "a corner beyond +-2^30");
    }
    const uint32_t n = H * W;
    uint32_t nb, n2; size_t fbytes;
    if (workspace_bytes < bd_masks_ws(n, &nb, &n2, &fbytes)) { xr_set_error("%s: workspace too small", __func__); return XR_ENOMEM; }
    uint8_t* flags = (uint8_t*)workspace;
    uint32_t* cb = (uint32_t*)(flags + fbytes);
    uint32_t* sb = cb + nb;
    uint32_t* ch = sb + n2;
    uint32_t* sh = ch + nb;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_body_flags, dim3(nb), dim3(BD_BLOCK), 0, st, c, msk, W, n, flags, cb, ch);
    xr_scan_two_level(st, nb, cb, sb, totals);
    xr_scan_two_level(st, nb, ch, sh, totals + 1);
    hipLaunchKernelGGL(k_body_lists, dim3(nb), dim3(BD_BLOCK), 0, st, (const uint8_t*)flags, n, (const uint32_t*)cb, (const uint32_t*)ch,
                       (const int32_t*)totals, bound_list, body_list);
    XR_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- rays and the box
static __device__ inline double bd_sqrt(double x) { return sqrt(x); }
static __device__ inline float bd_sqrt(float x) { return sqrtf(x); }

// NBGetRays for pixel (row, col): create.py:332-343 (np.arange is float32, exact; 1 * Ki[r][2] is Ki[r][2])
static __device__ inline void bd_ray(const double* c, uint32_t row, uint32_t col, double d[3]) {
    const double x = (double)col, y = (double)row;
    double pc[3];
    for (int r = 0; r < 3; ++r) pc[r] = ((x * c[3 * r] + y * c[3 * r + 1]) + c[3 * r + 2]) - c[18 + r];
    for (int k = 0; k < 3; ++k) d[k] = ((pc[0] * c[9 + k] + pc[1] * c[12 + k]) + pc[2] * c[15 + k]) - c[21 + k];
    const double n = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    for (int k = 0; k < 3; ++k) d[k] = d[k] / n;
}

// get_near_far (augment.py:135-150) in T; false when the ray misses the box
template <class T> static __device__ inline bool bd_box(const T bmin[3], const T bmax[3], const T o[3], const T d[3], T* near, T* far) {
    const T nd = bd_sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    T nr = 0, fr = 0;
    for (int k = 0; k < 3; ++k) {
        T v = d[k] / nd;
        if (v < (T)1e-5 && v > (T)-1e-10) v = (T)1e-5;
        if (v > (T)-1e-5 && v < (T)1e-10) v = (T)-1e-5;
        const T tmin = (bmin[k] - o[k]) / v, tmax = (bmax[k] - o[k]) / v;
        const T t1 = tmin < tmax ? tmin : tmax, t2 = tmin < tmax ? tmax : tmin;
        nr = k == 0 ? t1 : (t1 > nr ? t1 : nr);
        fr = k == 0 ? t2 : (t2 < fr ? t2 : fr);
    }
    *near = nr / nd;
    *far = fr / nd;
    return nr < fr;
}

// one (ray, sample) item of GetZvals / PerturbZvals / GetPts with per-ray near and far
static __device__ inline void bd_point(const float* rays_o, const float* rays_d, const float* near_in, const float* far_in, uint32_t S, const float* t_rand,
                                       size_t item, float* z_vals, float* pts) {
    const size_t r = item / S;
    const uint32_t k = (uint32_t)(item - r * S);
    const float near = near_in[r], far = far_in[r];
    float z = xr_mip_zval(near, far, S, k, 0);
    if (t_rand) {
        const float lower = k == 0 ? z : .5f * (z + xr_mip_zval(near, far, S, k - 1, 0));
        const float upper = k + 1 == S ? z : .5f * (xr_mip_zval(near, far, S, k + 1, 0) + z);
        z = lower + (upper - lower) * t_rand[item];
    }
    if (z_vals) z_vals[item] = z;
    if (pts)
        for (int i = 0; i < 3; ++i) pts[item * 3 + i] = rays_o[r * 3 + i] + rays_d[r * 3 + i] * z;
}

static __global__ void __launch_bounds__(BD_BLOCK) k_body_points(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                                 const float* __restrict__ near_in, const float* __restrict__ far_in, uint64_t R, uint32_t S,
                                                                 const float* __restrict__ t_rand, float* __restrict__ z_vals, float* __restrict__ pts) {
    const size_t item = (size_t)blockIdx.x * BD_BLOCK + threadIdx.x;
    if (item >= (size_t)R * S) return;
    bd_point(rays_o, rays_d, near_in, far_in, S, t_rand, item, z_vals, pts);
}

extern "C" int xr_body_points(const float* rays_o, const float* rays_d, const float* near_in, const float* far_in, uint64_t R, uint32_t S, const float* t_rand,
                              float* z_vals, float* pts, void* stream) {
    XR_REQUIRE(rays_o && rays_d && near_in && far_in, "null input");
    XR_REQUIRE(S >= 1 && (z_vals || pts), "S >= 1 and at least one output");
    XR_REQUIRE(R <= (0x7fffffffull * BD_BLOCK) / S, "more than 2^31 - 1 workgroups");
    if (R == 0) return 0;
    const uint32_t blocks = (uint32_t)((R * S + BD_BLOCK - 1) / BD_BLOCK);
    hipLaunchKernelGGL(k_body_points, dim3(blocks), dim3(BD_BLOCK), 0, (hipStream_t)stream, rays_o, rays_d, near_in, far_in, R, S, t_rand, z_vals, pts);
    XR_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- the training item
struct BdSampleArgs {
    const double* cam;
    const float *img, *t_rand;
    const int32_t *body_list, *bound_list;
    const int64_t* draws;
    uint32_t H, W, len_body, len_bound, sel_n, S;
    float *rays_o, *rays_d, *near_out, *far_out, *target_s, *z_vals, *pts;
    uint32_t* short_items;
};

static __global__ void __launch_bounds__(BD_BLOCK) k_body_sample(BdSampleArgs a) {
    double c[XR_BODY_CAM_DOUBLES];
    for (uint32_t i = 0; i < XR_BODY_CAM_DOUBLES; ++i) c[i] = a.cam[i];
    const uint32_t n_pix = a.H * a.W;
    uint32_t count = 0;                                            // survivors so far: the same in every thread
    for (uint32_t round = 0; round < XR_BODY_ROUNDS && count < a.sel_n; ++round) {
        const uint32_t rem = a.sel_n - count, n_body = rem / 2;    // augment.py:162-163
        for (uint32_t base = 0; base < rem; base += BD_BLOCK) {
            const uint32_t slot = base + threadIdx.x;
            bool hit = false;
            double d[3], near = 0, far = 0;
            uint32_t pix = 0;
            if (slot < rem) {
                const int64_t draw = a.draws[(size_t)round * a.sel_n + slot];
                const bool body = slot < n_body;
                const int64_t len = (int64_t)(body ? a.len_body : a.len_bound);
                int64_t e = draw % len;
                if (e < 0) e += len;                               // 0 <= e < len
                const int32_t p = (body ? a.body_list : a.bound_list)[e];
                if (p >= 0 && (uint32_t)p < n_pix) {               // a list entry outside the picture is never followed
                    pix = (uint32_t)p;
                    const uint32_t row = pix / a.W, col = pix - row * a.W;
                    bd_ray(c, row, col, d);
                    hit = bd_box<double>(c + 24, c + 27, c + 21, d, &near, &far);
                }
            }
            uint32_t sum;
            const uint32_t at = count + xr_block_excl_flag(hit, &sum);      // < count + rem <= sel_n
            if (hit) {
                for (int k = 0; k < 3; ++k) {
                    a.rays_o[(size_t)at * 3 + k] = (float)c[21 + k];
                    a.rays_d[(size_t)at * 3 + k] = (float)d[k];
                    if (a.target_s) a.target_s[(size_t)at * 3 + k] = a.img[(size_t)pix * 3 + k];
                }
                a.near_out[at] = (float)near;
                a.far_out[at] = (float)far;
            }
            count += sum;
        }
    }
    if (count < a.sel_n) {                                         // the item ran short: a NaN tail, and the persistent counter
        for (uint32_t i = count + threadIdx.x; i < a.sel_n; i += BD_BLOCK) {
            for (int k = 0; k < 3; ++k) {
                a.rays_o[(size_t)i * 3 + k] = NAN;
                a.rays_d[(size_t)i * 3 + k] = NAN;
                if (a.target_s) a.target_s[(size_t)i * 3 + k] = NAN;
            }
            a.near_out[i] = NAN;
            a.far_out[i] = NAN;
        }
        if (threadIdx.x == 0) a.short_items[0] = a.short_items[0] + 1u;
    }
    if (a.S == 0 || !(a.z_vals || a.pts)) return;
    __threadfence_block();
    __syncthreads();                                               // this workgroup's rays are in memory for all of its threads
    const size_t items = (size_t)a.sel_n * a.S;
    for (size_t item = threadIdx.x; item < items; item += BD_BLOCK)
        bd_point(a.rays_o, a.rays_d, a.near_out, a.far_out, a.S, a.t_rand, item, a.z_vals, a.pts);
}

extern "C" int xr_body_sample(const double* cam, uint32_t H, uint32_t W, const float* img, const int32_t* body_list, uint32_t len_body,
                              const int32_t* bound_list, uint32_t len_bound, const int64_t* draws, uint32_t sel_n, uint32_t S, const float* t_rand,
                              float* rays_o, float* rays_d, float* near_out, float* far_out, float* target_s, float* z_vals, float* pts,
                              uint32_t* short_items, void* stream) {
    XR_REQUIRE(cam && body_list && bound_list && draws && rays_o && rays_d && near_out && far_out && short_items, "null pointer");
    XR_REQUIRE(H >= 1 && W >= 1 && (uint64_t)H * W <= 0x7fffffffull, "H, W >= 1 and H W within int32");
    XR_REQUIRE(len_body >= 1 && len_bound >= 1 && len_body <= (uint64_t)H * W && len_bound <= (uint64_t)H * W, "an empty candidate list, or one longer than H W");
    XR_REQUIRE(sel_n >= 1 && sel_n <= XR_BODY_MAX_SEL, "sel_n must be 1 .. XR_BODY_MAX_SEL");
    XR_REQUIRE(!target_s || img, "target_s needs the prepared image");
    XR_REQUIRE(S >= 1 || (!z_vals && !pts && !t_rand), "z_vals, pts and t_rand need S >= 1");
    BdSampleArgs a;
    a.cam = cam; a.img = img; a.t_rand = t_rand; a.body_list = body_list; a.bound_list = bound_list; a.draws = draws;
    a.H = H; a.W = W; a.len_body = len_body; a.len_bound = len_bound; a.sel_n = sel_n; a.S = S;
    a.rays_o = rays_o; a.rays_d = rays_d; a.near_out = near_out; a.far_out = far_out; a.target_s = target_s; a.z_vals = z_vals; a.pts = pts;
    a.short_items = short_items;
    hipLaunchKernelGGL(k_body_sample, dim3(1), dim3(BD_BLOCK), 0, (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- the whole frame
// select_all_rays (augment.py:199-221): rays_o and rays_d are cast to fp32 BEFORE get_near_far, which then runs in fp32
static __device__ inline bool bd_frame_ray(const double* c, uint32_t W, uint32_t pix, float o[3], float d[3], float* near, float* far) {
    const uint32_t row = pix / W, col = pix - row * W;
    double dd[3];
    bd_ray(c, row, col, dd);
    float bmin[3], bmax[3];
    for (int k = 0; k < 3; ++k) { o[k] = (float)c[21 + k]; d[k] = (float)dd[k]; bmin[k] = (float)c[24 + k]; bmax[k] = (float)c[27 + k]; }
    return bd_box<float>(bmin, bmax, o, d, near, far);
}

static __global__ void __launch_bounds__(BD_BLOCK) k_body_frame_count(const double* __restrict__ cam, uint32_t W, uint32_t n, uint8_t* __restrict__ mask_at_box,
                                                                      uint32_t* __restrict__ counts) {
    double c[XR_BODY_CAM_DOUBLES];
    for (uint32_t i = 0; i < XR_BODY_CAM_DOUBLES; ++i) c[i] = cam[i];
    const uint32_t pix = blockIdx.x * BD_BLOCK + threadIdx.x;
    bool hit = false;
    if (pix < n) {
        float o[3], d[3], near, far;
        hit = bd_frame_ray(c, W, pix, o, d, &near, &far);
        mask_at_box[pix] = hit ? 1 : 0;
    }
    uint32_t sum;
    xr_block_excl_flag(hit, &sum);
    if (threadIdx.x == 0) counts[blockIdx.x] = sum;
}

static __global__ void __launch_bounds__(BD_BLOCK) k_body_frame_write(const double* __restrict__ cam, uint32_t W, uint32_t n, const float* __restrict__ img,
                                                                      const uint8_t* __restrict__ mask_at_box, const uint32_t* __restrict__ bases, uint32_t M,
                                                                      float* __restrict__ rays_o, float* __restrict__ rays_d, float* __restrict__ near_out,
                                                                      float* __restrict__ far_out, float* __restrict__ target_s) {
    double c[XR_BODY_CAM_DOUBLES];
    for (uint32_t i = 0; i < XR_BODY_CAM_DOUBLES; ++i) c[i] = cam[i];
    const uint32_t pix = blockIdx.x * BD_BLOCK + threadIdx.x;
    const bool hit = pix < n && mask_at_box[pix] != 0;
    uint32_t sum;
    const uint32_t rank = xr_block_excl_flag(hit, &sum);
    if (!hit) return;
    const size_t at = (size_t)bases[blockIdx.x] + rank;
    if (at >= M) return;                                           // (the caller's M is the count's total: never taken)
    float o[3], d[3], near, far;
    bd_frame_ray(c, W, pix, o, d, &near, &far);
    for (int k = 0; k < 3; ++k) {
        rays_o[at * 3 + k] = o[k];
        rays_d[at * 3 + k] = d[k];
        if (target_s) target_s[at * 3 + k] = img[(size_t)pix * 3 + k];
    }
    near_out[at] = near;
    far_out[at] = far;
}

extern "C" size_t xr_body_frame_workspace_bytes(uint32_t H, uint32_t W) {
    const uint32_t nb = xr_div_up((uint64_t)H * W, BD_BLOCK);
    return (size_t)(nb + xr_div_up(nb, BD_BLOCK)) * sizeof(uint32_t);
}

extern "C" int xr_body_frame_count(const double* cam, uint32_t H, uint32_t W, uint8_t* mask_at_box, int32_t* total, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    XR_REQUIRE(cam && mask_at_box && total && workspace, "null pointer");
    XR_REQUIRE(H >= 1 && W >= 1 && (uint64_t)H * W <= 0x7fffffffull, "H, W >= 1 and H W within int32");
    XR_REQUIRE(((uintptr_t)workspace & 3u) == 0, "the workspace must be 4-byte aligned");
    if (workspace_bytes < xr_body_frame_workspace_bytes(H, W)) { xr_set_error("%s: workspace too small", __func__); return XR_ENOMEM; }
    const uint32_t n = H * W, nb = xr_div_up(n, BD_BLOCK);
    uint32_t* counts = (uint32_t*)workspace;
    hipLaunchKernelGGL(k_body_frame_count, dim3(nb), dim3(BD_BLOCK), 0, (hipStream_t)stream, cam, W, n, mask_at_box, counts);
    xr_scan_two_level((hipStream_t)stream, nb, counts, counts + nb, total);
    XR_LAUNCH_CHECK();
    return 0;
}

extern "C" int xr_body_frame_write(const double* cam, uint32_t H, uint32_t W, const float* img, const uint8_t* mask_at_box, const void* workspace,
                                   size_t workspace_bytes, uint32_t M, float* rays_o, float* rays_d, float* near_out, float* far_out, float* target_s,
                                   void* stream) {
    XR_REQUIRE(cam && mask_at_box && workspace, "null pointer");
    XR_REQUIRE(H >= 1 && W >= 1 && (uint64_t)H * W <= 0x7fffffffull && M <= (uint64_t)H * W, "H, W >= 1, H W within int32, M <= H W");
    XR_REQUIRE(((uintptr_t)workspace & 3u) == 0, "the workspace must be 4-byte aligned");
    XR_REQUIRE(!target_s || img, "target_s needs the prepared image");
    if (workspace_bytes < xr_body_frame_workspace_bytes(H, W)) { xr_set_error("%s: workspace too small", __func__); return XR_ENOMEM; }
    if (M == 0) return 0;
    XR_REQUIRE(rays_o && rays_d && near_out && far_out, "null output");
    const uint32_t n = H * W, nb = xr_div_up(n, BD_BLOCK);
    hipLaunchKernelGGL(k_body_frame_write, dim3(nb), dim3(BD_BLOCK), 0, (hipStream_t)stream, cam, W, n, img, mask_at_box, (const uint32_t*)workspace, M,
                       rays_o, rays_d, near_out, far_out, target_s);
    XR_LAUNCH_CHECK();
    return 0;
}
