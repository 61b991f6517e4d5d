// Mip-NeRF multiscale data for gfx950: the rays of the drawn pixels of a multi-camera, multi-resolution image set
// in one launch, and the converter's box pyramid.  The reference materialises seven per-ray float64 arrays for every pixel of every
// image at every scale, flattens them into fp32 tables (16 floats per ray) and indexes the tables; fifteen of the sixteen floats are a
// function of the image's 3x3 and 3x4 matrices, three scalars and the pixel's position.  Here the images and a camera table stay
// resident and an item makes the rays it drew:
//   k_ms_rays     thread = one (ray, sample) item of the flat R x max(S, 1) range, 256-thread workgroups.  A map: no scan, no atomics,
//                 no LDS.  Every thread finds its ray's image (binary search of the int64 prefix, <= 20 steps) for near / far and makes
//                 z[k-1], z[k], z[k+1] from the linspace formula in fp32; the thread with k == 0 does the ray's double arithmetic and
//                 writes the per-ray outputs, each rounded to fp32 once.  All index arithmetic is 64-bit.
//   k_ms_pyramid  thread = one pixel of one level of one view, in packed order.  Level j's float is down2 of level j-1's FLOAT, so a
//                 level-j pixel is re-derived from its 4^j base bytes by j nested 4-iteration loops (one template instance per level,
//                 one running sum per loop: registers only).  Every level reads the base once: n_down reads of the bytes in all.
// Reference lines:
//   xrnerf/datasets/load_data/get_rays.py:101-153   load_rays_multiscale        xrnerf/datasets/utils/flatten.py:5-9   flatten
//   xrnerf/datasets/pipelines/create.py:59-75       MipMultiScaleSample          create.py:508-530                       GetZvals
//   tools/convert_blender_data.py:43-45,73-89       down2, np.uint8(img * 255)   xrnerf/datasets/load_data/load_multiscale.py:15-22
// Built with -ffp-contract=off: nothing is fused, and the host build of this file (tests/hip_emu) produces the same bits.
#include "xr_common.h"
#include "xr_mip_math.h"      // xr_mip_zval: GetZvals' t and z, as xr_pipe_ray_front makes them
#include "../../include/xrnerf_mi355_multiscale.h"

#define MS_BLOCK 256

struct MsRayArgs {
    const double* cams;
    const int32_t* hw;
    const int64_t *prefix, *idx;
    const float *images, *t_rand;
    uint32_t n_images, image, S, Sd;
    uint64_t total, first_pixel, R;
    int lindisp;
    float *rays_o, *rays_d, *viewdirs, *radii, *lossmult, *near_out, *far_out, *z_vals, *target_s;
};

// d of pixel (row, col): get_rays.py:115-117, a 3-term dot product added in index order, twice
static __device__ inline void ms_dir(const double* P, const double* C, uint32_t row, uint32_t col, double d[3]) {
    const double x = (double)col + 0.5, y = (double)row + 0.5;
    double cam[3];
    for (int r = 0; r < 3; ++r) cam[r] = (x * P[3 * r] + y * P[3 * r + 1]) + P[3 * r + 2];
    for (int r = 0; r < 3; ++r) d[r] = (cam[0] * C[4 * r] + cam[1] * C[4 * r + 1]) + cam[2] * C[4 * r + 2];
}

static __global__ void __launch_bounds__(MS_BLOCK) k_ms_rays(MsRayArgs a) {
    const size_t item = (size_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (item >= (size_t)a.R * a.Sd) return;
    const size_t r = item / a.Sd;
    const uint32_t k = (uint32_t)(item - r * a.Sd);
    // the ray's image and its pixel
    uint32_t img = a.image;
    uint64_t pix = a.first_pixel + r, flat = 0;
    bool valid = true;
    if (a.idx) {
        const int64_t f = a.idx[r];
        valid = f >= 0 && (uint64_t)f < a.total;
        if (valid) {                                               // the last image whose prefix is <= f
            uint32_t lo = 0, hi = a.n_images;                      // prefix[lo] <= f < prefix[hi]
            while (hi - lo > 1) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (a.prefix[mid] <= f) lo = mid; else hi = mid;
            }
            img = lo;
            pix = (uint64_t)f - (uint64_t)a.prefix[lo];
        }
    }
    uint32_t H = 0, W = 1;
    if (valid) {
        H = (uint32_t)a.hw[2 * img];
        W = (uint32_t)a.hw[2 * img + 1];
        valid = W >= 1 && pix < (uint64_t)H * W;
        flat = (uint64_t)a.prefix[img] + pix;
        valid = valid && flat < a.total;
    }
    const double* cam = a.cams + (size_t)(valid ? img : 0) * XR_MS_CAM_DOUBLES;
    const float lossmult = valid ? (float)cam[21] : NAN, near = valid ? (float)cam[22] : NAN, far = valid ? (float)cam[23] : NAN;
    if (k == 0) {
        float o[3] = {NAN, NAN, NAN}, d[3] = {NAN, NAN, NAN}, v[3] = {NAN, NAN, NAN}, radius = NAN, rgb[3] = {NAN, NAN, NAN};
        if (valid) {
            const uint32_t row = (uint32_t)(pix / W), col = (uint32_t)(pix - (uint64_t)row * W);
            double P[9], C[12], dd[3];
            for (int i = 0; i < 9; ++i) P[i] = cam[i];
            for (int i = 0; i < 12; ++i) C[i] = cam[9 + i];
            ms_dir(P, C, row, col, dd);
            const double n = sqrt((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]);      // np.linalg.norm over 3 elements
            for (int i = 0; i < 3; ++i) { o[i] = (float)C[4 * i + 3]; d[i] = (float)dd[i]; v[i] = (float)(dd[i] / n); }
            if (a.radii && H >= 3) {                               // get_rays.py:137-144
                const uint32_t rp = row + 1 < H ? row : H - 3;     // np.concatenate([dx, dx[-2:-1]]): the last row repeats dx[H - 3]
                double da[3], db[3], sq[3];
                ms_dir(P, C, rp, col, da);
                ms_dir(P, C, rp + 1, col, db);
                for (int i = 0; i < 3; ++i) { const double e = da[i] - db[i]; sq[i] = e * e; }
                radius = (float)((sqrt((sq[0] + sq[1]) + sq[2]) * 2.0) / sqrt(12.0));
            }
            if (a.target_s)
                for (int c = 0; c < 3; ++c) rgb[c] = a.images[flat * 3 + c];
        }
        for (int i = 0; i < 3; ++i) {
            if (a.rays_o) a.rays_o[r * 3 + i] = o[i];
            if (a.rays_d) a.rays_d[r * 3 + i] = d[i];
            if (a.viewdirs) a.viewdirs[r * 3 + i] = v[i];
            if (a.target_s) a.target_s[r * 3 + i] = rgb[i];
        }
        if (a.radii) a.radii[r] = radius;
        if (a.lossmult) a.lossmult[r] = lossmult;
        if (a.near_out) a.near_out[r] = near;
        if (a.far_out) a.far_out[r] = far;
    }
    if (a.S == 0 || !a.z_vals) return;
    float z = xr_mip_zval(near, far, a.S, k, a.lindisp);             // create.py:510-516
    if (a.t_rand) {                                                 // create.py:518-525
        const float lower = k == 0 ? z : .5f * (z + xr_mip_zval(near, far, a.S, k - 1, a.lindisp));
        const float upper = k + 1 == a.S ? z : .5f * (xr_mip_zval(near, far, a.S, k + 1, a.lindisp) + z);
        z = lower + (upper - lower) * a.t_rand[item];
    }
    a.z_vals[item] = z;
}

extern "C" int xr_ms_rays(const double* cams, const int32_t* hw, const int64_t* prefix, uint32_t n_images, uint64_t total, const float* images,
                          const int64_t* idx, uint32_t image, uint64_t first_pixel, uint64_t R, uint32_t S, int lindisp, const float* t_rand,
                          float* rays_o, float* rays_d, float* viewdirs, float* radii, float* lossmult, float* near_out, float* far_out,
                          float* z_vals, float* target_s, void* stream) {
    XR_REQUIRE(cams && hw && prefix, "cams, hw and prefix are required");
    XR_REQUIRE(n_images >= 1 && n_images <= XR_MS_MAX_IMAGES, "1 .. XR_MS_MAX_IMAGES images");
    XR_REQUIRE(total >= 1 && total <= (1ull << 62), "total pixels of 0 or beyond 2^62");
    XR_REQUIRE(!target_s || images, "target_s needs the packed images");
    XR_REQUIRE(idx || (image < n_images && first_pixel <= total && R <= total - first_pixel), "image >= n_images or first_pixel + R exceeds the total");
    XR_REQUIRE(S >= 1 || (!z_vals && !t_rand), "z_vals and t_rand need S >= 1");
    const uint32_t Sd = S ? S : 1u;
    XR_REQUIRE(R <= (0x7fffffffull * MS_BLOCK) / Sd, "more than 2^31 - 1 workgroups");
    if (R == 0) return 0;
    MsRayArgs a;
    a.cams = cams; a.hw = hw; a.prefix = prefix; a.idx = idx; a.images = images; a.t_rand = t_rand;
    a.n_images = n_images; a.image = idx ? 0u : image; a.S = S; a.Sd = Sd; a.total = total; a.first_pixel = idx ? 0ull : first_pixel; a.R = R;
    a.lindisp = lindisp;
    a.rays_o = rays_o; a.rays_d = rays_d; a.viewdirs = viewdirs; a.radii = radii; a.lossmult = lossmult; a.near_out = near_out; a.far_out = far_out;
    a.z_vals = z_vals; a.target_s = target_s;
    const uint32_t blocks = (uint32_t)((R * Sd + MS_BLOCK - 1) / MS_BLOCK);
    hipLaunchKernelGGL(k_ms_rays, dim3(blocks), dim3(MS_BLOCK), 0, (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- the pyramid
struct MsPyrArgs {
    const uint8_t* base;
    uint32_t N, H, W, C, n_down;
    uint64_t per_view;
    int white_bkgd;
    uint8_t* bytes_out;
    float* pixels_out;
};

// level L's float at (r, c), channel ch, of view `img` (a pointer to its [H,W,C] bytes): convert_blender_data.py:43-45 applied L times
template <int L>
static __device__ inline float ms_level(const uint8_t* img, uint32_t W, uint32_t C, uint32_t r, uint32_t c, uint32_t ch) {
    if constexpr (L == 0) {
        return (float)img[((size_t)r * W + c) * C + ch] / 255.f;
    } else {
        float s = 0.f;
#pragma unroll 1
        for (uint32_t q = 0; q < 4; ++q) {                          // a, b, c, d: (2r, 2c), (2r, 2c+1), (2r+1, 2c), (2r+1, 2c+1)
            const float v = ms_level<L - 1>(img, W, C, 2 * r + (q >> 1), 2 * c + (q & 1), ch);
            s = q == 0 ? v : s + v;
        }
        return s / 4.f;
    }
}

static __device__ inline float ms_level_at(uint32_t L, const uint8_t* img, uint32_t W, uint32_t C, uint32_t r, uint32_t c, uint32_t ch) {
    switch (L) {
        case 0: return ms_level<0>(img, W, C, r, c, ch);
        case 1: return ms_level<1>(img, W, C, r, c, ch);
        case 2: return ms_level<2>(img, W, C, r, c, ch);
        case 3: return ms_level<3>(img, W, C, r, c, ch);
        case 4: return ms_level<4>(img, W, C, r, c, ch);
        case 5: return ms_level<5>(img, W, C, r, c, ch);
        case 6: return ms_level<6>(img, W, C, r, c, ch);
        default: return ms_level<7>(img, W, C, r, c, ch);
    }
}

static __global__ void __launch_bounds__(MS_BLOCK) k_ms_pyramid(MsPyrArgs a) {
    const size_t item = (size_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (item >= (size_t)a.N * a.per_view) return;
    const size_t view = item / a.per_view;
    uint64_t p = item - view * a.per_view;
    uint32_t L = 0;
    for (; L + 1 < a.n_down; ++L) {                                 // the level this packed pixel belongs to
        const uint64_t n = (uint64_t)(a.H >> L) * (a.W >> L);
        if (p < n) break;
        p -= n;
    }
    const uint32_t wl = a.W >> L, r = (uint32_t)(p / wl), c = (uint32_t)(p - (uint64_t)r * wl);
    const uint8_t* img = a.base + view * ((size_t)a.H * a.W * a.C);
    float px[4];
    for (uint32_t ch = 0; ch < 4; ++ch) {
        if (ch < a.C) {
            const uint8_t b = (uint8_t)(ms_level_at(L, img, a.W, a.C, r, c, ch) * 255.f);   // np.uint8(img * 255): truncation
            if (a.bytes_out) a.bytes_out[item * a.C + ch] = b;
            px[ch] = (float)b / 255.f;                              // load_multiscale.py:18
        } else {
            px[ch] = 0.f;
        }
    }
    if (!a.pixels_out) return;
    const float alpha = a.C == 4 ? px[3] : px[2];                   // image[..., -1:], whatever C is
    for (int ch = 0; ch < 3; ++ch)
        a.pixels_out[item * 3 + ch] = a.white_bkgd ? px[ch] * alpha + (1.f - alpha) : px[ch];
}

extern "C" int xr_ms_pyramid(const uint8_t* base, uint32_t N, uint32_t H, uint32_t W, uint32_t C, uint32_t n_down, int white_bkgd,
                             uint8_t* bytes_out, float* pixels_out, void* stream) {
    XR_REQUIRE(base && (bytes_out || pixels_out), "base and at least one output are required");
    XR_REQUIRE(N >= 1 && H >= 1 && W >= 1, "N, H, W >= 1");
    XR_REQUIRE(C == 3 || C == 4, "3 or 4 channels");
    XR_REQUIRE(n_down >= 1 && n_down <= XR_MS_MAX_DOWN, "1 .. XR_MS_MAX_DOWN levels");
    const uint32_t m = 1u << (n_down - 1);
    XR_REQUIRE(H % m == 0 && W % m == 0, "H and W must be divisible by 2^(n_down - 1)");
    uint64_t per_view = 0;
    for (uint32_t j = 0; j < n_down; ++j) per_view += (uint64_t)(H >> j) * (W >> j);
    XR_REQUIRE((uint64_t)N * per_view <= (1ull << 40), "N per_view beyond 2^40");
    MsPyrArgs a;
    a.base = base; a.N = N; a.H = H; a.W = W; a.C = C; a.n_down = n_down; a.per_view = per_view; a.white_bkgd = white_bkgd;
    a.bytes_out = bytes_out; a.pixels_out = pixels_out;
    const uint64_t blocks = ((uint64_t)N * per_view + MS_BLOCK - 1) / MS_BLOCK;
    XR_REQUIRE(blocks <= 0x7fffffffull, "more than 2^31 - 1 workgroups");
    hipLaunchKernelGGL(k_ms_pyramid, dim3((uint32_t)blocks), dim3(MS_BLOCK), 0, (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return 0;
}
