// BungeeNeRF data for gfx950: a training item and a validation frame, each in one launch.  The reference
// materialises a float64 [N H W, 3, 3] table, a float64 radius and an int64 scale code per pixel of every train image (88 bytes per ray),
// shuffles them on the host and then runs a chain of small tensor ops per item (BungeeBatchSample, GetViewdirs, BungeeGetBounds,
// BungeeGetZvals, PerturbZvals); everything but the colour is a function of the image's 3x4 matrix, its scale code and the pixel's
// position.  Here the images, a camera table and the permutation stay resident and an item makes the rays of its slice:
//   k_bgd_item    thread = one (ray, edge) item, 256-thread workgroups, a workgroup owns max(1, 256 / S) whole rays (S > 256: one ray,
//                 its threads loop).  The lane of edge 0 does the ray's double arithmetic, writes the per-ray outputs (each rounded to
//                 fp32 once) and leaves near / far in LDS; every lane then makes its own edge of the row before the sort, the row is
//                 sorted by rank through LDS (each lane counts the edges that go before its own: the stable order of the reference's
//                 torch.sort, NaN last) and every lane reads its sorted neighbours for PerturbZvals.  All index arithmetic is 64-bit.
//   k_bgd_frame   the same layout over the H W pixels of one pose, the ray in fp32 as GetRays(include_radius=True) writes it.
// The bounds and the edges are xr_bungee_zvals.h, the code k_bungee_zvals runs: the bits of xr_bungee_zvals on the rays written here.
// Reference lines:
//   xrnerf/datasets/load_data/get_rays.py:156-206   get_rays_np_bungee, load_rays_bungee
//   xrnerf/datasets/pipelines/create.py:116-145     BungeeBatchSample     create.py:211-245   GetRays     create.py:539-576   BungeeGetZvals
//   create.py:835-915   BungeeGetBounds             augment.py:261-286    PerturbZvals        transforms.py:70-82   FlattenRays
// Built with -ffp-contract=off: nothing is fused but the explicit fma calls, and the host build of this file (tests/hip_emu) produces
// the same bits.
#include "xr_common.h"
#include "xr_mip_math.h"
#include "xr_bungee_zvals.h"
#include "../../include/xrnerf_mi355_bungeedata.h"

#define BGD_BLOCK 256

struct BgdTail {                               // what follows the ray: bounds, edges, perturbation
    uint32_t S, Sd, rpw;                       // edges per ray, max(S, 1), rays per workgroup
    uint64_t R;
    BgBounds b;
    const float* t_rand;
    float *near_out, *far_out, *z_vals;
};

struct BgdItemArgs {
    const double* cams;
    const int64_t *codes, *perm;
    const float* images;
    const int32_t* i_train;
    uint32_t n_images, n_train, H, W;
    double focal;
    float half_w, half_h;
    uint64_t start, total;
    float *rays_o, *rays_d, *target_s, *radii, *viewdirs;
    int64_t* scale_code;
    BgdTail t;
};

struct BgdFrameArgs {
    const float* c2w;
    uint32_t H, W;
    float fx, fy, cx, cy, radius_div;
    float *rays_o, *rays_d, *radii, *viewdirs;
    BgdTail t;
};

// rays_d of pixel (row, col) of a training image: get_rays.py:157-163
static __device__ inline void bgd_train_dir(const BgdItemArgs& a, const double* C, uint32_t row, uint32_t col, double d[3]) {
    const float xf = (float)col - a.half_w, yf = -((float)row - a.half_h);      // the fp32 meshgrid minus W .5 stays fp32
    const double x = (double)xf / a.focal, y = (double)yf / a.focal, z = -1.0;  // focal is a float64 scalar: double from here on
    const double n = sqrt((x * x + y * y) + z * z);                            // np.linalg.norm over 3 elements
    const double u[3] = {x / n, y / n, z / n};
    for (int r = 0; r < 3; ++r) d[r] = (u[0] * C[4 * r] + u[1] * C[4 * r + 1]) + u[2] * C[4 * r + 2];
}

// rays_d of pixel (row, col) of a frame: create.py:223-230, the three products added in index order
static __device__ inline void bgd_frame_dir(const BgdFrameArgs& a, const float* c, uint32_t row, uint32_t col, float d[3]) {
    const float i = xr_torch_linspace(0.f, (float)(a.W - 1), a.W, col), j = xr_torch_linspace(0.f, (float)(a.H - 1), a.H, row);
    const float dx = (i - a.cx) / a.fx, dy = -(j - a.cy) / a.fy, dz = -1.f;
    for (int r = 0; r < 3; ++r) d[r] = (dx * c[4 * r] + dy * c[4 * r + 1]) + dz * c[4 * r + 2];
}

// one ray of the item, on the lane of its edge 0: the per-ray outputs; o, v = the fp32 rays_o and viewdirs the bounds are made from
static __device__ inline void bgd_item_ray(const BgdItemArgs& a, uint64_t r, float o[3], float v[3]) {
    float d[3] = {NAN, NAN, NAN}, rgb[3] = {NAN, NAN, NAN}, radius = NAN;
    int64_t code = -1;
    o[0] = o[1] = o[2] = v[0] = v[1] = v[2] = NAN;
    const int64_t f = a.perm[a.start + r];
    bool valid = f >= 0 && (uint64_t)f < a.total;
    if (valid) {
        const uint64_t hw = (uint64_t)a.H * a.W, slot = (uint64_t)f / hw, pix = (uint64_t)f - slot * hw;
        const int32_t img = a.i_train[slot];
        valid = img >= 0 && (uint32_t)img < a.n_images;
        if (valid) {
            const uint32_t row = (uint32_t)(pix / a.W), col = (uint32_t)(pix - (uint64_t)row * a.W);
            double C[12], dd[3], da[3], db[3], sq[3];
            for (int i = 0; i < 12; ++i) C[i] = a.cams[(size_t)img * XR_BGD_CAM_DOUBLES + i];
            bgd_train_dir(a, C, row, col, dd);
            const double n = sqrt(fma(dd[2], dd[2], fma(dd[1], dd[1], dd[0] * dd[0])));      // torch.norm: acc = fma(x, x, acc)
            for (int i = 0; i < 3; ++i) { o[i] = (float)C[4 * i + 3]; d[i] = (float)dd[i]; v[i] = (float)(dd[i] / n); }
            const uint32_t rp = row + 1 < a.H ? row : a.H - 3;     // np.concatenate([dx, dx[:, -2:-1]]): the last row repeats dx[H - 3]
            bgd_train_dir(a, C, rp, col, da);
            bgd_train_dir(a, C, rp + 1, col, db);
            for (int i = 0; i < 3; ++i) { const double e = da[i] - db[i]; sq[i] = e * e; }
            radius = (float)((sqrt((sq[0] + sq[1]) + sq[2]) * 2.0) / sqrt(12.0));
            if (a.target_s)
                for (int c = 0; c < 3; ++c) rgb[c] = a.images[((size_t)img * hw + pix) * 3 + c];
            if (a.codes) code = a.codes[img];
        }
    }
    for (int i = 0; i < 3; ++i) {
        if (a.rays_o) a.rays_o[r * 3 + i] = o[i];
        if (a.rays_d) a.rays_d[r * 3 + i] = d[i];
        if (a.viewdirs) a.viewdirs[r * 3 + i] = v[i];
        if (a.target_s) a.target_s[r * 3 + i] = rgb[i];
    }
    if (a.radii) a.radii[r] = radius;
    if (a.scale_code) a.scale_code[r] = code;
}

static __device__ inline void bgd_frame_ray(const BgdFrameArgs& a, uint64_t r, float o[3], float v[3]) {
    const uint32_t row = (uint32_t)(r / a.W), col = (uint32_t)(r - (uint64_t)row * a.W);
    float c[12], d[3];
    for (int i = 0; i < 12; ++i) c[i] = a.c2w[i];
    bgd_frame_dir(a, c, row, col, d);
    const float n = sqrtf(fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0])));                  // torch.norm: acc = fma(x, x, acc)
    for (int i = 0; i < 3; ++i) { o[i] = c[4 * i + 3]; v[i] = d[i] / n; }
    if (a.radii) {                                                 // create.py:239-243
        const uint32_t rp = row + 1 < a.H ? row : a.H - 3;         // torch.cat([dx, dx[-2:-1]]): the last row repeats dx[H - 3]
        float da[3], db[3], sq[3];
        bgd_frame_dir(a, c, rp, col, da);
        bgd_frame_dir(a, c, rp + 1, col, db);
        for (int i = 0; i < 3; ++i) { const float e = da[i] - db[i]; sq[i] = e * e; }
        a.radii[r] = (sqrtf((sq[0] + sq[1]) + sq[2]) * 2.f) / a.radius_div;
    }
    for (int i = 0; i < 3; ++i) {
        if (a.rays_o) a.rays_o[r * 3 + i] = o[i];
        if (a.rays_d) a.rays_d[r * 3 + i] = d[i];
        if (a.viewdirs) a.viewdirs[r * 3 + i] = v[i];
    }
}

// the workgroup's rays ray0 .. ray0 + n_here: Ray(r, o, v) on the lane of edge 0, then the bounds, the sorted row and the perturbation.
// Every thread of the workgroup reaches every barrier.
template <typename Ray>
static __device__ inline void bgd_block(const BgdTail& t, Ray ray) {
    __shared__ float s_near[BGD_BLOCK], s_far[BGD_BLOCK];
    __shared__ float s_raw[XR_BGD_MAX_SAMPLES], s_sorted[XR_BGD_MAX_SAMPLES];      // rpw Sd <= max(256, Sd) floats each
    const uint64_t ray0 = (uint64_t)blockIdx.x * t.rpw;
    const uint32_t n_here = (uint32_t)(t.R - ray0 < t.rpw ? t.R - ray0 : t.rpw), n_items = n_here * t.Sd;
    const bool tail = t.b.mode != 0;                               // bounds or z-values are asked for
    for (uint32_t i = threadIdx.x; i < n_items; i += BGD_BLOCK) {
        const uint32_t q = i / t.Sd;
        if (i - q * t.Sd != 0) continue;
        const uint64_t r = ray0 + q;
        float o[3], v[3], nr = NAN, fr = NAN;
        ray(r, o, v);
        if (tail) {
            bg_bounds(t.b, o, v, &nr, &fr);
            if (t.near_out) t.near_out[r] = nr;
            if (t.far_out) t.far_out[r] = fr;
            s_near[q] = nr; s_far[q] = fr;
        }
    }
    if (!t.z_vals) return;                                         // uniform over the launch
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_items; i += BGD_BLOCK) {
        const uint32_t q = i / t.Sd;
        s_raw[i] = bg_zval_edge(s_near[q], s_far[q], t.S, i - q * t.Sd);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_items; i += BGD_BLOCK) {   // the rank of this edge in the stable order of torch.sort
        const uint32_t q = i / t.Sd, k = i - q * t.Sd;
        const float* row = s_raw + q * t.Sd;
        const float z = row[k];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < t.S; ++j) rank += (bg_before(row[j], z) || (j < k && !bg_before(z, row[j]))) ? 1u : 0u;
        s_sorted[q * t.Sd + rank] = z;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_items; i += BGD_BLOCK) {
        const uint32_t q = i / t.Sd, k = i - q * t.Sd;
        const float* row = s_sorted + q * t.Sd;
        const uint64_t item = (ray0 + q) * t.S + k;
        float z = row[k];
        if (t.t_rand) {                                            // augment.py:276-282
            const float lower = k == 0 ? z : .5f * (z + row[k - 1]);
            const float upper = k + 1 == t.S ? z : .5f * (row[k + 1] + z);
            z = lower + (upper - lower) * t.t_rand[item];
        }
        t.z_vals[item] = z;
    }
}

static __global__ void __launch_bounds__(BGD_BLOCK) k_bgd_item(BgdItemArgs a) {
    bgd_block(a.t, [&](uint64_t r, float* o, float* v) { bgd_item_ray(a, r, o, v); });
}

static __global__ void __launch_bounds__(BGD_BLOCK) k_bgd_frame(BgdFrameArgs a) {
    bgd_block(a.t, [&](uint64_t r, float* o, float* v) { bgd_frame_ray(a, r, o, v); });
}

// the checks and the fields both entry points share; 0 or XR_EINVAL
static int bgd_tail(BgdTail* t, uint64_t R, uint32_t S, int bounds_mode, const float* globe_center, float r2_top, float r2_earth, float scaling,
                    const float* t_rand, float* near_out, float* far_out, float* z_vals, uint32_t* blocks) {
    const bool tail = near_out || far_out || z_vals || t_rand;
    XR_REQUIRE(!t_rand || z_vals, "t_rand needs z_vals");
    XR_REQUIRE(!tail || (bounds_mode >= 1 && bounds_mode <= 2), "bounds_mode: 1 = sphere, 2 = flat");
    XR_REQUIRE(!tail || bounds_mode != 1 || globe_center, "sphere bounds need the globe centre");
    XR_REQUIRE(z_vals ? (S >= 2 && S <= XR_BGD_MAX_SAMPLES) : S <= XR_BGD_MAX_SAMPLES, "z_vals need 2 <= S <= XR_BGD_MAX_SAMPLES");
    t->S = z_vals ? S : 0u; t->Sd = z_vals ? S : 1u;
    t->rpw = t->Sd >= BGD_BLOCK ? 1u : BGD_BLOCK / t->Sd;
    t->R = R;
    t->b = BgBounds{tail ? bounds_mode : 0, 0.f, 0.f, 0.f, r2_top, r2_earth, scaling};
    if (tail && bounds_mode == 1) { t->b.cx = globe_center[0]; t->b.cy = globe_center[1]; t->b.cz = globe_center[2]; }
    t->t_rand = t_rand; t->near_out = near_out; t->far_out = far_out; t->z_vals = z_vals;
    const uint64_t n = (R + t->rpw - 1) / t->rpw;
    XR_REQUIRE(n <= 0x7fffffffull, "more than 2^31 - 1 workgroups");
    *blocks = (uint32_t)n;
    return 0;
}

extern "C" int xr_bgd_item(const double* cams, const int64_t* codes, const float* images, const int32_t* i_train, uint32_t n_images,
                           uint32_t n_train, uint32_t H, uint32_t W, double focal, float half_w, float half_h, const int64_t* perm, uint64_t start,
                           uint64_t R, uint32_t S, int bounds_mode, const float* globe_center, float r2_top, float r2_earth, float scaling,
                           const float* t_rand, float* rays_o, float* rays_d, float* target_s, float* radii, int64_t* scale_code,
                           float* viewdirs, float* near_out, float* far_out, float* z_vals, void* stream) {
    XR_REQUIRE(cams && i_train && perm, "cams, i_train and perm are required");
    XR_REQUIRE(!target_s || images, "target_s needs the images");
    XR_REQUIRE(!scale_code || codes, "scale_code needs the codes");
    XR_REQUIRE(n_images >= 1 && n_train >= 1, "no images");
    XR_REQUIRE(H >= 3 && W >= 1, "H >= 3 and W >= 1");
    XR_REQUIRE((uint64_t)H * W <= (1ull << 62) / n_train, "n_train H W beyond 2^62");
    XR_REQUIRE(focal == focal && focal != 0.0 && focal - focal == 0.0, "focal must be finite and not 0");
    XR_REQUIRE(start <= (1ull << 62) && R <= (1ull << 62), "start or R beyond 2^62");
    BgdItemArgs a;
    uint32_t blocks = 0;
    const int rc = bgd_tail(&a.t, R, S, bounds_mode, globe_center, r2_top, r2_earth, scaling, t_rand, near_out, far_out, z_vals, &blocks);
    if (rc != 0) return rc;
    if (R == 0) return 0;
    a.cams = cams; a.codes = codes; a.perm = perm; a.images = images; a.i_train = i_train;
    a.n_images = n_images; a.n_train = n_train; a.H = H; a.W = W; a.focal = focal; a.half_w = half_w; a.half_h = half_h;
    a.start = start; a.total = (uint64_t)n_train * H * W;
    a.rays_o = rays_o; a.rays_d = rays_d; a.target_s = target_s; a.radii = radii; a.viewdirs = viewdirs; a.scale_code = scale_code;
    hipLaunchKernelGGL(k_bgd_item, dim3(blocks), dim3(BGD_BLOCK), 0, (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return 0;
}

extern "C" int xr_bgd_frame(const float* c2w, uint32_t H, uint32_t W, float fx, float fy, float cx, float cy, uint32_t S, int bounds_mode,
                            const float* globe_center, float r2_top, float r2_earth, float scaling, float* rays_o, float* rays_d, float* radii,
                            float* viewdirs, float* near_out, float* far_out, float* z_vals, void* stream) {
    XR_REQUIRE(c2w, "c2w is required");
    XR_REQUIRE(H >= 3 && W >= 1, "H >= 3 and W >= 1");
    BgdFrameArgs a;
    uint32_t blocks = 0;
    const int rc = bgd_tail(&a.t, (uint64_t)H * W, S, bounds_mode, globe_center, r2_top, r2_earth, scaling, nullptr, near_out, far_out, z_vals, &blocks);
    if (rc != 0) return rc;
    a.c2w = c2w; a.H = H; a.W = W; a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.radius_div = sqrtf(12.f);
    a.rays_o = rays_o; a.rays_d = rays_d; a.radii = radii; a.viewdirs = viewdirs;
    hipLaunchKernelGGL(k_bgd_frame, dim3(blocks), dim3(BGD_BLOCK), 0, (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return 0;
}
