// GeneBody data for gfx950: the crop-and-resize frame preparation.  The reference crops every view of every item to
// its mask's box, resizes picture, mask and depth with OpenCV, normalises, masks and measures the body against every camera -- on the
// host, 5 views per training item and 4 + 48 per evaluation item.  Here a view is prepared once and an item is two launches:
//   k_gb_crop_box   ONE workgroup per raw mask: min / max row and column of mask != 0 (8 bytes per load where the rows allow it), reduced
//                   through the wave and LDS, then image_cropping's rule by one lane, in double, with the reference's quirks
//   k_gb_resize     thread = one output pixel of one view: OpenCV's INTER_NEAREST for mask and depth and its 8-bit fixed-point INTER_CUBIC
//                   for the picture (restated from memory: tests/genebody_restatement.py is the specification), a direct 16-tap gather
//   k_gb_assemble   thread = one pixel of one view in its role: threshold, depth union, ToTensor, Normalize or white background, mask
//                   product; the final mask's box by wave reduction and one int32 atomicMin / atomicMax per wave (order-free)
//   k_gb_calib      ONE workgroup per view over the body vertices: adjusted K, near / far, persps; workgroup 0 also makes the input views'
//                   spatial_freq, the item's bbox, min(spatial_freq) and center
// No locks, no device-side allocation, no scratch.  Reference lines: xrnerf/datasets/genebody_dataset.py:116-182 (image_cropping,
// get_near_far, get_realworld_scale), 228-328 (get_image's loop and the item's bbox).
// Built with -ffp-contract=off, and every expression that has to equal the host's bits is written in explicitly rounded single operations.
#include "xr_common.h"
#include "../../include/xrnerf_mi355_genebody.h"

#define GB_BLOCK 256
#define GB_WAVES (GB_BLOCK / XR_WAVE)
#define GB_INT_MAX 0x7fffffff

// one correctly rounded double operation that the compiler may not contract or reassociate.  The host build of this file (tests/hip_emu)
// has the float forms only, so the double forms are spelled here for it
#ifdef __HIP_EMU__
static inline double gb_dmul(double a, double b) { volatile double r = a * b; return r; }
static inline double gb_dadd(double a, double b) { volatile double r = a + b; return r; }
static inline double gb_dsub(double a, double b) { volatile double r = a - b; return r; }
static inline double gb_ddiv(double a, double b) { volatile double r = a / b; return r; }
#else
static __device__ __forceinline__ double gb_dmul(double a, double b) { return __dmul_rn(a, b); }
static __device__ __forceinline__ double gb_dadd(double a, double b) { return __dadd_rn(a, b); }
static __device__ __forceinline__ double gb_dsub(double a, double b) { return __dsub_rn(a, b); }
static __device__ __forceinline__ double gb_ddiv(double a, double b) { return __ddiv_rn(a, b); }
#endif

struct GbPtrs { const void* p[XR_GB_MAX_VIEWS]; };

// min of lo[] and max of hi[] over the workgroup's 256 threads; every thread receives the result
template <typename T, int K> static __device__ inline void gb_block_minmax(T (&lo)[K], T (&hi)[K]) {
    __shared__ T s_lo[GB_WAVES][K], s_hi[GB_WAVES][K];
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int m = XR_WAVE / 2; m >= 1; m >>= 1) {
            const T a = __shfl_xor(lo[k], m), b = __shfl_xor(hi[k], m);
            lo[k] = a < lo[k] ? a : lo[k];
            hi[k] = b > hi[k] ? b : hi[k];
        }
    const int wave = threadIdx.x / XR_WAVE, lane = threadIdx.x % XR_WAVE;
    __syncthreads();                                       // the previous call's readers are done
    if (lane == 0)
        for (int k = 0; k < K; ++k) { s_lo[wave][k] = lo[k]; s_hi[wave][k] = hi[k]; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        lo[k] = s_lo[0][k]; hi[k] = s_hi[0][k];
        for (int w = 1; w < GB_WAVES; ++w) {
            lo[k] = s_lo[w][k] < lo[k] ? s_lo[w][k] : lo[k];
            hi[k] = s_hi[w][k] > hi[k] ? s_hi[w][k] : hi[k];
        }
    }
}

// ---------------------------------------------------------------------------------------------- a. the crop box
struct GbCropArgs {
    const uint8_t* masks;
    long long off[XR_GB_MAX_VIEWS];
    int h[XR_GB_MAX_VIEWS], w[XR_GB_MAX_VIEWS];
    int32_t* boxes;
};

// genebody_dataset.py:124-158 on the tight box (top, left, bottom, right) of a non-empty mask
static __device__ inline void gb_crop_rule(int top, int left, int bottom, int right, int h, int w, int32_t* out) {
    int bh = bottom - top, bw = right - left;
    const double ph = gb_dmul((double)bh, 0.1), pw = gb_dmul((double)bw, 0.1);
    const int b2 = (int)gb_dadd(ph, (double)bottom), t2 = (int)gb_dsub((double)top, ph);
    const int r2 = (int)gb_dadd(pw, (double)right), l2 = (int)gb_dsub((double)left, ph);       // ph: the reference pads `left` by the height
    bottom = b2 < h ? b2 : h; top = t2 > 0 ? t2 : 0;
    right = r2 < w ? r2 : w; left = l2 > 0 ? l2 : 0;
    bh = bottom - top; bw = right - left;
    if (bh >= bw) {
        const double c = gb_ddiv((double)(left + right), 2.0), half = gb_ddiv((double)bh, 2.0);
        if (gb_dsub(c, half) < 0.0) { left = 0; right = bh; }
        else if (gb_dadd(c, half) >= (double)w) { left = w - bh; right = w; }
        else { left = (int)gb_dsub(c, half); right = left + bh; }
    } else {
        const double c = gb_ddiv((double)(top + bottom), 2.0), half = gb_ddiv((double)bw, 2.0);
        if (gb_dsub(c, half) < 0.0) { top = 0; bottom = bw; }
        else if (gb_dadd(c, half) >= (double)h) { top = h - bw; bottom = h; }
        else { top = (int)gb_dsub(c, half); bottom = top + bw; }
    }
    out[0] = top; out[1] = left; out[2] = bottom; out[3] = right;
}

static __global__ void __launch_bounds__(GB_BLOCK) k_gb_crop_box(GbCropArgs a) {
    const int v = blockIdx.x, h = a.h[v], w = a.w[v];
    const uint8_t* m = a.masks + a.off[v];
    int lo[2] = {GB_INT_MAX, GB_INT_MAX}, hi[2] = {-1, -1};           // row, column
    if ((w & 7) == 0 && (((uintptr_t)m) & 7) == 0) {                   // every row starts on 8 bytes
        const size_t words = (size_t)h * (size_t)(w >> 3);
        const int wpr = w >> 3;
        for (size_t i = threadIdx.x; i < words; i += GB_BLOCK) {
            const unsigned long long u = reinterpret_cast<const unsigned long long*>(m)[i];
            if (u) {
                const int r = (int)(i / wpr), c = (int)(i - (size_t)r * wpr) << 3;
                const int c0 = c + (__builtin_ctzll(u) >> 3), c1 = c + 7 - (__builtin_clzll(u) >> 3);        // little endian: byte j is column c + j
                lo[0] = r < lo[0] ? r : lo[0]; hi[0] = r > hi[0] ? r : hi[0];
                lo[1] = c0 < lo[1] ? c0 : lo[1]; hi[1] = c1 > hi[1] ? c1 : hi[1];
            }
        }
    } else {
        const size_t n = (size_t)h * w;
        for (size_t i = threadIdx.x; i < n; i += GB_BLOCK)
            if (m[i]) {
                const int r = (int)(i / w), c = (int)(i - (size_t)r * w);
                lo[0] = r < lo[0] ? r : lo[0]; hi[0] = r > hi[0] ? r : hi[0];
                lo[1] = c < lo[1] ? c : lo[1]; hi[1] = c > hi[1] ? c : hi[1];
            }
    }
    gb_block_minmax<int, 2>(lo, hi);
    if (threadIdx.x == 0) {
        int32_t* out = a.boxes + 4 * v;
        if (hi[0] < 0) { out[0] = 0; out[1] = 0; out[2] = h; out[3] = w; }
        else gb_crop_rule(lo[0], lo[1], hi[0], hi[1], h, w, out);
    }
}

static bool gb_size_ok(long long h, long long w) { return h >= 1 && w >= 1 && h <= (long long)XR_GB_MAX_SIDE && w <= (long long)XR_GB_MAX_SIDE; }

extern "C" int xr_gb_crop_box(const uint8_t* masks, const int64_t* table, uint32_t n, int32_t* boxes, void* stream) {
    XR_REQUIRE(masks && table && boxes, "null pointer");
    XR_REQUIRE(n >= 1 && n <= XR_GB_MAX_VIEWS, "n must be 1 .. XR_GB_MAX_VIEWS");
    GbCropArgs a;
    memset(&a, 0, sizeof(a));
    a.masks = masks; a.boxes = boxes;
    for (uint32_t i = 0; i < n; ++i) {
        XR_REQUIRE(table[3 * i] >= 0 && gb_size_ok(table[3 * i + 1], table[3 * i + 2]), "a negative offset, or a size of 0 or above XR_GB_MAX_SIDE");
        a.off[i] = table[3 * i]; a.h[i] = (int)table[3 * i + 1]; a.w[i] = (int)table[3 * i + 2];
    }
    hipLaunchKernelGGL(k_gb_crop_box, dim3(n), dim3(GB_BLOCK), 0, (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- b. the resizes
struct GbResizeArgs {
    const uint8_t *imgs, *masks;
    const uint16_t* depths;
    long long img_off[XR_GB_MAX_VIEWS], msk_off[XR_GB_MAX_VIEWS], dep_off[XR_GB_MAX_VIEWS];
    int h[XR_GB_MAX_VIEWS], w[XR_GB_MAX_VIEWS];
    const int32_t* boxes;
    uint32_t S;
    uint8_t *rgb, *m8;
    float* depth;
};

static __device__ inline double gb_scale(int n, uint32_t S) { return gb_ddiv(1.0, gb_ddiv((double)S, (double)n)); }

static __device__ inline int gb_nearest(uint32_t x, double scale, int n) {
    const int s = (int)floor(gb_dmul((double)x, scale));
    return s < n - 1 ? s : n - 1;
}

// the four taps of output coordinate x over n source pixels: clamped indices and 11-bit coefficients
static __device__ inline void gb_cubic_taps(uint32_t x, double scale, int n, int* idx, int* coef) {
    const float fx = (float)gb_dsub(gb_dmul(gb_dadd((double)x, 0.5), scale), 0.5);
    const float sf = floorf(fx);
    const float f = __fsub_rn(fx, sf);
    const float t = __fadd_rn(f, 1.f), g = __fsub_rn(1.f, f);
    float c[4];
    c[0] = __fsub_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fsub_rn(__fmul_rn(-0.75f, t), -3.75f), t), -6.f), t), -3.f);
    c[1] = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(1.25f, f), 2.25f), f), f), 1.f);
    c[2] = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(1.25f, g), 2.25f), g), g), 1.f);
    c[3] = __fsub_rn(__fsub_rn(__fsub_rn(1.f, c[0]), c[1]), c[2]);
    const int sx = (int)sf;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float r = rintf(__fmul_rn(c[k], 2048.f));                   // round half to even
        coef[k] = r < -32768.f ? -32768 : (r > 32767.f ? 32767 : (int)r);
        const int i = sx - 1 + k;
        idx[k] = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
    }
}

static __global__ void __launch_bounds__(GB_BLOCK) k_gb_resize(GbResizeArgs a) {
    const uint32_t v = blockIdx.y, S = a.S;
    const size_t SS = (size_t)S * S, p = (size_t)blockIdx.x * GB_BLOCK + threadIdx.x;
    if (p >= SS) return;
    const uint32_t y = (uint32_t)(p / S), x = (uint32_t)(p - (size_t)y * S);
    const int h = a.h[v], w = a.w[v];
    int top = a.boxes[4 * v], left = a.boxes[4 * v + 1], bottom = a.boxes[4 * v + 2], right = a.boxes[4 * v + 3];
    top = top > 0 ? top : 0; left = left > 0 ? left : 0;                  // nothing is read outside the picture, whatever the box holds
    bottom = bottom < h ? bottom : h; right = right < w ? right : w;
    uint8_t* rgb = a.rgb + ((size_t)v * SS + p) * 3;
    const bool has_depth = a.dep_off[v] >= 0;
    if (bottom <= top || right <= left) {
        rgb[0] = rgb[1] = rgb[2] = 0;
        a.m8[(size_t)v * SS + p] = 0;
        if (has_depth) a.depth[(size_t)v * SS + p] = 0.f;
        return;
    }
    const int ch = bottom - top, cw = right - left;
    const double sy = gb_scale(ch, S), sx = gb_scale(cw, S);
    const size_t near = (size_t)(top + gb_nearest(y, sy, ch)) * w + (size_t)(left + gb_nearest(x, sx, cw));
    a.m8[(size_t)v * SS + p] = a.masks[a.msk_off[v] + near];
    if (has_depth) a.depth[(size_t)v * SS + p] = __fdiv_rn((float)a.depths[a.dep_off[v] + near], 1000.f);
    int iy[4], cy[4], ix[4], cx[4];
    gb_cubic_taps(y, sy, ch, iy, cy);
    gb_cubic_taps(x, sx, cw, ix, cx);
    const uint8_t* img = a.imgs + a.img_off[v];
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) {
        const uint8_t* row = img + (size_t)(top + iy[ky]) * w * 3;
        int hor[3] = {0, 0, 0};
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) {
            const uint8_t* px = row + (size_t)(left + ix[kx]) * 3;
            hor[0] += cx[kx] * px[0]; hor[1] += cx[kx] * px[1]; hor[2] += cx[kx] * px[2];
        }
        acc[0] += cy[ky] * hor[0]; acc[1] += cy[ky] * hor[1]; acc[2] += cy[ky] * hor[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int q = (acc[c] + (1 << 21)) >> 22;
        rgb[c] = (uint8_t)(q < 0 ? 0 : (q > 255 ? 255 : q));
    }
}

extern "C" int xr_gb_resize(const uint8_t* imgs, const uint8_t* masks, const uint16_t* depths, const int64_t* table, uint32_t n, const int32_t* boxes,
                            uint32_t S, uint8_t* rgb, uint8_t* m8, float* depth, void* stream) {
    XR_REQUIRE(imgs && masks && table && boxes && rgb && m8, "null pointer");
    XR_REQUIRE(n >= 1 && n <= XR_GB_MAX_VIEWS, "n must be 1 .. XR_GB_MAX_VIEWS");
    XR_REQUIRE(S >= 1 && S <= XR_GB_MAX_SIDE, "S must be 1 .. XR_GB_MAX_SIDE");
    GbResizeArgs a;
    memset(&a, 0, sizeof(a));
    a.imgs = imgs; a.masks = masks; a.depths = depths; a.boxes = boxes; a.S = S; a.rgb = rgb; a.m8 = m8; a.depth = depth;
    for (uint32_t i = 0; i < n; ++i) {
        const int64_t* t = table + 5 * i;
        XR_REQUIRE(t[0] >= 0 && t[1] >= 0 && gb_size_ok(t[3], t[4]), "a negative offset, or a size of 0 or above XR_GB_MAX_SIDE");
        XR_REQUIRE(t[2] < 0 || (depths && depth), "a depth offset without depths / depth");
        a.img_off[i] = t[0]; a.msk_off[i] = t[1]; a.dep_off[i] = t[2] < 0 ? -1 : t[2]; a.h[i] = (int)t[3]; a.w[i] = (int)t[4];
    }
    hipLaunchKernelGGL(k_gb_resize, dim3(xr_div_up((uint64_t)S * S, GB_BLOCK), n), dim3(GB_BLOCK), 0, (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- c. a view in its role
struct GbAssembleArgs {
    GbPtrs rgb, m8, depth;
    uint32_t V, num_views, S;
    int white, has_depth;
    float *img, *mask, *smpl_depth;
    int32_t* acc;
};

static __global__ void __launch_bounds__(GB_BLOCK) k_gb_assemble(GbAssembleArgs a) {
    const uint32_t v = blockIdx.y, S = a.S;
    const size_t SS = (size_t)S * S, p = (size_t)blockIdx.x * GB_BLOCK + threadIdx.x;
    const bool live = p < SS, input = v < a.num_views;
    bool m = false;
    if (live) {
        m = static_cast<const uint8_t*>(a.m8.p[v])[p] > 128;
        if (input && a.has_depth) {
            const float d = static_cast<const float*>(a.depth.p[v])[p];
            m = m || d > 0.f;
            a.smpl_depth[(size_t)v * SS + p] = d;
        }
        const float mf = m ? 1.f : 0.f;
        const uint8_t* px = static_cast<const uint8_t*>(a.rgb.p[v]) + p * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float x = __fdiv_rn((float)px[c], 255.f);
            if (input) x = __fdiv_rn(__fsub_rn(x, 0.5f), 0.5f);
            else if (a.white) x = __fadd_rn(__fmul_rn(x, mf), __fsub_rn(1.f, mf));
            a.img[((size_t)v * 3 + c) * SS + p] = __fmul_rn(mf, x);
        }
        if (input) a.mask[(size_t)v * SS + p] = mf;
    }
    // the final mask's box: the wave's extremes, then one atomic per wave and bound
    const int r = (int)(p / S), c = (int)(p - (size_t)r * S);
    int lo[2] = {m ? r : GB_INT_MAX, m ? c : GB_INT_MAX}, hi[2] = {m ? r : -1, m ? c : -1};
#pragma unroll
    for (int k = 0; k < 2; ++k)
        for (int s = XR_WAVE / 2; s >= 1; s >>= 1) {
            const int x = __shfl_xor(lo[k], s), y = __shfl_xor(hi[k], s);
            lo[k] = x < lo[k] ? x : lo[k];
            hi[k] = y > hi[k] ? y : hi[k];
        }
    if (threadIdx.x % XR_WAVE == 0 && hi[0] >= 0) {
        atomicMin(a.acc + 2 * v, lo[0]); atomicMin(a.acc + 2 * v + 1, lo[1]);
        atomicMax(a.acc + 2 * (a.V + v), hi[0]); atomicMax(a.acc + 2 * (a.V + v) + 1, hi[1]);
    }
}

extern "C" int xr_gb_assemble(const void* const* rgb, const void* const* m8, const void* const* depth, uint32_t V, uint32_t num_views, uint32_t S,
                              int white_bkgd, float* img, float* mask, float* smpl_depth, int32_t* acc, void* stream) {
    XR_REQUIRE(rgb && m8 && img && acc && (mask || num_views == 0), "null pointer");
    XR_REQUIRE(V >= 1 && V <= XR_GB_MAX_VIEWS && num_views <= V, "V must be 1 .. XR_GB_MAX_VIEWS and num_views <= V");
    XR_REQUIRE(S >= 1 && S <= XR_GB_MAX_SIDE, "S must be 1 .. XR_GB_MAX_SIDE");
    XR_REQUIRE((depth != nullptr) == (smpl_depth != nullptr), "depth and smpl_depth go together");
    GbAssembleArgs a;
    memset(&a, 0, sizeof(a));
    for (uint32_t i = 0; i < V; ++i) {
        XR_REQUIRE(rgb[i] && m8[i], "null view pointer");
        a.rgb.p[i] = rgb[i]; a.m8.p[i] = m8[i];
    }
    for (uint32_t i = 0; depth && i < num_views; ++i) {
        XR_REQUIRE(depth[i], "null depth pointer");
        a.depth.p[i] = depth[i];
    }
    a.V = V; a.num_views = num_views; a.S = S; a.white = white_bkgd != 0; a.has_depth = depth != nullptr;
    a.img = img; a.mask = mask; a.smpl_depth = smpl_depth; a.acc = acc;
    XR_HIP(hipMemsetAsync(acc, 0x7f, sizeof(int32_t) * 2 * V, (hipStream_t)stream));
    XR_HIP(hipMemsetAsync(acc + 2 * V, 0xff, sizeof(int32_t) * 2 * V, (hipStream_t)stream));
    hipLaunchKernelGGL(k_gb_assemble, dim3(xr_div_up((uint64_t)S * S, GB_BLOCK), V), dim3(GB_BLOCK), 0, (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- d. the camera rows and the item's scalars
struct GbCalibArgs {
    const float *verts, *K, *D, *w2c;
    GbPtrs crop;
    const int32_t* acc;
    uint32_t N, nd, V, num_views, S;
    float* persps;
    int32_t* vboxes;
    double *sf_views, *bbox, *spatial_freq;
    float* center;
};

// genebody_dataset.py:292-297: every step rounds to fp32
static __device__ inline void gb_adjust_K(const float* K, const int32_t* crop, uint32_t S, float* A) {
    const int top = crop[0], left = crop[1], bottom = crop[2], right = crop[3];
    for (int i = 0; i < 9; ++i) A[i] = K[i];
    A[2] = __fsub_rn(A[2], (float)left);
    A[5] = __fsub_rn(A[5], (float)top);
    const float sx = (float)gb_ddiv((double)S, (double)(right - left)), sy = (float)gb_ddiv((double)S, (double)(bottom - top));
    for (int i = 0; i < 3; ++i) { A[i] = __fmul_rn(A[i], sx); A[3 + i] = __fmul_rn(A[3 + i], sy); }
}

static __device__ inline void gb_view_box(const int32_t* acc, uint32_t V, uint32_t v, uint32_t S, int* box) {
    if (acc[2 * (V + v)] < 0) { box[0] = 0; box[1] = 0; box[2] = (int)S; box[3] = (int)S; }
    else { box[0] = acc[2 * v]; box[1] = acc[2 * v + 1]; box[2] = acc[2 * (V + v)]; box[3] = acc[2 * (V + v) + 1]; }
}

// extremes over the vertices seen from view v: lo / hi [0] = camera z, [1], [2] = the projection's u, v through AK (with_uv)
static __device__ inline void gb_project(const GbCalibArgs& a, uint32_t v, const float* AK, bool with_uv, float (&lo)[3], float (&hi)[3]) {
    const float* M = a.w2c + 16 * v;
    for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    for (uint32_t i = threadIdx.x; i < a.N; i += GB_BLOCK) {
        const float x = a.verts[3 * i], y = a.verts[3 * i + 1], z = a.verts[3 * i + 2];
        float q[3];
        for (int r = 0; r < 3; ++r)
            q[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(x, M[4 * r]), __fmul_rn(y, M[4 * r + 1])), __fmul_rn(z, M[4 * r + 2])), M[4 * r + 3]);
        float e[3] = {q[2], 0.f, 0.f};
        if (with_uv) {
            float pr[3];
            for (int r = 0; r < 3; ++r)
                pr[r] = __fadd_rn(__fadd_rn(__fmul_rn(q[0], AK[3 * r]), __fmul_rn(q[1], AK[3 * r + 1])), __fmul_rn(q[2], AK[3 * r + 2]));
            const float den = __fadd_rn(pr[2], 1e-8f);
            e[1] = __fdiv_rn(pr[0], den); e[2] = __fdiv_rn(pr[1], den);
        }
        for (int k = 0; k < 3; ++k) { lo[k] = e[k] < lo[k] ? e[k] : lo[k]; hi[k] = e[k] > hi[k] ? e[k] : hi[k]; }
    }
    gb_block_minmax<float, 3>(lo, hi);
}

static __global__ void __launch_bounds__(GB_BLOCK) k_gb_calib(GbCalibArgs a) {
    const uint32_t v = blockIdx.x, S = a.S;
    float AK[9], lo[3], hi[3];
    gb_adjust_K(a.K + 9 * v, static_cast<const int32_t*>(a.crop.p[v]), S, AK);
    gb_project(a, v, AK, false, lo, hi);
    if (threadIdx.x == 0) {
        float* row = a.persps + (size_t)v * (4 + a.nd + 2);
        row[0] = AK[0]; row[1] = AK[4]; row[2] = AK[2]; row[3] = AK[5];
        for (uint32_t i = 0; i < a.nd; ++i) row[4 + i] = a.D[(size_t)v * a.nd + i];
        const float half = __fdiv_rn(__fsub_rn(hi[0], lo[0]), 2.f);
        row[4 + a.nd] = __fsub_rn(lo[0], half);
        row[5 + a.nd] = __fadd_rn(hi[0], half);
        int box[4];
        gb_view_box(a.acc, a.V, v, S, box);
        for (int k = 0; k < 4; ++k) a.vboxes[4 * v + k] = box[k];
    }
    if (v != 0) return;
    // ---- the item's values, by workgroup 0
    float vlo[3], vhi[3];
    for (int k = 0; k < 3; ++k) { vlo[k] = INFINITY; vhi[k] = -INFINITY; }
    for (uint32_t i = threadIdx.x; i < a.N; i += GB_BLOCK)
        for (int k = 0; k < 3; ++k) {
            const float e = a.verts[3 * i + k];
            vlo[k] = e < vlo[k] ? e : vlo[k]; vhi[k] = e > vhi[k] ? e : vhi[k];
        }
    gb_block_minmax<float, 3>(vlo, vhi);
    double sf_min = INFINITY;
    for (uint32_t i = 0; i < a.num_views; ++i) {
        gb_adjust_K(a.K + 9 * i, static_cast<const int32_t*>(a.crop.p[i]), S, AK);
        gb_project(a, i, AK, true, lo, hi);
        int box[4];
        gb_view_box(a.acc, a.V, i, S, box);
        const int bh = box[2] - box[0], bw = box[3] - box[1];
        const int ax = bh > bw ? 1 : 0;                                                     // axis 1 = image rows = the body's y
        const double side = (double)(ax ? bh : bw);
        const double ext_p = (double)__fsub_rn(hi[1 + ax], lo[1 + ax]), ext_s = (double)__fsub_rn(vhi[ax], vlo[ax]);
        const double long_axis = gb_dmul(gb_ddiv(side, ext_p), ext_s);
        const double sf = gb_ddiv(gb_ddiv(180.0, long_axis), 0.5);
        if (threadIdx.x == 0) a.sf_views[i] = sf;
        sf_min = sf < sf_min ? sf : sf_min;
    }
    if (threadIdx.x == 0) {
        a.spatial_freq[0] = sf_min;
        for (int k = 0; k < 3; ++k) a.center[k] = __fdiv_rn(__fadd_rn(vhi[k], vlo[k]), 2.f);
        const double c = gb_ddiv((double)S, 2.0);
        double far_[2] = {0.0, 0.0};
        for (uint32_t i = a.num_views; i < a.V; ++i) {
            int box[4];
            gb_view_box(a.acc, a.V, i, S, box);
            for (int k = 0; k < 4; ++k) {
                const double d = fabs(gb_dsub((double)box[k], c));
                far_[k & 1] = d > far_[k & 1] ? d : far_[k & 1];
            }
        }
        const int b0 = (int)far_[0], b1 = (int)gb_dmul(far_[1], 1.4142135623730951);
        const double s = (double)S;
        const double out[4] = {c - (double)b0, c + (double)b0, c - (double)b1, c + (double)b1};
        for (int k = 0; k < 4; ++k) a.bbox[k] = out[k] < 0.0 ? 0.0 : (out[k] > s ? s : out[k]);
    }
}

extern "C" int xr_gb_calib(const float* verts, uint32_t N, const float* K, const float* D, uint32_t nd, const float* w2c, const void* const* crop,
                           const int32_t* acc, uint32_t V, uint32_t num_views, uint32_t S, float* persps, int32_t* vboxes, double* sf_views, double* bbox,
                           double* spatial_freq, float* center, void* stream) {
    XR_REQUIRE(verts && K && w2c && crop && acc && persps && vboxes && sf_views && bbox && spatial_freq && center && (D || nd == 0), "null pointer");
    XR_REQUIRE(N >= 1, "N must be at least 1");
    XR_REQUIRE(V >= 1 && V <= XR_GB_MAX_VIEWS && num_views >= 1 && num_views < V, "V must be 1 .. XR_GB_MAX_VIEWS and 1 <= num_views < V");
    XR_REQUIRE(nd <= XR_GB_MAX_DIST, "nd above XR_GB_MAX_DIST");
    XR_REQUIRE(S >= 1 && S <= XR_GB_MAX_SIDE, "S must be 1 .. XR_GB_MAX_SIDE");
    GbCalibArgs a;
    memset(&a, 0, sizeof(a));
    for (uint32_t i = 0; i < V; ++i) {
        XR_REQUIRE(crop[i], "null crop pointer");
        a.crop.p[i] = crop[i];
    }
    a.verts = verts; a.K = K; a.D = D; a.w2c = w2c; a.acc = acc; a.N = N; a.nd = nd; a.V = V; a.num_views = num_views; a.S = S;
    a.persps = persps; a.vboxes = vboxes; a.sf_views = sf_views; a.bbox = bbox; a.spatial_freq = spatial_freq; a.center = center;
    hipLaunchKernelGGL(k_gb_calib, dim3(V), dim3(GB_BLOCK), 0, (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return 0;
}
