// Test-set evaluation for gfx950: skimage's structural_similarity as the reference's hooks call it (core/hooks/utils.py:
// calculate_ssim = structural_similarity(..., full=True)[1].mean()), the squared error of img2mse and the 8-bit image of to8b
// (DESIGN.md section 19).  The reference copies every frame to the host and runs five scipy.ndimage filters per channel in float64;
// here the frame is measured where it was rendered:
//   k_ev_tiles    workgroup = one 8 x 32 tile of one image, every channel.  The tile and its halo of r pixels (both images, fp32) are
//                 staged in LDS once, out-of-image indices reflected about the edge.  Per channel the window is applied separably in
//                 double: thread = (halo row, tile column) forms the five row moments x, y, xx, yy, xy into LDS, then thread = pixel
//                 adds them down its column, evaluates S and (x - y)^2 and keeps its own running sums.  The workgroup's two sums --
//                 a wave butterfly (xr_wave.h), the four waves in wave order -- go to the tile's slot of the workspace
//   k_ev_fold     workgroup = image: thread t adds the partials of its run of consecutive tiles in index order, the runs are added by
//                 the same butterfly, the waves in wave order
//   k_ev_to8b     thread = one byte of the [H, 2 W, C] side-by-side image
// No atomics, no device-side allocation, no "last block": the same input gives the same bits.
// LDS per workgroup at r = 5, C = 4: 2 x 18 x 42 x 4 fp32 (24192 B) + 5 x 18 x 32 doubles (23040 B) + 64 B = 47296 B: three workgroups
// per CU beside 160 KiB.  Built with -ffp-contract=off: the host build of this file (tests/hip_emu) then produces the same bits.
#include "xr_common.h"
#include "xr_wave.h"
#include "../../include/xrnerf_mi355_eval.h"

#define EV_BLOCK 256
#define EV_WAVES (EV_BLOCK / 64)
#define EV_TW XR_EVAL_TILE_W
#define EV_TH XR_EVAL_TILE_H
#define EV_R XR_EVAL_MAX_RADIUS
#define EV_C XR_EVAL_MAX_CHANNELS
#define EV_HR (EV_TH + 2 * EV_R)          // halo rows at the largest radius
#define EV_HC (EV_TW + 2 * EV_R)          // halo columns
static_assert(EV_TW * EV_TH == EV_BLOCK, "one thread per pixel of the tile");
static_assert(2 * EV_HR * EV_HC * EV_C * 4 + 5 * EV_HR * EV_TW * 8 + 2 * EV_WAVES * 8 <= 80 * 1024, "two workgroups per CU");

struct EvArgs {
    const float *x, *y;
    uint32_t B, H, W, C, r, tiles_x, tiles_y;
    int64_t sb, sr, sp, sc;
    double taps[2 * EV_R + 1];
    double cov_norm, C1, C2;
};

// scipy's mode='reflect' (numpy's 'symmetric'): -1 -> 0, -2 -> 1, n -> n-1.  One reflection suffices for the pixels of the image
// (n >= 2 r + 1); the halo of a ragged tile's out-of-image pixels is clamped, and nothing reads what is formed from it
static __device__ inline uint32_t ev_reflect(int i, uint32_t n) {
    if (i < 0) i = -i - 1;
    if (i >= (int)n) i = 2 * (int)n - 1 - i;
    return (uint32_t)(i < 0 ? 0 : (i >= (int)n ? (int)n - 1 : i));
}

// the sum of v over the workgroup, valid in thread 0: butterfly inside a wave, the waves in wave order
static __device__ inline double ev_block_sum(double v, double* s_w) {
    v = xr_wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    double all = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < EV_WAVES; ++w) all += s_w[w];
    return all;
}

static __global__ void __launch_bounds__(EV_BLOCK) k_ev_tiles(EvArgs a, double* __restrict__ map, double* __restrict__ part) {
    __shared__ float s_x[EV_HR * EV_HC * EV_C], s_y[EV_HR * EV_HC * EV_C];
    __shared__ double s_h[5][EV_HR][EV_TW];
    __shared__ double s_w[2][EV_WAVES];
    const uint32_t tile = blockIdx.x, tid = threadIdx.x;
    const uint32_t per = a.tiles_x * a.tiles_y;
    const uint32_t b = tile / per, t2 = tile - b * per;
    const uint32_t ty0 = (t2 / a.tiles_x) * EV_TH, tx0 = (t2 % a.tiles_x) * EV_TW;
    const int r = (int)a.r, win = 2 * r + 1;
    const uint32_t hr = EV_TH + 2 * a.r, hc = EV_TW + 2 * a.r, C = a.C;
    const float* xb = a.x + (int64_t)b * a.sb;
    const float* yb = a.y + (int64_t)b * a.sb;
    // the tile and its halo, channel fastest (the order of a channel-last image's memory)
    for (uint32_t i = tid; i < hr * hc * C; i += EV_BLOCK) {
        const uint32_t c = i % C, q = i / C, col = q % hc, row = q / hc;
        const uint32_t gy = ev_reflect((int)(ty0 + row) - r, a.H), gx = ev_reflect((int)(tx0 + col) - r, a.W);
        const int64_t at = (int64_t)gy * a.sr + (int64_t)gx * a.sp + (int64_t)c * a.sc;
        s_x[i] = xb[at];
        s_y[i] = yb[at];
    }
    __syncthreads();
    const uint32_t lx = tid % EV_TW, ly = tid / EV_TW;
    const uint32_t px = tx0 + lx, py = ty0 + ly;
    const bool inside = px < a.W && py < a.H;
    double sum_s = 0.0, sum_q = 0.0;
    for (uint32_t c = 0; c < C; ++c) {
        // rows: the five moments of (halo row, tile column)
        for (uint32_t i = tid; i < hr * EV_TW; i += EV_BLOCK) {
            const uint32_t col = i % EV_TW, row = i / EV_TW;
            double mx = 0.0, my = 0.0, mxx = 0.0, myy = 0.0, mxy = 0.0;
            for (int k = 0; k < win; ++k) {
                const uint32_t at = (row * hc + col + (uint32_t)k) * C + c;
                const double w = a.taps[k], vx = (double)s_x[at], vy = (double)s_y[at];
                mx += w * vx;
                my += w * vy;
                mxx += w * (vx * vx);
                myy += w * (vy * vy);
                mxy += w * (vx * vy);
            }
            s_h[0][row][col] = mx; s_h[1][row][col] = my; s_h[2][row][col] = mxx; s_h[3][row][col] = myy; s_h[4][row][col] = mxy;
        }
        __syncthreads();
        // columns: the pixel's moments, S and the squared error
        if (inside) {
            double ux = 0.0, uy = 0.0, uxx = 0.0, uyy = 0.0, uxy = 0.0;
            for (int k = 0; k < win; ++k) {
                const double w = a.taps[k];
                ux += w * s_h[0][ly + k][lx];
                uy += w * s_h[1][ly + k][lx];
                uxx += w * s_h[2][ly + k][lx];
                uyy += w * s_h[3][ly + k][lx];
                uxy += w * s_h[4][ly + k][lx];
            }
            const double vx = a.cov_norm * (uxx - ux * ux), vy = a.cov_norm * (uyy - uy * uy), vxy = a.cov_norm * (uxy - ux * uy);
            const double A1 = 2.0 * ux * uy + a.C1, A2 = 2.0 * vxy + a.C2;
            const double B1 = ux * ux + uy * uy + a.C1, B2 = vx + vy + a.C2;
            const double S = (A1 * A2) / (B1 * B2);
            if (map) map[(((size_t)b * a.H + py) * a.W + px) * C + c] = S;
            sum_s += S;
            const uint32_t at = ((ly + a.r) * hc + lx + a.r) * C + c;
            const float d = s_x[at] - s_y[at];                       // rounded to fp32, as numpy rounds x - y
            sum_q += (double)d * (double)d;
        }
        __syncthreads();                                             // s_h is rewritten for the next channel
    }
    const double ts = ev_block_sum(sum_s, s_w[0]), tq = ev_block_sum(sum_q, s_w[1]);
    if (tid == 0) { part[2 * (size_t)tile] = ts; part[2 * (size_t)tile + 1] = tq; }
}

static __global__ void __launch_bounds__(EV_BLOCK) k_ev_fold(uint32_t per, const double* __restrict__ part, double* __restrict__ ssim_sum,
                                                             double* __restrict__ sq_sum) {
    __shared__ double s_w[2][EV_WAVES];
    const uint32_t b = blockIdx.x, run = (per + EV_BLOCK - 1) / EV_BLOCK;
    const uint32_t t0 = threadIdx.x * run, t1 = t0 + run < per ? t0 + run : per;
    double s = 0.0, q = 0.0;
    for (uint32_t t = t0; t < t1; ++t) {
        s += part[2 * ((size_t)b * per + t)];
        q += part[2 * ((size_t)b * per + t) + 1];
    }
    const double ts = ev_block_sum(s, s_w[0]), tq = ev_block_sum(q, s_w[1]);
    if (threadIdx.x == 0) { ssim_sum[b] = ts; sq_sum[b] = tq; }
}

static __global__ void __launch_bounds__(EV_BLOCK) k_ev_to8b(const float* __restrict__ rgb, const float* __restrict__ gt, uint32_t H, uint32_t W,
                                                             uint32_t C, int64_t sr, int64_t sp, int64_t sc, uint8_t* __restrict__ out) {
    const uint32_t ow = gt ? 2 * W : W;
    const uint32_t i = blockIdx.x * EV_BLOCK + threadIdx.x;
    if (i >= H * ow * C) return;
    const uint32_t c = i % C, q = i / C, col = q % ow, row = q / ow;
    const float* src = col < W ? rgb : gt;
    const float v = src[(int64_t)row * sr + (int64_t)(col < W ? col : col - W) * sp + (int64_t)c * sc];
    const float clipped = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
    const float p = 255.f * clipped;                                 // the fp32 product numpy forms
    out[i] = p == p ? (uint8_t)(int)p : (uint8_t)0;                 // truncated; NaN -> 0
}

static bool ev_layout(uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint32_t* tiles_x, uint32_t* tiles_y, size_t* bytes) {
    if (B == 0 || H == 0 || W == 0 || C == 0 || C > EV_C) return false;
    if ((uint64_t)B * H * W * C > 0x7fffffffull) return false;
    *tiles_x = xr_div_up(W, EV_TW);
    *tiles_y = xr_div_up(H, EV_TH);
    *bytes = (size_t)B * *tiles_x * *tiles_y * 2 * sizeof(double);
    return true;
}

extern "C" size_t xr_eval_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t C) {
    uint32_t tx, ty;
    size_t bytes;
    return ev_layout(B, H, W, C, &tx, &ty, &bytes) ? bytes : 0;
}

extern "C" int xr_eval_ssim(const float* x, const float* y, uint32_t B, uint32_t H, uint32_t W, uint32_t C, int64_t batch_stride, int64_t row_stride,
                            int64_t pixel_stride, int64_t channel_stride, const double* taps, uint32_t r, double cov_norm, double C1, double C2,
                            double* ssim_sum, double* sq_sum, double* map, void* workspace, size_t workspace_bytes, void* stream) {
    EvArgs a;
    size_t bytes;
    XR_REQUIRE(x && y && taps && ssim_sum && sq_sum && workspace, "null pointer");
    XR_REQUIRE(r <= EV_R, "the window radius is at most XR_EVAL_MAX_RADIUS");
    XR_REQUIRE(C >= 1 && C <= EV_C, "1 .. XR_EVAL_MAX_CHANNELS channels");
    XR_REQUIRE(H >= 2 * r + 1 && W >= 2 * r + 1, "win_size exceeds image extent");
    XR_REQUIRE(batch_stride >= 0 && row_stride >= 0 && pixel_stride >= 0 && channel_stride >= 0, "negative stride");
    XR_REQUIRE(ev_layout(B, H, W, C, &a.tiles_x, &a.tiles_y, &bytes), "sizes: B >= 1, B H W C within int32");
    XR_REQUIRE(((uintptr_t)workspace & 7u) == 0, "the workspace must be 8-byte aligned");
    if (workspace_bytes < bytes) { xr_set_error("%s: workspace too small", __func__); return XR_ENOMEM; }
    a.x = x; a.y = y; a.B = B; a.H = H; a.W = W; a.C = C; a.r = r;
    a.sb = batch_stride; a.sr = row_stride; a.sp = pixel_stride; a.sc = channel_stride;
    for (uint32_t k = 0; k < 2 * EV_R + 1; ++k) a.taps[k] = k < 2 * r + 1 ? taps[k] : 0.0;
    a.cov_norm = cov_norm; a.C1 = C1; a.C2 = C2;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t per = a.tiles_x * a.tiles_y;
    double* part = (double*)workspace;
    hipLaunchKernelGGL(k_ev_tiles, dim3(B * per), dim3(EV_BLOCK), 0, st, a, map, part);
    hipLaunchKernelGGL(k_ev_fold, dim3(B), dim3(EV_BLOCK), 0, st, per, (const double*)part, ssim_sum, sq_sum);
    XR_LAUNCH_CHECK();
    return 0;
}

extern "C" int xr_eval_to8b_pair(const float* rgb, const float* gt, uint32_t H, uint32_t W, uint32_t C, int64_t row_stride, int64_t pixel_stride,
                                 int64_t channel_stride, uint8_t* out, void* stream) {
    XR_REQUIRE(rgb && out, "null pointer");
    XR_REQUIRE(H >= 1 && W >= 1 && C >= 1 && C <= EV_C, "H, W >= 1 and 1 .. XR_EVAL_MAX_CHANNELS channels");
    XR_REQUIRE(row_stride >= 0 && pixel_stride >= 0 && channel_stride >= 0, "negative stride");
    XR_REQUIRE(2ull * H * W * C <= 0x7fffffffull, "2 H W C within int32");
    const uint32_t n = H * (gt ? 2 * W : W) * C;
    hipLaunchKernelGGL(k_ev_to8b, dim3(xr_div_up(n, EV_BLOCK)), dim3(EV_BLOCK), 0, (hipStream_t)stream, rgb, gt, H, W, C, row_stride, pixel_stride,
                       channel_stride, out);
    XR_LAUNCH_CHECK();
    return 0;
}
