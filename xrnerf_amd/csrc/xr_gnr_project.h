// The projection of a point into GNR's source views and the attention directions of make_att_input: the device functions the hull
// kernels of xr_gnr_render.hip and the reconstruction kernels of xr_gnr_recon.hip share, so that a grid point and a ray sample are
// projected by the same arithmetic (fp32 in the reference's order; both sources are compiled with -ffp-contract=off).
#pragma once
#include "xr_common.h"

struct GrHull {
    const float* rays; const float* t_vals; uint32_t R, S, V;
    const float* w2c; const float* cams; uint32_t cam_cols;
    const float* masks; const float* depth; int H, W;
    float width, height;
    const float* cam_c; const float* rot;
};

// camera-space point of view v, sum_k ascending, then the translation
static __device__ inline void gr_camera(const GrHull& a, uint32_t v, const float* p, float* c) {
    const float* m = a.w2c + 16ull * v;
#pragma unroll
    for (int j = 0; j < 3; ++j) c[j] = ((m[4 * j] * p[0] + m[4 * j + 1] * p[1]) + m[4 * j + 2] * p[2]) + m[4 * j + 3];
}

// perspective() and the normalisation to [-1, 1]: xy[2], and the depth c[2] comes back in *z
static __device__ inline void gr_project(const GrHull& a, uint32_t v, const float* p, float* xy, float* z) {
    float c[3];
    gr_camera(a, v, p, c);
    const float zc = c[2] < 1e-9f ? 1e-9f : c[2];                  // (a NaN depth stays NaN: no comparison holds)
    float x = c[0] / zc, y = c[1] / zc;
    const float* cam = a.cams + (uint64_t)v * a.cam_cols;
    if (a.cam_cols > 6) {
        const float x2 = x * x, y2 = y * y, xy_ = x * y, r2 = x2 + y2;
        const float k = 1.f + r2 * (cam[4] + r2 * (cam[5] + r2 * cam[8]));
        const float dx = cam[6] * 2.f * xy_ + cam[7] * (r2 + 2.f * x2);
        const float dy = cam[7] * 2.f * xy_ + cam[6] * (r2 + 2.f * y2);
        x = k * x + dx;
        y = k * y + dy;
    }
    x = cam[0] * x + cam[2];
    y = cam[1] * y + cam[3];
    xy[0] = x / a.width * 2.f - 1.f;
    xy[1] = y / a.height * 2.f - 1.f;
    *z = c[2];
}

static __device__ inline bool gr_finite(float x) { return x - x == 0.f; }

// grid_sample(mode='nearest', align_corners=False, zero padding): the source pixel of a normalised coordinate, or false
static __device__ inline bool gr_nearest_pixel(float nx, float ny, int H, int W, int* px, int* py) {
    if (!gr_finite(nx) || !gr_finite(ny)) return false;
    const float fx = rintf(((nx + 1.f) * (float)W - 1.f) / 2.f), fy = rintf(((ny + 1.f) * (float)H - 1.f) / 2.f);
    if (!(fx >= 0.f && fx <= (float)(W - 1) && fy >= 0.f && fy <= (float)(H - 1))) return false;
    *px = (int)fx; *py = (int)fy;
    return true;
}

// make_att_input, perspective branch: [query direction q | camera centres - point], through rot, over clamp(norm, 1e-9) -> out [V + 1, 3]
static __device__ inline void gr_att_directions(const GrHull& a, const float* p, const float* q, float* out) {
    float rot[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) rot[c] = a.rot ? a.rot[c] : ((c == 0 || c == 4 || c == 8) ? 1.f : 0.f);
    for (uint32_t v = 0; v <= a.V; ++v) {
        float d[3], y[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = v == 0 ? q[c] : a.cam_c[3ull * (v - 1) + c] - p[c];
        if (a.rot) {
#pragma unroll
            for (int j = 0; j < 3; ++j) y[j] = (d[0] * rot[j] + d[1] * rot[3 + j]) + d[2] * rot[6 + j];
        } else { y[0] = d[0]; y[1] = d[1]; y[2] = d[2]; }
        float n = sqrtf((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]);
        if (n < 1e-9f) n = 1e-9f;
        out[3 * v] = y[0] / n; out[3 * v + 1] = y[1] / n; out[3 * v + 2] = y[2] / n;
    }
}
