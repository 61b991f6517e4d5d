// BungeeGetBounds + BungeeGetZvals (datasets/pipelines/create.py) as device functions: the one copy that k_bungee_zvals (xr_bungee.hip,
// thread = ray) and the fused data kernels (xr_bungeedata.hip, thread = (ray, edge)) both run.  Every expression is fp32 in the
// reference's operation order; the sources that include this are built with -ffp-contract=off.
#ifndef XR_BUNGEE_ZVALS_H
#define XR_BUNGEE_ZVALS_H
#include "xr_mip_math.h"

struct BgBounds {
    int mode;                                // 0 none, 1 sphere, 2 flat
    float cx, cy, cz;                        // float32(scene_origin * scaling)
    float r2_top, r2_earth;                  // float32(((6371011 + 250) s)^2), float32((6371011 s)^2)
    float s;                                 // float32(scaling)
};

// torch.norm(x, dim=-1) of a 3-vector: sqrt of the sequential sum of squares
static __device__ inline float bg_norm3(float x, float y, float z) { return sqrtf(x * x + y * y + z * z); }

// create.py BungeeGetBounds, sphere: the smaller root of |o + t v - c|^2 = r^2 in the reference's expression order
static __device__ inline float bg_sphere_dist(const float oc[3], const float o[3], const float v[3], float b, float nv2, float r2) {
    const float no = bg_norm3(oc[0], oc[1], oc[2]);
    const float tb = 2.f * b;
    const float delta = tb * tb - 4.f * nv2 * (no * no - r2);
    const float t = (-2.f * b - sqrtf(delta)) / (2.f * nv2);
    // |o - (o + t v)|
    const float e[3] = {o[0] - (o[0] + t * v[0]), o[1] - (o[1] + t * v[1]), o[2] - (o[2] + t * v[2])};
    return bg_norm3(e[0], e[1], e[2]);
}

// near and far of one ray, modes 1 (sphere) and 2 (flat)
static __device__ inline void bg_bounds(const BgBounds& a, const float o[3], const float v[3], float* near, float* far) {
    float nr, fr;
    if (a.mode == 1) {
        const float oc[3] = {o[0] - a.cx, o[1] - a.cy, o[2] - a.cz};
        const float b = oc[0] * v[0] + oc[1] * v[1] + oc[2] * v[2];
        const float nv = bg_norm3(v[0], v[1], v[2]);
        const float nv2 = nv * nv;
        nr = bg_sphere_dist(oc, o, v, b, nv2, a.r2_top) * 0.9f;
        fr = bg_sphere_dist(oc, o, v, b, nv2, a.r2_earth) * 1.1f;
    } else {
        // planes z = 250 s (near) and z = 0 (far); the x / y terms of the reference's dot products are signed zeros
        const float den = v[2] * a.s;
        const float oz = o[2] * a.s;
        nr = (250.f * a.s - oz) / den;
        fr = (0.f - oz) / den;
        nr = nr != nr ? nr : fmaxf(nr, 1e-6f);                           // clamp(min=1e-6) keeps NaN
    }
    *near = nr; *far = fr;
}

// BungeeGetZvals: the first n1 = floor(2N/3) edges linear in disparity, the rest linear in depth from edge n1-1 to far
static __device__ inline uint32_t bg_n_disparity(uint32_t N) { return (2u * N) / 3u; }

// edge j >= 1 of the n2 = N - n1 + 1 depth-linear ones that start at edge n1-1 (`start`)
static __device__ inline float bg_zval_linear(float start, float far, uint32_t n2, uint32_t j) {
    const float t = xr_torch_linspace(0.f, 1.f, n2, j);
    return start * (1.f - t) + far * t;
}

// edge j of the row before the sort
static __device__ inline float bg_zval_edge(float near, float far, uint32_t N, uint32_t j) {
    const uint32_t n1 = bg_n_disparity(N);
    if (j < n1) return xr_mip_zval(near, far, N, j, 1);
    return bg_zval_linear(xr_mip_zval(near, far, N, n1 - 1, 1), far, N - n1 + 1, j - n1 + 1);
}

// the sort's order (torch.sort: ascending, NaN last): a goes before b
static __device__ inline bool bg_before(float a, float b) { return a < b || (b != b && a == a); }

// the whole row of one ray into z[0 .. N)
static __device__ inline void bg_zvals_row(float nr, float fr, uint32_t N, float* z) {
    const uint32_t n1 = bg_n_disparity(N), n2 = N - n1 + 1;
    for (uint32_t j = 0; j < n1; ++j) z[j] = xr_mip_zval(nr, fr, N, j, 1);
    const float start = z[n1 - 1];
    for (uint32_t j = 1; j < n2; ++j) z[n1 + j - 1] = bg_zval_linear(start, fr, n2, j);
    // insertion sort; the edges are almost always in order already, so this is one pass
    for (uint32_t j = 1; j < N; ++j) {
        const float v = z[j];
        uint32_t k = j;
        while (k > 0 && bg_before(v, z[k - 1])) { z[k] = z[k - 1]; --k; }
        z[k] = v;
    }
}
#endif
