// GNR's body depth maps for gfx950: the z-buffer rasteriser and per-vertex visibility of the reference's extensions/mesh_grid
// (render.h: zbuffer_forward, process_one_tri, normalize_coeff), restated with its arithmetic order and its quirks.
// The reference's GPU form is one block of 512 threads with a device-side malloc behind a spin lock per pixel; here
//   k_rs_init     thread = pixel: the z-buffer key to "empty", the per-pixel vertex count to 0
//   k_rs_verts    thread = (view, vertex): project (x / z, y / z with persp), floor -> the vertex's pixel or none; `visual` starts as
//                 "lies in the image"; the pixel's count grows by one (integer atomicAdd, whose return value is the vertex's slot)
//   scan          xr_scan.h's two-level exclusive scan of the counts -> the CSR row starts (this replaces the reference's vector_gpu)
//   k_rs_fill     thread = (view, vertex): the vertex into its pixel's row at its slot
//   k_rs_faces    wave = (view, triangle): every lane sets the triangle up (process_one_tri), the lanes stride over the clipped bounding
//                 box -- a triangle that covers the whole image costs what its pixels cost.  Per pixel: the key
//                 (order-preserving bits of z) << 32 | face into a 64-bit atomicMin (strict order on z, then the lowest face: the
//                 serial loop's `zbuf > z`), then the pixel's vertex row: a vertex that is no corner of the face, lies inside it by
//                 normalize_coeff and has z_face <= z_vertex is hidden
//   k_rs_resolve  thread = pixel: the winner's coefficients and z recomputed by the same device functions (same operations, same
//                 bits), written with the face index; -1 / 0 / 0 where empty
// No device-side allocation, no locks, no floating-point atomics; `visual` is only ever cleared: the same input gives the same bits.
// Built with -ffp-contract=off: inside / outside is a comparison of c = A0 u + A3 v + A6 with -eps, and the stored coefficients are
// compared bit for bit with the reference's host build.
#include "xr_common.h"
#define XR_SCAN_TWO_LEVEL
#include "xr_scan.h"
#include "../../include/xrnerf_mi355_gnr_raster.h"
#include <cfloat>

#define RS_BLOCK 256
static_assert(RS_BLOCK == XR_SCAN_BLOCK, "the shared workgroup routines are written for 256 threads");
#define RS_WAVES (RS_BLOCK / 64)
#define RS_EMPTY 0xffffffffffffffffull

struct RsArgs {
    const float* verts;         // [V,N,3]
    const int32_t* faces;       // [F,3]
    uint32_t V, N, F, H, W;
    int persp, double_face;
    float eps;
};

// process_one_tri's result: Ainv, the type (7 full; 3 / 5 / 6 line; 1 / 2 / 4 point), the clipped box, the corners and their z
struct RsTri {
    float A[9], z0, z1, z2;
    int type, x0, x1, y0, y1;
    uint32_t i0, i1, i2;
};

// the line triangle whose longest side is opposite corner I (render.h:86-95)
template <int I> static __device__ inline void rs_line(const float* v, float l2, float* A) {
    constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
    A[J] = -(A[K] = (v[3 * K] - v[3 * J]) / l2);
    A[J + 3] = -(A[K + 3] = (v[3 * K + 1] - v[3 * J + 1]) / l2);
    A[J + 6] = (v[3 * K] * (v[3 * K] - v[3 * J]) + v[3 * K + 1] * (v[3 * K + 1] - v[3 * J + 1])) / l2;
    A[K + 6] = (v[3 * J] * (v[3 * J] - v[3 * K]) + v[3 * J + 1] * (v[3 * J + 1] - v[3 * K + 1])) / l2;
    const float l = __fsqrt_rn(l2);
    A[I] = (v[3 * J + 1] - v[3 * K + 1]) / l;
    A[I + 3] = (v[3 * K] - v[3 * J]) / l;
    A[I + 6] = (v[3 * J] * v[3 * K + 1] - v[3 * K] * v[3 * J + 1]) / l;
}

// zbuffer_forward's lines in front of the pixel loop and process_one_tri: false = the face draws nothing.  Deviations, all on inputs
// the reference has no defined answer for: a corner index outside 0 .. N-1 drops the face, and so does a box that is not finite
// (the reference casts it to an integer).
static __device__ inline bool rs_setup(const RsArgs& a, const float* vv, uint32_t f, RsTri* t) {
    const uint32_t i0 = (uint32_t)a.faces[3 * (uint64_t)f], i1 = (uint32_t)a.faces[3 * (uint64_t)f + 1], i2 = (uint32_t)a.faces[3 * (uint64_t)f + 2];
    if (i0 >= a.N || i1 >= a.N || i2 >= a.N) return false;
    float v[9];
#pragma unroll
    for (int q = 0; q < 3; ++q) { v[q] = vv[3 * (uint64_t)i0 + q]; v[3 + q] = vv[3 * (uint64_t)i1 + q]; v[6 + q] = vv[3 * (uint64_t)i2 + q]; }
    const float eps = a.eps;
    if (a.persp) {
        if (v[2] <= eps || v[5] <= eps || v[8] <= eps) return false;
#pragma unroll
        for (int j = 0; j < 3; ++j) { v[3 * j] /= v[3 * j + 2]; v[3 * j + 1] /= v[3 * j + 2]; }
    }
    float umin = v[0], umax = v[0], vmin = v[1], vmax = v[1];
#pragma unroll
    for (int i = 1; i < 3; ++i) {
        if (umin > v[3 * i]) umin = v[3 * i];
        else if (umax < v[3 * i]) umax = v[3 * i];
        if (vmin > v[3 * i + 1]) vmin = v[3 * i + 1];
        else if (vmax < v[3 * i + 1]) vmax = v[3 * i + 1];
    }
    umin = floorf(umin); umax = ceilf(umax); vmin = floorf(vmin); vmax = ceilf(vmax);
    const float bx0 = umin < 0.f ? 0.f : umin, bx1 = umax >= (float)a.W ? (float)(a.W - 1) : umax;
    const float by0 = vmin < 0.f ? 0.f : vmin, by1 = vmax >= (float)a.H ? (float)(a.H - 1) : vmax;
    if (!(bx1 >= bx0) || !(by1 >= by0)) return false;
    t->x0 = (int)bx0; t->x1 = (int)bx1; t->y0 = (int)by0; t->y1 = (int)by1;
    float* A = t->A;
    A[6] = v[3] * v[7] - v[6] * v[4];
    A[7] = v[6] * v[1] - v[0] * v[7];
    A[8] = v[0] * v[4] - v[3] * v[1];
    const float det = A[6] + A[7] + A[8];
    if (!a.double_face && det > eps) return false;
    A[0] = v[4] - v[7];
    A[1] = v[7] - v[1];
    A[2] = v[1] - v[4];
    A[3] = v[6] - v[3];
    A[4] = v[0] - v[6];
    A[5] = v[3] - v[0];
    if (det <= eps && det >= -eps) {
        const float l20 = A[0] * A[0] + A[3] * A[3], l21 = A[1] * A[1] + A[4] * A[4], l22 = A[2] * A[2] + A[5] * A[5];
        int i = l20 > l21 ? 0 : 1;
        float l2 = i == 0 ? l20 : l21;
        if (!(l2 > l22)) { i = 2; l2 = l22; }
        if (l2 > eps * eps) {
            const int j = (i + 1) % 3, k = (j + 1) % 3;
            t->type = (1 << j) + (1 << k);
            if (i == 0) rs_line<0>(v, l2, A);
            else if (i == 1) rs_line<1>(v, l2, A);
            else rs_line<2>(v, l2, A);
        } else {
            t->type = 1 << i;
            A[0] = i == 0 ? v[0] : (i == 1 ? v[3] : v[6]);
            A[1] = i == 0 ? v[1] : (i == 1 ? v[4] : v[7]);
        }
    } else {
        t->type = 7;
#pragma unroll
        for (int i = 0; i < 9; ++i) A[i] /= det;
    }
    t->z0 = v[2]; t->z1 = v[5]; t->z2 = v[8];
    t->i0 = i0; t->i1 = i1; t->i2 = i2;
    return true;
}

// normalize_coeff
static __device__ inline bool rs_coeff(const RsTri& t, float u, float v, float eps, float* c) {
    const float* A = t.A;
    if (t.type == 7 || t.type == 3 || t.type == 5 || t.type == 6) {
        c[0] = A[0] * u + A[3] * v + A[6];
        c[1] = A[1] * u + A[4] * v + A[7];
        c[2] = A[2] * u + A[5] * v + A[8];
        if (t.type == 7) return c[0] >= -eps && c[1] >= -eps && c[2] >= -eps;
        const int i = (7 - t.type) / 2;
        const float ci = i == 0 ? c[0] : (i == 1 ? c[1] : c[2]);
        if (ci * ci > eps * eps) return false;
        bool in = true;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (q == i) c[q] = 0.f;
            else in = in && c[q] >= -eps;
        }
        return in;
    }
    const int i = t.type / 2;                   // 1, 2, 4 -> corner 0, 1, 2
    const float cj = u - A[0], ck = v - A[1];
    if (cj * cj + ck * ck > eps * eps) return false;
#pragma unroll
    for (int q = 0; q < 3; ++q) c[q] = q == i ? 1.f : 0.f;
    return true;
}

// the lines behind a successful normalize_coeff: false where the reference `continue`s (perspective and a sum <= eps).  The
// perspective z is a DOUBLE division rounded to float; the orthographic z takes c[2] twice, as written there.
static __device__ inline bool rs_depth(const RsTri& t, int persp, float eps, float* c, float* z) {
    if (persp) {
        c[0] /= t.z0; c[1] /= t.z1; c[2] /= t.z2;
        const float s = c[0] + c[1] + c[2];
        if (s <= eps) return false;
        c[0] /= s; c[1] /= s; c[2] /= s;
        *z = (float)(1. / (double)s);
    } else {
        *z = c[0] * t.z0 + c[2] * t.z1 + c[2] * t.z2;
    }
    return true;
}

// (z, face) as one integer whose order is: z first (as floats compare; -0 = +0), then the face.  An orthographic z may be negative.
static __device__ inline unsigned long long rs_key(float z, uint32_t f) {
    uint32_t b = z == 0.f ? 0u : __float_as_uint(z);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)b << 32) | f;
}

__global__ void __launch_bounds__(RS_BLOCK) k_rs_init(uint32_t P, unsigned long long* __restrict__ zkey, uint32_t* __restrict__ counts) {
    const uint32_t p = blockIdx.x * RS_BLOCK + threadIdx.x;
    if (p > P) return;
    counts[p] = 0;                              // P + 1 counts: the scan leaves the total in the last one
    if (p < P) zkey[p] = RS_EMPTY;
}

__global__ void __launch_bounds__(RS_BLOCK) k_rs_verts(RsArgs a, uint32_t* __restrict__ counts, int32_t* __restrict__ vpix, uint32_t* __restrict__ vslot,
                                                      uint8_t* __restrict__ visual) {
    const uint32_t id = blockIdx.x * RS_BLOCK + threadIdx.x;
    if (id >= a.V * a.N) return;
    const uint32_t view = id / a.N;
    float x = a.verts[3 * (uint64_t)id], y = a.verts[3 * (uint64_t)id + 1];
    const float z = a.verts[3 * (uint64_t)id + 2];
    bool on = true;
    if (a.persp) {
        if (z <= a.eps) on = false;
        else { x /= z; y /= z; }
    }
    int32_t pix = -1;
    if (on) {
        x = floorf(x); y = floorf(y);
        on = x >= 0.f && y >= 0.f && x < (float)a.W && y < (float)a.H;          // (a coordinate that is not finite lies outside)
        if (on) {
            pix = (int32_t)((view * a.H + (uint32_t)y) * a.W + (uint32_t)x);
            vslot[id] = atomicAdd(&counts[pix], 1u);
        }
    }
    vpix[id] = pix;
    visual[id] = on ? 1 : 0;
}

__global__ void __launch_bounds__(RS_BLOCK) k_rs_fill(uint32_t VN, uint32_t N, const uint32_t* __restrict__ offs, const int32_t* __restrict__ vpix,
                                                     const uint32_t* __restrict__ vslot, uint32_t* __restrict__ list) {
    const uint32_t id = blockIdx.x * RS_BLOCK + threadIdx.x;
    if (id >= VN || vpix[id] < 0) return;
    const uint32_t at = offs[vpix[id]] + vslot[id];
    if (at < VN) list[at] = id % N;             // (the rows hold VN entries in all: the test never fails)
}

__global__ void __launch_bounds__(RS_BLOCK) k_rs_faces(RsArgs a, const uint32_t* __restrict__ offs, const uint32_t* __restrict__ list,
                                                      unsigned long long* __restrict__ zkey, uint8_t* __restrict__ visual) {
    const uint64_t wid = (uint64_t)blockIdx.x * RS_WAVES + (threadIdx.x >> 6);
    if (wid >= (uint64_t)a.V * a.F) return;
    const uint32_t view = (uint32_t)(wid / a.F), f = (uint32_t)(wid % a.F), lane = threadIdx.x & 63;
    const float* vv = a.verts + 3 * (uint64_t)view * a.N;
    RsTri t;
    if (!rs_setup(a, vv, f, &t)) return;
    const uint32_t bw = (uint32_t)(t.x1 - t.x0 + 1), npx = bw * (uint32_t)(t.y1 - t.y0 + 1);
    for (uint32_t i = lane; i < npx; i += 64) {
        const int x = t.x0 + (int)(i % bw), y = t.y0 + (int)(i / bw);
        const uint32_t p = (view * a.H + (uint32_t)y) * a.W + (uint32_t)x;
        float c[3], z;
        if (rs_coeff(t, (float)x, (float)y, a.eps, c)) {
            if (!rs_depth(t, a.persp, a.eps, c, &z)) continue;           // (the reference's `continue` skips the pixel's vertices too)
            if (z < FLT_MAX) atomicMin(&zkey[p], rs_key(z, f));         // the buffer starts at FLT_MAX and only `zbuf > z` wins
        }
        const uint32_t end = offs[p + 1];
        for (uint32_t k = offs[p]; k < end; ++k) {
            const uint32_t vi = list[k];
            if (vi == t.i0 || vi == t.i1 || vi == t.i2) continue;
            float u = vv[3 * (uint64_t)vi], w = vv[3 * (uint64_t)vi + 1];
            const float vz = vv[3 * (uint64_t)vi + 2];
            if (a.persp) { u /= vz; w /= vz; }
            if (rs_coeff(t, u, w, a.eps, c)) {
                if (!rs_depth(t, a.persp, a.eps, c, &z)) continue;
                if (z <= vz) visual[(uint64_t)view * a.N + vi] = 0;
            }
        }
    }
}

__global__ void __launch_bounds__(RS_BLOCK) k_rs_resolve(RsArgs a, const unsigned long long* __restrict__ zkey, int64_t* __restrict__ index,
                                                        float* __restrict__ coeff, float* __restrict__ depth) {
    const uint32_t p = blockIdx.x * RS_BLOCK + threadIdx.x;
    if (p >= a.V * a.H * a.W) return;
    const unsigned long long key = zkey[p];
    int64_t win = -1;
    float c[3] = {0.f, 0.f, 0.f}, z = 0.f;
    if (key != RS_EMPTY) {
        const uint32_t f = (uint32_t)key, view = p / (a.H * a.W), y = p / a.W % a.H, x = p % a.W;
        RsTri t;
        if (rs_setup(a, a.verts + 3 * (uint64_t)view * a.N, f, &t) && rs_coeff(t, (float)x, (float)y, a.eps, c) && rs_depth(t, a.persp, a.eps, c, &z))
            win = (int64_t)f;
        else { c[0] = c[1] = c[2] = 0.f; z = 0.f; }                    // (the same operations found the winner: never taken)
    }
    index[p] = win;
    coeff[3 * (uint64_t)p] = c[0]; coeff[3 * (uint64_t)p + 1] = c[1]; coeff[3 * (uint64_t)p + 2] = c[2];
    depth[p] = z;
}

// ------------------------------------------------------------------------------------------ entry points
struct RsLayout { uint64_t P, VN, n2; size_t zkey, counts, sums, total, vpix, vslot, list, bytes; };

static bool rs_layout(uint32_t V, uint32_t N, uint32_t H, uint32_t W, RsLayout* l) {
    if (V < 1 || N < 1 || H < 1 || W < 1 || H > XR_GNR_RASTER_MAX_SIDE || W > XR_GNR_RASTER_MAX_SIDE || N > 0x7fffffffu) return false;
    l->P = (uint64_t)V * H * W;
    l->VN = (uint64_t)V * N;
    if (l->P >= 0x7fffffffull || l->VN > 0x7fffffffull) return false;
    l->n2 = xr_div_up(l->P + 1, XR_SCAN_BLOCK);
    auto up8 = [](size_t b) { return (b + 7) & ~(size_t)7; };
    size_t at = 0;
    l->zkey = at; at += 8 * l->P;
    l->counts = at; at = up8(at + 4 * (l->P + 1));
    l->sums = at; at = up8(at + 4 * (l->n2 + xr_div_up(l->n2, XR_SCAN_BLOCK) + 1));
    l->total = at; at += 8;
    l->vpix = at; at = up8(at + 4 * l->VN);
    l->vslot = at; at = up8(at + 4 * l->VN);
    l->list = at; at = up8(at + 4 * l->VN);
    l->bytes = at;
    return true;
}

extern "C" size_t xr_gnr_raster_workspace_bytes(uint32_t V, uint32_t N, uint32_t H, uint32_t W) {
    RsLayout l;
    return rs_layout(V, N, H, W, &l) ? l.bytes : 0;
}

extern "C" int xr_gnr_raster_forward(const float* verts, uint32_t V, uint32_t N, const int32_t* faces, uint32_t F, uint32_t H, uint32_t W, int persp,
                                     int double_face, float eps, int64_t* index, float* coeff, uint8_t* visual, float* depth, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    RsLayout l;
    XR_REQUIRE(eps >= 0.f, "eps must not be negative");
    XR_REQUIRE(rs_layout(V, N, H, W, &l), "sizes: 1 <= H, W <= XR_GNR_RASTER_MAX_SIDE, V H W and V N within int32");
    XR_REQUIRE(F < 0xffffffffu, "fewer than 2^32 - 1 faces");
    XR_REQUIRE((uint64_t)V * F < (1ull << 33), "V F beyond the launch grid");
    XR_REQUIRE(verts && index && coeff && visual && depth && workspace && (F == 0 || faces), "null pointer");
    XR_REQUIRE(((uintptr_t)workspace & 7u) == 0, "the workspace must be 8-byte aligned");
    if (workspace_bytes < l.bytes) { xr_set_error("%s: workspace too small", __func__); return XR_ENOMEM; }
    char* ws = (char*)workspace;
    unsigned long long* zkey = (unsigned long long*)(ws + l.zkey);
    uint32_t* counts = (uint32_t*)(ws + l.counts);
    uint32_t* sums = (uint32_t*)(ws + l.sums);
    int32_t* total = (int32_t*)(ws + l.total);
    int32_t* vpix = (int32_t*)(ws + l.vpix);
    uint32_t* vslot = (uint32_t*)(ws + l.vslot);
    uint32_t* list = (uint32_t*)(ws + l.list);
    RsArgs a;
    a.verts = verts; a.faces = faces; a.V = V; a.N = N; a.F = F; a.H = H; a.W = W; a.persp = persp != 0; a.double_face = double_face != 0; a.eps = eps;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t P = (uint32_t)l.P, VN = (uint32_t)l.VN;
    hipLaunchKernelGGL(k_rs_init, dim3(xr_div_up(l.P + 1, RS_BLOCK)), dim3(RS_BLOCK), 0, st, P, zkey, counts);
    hipLaunchKernelGGL(k_rs_verts, dim3(xr_div_up(VN, RS_BLOCK)), dim3(RS_BLOCK), 0, st, a, counts, vpix, vslot, visual);
    xr_scan_two_level(st, P + 1, counts, sums, total);
    hipLaunchKernelGGL(k_rs_fill, dim3(xr_div_up(VN, RS_BLOCK)), dim3(RS_BLOCK), 0, st, VN, N, (const uint32_t*)counts, (const int32_t*)vpix,
                       (const uint32_t*)vslot, list);
    if (F > 0)
        hipLaunchKernelGGL(k_rs_faces, dim3(xr_div_up((uint64_t)V * F, RS_WAVES)), dim3(RS_BLOCK), 0, st, a, (const uint32_t*)counts, (const uint32_t*)list, zkey,
                           visual);
    hipLaunchKernelGGL(k_rs_resolve, dim3(xr_div_up(l.P, RS_BLOCK)), dim3(RS_BLOCK), 0, st, a, (const unsigned long long*)zkey, index, coeff, depth);
    XR_LAUNCH_CHECK();
    return 0;
}
