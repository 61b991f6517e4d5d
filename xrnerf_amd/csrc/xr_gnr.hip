// GNR body-shape queries (configs/gnr/gnr_genebody.py) for gfx950: what the `mesh_grid` extension (MeshGridSearcher) and the embedding
// half of GnrRenderer.make_nerf_input are to the reference.  The reference's kernels are the specification, quirks included
// (DESIGN.md section 14); every expression below is fp32 in the reference's order, compiled with -ffp-contract=off.
//   k_gnr_count / k_gnr_fill   thread = face: the cells of the face's box, enumerated with the reference's double-precision
//                              `k / (width + 1e-8)` truncation (some cells get the face twice, others never); integer atomic adds on the
//                              cell's count / cursor
//   k_gnr_sort                 thread = cell: insertion sort of its segment (tens of entries): the reference's serial fill order
//   k_gnr_nearest              thread = point: shells of cells in Linf order, per face the Lagrange-multiplier solve gnr_proj
//   k_gnr_inside               thread = point: cells toward the nearest grid face, distinct crossed faces in a 15-entry buffer
//   k_gnr_embed                thread = point: normalised point, T-pose mean, SDF direction and tanh(20 sdf)
// The per-thread arrays (the 4x4 / 3x3 systems, the Gram matrix, the visited buffer) are indexed with compile-time constants only --
// a dynamic row or entry is a chain of selects -- so they live in registers (profiles/gnr_resources.txt).
#include "xr_common.h"
#include "../../include/xrnerf_mi355_gnr.h"

#define GNR_BLOCK 256
#define GNR_ABS(a) ((a) < 0 ? -(a) : (a))
#define GNR_EPS 1e-9f

struct GnrGrid {
    const float* verts; const int32_t* faces; uint32_t V, F;
    float step; float mn[3]; int n[3]; int cells;
    const int32_t* tri_num; const int32_t* tri_idx; int32_t total;
};

static int gnr_grid(GnrGrid* g, const char* fn, const float* verts, const int32_t* faces, uint32_t V, uint32_t F, float step, const float* min3,
                    const int32_t* num3) {
    if (!verts || !faces || !min3 || !num3) { xr_set_error("%s: null pointer", fn); return XR_EINVAL; }
    if (!(step > 0.f) || !(step <= 3.0e38f)) { xr_set_error("%s: the cell edge must be positive and finite (a flat mesh has none)", fn); return XR_EINVAL; }
    if (V == 0 || F == 0 || V > (1u << 30) || F > (1u << 30)) { xr_set_error("%s: bad vertex or face count", fn); return XR_EINVAL; }
    uint64_t cells = 1;
    for (int d = 0; d < 3; ++d) {
        if (num3[d] < 1) { xr_set_error("%s: cells per axis must be >= 1", fn); return XR_EINVAL; }
        cells *= (uint64_t)num3[d];
        if (cells > (uint64_t)XR_GNR_MAX_CELLS) { xr_set_error("%s: more than XR_GNR_MAX_CELLS cells", fn); return XR_EINVAL; }
        if (!(min3[d] == min3[d])) { xr_set_error("%s: the grid corner is not a number", fn); return XR_EINVAL; }
        g->mn[d] = min3[d]; g->n[d] = num3[d];
    }
    g->verts = verts; g->faces = faces; g->V = V; g->F = F; g->step = step; g->cells = (int)cells;
    g->tri_num = nullptr; g->tri_idx = nullptr; g->total = 0;
    return 0;
}

// ------------------------------------------------------------------------------------------ grid build
// x < 0 ? 0 : (x >= n ? n - 1 : floor(x)); a NaN coordinate (no comparison holds) goes to cell 0 instead of through a conversion
static __device__ inline int gnr_box_cell(float x, int n) {
    if (x < 0.f) return 0;
    if (x >= (float)n) return n - 1;
    if (!(x == x)) return 0;
    return (int)floorf(x);
}

// the face's box of cells: lo[d], width w[d] >= 1.  false: a vertex id outside [0, V)
static __device__ inline bool gnr_face_box(const GnrGrid& g, uint32_t f, int* lo, int* w) {
    const int32_t v0 = g.faces[3ull * f], v1 = g.faces[3ull * f + 1], v2 = g.faces[3ull * f + 2];
    if (v0 < 0 || v1 < 0 || v2 < 0 || (uint32_t)v0 >= g.V || (uint32_t)v1 >= g.V || (uint32_t)v2 >= g.V) return false;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        float a = g.verts[3ull * (uint32_t)v0 + d], b = a;
        const float x1 = g.verts[3ull * (uint32_t)v1 + d], x2 = g.verts[3ull * (uint32_t)v2 + d];
        if (a > x1) a = x1; else if (b < x1) b = x1;
        if (a > x2) a = x2; else if (b < x2) b = x2;
        lo[d] = gnr_box_cell((a - g.mn[d]) / g.step, g.n[d]);
        w[d] = gnr_box_cell((b - g.mn[d]) / g.step, g.n[d]) + 1 - lo[d];
    }
    return true;
}

// the j-th cell of the box, the reference's way: the quotient is taken in double by (width + 1e-8) and truncated, so for k an exact
// multiple of the width it comes out one too small
static __device__ inline int gnr_box_item(const GnrGrid& g, const int* lo, const int* w, int j) {
    int ind = 0, k = j;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if (d > 0) ind *= g.n[d];
        ind += lo[d] + k % w[d];
        k = (int)((double)k / ((double)w[d] + 1e-8));
    }
    return ind;
}

__global__ void __launch_bounds__(GNR_BLOCK) k_gnr_count(GnrGrid g, int32_t* __restrict__ count, int32_t* __restrict__ status) {
    const uint32_t f = blockIdx.x * GNR_BLOCK + threadIdx.x;
    if (f >= g.F) return;
    int lo[3], w[3];
    if (!gnr_face_box(g, f, lo, w)) { atomicMax(status + 1, (int32_t)1); return; }
    const int items = w[0] * w[1] * w[2];
    for (int j = 0; j < items; ++j) {
        const int ind = gnr_box_item(g, lo, w, j);
        if (ind >= 0 && ind < g.cells) atomicAdd(count + ind, (int32_t)1);
    }
}

__global__ void __launch_bounds__(GNR_BLOCK) k_gnr_fill(GnrGrid g, int32_t* __restrict__ cursor, int32_t* __restrict__ tri_idx) {
    const uint32_t f = blockIdx.x * GNR_BLOCK + threadIdx.x;
    if (f >= g.F) return;
    int lo[3], w[3];
    if (!gnr_face_box(g, f, lo, w)) return;
    const int items = w[0] * w[1] * w[2];
    for (int j = 0; j < items; ++j) {
        const int ind = gnr_box_item(g, lo, w, j);
        if (ind < 0 || ind >= g.cells) continue;
        const int32_t b = ind == 0 ? 0 : g.tri_num[ind - 1], e = g.tri_num[ind];
        const int32_t slot = b + atomicAdd(cursor + ind, (int32_t)1);
        if (slot >= 0 && slot < e && slot < g.total) tri_idx[slot] = (int32_t)f + 1;
    }
}

__global__ void __launch_bounds__(GNR_BLOCK) k_gnr_sort(GnrGrid g, int32_t* __restrict__ tri_idx) {
    const uint32_t c = blockIdx.x * GNR_BLOCK + threadIdx.x;
    if (c >= (uint32_t)g.cells) return;
    int32_t b = c == 0 ? 0 : g.tri_num[c - 1], e = g.tri_num[c];
    if (b < 0) b = 0;
    if (e > g.total) e = g.total;
    for (int32_t i = b + 1; i < e; ++i) {
        const int32_t v = tri_idx[i];
        int32_t j = i;
        while (j > b && tri_idx[j - 1] > v) { tri_idx[j] = tri_idx[j - 1]; --j; }
        tri_idx[j] = v;
    }
}

extern "C" int xr_gnr_grid_count(const float* verts, const int32_t* faces, uint32_t V, uint32_t F, float step, const float* min3,
                                 const int32_t* num3, int32_t* tri_num, int32_t* status, void* stream) {
    if (F == 0) return 0;
    GnrGrid g;
    const int rc = gnr_grid(&g, __func__, verts, faces, V, F, step, min3, num3);
    if (rc != 0) return rc;
    XR_REQUIRE(tri_num && status, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    XR_HIP(hipMemsetAsync(tri_num, 0, (size_t)g.cells * sizeof(int32_t), st));
    XR_HIP(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_gnr_count, dim3(xr_div_up(F, GNR_BLOCK)), dim3(GNR_BLOCK), 0, st, g, tri_num, status);
    XR_LAUNCH_CHECK();
    return 0;
}

extern "C" int xr_gnr_grid_fill(const float* verts, const int32_t* faces, uint32_t V, uint32_t F, float step, const float* min3,
                                const int32_t* num3, const int32_t* tri_num, int32_t total, int32_t* tri_idx, int32_t* cursor, void* stream) {
    if (F == 0 || total == 0) return 0;
    GnrGrid g;
    const int rc = gnr_grid(&g, __func__, verts, faces, V, F, step, min3, num3);
    if (rc != 0) return rc;
    XR_REQUIRE(tri_num && tri_idx && cursor && total > 0, "null pointer or negative slot count");
    g.tri_num = tri_num; g.total = total;
    hipStream_t st = (hipStream_t)stream;
    XR_HIP(hipMemsetAsync(cursor, 0, (size_t)g.cells * sizeof(int32_t), st));
    XR_HIP(hipMemsetAsync(tri_idx, 0, (size_t)total * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_gnr_fill, dim3(xr_div_up(F, GNR_BLOCK)), dim3(GNR_BLOCK), 0, st, g, cursor, tri_idx);
    hipLaunchKernelGGL(k_gnr_sort, dim3(xr_div_up((uint32_t)g.cells, GNR_BLOCK)), dim3(GNR_BLOCK), 0, st, g, tri_idx);
    XR_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------ the closest-point solve
static __device__ inline void gnr_swapf(float& a, float& b) { const float t = a; a = b; b = t; }

// The reference's 4x4 elimination for the system the closest-point solve gives it: unknown c, equation r at A[4 c + r], the first
// unknown's column ends in 1, so its pivot is never below eps and that stage never loses rank (its three fallbacks are not restated).
// Per stage: the pivot row comes to the front, the rows behind it lose f = a_r / a_pivot times it -- the reference's in-place
// `t = x_p; x_p = x_0 - f t; x_0 = t` with the same operands.  A pivot <= eps moves the unknown to the back (perm*) and lowers the rank.
static __device__ inline bool gnr_solve4(float* A, float* b, float eps) {
    int rank = 4, perm2 = 2, perm3 = 3, pv = 0;
    float best = A[0];
    if (GNR_ABS(best) < GNR_ABS(A[1])) { pv = 1; best = A[1]; }
    if (GNR_ABS(best) < GNR_ABS(A[2])) { pv = 2; best = A[2]; }
    if (GNR_ABS(best) < GNR_ABS(A[3])) { pv = 3; best = A[3]; }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (pv == 1) gnr_swapf(A[4 * c], A[4 * c + 1]);
        else if (pv == 2) gnr_swapf(A[4 * c], A[4 * c + 2]);
        else if (pv == 3) gnr_swapf(A[4 * c], A[4 * c + 3]);
    }
    if (pv == 1) gnr_swapf(b[0], b[1]);
    else if (pv == 2) gnr_swapf(b[0], b[2]);
    else if (pv == 3) gnr_swapf(b[0], b[3]);
#pragma unroll
    for (int r = 1; r < 4; ++r) {
        const float f = A[r] / A[0];
        A[4 + r] = A[4 + r] - f * A[4];
        A[8 + r] = A[8 + r] - f * A[8];
        A[12 + r] = A[12 + r] - f * A[12];
        b[r] = b[r] - f * b[0];
    }
    // second unknown
#define GNR_PIVOT2() do { pv = 1; best = A[5]; \
        if (GNR_ABS(best) < GNR_ABS(A[6])) { pv = 2; best = A[6]; } \
        if (GNR_ABS(best) < GNR_ABS(A[7])) { pv = 3; best = A[7]; } } while (0)
    GNR_PIVOT2();
    if (GNR_ABS(best) <= eps) {
#pragma unroll
        for (int r = 0; r < 4; ++r) gnr_swapf(A[4 + r], A[12 + r]);
        perm3 = 1; rank = 3;
        GNR_PIVOT2();
        if (GNR_ABS(best) <= eps) {
#pragma unroll
            for (int r = 0; r < 4; ++r) gnr_swapf(A[4 + r], A[8 + r]);
            perm2 = 1; rank = 2;
            GNR_PIVOT2();
        }
    }
#undef GNR_PIVOT2
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        if (pv == 2) gnr_swapf(A[4 * c + 1], A[4 * c + 2]);
        else if (pv == 3) gnr_swapf(A[4 * c + 1], A[4 * c + 3]);
    }
    if (pv == 2) gnr_swapf(b[1], b[2]);
    else if (pv == 3) gnr_swapf(b[1], b[3]);
#pragma unroll
    for (int r = 2; r < 4; ++r) {
        const float f = A[4 + r] / A[5];
        A[8 + r] = A[8 + r] - f * A[9];
        A[12 + r] = A[12 + r] - f * A[13];
        b[r] = b[r] - f * b[1];
    }
    // third unknown
    if (rank > 2) {
        pv = GNR_ABS(A[10]) < GNR_ABS(A[11]) ? 3 : 2;
        best = pv == 3 ? A[11] : A[10];
        if (GNR_ABS(best) <= eps) {
            if (rank > 3) {
#pragma unroll
                for (int r = 0; r < 4; ++r) gnr_swapf(A[8 + r], A[12 + r]);
                perm3 = 2; rank = 3;
                pv = GNR_ABS(A[10]) < GNR_ABS(A[11]) ? 3 : 2;
                best = pv == 3 ? A[11] : A[10];
                if (GNR_ABS(best) <= eps) { perm2 = 2; rank = 2; }
            } else {
                perm2 = 2; rank = 2;
            }
        }
    }
    if (rank > 2) {
        if (pv == 3) { gnr_swapf(A[10], A[11]); gnr_swapf(A[14], A[15]); gnr_swapf(b[2], b[3]); }
        const float f = A[11] / A[10];
        A[15] = A[15] - f * A[14];
        b[3] = b[3] - f * b[2];
        if (rank > 3 && GNR_ABS(A[15]) <= eps) { perm3 = 3; rank = 3; }
    }
    bool valid = true;
    if (rank >= 4) b[3] = b[3] / A[15];
    else if (GNR_ABS(b[3]) > eps) valid = false;
    if (rank >= 3) b[2] = (b[2] - A[14] * b[3]) / A[10];
    else if (GNR_ABS(b[1]) > eps) valid = false;                     // (b[1]: the reference's index)
    b[1] = (b[1] - A[9] * b[2] - A[13] * b[3]) / A[5];
    b[0] = (b[0] - A[4] * b[1] - A[8] * b[2] - A[12] * b[3]) / A[0];
    if (rank <= 2 && perm2 == 1) gnr_swapf(b[2], b[1]);
    if (rank <= 3 && perm3 == 1) gnr_swapf(b[3], b[1]);
    else if (rank <= 3 && perm3 == 2) gnr_swapf(b[3], b[2]);
    return valid;
}

// The 3x3 elimination (unknown c, equation r at A[3 c + r]; the first column ends in 1 as well).  The reference tests the second
// pivot on A[pivot] -- the FIRST column, where by then a row factor or the first pivot itself stands -- not on A[pivot + 3]: q1 / q2
// carry what its A[1] / A[2] hold at that point.
static __device__ inline bool gnr_solve3(float* A, float* b, float eps) {
    int rank = 3, perm2 = 2, pv = 0;
    float best = A[0];
    if (GNR_ABS(best) < GNR_ABS(A[1])) { pv = 1; best = A[1]; }
    if (GNR_ABS(best) < GNR_ABS(A[2])) { pv = 2; best = A[2]; }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (pv == 1) gnr_swapf(A[3 * c], A[3 * c + 1]);
        else if (pv == 2) gnr_swapf(A[3 * c], A[3 * c + 2]);
    }
    if (pv == 1) gnr_swapf(b[0], b[1]);
    else if (pv == 2) gnr_swapf(b[0], b[2]);
    const float f1 = A[1] / A[0], f2 = A[2] / A[0];
    A[4] = A[4] - f1 * A[3]; A[7] = A[7] - f1 * A[6]; b[1] = b[1] - f1 * b[0];
    A[5] = A[5] - f2 * A[3]; A[8] = A[8] - f2 * A[6]; b[2] = b[2] - f2 * b[0];
    const float q1 = pv == 1 ? best : f1, q2 = pv == 2 ? best : f2;
    int p2 = GNR_ABS(A[4]) < GNR_ABS(A[5]) ? 2 : 1;
    float q = p2 == 2 ? q2 : q1;
    if (GNR_ABS(q) <= eps) {
#pragma unroll
        for (int r = 0; r < 3; ++r) gnr_swapf(A[3 + r], A[6 + r]);
        perm2 = 1; rank = 2;
        p2 = GNR_ABS(A[4]) < GNR_ABS(A[5]) ? 2 : 1;
        q = p2 == 2 ? q2 : q1;
        if (GNR_ABS(q) <= eps) rank = 1;
    }
    if (rank > 1) {
        if (p2 == 2) { gnr_swapf(A[4], A[5]); gnr_swapf(A[7], A[8]); gnr_swapf(b[1], b[2]); }
        const float f = A[5] / A[4];
        A[8] = A[8] - f * A[7];
        b[2] = b[2] - f * b[1];
        if (rank >= 3 && GNR_ABS(A[8]) <= eps) { perm2 = 2; rank = 2; }
    }
    bool valid = true;
    if (rank >= 3) b[2] = b[2] / A[8];
    else if (GNR_ABS(b[2]) > eps) valid = false;
    if (rank >= 2) b[1] = (b[1] - A[7] * b[2]) / A[4];
    else if (GNR_ABS(b[1]) > eps) valid = false;
    b[0] = (b[0] - A[6] * b[2] - A[3] * b[1]) / A[0];
    if (rank <= 2 && perm2 == 1) gnr_swapf(b[2], b[1]);
    return valid;
}

// co[i] = vi, co[(i + 1) % 3] = vj, co[3 - i - j] = vk
static __device__ inline void gnr_set3(float* co, int i, float vi, float vj, float vk) {
    if (i == 0) { co[0] = vi; co[1] = vj; co[2] = vk; }
    else if (i == 1) { co[1] = vi; co[2] = vj; co[0] = vk; }
    else { co[2] = vi; co[0] = vj; co[1] = vk; }
}

// the closest point of the edge opposite vertex i (G: the Gram matrix of the three vertex offsets)
static __device__ inline float gnr_edge(const float* G, int i, bool checked, float* co) {
    const float gjj = i == 0 ? G[4] : (i == 1 ? G[8] : G[0]);
    const float gkk = i == 0 ? G[8] : (i == 1 ? G[0] : G[4]);
    const float gjk = i == 0 ? G[5] : (i == 1 ? G[6] : G[1]);
    const float gkj = i == 0 ? G[7] : (i == 1 ? G[2] : G[3]);
    float A[9] = {gjj, gjk, 1.f, gkj, gkk, 1.f, 1.f, 1.f, 0.f};
    float b[3] = {0.f, 0.f, 1.f};
    const bool valid = gnr_solve3(A, b, GNR_EPS);
    if (checked && !valid) { gnr_set3(co, i, 0.f, .5f, .5f); return (gjj + gkk) / 2; }
    if (b[0] < 0) { gnr_set3(co, i, 0.f, 0.f, 1.f); return gkk; }
    if (b[1] < 0) { gnr_set3(co, i, 0.f, 1.f, 0.f); return gjj; }
    gnr_set3(co, i, 0.f, b[0], b[1]);
    return GNR_ABS(b[2]);
}

// t: the three vertices minus the query (vertex v, coordinate c at t[3 v + c]) -> barycentric co[3]; returns the multiplier the
// reference ranks candidates by (the squared distance where the solve is regular)
static __device__ inline float gnr_proj(const float* t, float* co) {
    float G[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) s += t[3 * i + k] * t[3 * j + k];
            G[3 * i + j] = s; G[3 * j + i] = s;
        }
    float A[16] = {G[0], G[1], G[2], 1.f, G[3], G[4], G[5], 1.f, G[6], G[7], G[8], 1.f, 1.f, 1.f, 1.f, 0.f};
    float b[4] = {0.f, 0.f, 0.f, 1.f};
    if (!gnr_solve4(A, b, GNR_EPS)) {
        const float e0 = G[4] + G[8] - G[5] - G[7], e1 = G[8] + G[0] - G[6] - G[2], e2 = G[0] + G[4] - G[1] - G[3];
        int i = e0 < e1 ? 1 : 0;
        i = (i == 1 ? e1 : e0) < e2 ? 2 : i;
        return gnr_edge(G, i, true, co);
    }
    int i = b[0] > b[1] ? 1 : 0;
    i = (i == 1 ? b[1] : b[0]) > b[2] ? 2 : i;
    const float bi = i == 0 ? b[0] : (i == 1 ? b[1] : b[2]);
    if (bi < 0) return gnr_edge(G, i, false, co);
    co[0] = b[0]; co[1] = b[1]; co[2] = b[2];
    return GNR_ABS(b[3]);
}

static __device__ inline bool gnr_finite3(const float* p) {
    return fabsf(p[0]) <= 3.4028235e38f && fabsf(p[1]) <= 3.4028235e38f && fabsf(p[2]) <= 3.4028235e38f;
}

// the three vertices of slot s (face id + 1 in tri_idx) -> t[9]; false when the slot names no face of the mesh
static __device__ inline bool gnr_slot_face(const GnrGrid& g, int32_t s, int32_t* fid, float* t) {
    const int32_t f = g.tri_idx[s] - 1;
    if (f < 0 || (uint32_t)f >= g.F) return false;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const int32_t vi = g.faces[3ull * (uint32_t)f + v];
        if (vi < 0 || (uint32_t)vi >= g.V) return false;
#pragma unroll
        for (int c = 0; c < 3; ++c) t[3 * v + c] = g.verts[3ull * (uint32_t)vi + c];
    }
    *fid = f;
    return true;
}

static __device__ inline void gnr_segment(const GnrGrid& g, int lin, int32_t* b, int32_t* e) {
    int32_t lo = lin == 0 ? 0 : g.tri_num[lin - 1], hi = g.tri_num[lin];
    if (lo < 0) lo = 0;
    if (hi > g.total) hi = g.total;
    *b = lo; *e = hi;
}

// ------------------------------------------------------------------------------------------ nearest point
__global__ void __launch_bounds__(GNR_BLOCK) k_gnr_nearest(GnrGrid g, const float* __restrict__ pts, uint32_t N, int32_t* __restrict__ near_faces,
                                                           float* __restrict__ near_pts, float* __restrict__ coeff) {
    const uint32_t id = blockIdx.x * GNR_BLOCK + threadIdx.x;
    if (id >= N) return;
    const float p[3] = {pts[3ull * id], pts[3ull * id + 1], pts[3ull * id + 2]};
    if (!gnr_finite3(p)) {
        const float nan = __uint_as_float(0x7fc00000u);
        near_faces[id] = -1;
#pragma unroll
        for (int c = 0; c < 3; ++c) { near_pts[3ull * id + c] = nan; coeff[3ull * id + c] = nan; }
        return;
    }
    int cell[3], max_linf = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        float xf = (p[d] - g.mn[d]) / g.step;
        xf = xf < 0 ? 0 : (xf >= (float)g.n[d] ? (float)(g.n[d] - 1) : floorf(xf));
        cell[d] = (int)xf;
        const int far = cell[d] > g.n[d] - cell[d] ? cell[d] : g.n[d] - cell[d];
        max_linf = max_linf < far ? far : max_linf;
    }
    int32_t nearest = g.total;
    float dis2 = -1.f, best_co[3] = {0.f, 0.f, 0.f}, best_pt[3] = {0.f, 0.f, 0.f};
    for (int L = 0; L < max_linf; ++L) {
        int n = (2 * L + 1) * (2 * L + 1);
        const int faces_of_shell = L == 0 ? 1 : 6;
        int o0 = 0, o1 = 0, o2 = 0;                                  // the cell's offset from the query's cell
        for (int f = 0; f < faces_of_shell; ++f) {
            const int fixed = f < 3 ? -L : L;
            const int fa = f % 3;
            if (fa == 0) o0 = fixed; else if (fa == 1) o1 = fixed; else o2 = fixed;
            for (int k = 0; k < n; ++k) {
                int j = k;
#pragma unroll
                for (int d = 1; d < 3; ++d) {
                    int v;
                    if (d + f >= 6) { v = j % (2 * L - 1) - L + 1; j = j / (2 * L - 1); }
                    else if (d + f >= 3) { v = j % (2 * L) - L + 1; j = j / (2 * L); }
                    else { v = j % (2 * L + 1) - L; j = j / (2 * L + 1); }
                    const int a = (d + f) % 3;
                    if (a == 0) o0 = v; else if (a == 1) o1 = v; else o2 = v;
                }
                const int off[3] = {o0, o1, o2};
                float dist2 = 0.f;
                int lin = 0;
                bool in = true;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    if (!in) continue;
                    const int y = cell[d] + off[d];
                    if (y < 0 || y >= g.n[d]) { in = false; continue; }
                    if (off[d] < 0) { const float e = p[d] - g.mn[d] - g.step * (float)(y + 1); dist2 += e * e; }
                    else if (off[d] > 0) { const float e = -p[d] + g.mn[d] + g.step * (float)y; dist2 += e * e; }
                    lin = d > 0 ? lin * g.n[d] + y : y;
                }
                if (!in || lin >= g.cells) continue;
                if (dis2 >= 0 && dis2 < dist2) continue;
                int32_t sb, se;
                gnr_segment(g, lin, &sb, &se);
                for (int32_t s = sb; s < se; ++s) {
                    float t[9], co[3] = {0.33f, 0.33f, 0.33f};
                    int32_t fid;
                    if (!gnr_slot_face(g, s, &fid, t)) continue;
#pragma unroll
                    for (int q = 0; q < 9; ++q) t[q] = t[q] - p[q % 3];
                    const float d2 = gnr_proj(t, co);
                    if (dis2 < 0 || d2 < dis2) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            best_co[c] = co[c];
                            best_pt[c] = p[c] + co[0] * t[c] + co[1] * t[3 + c] + co[2] * t[6 + c];
                        }
                        nearest = fid;
                        dis2 = d2;
                    }
                }
            }
            if (f < 2) n = n / (2 * L + 1) * (2 * L);
            else if (f >= 3) n = n / (2 * L) * (2 * L - 1);
        }
        if (dis2 >= 0 && dis2 < (float)(L * L) * g.step * g.step) break;
    }
    near_faces[id] = nearest;
#pragma unroll
    for (int c = 0; c < 3; ++c) { near_pts[3ull * id + c] = best_pt[c]; coeff[3ull * id + c] = best_co[c]; }
}

// ------------------------------------------------------------------------------------------ inside test
// does the half line from s along -x (the first of the two coordinates) cross the segment a-b, the reference's sign test
static __device__ inline bool gnr_cross2(float s0, float s1, float a0, float a1, float b0, float b1) {
    if (!(a0 < s0 || b0 < s0)) return false;
    a0 = a0 - s0; a1 = a1 - s1; b0 = b0 - s0; b1 = b1 - s1;
    const float q0 = b1, q1 = -a1;
    const float det = a0 * b1 - a1 * b0;
    if (det == 0) return false;
    const bool pos = det > 0;
    if (pos != (q0 < 0)) return false;
    if (pos != (q1 < 0)) return false;
    return true;
}

// does the half line from s = (s0, s1, s2) toward grid face `dir` (axis dir / 2, upward when dir is odd) cross the triangle t (absolute vertices)
static __device__ inline bool gnr_cross3(float s0, float s1, float s2, int dir, float* t) {
    const int a = dir / 2, up = dir % 2;
    // (selects of VALUES: a select between the addresses of two array elements would put the array into scratch memory)
    const float t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3], t4 = t[4], t5 = t[5], t6 = t[6], t7 = t[7], t8 = t[8];
    const float sa = a == 0 ? s0 : (a == 1 ? s1 : s2);
    const float ta0 = a == 0 ? t0 : (a == 1 ? t1 : t2);
    const float ta1 = a == 0 ? t3 : (a == 1 ? t4 : t5);
    const float ta2 = a == 0 ? t6 : (a == 1 ? t7 : t8);
    if (up) { if (!(ta0 > sa || ta1 > sa || ta2 > sa)) return false; }
    else { if (!(ta0 < sa || ta1 < sa || ta2 < sa)) return false; }
    // the triangle's three edges in the plane of the other two axes: coordinates (a + 1) % 3 and (a + 2) % 3 of s and of the vertices
    const float su = a == 0 ? s1 : (a == 1 ? s2 : s0), sv = a == 0 ? s2 : (a == 1 ? s0 : s1);
    const float u[3] = {a == 0 ? t1 : (a == 1 ? t2 : t0), a == 0 ? t4 : (a == 1 ? t5 : t3), a == 0 ? t7 : (a == 1 ? t8 : t6)};
    const float v[3] = {a == 0 ? t2 : (a == 1 ? t0 : t1), a == 0 ? t5 : (a == 1 ? t3 : t4), a == 0 ? t8 : (a == 1 ? t6 : t7)};
    int r = 0;
    r += gnr_cross2(su, sv, u[1], v[1], u[2], v[2]) ? 1 : 0;        // d = 0: vertices 1, 2
    r += gnr_cross2(su, sv, u[2], v[2], u[0], v[0]) ? 1 : 0;        // d = 1: vertices 2, 0
    r += gnr_cross2(su, sv, u[0], v[0], u[1], v[1]) ? 1 : 0;        // d = 2: vertices 0, 1
    if (r % 2 == 0) return false;
#pragma unroll
    for (int q = 0; q < 9; ++q) t[q] = t[q] - (q % 3 == 0 ? s0 : (q % 3 == 1 ? s1 : s2));
    float q0, q1, q2, det;
    if (a == 0) {
        q0 = t[4] * t[8] - t[5] * t[7]; q1 = t[2] * t[7] - t[1] * t[8]; q2 = t[1] * t[5] - t[2] * t[4];
        det = q0 * t[0] + q1 * t[3] + q2 * t[6];
    } else if (a == 1) {
        q0 = t[5] * t[6] - t[3] * t[8]; q1 = t[0] * t[8] - t[2] * t[6]; q2 = t[2] * t[3] - t[0] * t[5];
        det = q0 * t[1] + q1 * t[4] + q2 * t[7];
    } else {
        q0 = t[3] * t[7] - t[4] * t[6]; q1 = t[1] * t[6] - t[0] * t[7]; q2 = t[0] * t[4] - t[1] * t[3];
        det = q0 * t[2] + q1 * t[5] + q2 * t[8];
    }
    if (det == 0) return false;
    const bool pos = (det > 0) != (up != 0);
    if (pos != (q0 < 0)) return false;
    if (pos != (q1 < 0)) return false;
    if (pos != (q2 < 0)) return false;
    return true;
}

__global__ void __launch_bounds__(GNR_BLOCK) k_gnr_inside(GnrGrid g, const float* __restrict__ pts, uint32_t N, float* __restrict__ signs) {
    const uint32_t id = blockIdx.x * GNR_BLOCK + threadIdx.x;
    if (id >= N) return;
    const float p[3] = {pts[3ull * id], pts[3ull * id + 1], pts[3ull * id + 2]};
    if (!gnr_finite3(p)) { signs[id] = -1.f; return; }
    int c0, c1, c2, to_end[6];
    {
        int cell[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float xf = (p[d] - g.mn[d]) / g.step;
            if (xf < 0 || xf >= (float)g.n[d]) { signs[id] = -1.f; return; }
            cell[d] = (int)xf;
            to_end[2 * d] = cell[d];
            to_end[2 * d + 1] = g.n[d] - 1 - cell[d];
        }
        c0 = cell[0]; c1 = cell[1]; c2 = cell[2];
    }
    int out = 0, steps = to_end[0];
#pragma unroll
    for (int d = 1; d < 6; ++d)
        if (to_end[d] < steps) { out = d; steps = to_end[d]; }
    // the reference's visited[16]: entry 0 unused, entries 1..15 the crossed faces; when full the entries shift down by one and the
    // count keeps growing (the parity comes from the count).  The search looks at the entries that exist.
    int32_t vis[XR_GNR_VISITED];
#pragma unroll
    for (int q = 0; q < XR_GNR_VISITED; ++q) vis[q] = 0;
    int vsize = 1;
    const int axis = out / 2, delta = out % 2 == 1 ? 1 : -1;
    for (int i = 0; i <= steps; ++i) {
        const int lin = (c0 * g.n[1] + c1) * g.n[2] + c2;
        if (c0 < 0 || c0 >= g.n[0] || c1 < 0 || c1 >= g.n[1] || c2 < 0 || c2 >= g.n[2]) break;
        int32_t sb, se;
        gnr_segment(g, lin, &sb, &se);
        for (int32_t s = sb; s < se; ++s) {
            float t[9];
            int32_t fid;
            if (!gnr_slot_face(g, s, &fid, t)) continue;
            if (!gnr_cross3(p[0], p[1], p[2], out, t)) continue;
            bool found = false;
#pragma unroll
            for (int q = 1; q < XR_GNR_VISITED; ++q)
                if (q < vsize && vis[q] == fid) found = true;
            if (found) continue;
            if (vsize < XR_GNR_VISITED) {
#pragma unroll
                for (int q = 1; q < XR_GNR_VISITED; ++q)
                    if (q == vsize) vis[q] = fid;
            } else {
#pragma unroll
                for (int q = 1; q + 1 < XR_GNR_VISITED; ++q) vis[q] = vis[q + 1];
                vis[XR_GNR_VISITED - 1] = fid;
            }
            ++vsize;
        }
        if (axis == 0) c0 += delta; else if (axis == 1) c1 += delta; else c2 += delta;
    }
    signs[id] = vsize % 2 == 0 ? 1.f : -1.f;
}

static int gnr_search_grid(GnrGrid* g, const char* fn, const float* verts, const int32_t* faces, uint32_t V, uint32_t F, float step,
                           const float* min3, const int32_t* num3, const int32_t* tri_num, const int32_t* tri_idx, int32_t total) {
    const int rc = gnr_grid(g, fn, verts, faces, V, F, step, min3, num3);
    if (rc != 0) return rc;
    if (!tri_num || total < 0 || (total > 0 && !tri_idx)) { xr_set_error("%s: null table or negative slot count", fn); return XR_EINVAL; }
    g->tri_num = tri_num; g->tri_idx = tri_idx; g->total = total;
    return 0;
}

extern "C" int xr_gnr_nearest(const float* verts, const int32_t* faces, uint32_t V, uint32_t F, float step, const float* min3,
                              const int32_t* num3, const int32_t* tri_num, const int32_t* tri_idx, int32_t total, const float* pts, uint32_t N,
                              int32_t* near_faces, float* near_pts, float* coeff, void* stream) {
    GnrGrid g;
    const int rc = gnr_search_grid(&g, __func__, verts, faces, V, F, step, min3, num3, tri_num, tri_idx, total);
    if (rc != 0) return rc;
    if (N == 0) return 0;
    XR_REQUIRE(pts && near_faces && near_pts && coeff, "null pointer");
    XR_REQUIRE(N <= (1u << 30), "too many points");
    hipLaunchKernelGGL(k_gnr_nearest, dim3(xr_div_up(N, GNR_BLOCK)), dim3(GNR_BLOCK), 0, (hipStream_t)stream, g, pts, N, near_faces, near_pts,
                       coeff);
    XR_LAUNCH_CHECK();
    return 0;
}

extern "C" int xr_gnr_inside(const float* verts, const int32_t* faces, uint32_t V, uint32_t F, float step, const float* min3,
                             const int32_t* num3, const int32_t* tri_num, const int32_t* tri_idx, int32_t total, const float* pts, uint32_t N,
                             float* signs, void* stream) {
    GnrGrid g;
    const int rc = gnr_search_grid(&g, __func__, verts, faces, V, F, step, min3, num3, tri_num, tri_idx, total);
    if (rc != 0) return rc;
    if (N == 0) return 0;
    XR_REQUIRE(pts && signs, "null pointer");
    XR_REQUIRE(N <= (1u << 30), "too many points");
    hipLaunchKernelGGL(k_gnr_inside, dim3(xr_div_up(N, GNR_BLOCK)), dim3(GNR_BLOCK), 0, (hipStream_t)stream, g, pts, N, signs);
    XR_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------ embedding
struct GnrEmbed {
    const float* pts; uint32_t N; const int32_t* near_faces; const float* near_pts; const float* signs;
    const int32_t* faces; uint32_t F; const float* t_verts; uint32_t V;
    const float* center_d; const float* rot_d;        // [3] / [9] on the device (per-frame data: no host read per call)
    float scale, half;
    int use_nml, use_t_pose, use_sdf;
    float* out; uint32_t ld; float* alpha;
};

// (x scale / half) R, sum_k ascending
static __device__ inline void gnr_normalise(const GnrEmbed& a, const float* rot, const float* x, float* y) {
    float s[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = x[c] * a.scale / a.half;
#pragma unroll
    for (int j = 0; j < 3; ++j) y[j] = s[0] * rot[j] + s[1] * rot[3 + j] + s[2] * rot[6 + j];
}

__global__ void __launch_bounds__(GNR_BLOCK) k_gnr_embed(GnrEmbed a) {
    const uint32_t id = blockIdx.x * GNR_BLOCK + threadIdx.x;
    if (id >= a.N) return;
    const float p[3] = {a.pts[3ull * id], a.pts[3ull * id + 1], a.pts[3ull * id + 2]};
    float* o = a.out + (uint64_t)id * a.ld;
    uint32_t col = 0;
    float rot[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) rot[c] = (a.use_nml && a.use_sdf) ? a.rot_d[c] : 0.f;
    if (a.use_nml) {
        const float d[3] = {p[0] - a.center_d[0], p[1] - a.center_d[1], p[2] - a.center_d[2]};
        float y[3];
        if (a.use_sdf) gnr_normalise(a, rot, d, y);
        else { y[0] = d[0] * a.scale / a.half; y[1] = d[1] * a.scale / a.half; y[2] = d[2] * a.scale / a.half; }
        o[0] = y[0]; o[1] = y[1]; o[2] = y[2];
    } else {
        o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
    }
    col = 3;
    if (a.use_t_pose) {
        const int32_t f = a.near_faces[id];
        float m[3];
        const float nan = __uint_as_float(0x7fc00000u);
        m[0] = nan; m[1] = nan; m[2] = nan;
        if (f >= 0 && (uint32_t)f < a.F) {
            const int32_t v0 = a.faces[3ull * (uint32_t)f], v1 = a.faces[3ull * (uint32_t)f + 1], v2 = a.faces[3ull * (uint32_t)f + 2];
            if (v0 >= 0 && v1 >= 0 && v2 >= 0 && (uint32_t)v0 < a.V && (uint32_t)v1 < a.V && (uint32_t)v2 < a.V) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    m[c] = (a.t_verts[3ull * (uint32_t)v0 + c] + a.t_verts[3ull * (uint32_t)v1 + c] + a.t_verts[3ull * (uint32_t)v2 + c]) / 3.f;
            }
        }
        o[col] = m[0]; o[col + 1] = m[1]; o[col + 2] = m[2];
        col += 3;
    }
    if (a.use_sdf) {
        float r[3] = {p[0] - a.near_pts[3ull * id], p[1] - a.near_pts[3ull * id + 1], p[2] - a.near_pts[3ull * id + 2]};
        if (a.use_nml) { float y[3]; gnr_normalise(a, rot, r, y); r[0] = y[0]; r[1] = y[1]; r[2] = y[2]; }
        const float sign = a.signs[id];
        const float norm = sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) + 1e-8f;
        o[col] = r[0] / norm; o[col + 1] = r[1] / norm; o[col + 2] = r[2] / norm;
        o[col + 3] = tanhf(norm * sign * 20.f);
        if (a.alpha) a.alpha[id] = (sign + 1.f) / 2.f;
    }
}

extern "C" int xr_gnr_shape_embed(const float* pts, uint32_t N, const int32_t* near_faces, const float* near_pts, const float* signs,
                                  const int32_t* faces, uint32_t F, const float* t_verts, uint32_t V, const float* center3, const float* rot9,
                                  float scale, float half, int use_nml, int use_t_pose, int use_smpl_sdf, float* out, uint32_t ld, float* alpha,
                                  void* stream) {
    if (N == 0) return 0;
    XR_REQUIRE(pts && out, "null pointer");
    XR_REQUIRE(N <= (1u << 30), "too many points");
    const uint32_t cols = 3u + (use_t_pose ? 3u : 0u) + (use_smpl_sdf ? 4u : 0u);
    XR_REQUIRE(ld >= cols, "the row stride is smaller than the embedding");
    GnrEmbed a;
    memset(&a, 0, sizeof(a));
    if (use_nml) {
        XR_REQUIRE(center3 != nullptr && half > 0.f, "use_nml needs the centre and a positive half width");
        a.center_d = center3;
    }
    if (use_nml && use_smpl_sdf) {
        XR_REQUIRE(rot9 != nullptr, "use_smpl_sdf needs the rotation");
        a.rot_d = rot9;
    }
    if (use_t_pose) XR_REQUIRE(near_faces && faces && t_verts && F > 0 && V > 0, "use_t_pose needs the nearest faces and the T-pose mesh");
    if (use_smpl_sdf) XR_REQUIRE(near_pts && signs, "use_smpl_sdf needs the nearest points and the signs");
    a.pts = pts; a.N = N; a.near_faces = near_faces; a.near_pts = near_pts; a.signs = signs; a.faces = faces; a.F = F; a.t_verts = t_verts; a.V = V;
    a.scale = scale; a.half = half; a.use_nml = use_nml ? 1 : 0; a.use_t_pose = use_t_pose ? 1 : 0; a.use_sdf = use_smpl_sdf ? 1 : 0;
    a.out = out; a.ld = ld; a.alpha = alpha;
    hipLaunchKernelGGL(k_gnr_embed, dim3(xr_div_up(N, GNR_BLOCK)), dim3(GNR_BLOCK), 0, (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return 0;
}
