// Animatable NeRF (configs/animatable_nerf/an_h36m_s9_train_pose.py) stages for gfx950: what stands around the 256-wide MLPs in a step.
// The reference composes each from tensor ops (models/networks/utils/aninerf.py, models/mlps/aninerf_mlp.py) -- a nearest-vertex query
// there is a [N, V] distance matrix; here each is a launch of its own:
//   k_ani_closest        thread = point, 256 per workgroup.  The vertices pass through LDS in tiles of 1024 float4 (16 KiB, so several
//                        workgroups share a CU); every lane reads the SAME tile entry (an LDS broadcast), keeps the smallest
//                        d2 = (dx dx + dy dy) + dz dz and its index; ascending order + strict `<` = lowest index on a tie
//   k_ani_select_*       pind = flags | argmin(dist) and nonzero(pind): per-workgroup counts and minima, ONE workgroup that finds the
//                        global minimum and scans the counts, then the ranked write (the scans: xr_scan.h).  Three launches, no
//                        workgroup waits for another
//   k_ani_blend_fwd/bwd  thread = point: softmax over 24 channels of log(smpl_bw[idx] + 1e-9) + logits, the gathered row never stored
//   k_ani_skin_fwd/bwd   thread = point: the 2 x 24 matrices (top three rows) in LDS, read as broadcasts; blend, invert by adjugate /
//                        determinant, transform.  The backward recomputes all of it and contracts dL/dA, dL/dB with the matrices
//   k_ani_encode_bwd     workgroup = 64 rows: the gradient tile comes in coalesced through LDS, then one (row, axis) item per lane
// No atomics anywhere, every reduction / scan has a fixed order: the same input gives the same bits on every launch.
// Compiled with -ffp-contract=off: every expression is fp32 in the written order (the fp32 torch restatement of the query matches it
// bit for bit).
#include "xr_common.h"
#include "xr_scan.h"
#include "../../include/xrnerf_mi355_aninerf.h"

#define AN_BLOCK 256
static_assert(AN_BLOCK == XR_SCAN_BLOCK, "the shared workgroup routines are written for 256 threads");
#define AN_WAVES (AN_BLOCK / 64)
#define AN_J XR_ANI_JOINTS
#define AN_TILE XR_ANI_CLOSEST_TILE
#define AN_ENC_TILE 64
#define AN_MAX_FREQS 16

// ------------------------------------------------------------------------------------------ closest vertex
struct AnRigid { float r[9], t[3]; bool on; };

// world_points_to_pose_points: q_j = sum_k (p_k - T_k) R_kj, k ascending
static __device__ inline void an_to_pose(const AnRigid& g, float x, float y, float z, float* q) {
    if (!g.on) { q[0] = x; q[1] = y; q[2] = z; return; }
    const float d0 = x - g.t[0], d1 = y - g.t[1], d2 = z - g.t[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) q[j] = (d0 * g.r[j] + d1 * g.r[3 + j]) + d2 * g.r[6 + j];
}

__global__ void __launch_bounds__(AN_BLOCK) k_ani_closest(const float* __restrict__ pts, const float* __restrict__ verts,
                                                          const float* __restrict__ R, const float* __restrict__ T, uint32_t n, uint32_t V,
                                                          float th, float* __restrict__ q_out, int32_t* __restrict__ idx_out,
                                                          float* __restrict__ d2_out, float* __restrict__ dist_out,
                                                          int32_t* __restrict__ flag_out) {
    __shared__ float4 s_v[AN_TILE];
    AnRigid g;
    g.on = R != nullptr;
    if (g.on) {
        for (int k = 0; k < 9; ++k) g.r[k] = R[k];
        for (int k = 0; k < 3; ++k) g.t[k] = T[k];
    }
    const uint32_t i = blockIdx.x * AN_BLOCK + threadIdx.x;
    const bool live = i < n;
    float q[3] = {0.f, 0.f, 0.f};
    if (live) an_to_pose(g, pts[i * 3ull], pts[i * 3ull + 1], pts[i * 3ull + 2], q);
    float best = __uint_as_float(0x7f800000u);
    uint32_t bi = 0;
    for (uint32_t v0 = 0; v0 < V; v0 += AN_TILE) {
        const uint32_t tv = V - v0 < AN_TILE ? V - v0 : AN_TILE;
        __syncthreads();                                           // the previous tile has been read by every lane
        for (uint32_t e = threadIdx.x; e < tv; e += AN_BLOCK) {
            float w[3];
            an_to_pose(g, verts[(v0 + e) * 3ull], verts[(v0 + e) * 3ull + 1], verts[(v0 + e) * 3ull + 2], w);
            s_v[e] = make_float4(w[0], w[1], w[2], 0.f);
        }
        __syncthreads();
        if (live) {
#pragma unroll 4
            for (uint32_t j = 0; j < tv; ++j) {
                const float4 w = s_v[j];                           // one address for the whole wave: a broadcast
                const float dx = q[0] - w.x, dy = q[1] - w.y, dz = q[2] - w.z;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < best) { best = d2; bi = v0 + j; }
            }
        }
    }
    if (!live) return;
    const float dist = sqrtf(best);
    if (q_out != nullptr) { q_out[i * 3ull] = q[0]; q_out[i * 3ull + 1] = q[1]; q_out[i * 3ull + 2] = q[2]; }
    idx_out[i] = (int32_t)bi;
    if (d2_out != nullptr) d2_out[i] = best;
    dist_out[i] = dist;
    flag_out[i] = dist < th ? 1 : 0;
}

// ------------------------------------------------------------------------------------------ selection
// workspace of nb = ceil(n / 256) workgroups: count [nb] | min dist [nb] | min index [nb] | offset [nb] | forced index [1]  (4-byte words)
struct AnSelWs { uint32_t* cnt; float* mind; uint32_t* mini; uint32_t* off; uint32_t* forced; };

static __host__ __device__ inline AnSelWs an_sel_ws(void* ws, uint32_t nb) {
    uint32_t* w = (uint32_t*)ws;
    AnSelWs s;
    s.cnt = w; s.mind = (float*)(w + nb); s.mini = w + 2ull * nb; s.off = w + 3ull * nb; s.forced = w + 4ull * nb;
    return s;
}
// (d, i) order: smaller distance first, then the lower index; a NaN never wins
static __device__ inline bool an_before(float d, uint32_t i, float bd, uint32_t bi) { return d < bd || (d == bd && i < bi); }

__global__ void __launch_bounds__(AN_BLOCK) k_ani_select_count(const int32_t* __restrict__ flags, const float* __restrict__ dist, uint32_t n,
                                                               AnSelWs ws) {
    __shared__ uint32_t s_c[AN_WAVES];
    __shared__ float s_d[AN_WAVES];
    __shared__ uint32_t s_i[AN_WAVES];
    const uint32_t i = blockIdx.x * AN_BLOCK + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool live = i < n;
    const unsigned long long m = __ballot(live && flags[i] != 0);
    float d = __uint_as_float(0x7f800000u);
    uint32_t bi = 0xffffffffu;
    if (live) { const float x = dist[i]; if (x <= d) { d = x; bi = i; } }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float od = __shfl_xor(d, off, 64);
        const uint32_t oi = __shfl_xor(bi, off, 64);
        if (an_before(od, oi, d, bi)) { d = od; bi = oi; }
    }
    if (lane == 0) { s_c[wave] = (uint32_t)__popcll(m); s_d[wave] = d; s_i[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = s_c[0];
        for (int w = 1; w < AN_WAVES; ++w) {
            c += s_c[w];
            if (an_before(s_d[w], s_i[w], d, bi)) { d = s_d[w]; bi = s_i[w]; }
        }
        ws.cnt[blockIdx.x] = c; ws.mind[blockIdx.x] = d; ws.mini[blockIdx.x] = bi;
    }
}

__global__ void __launch_bounds__(AN_BLOCK) k_ani_select_order(const int32_t* __restrict__ flags, uint32_t nb, AnSelWs ws,
                                                               int32_t* __restrict__ count) {
    __shared__ float s_d[AN_BLOCK];
    __shared__ uint32_t s_i[AN_BLOCK];
    __shared__ uint32_t s_forced;
    const uint32_t t = threadIdx.x;
    float d = __uint_as_float(0x7f800000u);
    uint32_t bi = 0xffffffffu;
    for (uint32_t b = t; b < nb; b += AN_BLOCK)
        if (an_before(ws.mind[b], ws.mini[b], d, bi)) { d = ws.mind[b]; bi = ws.mini[b]; }
    s_d[t] = d; s_i[t] = bi;
    __syncthreads();
    if (t == 0) {
        for (uint32_t k = 1; k < AN_BLOCK; ++k)
            if (an_before(s_d[k], s_i[k], d, bi)) { d = s_d[k]; bi = s_i[k]; }
        s_forced = bi;
        ws.forced[0] = bi;
    }
    __syncthreads();
    const uint32_t forced = s_forced;
    const uint32_t extra_block = (forced != 0xffffffffu && flags[forced] == 0) ? forced / AN_BLOCK : 0xffffffffu;
    const uint64_t total = xr_scan_sweeps(nb, [&](uint32_t b) { return ws.cnt[b] + (b == extra_block ? 1u : 0u); },
                                          [&](uint32_t b, uint32_t base) { ws.off[b] = base; });
    if (t == 0) count[0] = xr_scan_total(total);
}

__global__ void __launch_bounds__(AN_BLOCK) k_ani_select_write(const int32_t* __restrict__ flags, uint32_t n, AnSelWs ws,
                                                               int32_t* __restrict__ list) {
    const uint32_t i = blockIdx.x * AN_BLOCK + threadIdx.x;
    const bool sel = i < n && (flags[i] != 0 || i == ws.forced[0]);
    uint32_t sum;
    const uint32_t rank = xr_block_excl_flag(sel, &sum);
    if (sel) list[ws.off[blockIdx.x] + rank] = (int32_t)i;
}

// ------------------------------------------------------------------------------------------ blend-weight head
static __device__ inline void an_load24(const float* __restrict__ row, float* v) {
    const float4* r4 = reinterpret_cast<const float4*>(row);
#pragma unroll
    for (int k = 0; k < AN_J / 4; ++k) { const float4 x = r4[k]; v[4 * k] = x.x; v[4 * k + 1] = x.y; v[4 * k + 2] = x.z; v[4 * k + 3] = x.w; }
}
static __device__ inline void an_store24(float* __restrict__ row, const float* v) {
    float4* r4 = reinterpret_cast<float4*>(row);
#pragma unroll
    for (int k = 0; k < AN_J / 4; ++k) r4[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
}

__global__ void __launch_bounds__(AN_BLOCK) k_ani_blend_fwd(const float* __restrict__ smpl_bw, const int32_t* __restrict__ idx,
                                                            const float* __restrict__ logits, uint32_t n, float* __restrict__ bw) {
    const uint32_t i = blockIdx.x * AN_BLOCK + threadIdx.x;
    if (i >= n) return;
    float w[AN_J], x[AN_J];
    an_load24(smpl_bw + (uint64_t)(uint32_t)idx[i] * AN_J, w);
    an_load24(logits + (uint64_t)i * AN_J, x);
    float mx = -__uint_as_float(0x7f800000u);
#pragma unroll
    for (int j = 0; j < AN_J; ++j) { x[j] = logf(w[j] + 1e-9f) + x[j]; mx = fmaxf(mx, x[j]); }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < AN_J; ++j) { x[j] = expf(x[j] - mx); sum += x[j]; }
#pragma unroll
    for (int j = 0; j < AN_J; ++j) x[j] = x[j] / sum;
    an_store24(bw + (uint64_t)i * AN_J, x);
}

__global__ void __launch_bounds__(AN_BLOCK) k_ani_blend_bwd(const float* __restrict__ bw, const float* __restrict__ grad_bw, uint32_t n,
                                                            float* __restrict__ grad_logits) {
    const uint32_t i = blockIdx.x * AN_BLOCK + threadIdx.x;
    if (i >= n) return;
    float w[AN_J], g[AN_J];
    an_load24(bw + (uint64_t)i * AN_J, w);
    an_load24(grad_bw + (uint64_t)i * AN_J, g);
    // bw_j (g_j - sum_k g_k bw_k) written as bw_j sum_k bw_k (g_j - g_k) (the rows sum to 1): on a peaked row -- one weight near 1, which
    // exact-zero initial weights produce -- the first form cancels g_j (1 - bw_j) out of fp32 values rounded at 6e-8, the second does not
    float o[AN_J];
#pragma unroll
    for (int j = 0; j < AN_J; ++j) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < AN_J; ++k) s += w[k] * (g[j] - g[k]);
        o[j] = w[j] * s;
    }
    an_store24(grad_logits + (uint64_t)i * AN_J, o);
}

// ------------------------------------------------------------------------------------------ skinning
// s_a: [2][24][12] = the top three rows (R | t) of a_from's and a_to's matrices
static __device__ inline void an_stage_matrices(float* s_a, const float* __restrict__ a_from, const float* __restrict__ a_to) {
    for (uint32_t e = threadIdx.x; e < 2u * AN_J * 12u; e += AN_BLOCK) {
        const uint32_t set = e / (AN_J * 12u), r = e - set * (AN_J * 12u), j = r / 12u, k = r - j * 12u;
        s_a[e] = (set ? a_to : a_from)[j * 16u + k];
    }
    __syncthreads();
}
// a, b [12] = sum_j bw_j (top three rows), j ascending
static __device__ inline void an_blend_matrices(const float* s_a, const float* w, float* a, float* b) {
#pragma unroll
    for (int k = 0; k < 12; ++k) { a[k] = 0.f; b[k] = 0.f; }
    for (int j = 0; j < AN_J; ++j) {
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            a[k] = a[k] + w[j] * s_a[j * 12 + k];
            b[k] = b[k] + w[j] * s_a[(AN_J + j) * 12 + k];
        }
    }
}
// m [9] = inverse of the 3x3 block of a [12] (row stride 4): adjugate / determinant
static __device__ inline void an_inverse(const float* a, float* m) {
    const float a00 = a[0], a01 = a[1], a02 = a[2], a10 = a[4], a11 = a[5], a12 = a[6], a20 = a[8], a21 = a[9], a22 = a[10];
    const float c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
    const float det = (a00 * c00 + a01 * c01) + a02 * c02;
    m[0] = c00 / det; m[1] = (a02 * a21 - a01 * a22) / det; m[2] = (a01 * a12 - a02 * a11) / det;
    m[3] = c01 / det; m[4] = (a00 * a22 - a02 * a20) / det; m[5] = (a02 * a10 - a00 * a12) / det;
    m[6] = c02 / det; m[7] = (a01 * a20 - a00 * a21) / det; m[8] = (a00 * a11 - a01 * a10) / det;
}
static __device__ inline void an_mat3(const float* m, int ld, const float* x, float* y) {          // y = M x
#pragma unroll
    for (int r = 0; r < 3; ++r) y[r] = (m[r * ld] * x[0] + m[r * ld + 1] * x[1]) + m[r * ld + 2] * x[2];
}
static __device__ inline void an_mat3t(const float* m, int ld, const float* x, float* y) {         // y = M^T x
#pragma unroll
    for (int c = 0; c < 3; ++c) y[c] = (m[c] * x[0] + m[ld + c] * x[1]) + m[2 * ld + c] * x[2];
}

__global__ void __launch_bounds__(AN_BLOCK) k_ani_skin_fwd(const float* __restrict__ pts, const float* __restrict__ dirs,
                                                           const float* __restrict__ bw, const float* __restrict__ a_from,
                                                           const float* __restrict__ a_to, uint32_t n, float* __restrict__ pts_out,
                                                           float* __restrict__ dirs_out) {
    __shared__ float s_a[2 * AN_J * 12];
    an_stage_matrices(s_a, a_from, a_to);
    const uint32_t i = blockIdx.x * AN_BLOCK + threadIdx.x;
    if (i >= n) return;
    float w[AN_J], a[12], b[12], m[9];
    an_load24(bw + (uint64_t)i * AN_J, w);
    an_blend_matrices(s_a, w, a, b);
    an_inverse(a, m);
    const float x[3] = {pts[i * 3ull] - a[3], pts[i * 3ull + 1] - a[7], pts[i * 3ull + 2] - a[11]};
    float p1[3], p2[3];
    an_mat3(m, 3, x, p1);
    an_mat3(b, 4, p1, p2);
    pts_out[i * 3ull] = p2[0] + b[3]; pts_out[i * 3ull + 1] = p2[1] + b[7]; pts_out[i * 3ull + 2] = p2[2] + b[11];
    if (dirs != nullptr) {
        const float d[3] = {dirs[i * 3ull], dirs[i * 3ull + 1], dirs[i * 3ull + 2]};
        float d1[3], d2[3];
        an_mat3(m, 3, d, d1);
        an_mat3(b, 4, d1, d2);
        dirs_out[i * 3ull] = d2[0]; dirs_out[i * 3ull + 1] = d2[1]; dirs_out[i * 3ull + 2] = d2[2];
    }
}

__global__ void __launch_bounds__(AN_BLOCK) k_ani_skin_bwd(const float* __restrict__ pts, const float* __restrict__ dirs,
                                                           const float* __restrict__ bw, const float* __restrict__ a_from,
                                                           const float* __restrict__ a_to, uint32_t n, const float* __restrict__ grad_pts,
                                                           const float* __restrict__ grad_dirs, float* __restrict__ grad_bw) {
    __shared__ float s_a[2 * AN_J * 12];
    an_stage_matrices(s_a, a_from, a_to);
    const uint32_t i = blockIdx.x * AN_BLOCK + threadIdx.x;
    if (i >= n) return;
    float w[AN_J], a[12], b[12], m[9];
    an_load24(bw + (uint64_t)i * AN_J, w);
    an_blend_matrices(s_a, w, a, b);
    an_inverse(a, m);
    // dA, dB [12]: dL/dA_R = -u p'^T, dL/dA_t = -u, dL/dB_R = g p'^T, dL/dB_t = g with u = M^T (B_R^T g); the directions add the
    // same terms without the translations
    float dA[12], dB[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { dA[k] = 0.f; dB[k] = 0.f; }
    if (grad_pts != nullptr) {
        const float x[3] = {pts[i * 3ull] - a[3], pts[i * 3ull + 1] - a[7], pts[i * 3ull + 2] - a[11]};
        const float g[3] = {grad_pts[i * 3ull], grad_pts[i * 3ull + 1], grad_pts[i * 3ull + 2]};
        float p1[3], t[3], u[3];
        an_mat3(m, 3, x, p1);
        an_mat3t(b, 4, g, t);
        an_mat3t(m, 3, t, u);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { dA[r * 4 + c] = -(u[r] * p1[c]); dB[r * 4 + c] = g[r] * p1[c]; }
            dA[r * 4 + 3] = -u[r];
            dB[r * 4 + 3] = g[r];
        }
    }
    if (grad_dirs != nullptr) {
        const float d[3] = {dirs[i * 3ull], dirs[i * 3ull + 1], dirs[i * 3ull + 2]};
        const float g[3] = {grad_dirs[i * 3ull], grad_dirs[i * 3ull + 1], grad_dirs[i * 3ull + 2]};
        float d1[3], t[3], u[3];
        an_mat3(m, 3, d, d1);
        an_mat3t(b, 4, g, t);
        an_mat3t(m, 3, t, u);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { dA[r * 4 + c] = dA[r * 4 + c] - u[r] * d1[c]; dB[r * 4 + c] = dB[r * 4 + c] + g[r] * d1[c]; }
        }
    }
    for (int j = 0; j < AN_J; ++j) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 12; ++k) s = (s + dA[k] * s_a[j * 12 + k]) + dB[k] * s_a[(AN_J + j) * 12 + k];
        w[j] = s;
    }
    an_store24(grad_bw + (uint64_t)i * AN_J, w);
}

// ------------------------------------------------------------------------------------------ BaseEmbedder backward (input gradient)
__global__ void __launch_bounds__(AN_BLOCK) k_ani_encode_bwd(const float* __restrict__ pts, const float* __restrict__ grad, uint32_t ld,
                                                             uint32_t n, int L, float* __restrict__ grad_pts) {
    extern __shared__ float an_tile[];                               // [AN_ENC_TILE][cp]
    const uint32_t cp = 3u + 6u * (uint32_t)L;
    const uint64_t g0 = (uint64_t)blockIdx.x * AN_ENC_TILE;
    const uint32_t tile = (uint32_t)(n - g0 < AN_ENC_TILE ? n - g0 : AN_ENC_TILE);
    for (uint32_t e = threadIdx.x; e < tile * cp; e += AN_BLOCK) {
        const uint32_t sl = e / cp, c = e - sl * cp;
        an_tile[e] = grad[(g0 + sl) * ld + c];
    }
    __syncthreads();
    const uint32_t e = threadIdx.x;
    if (e >= tile * 3u) return;
    const uint32_t sl = e / 3u, ax = e - sl * 3u;
    const float* row = an_tile + (size_t)sl * cp;
    const float p = pts[(g0 + sl) * 3 + ax];
    float acc = row[ax];
    for (int l = 0; l < L; ++l) {
        const float y = ldexpf(p, l);                                // p * 2^l: exact
        const float t = row[3 + 6 * l + ax] * cosf(y) - row[6 + 6 * l + ax] * sinf(y);
        acc = acc + ldexpf(t, l);
    }
    grad_pts[(g0 + sl) * 3 + ax] = acc;
}

// ------------------------------------------------------------------------------------------ C-ABI
#define AN_ALIGNED16(p) (((uintptr_t)(p) & 15) == 0)
#define AN_MAX_N 0x7fffff00u                     /* int32 indices; the grid rounds n up to a multiple of 256 */

extern "C" int xr_ani_closest(const float* pts, const float* verts, const float* R, const float* T, uint32_t n, uint32_t n_verts, float th,
                              float* q_out, int32_t* idx_out, float* d2_out, float* dist_out, int32_t* flag_out, void* stream) {
    XR_REQUIRE(n_verts >= 1 && n_verts <= 0x7fffffffu, "n_verts must be in [1, 2^31)");
    XR_REQUIRE((R == nullptr) == (T == nullptr), "R and T come together");
    XR_REQUIRE(n <= AN_MAX_N, "too many points");
    if (n == 0) return XR_OK;
    XR_REQUIRE(pts && verts && idx_out && dist_out && flag_out, "null pointer");
    hipLaunchKernelGGL(k_ani_closest, dim3(xr_div_up(n, AN_BLOCK)), dim3(AN_BLOCK), 0, (hipStream_t)stream, pts, verts, R, T, n, n_verts, th,
                       q_out, idx_out, d2_out, dist_out, flag_out);
    XR_LAUNCH_CHECK();
    return XR_OK;
}

extern "C" size_t xr_ani_select_workspace_bytes(uint32_t n) { return (4ull * xr_div_up(n, AN_BLOCK) + 1ull) * sizeof(uint32_t); }

extern "C" int xr_ani_select(const int32_t* flags, const float* dist, uint32_t n, int32_t* list, int32_t* count, void* workspace,
                             size_t workspace_bytes, void* stream) {
    XR_REQUIRE(count != nullptr, "null pointer");
    XR_REQUIRE(n <= AN_MAX_N, "too many points");
    if (n == 0) {
        XR_HIP(hipMemsetAsync(count, 0, sizeof(int32_t), (hipStream_t)stream));
        return XR_OK;
    }
    XR_REQUIRE(flags && dist && list && workspace, "null pointer");
    XR_REQUIRE(((uintptr_t)workspace & 3) == 0 && workspace_bytes >= xr_ani_select_workspace_bytes(n), "workspace too small or misaligned");
    const uint32_t nb = xr_div_up(n, AN_BLOCK);
    const AnSelWs ws = an_sel_ws(workspace, nb);
    hipLaunchKernelGGL(k_ani_select_count, dim3(nb), dim3(AN_BLOCK), 0, (hipStream_t)stream, flags, dist, n, ws);
    hipLaunchKernelGGL(k_ani_select_order, dim3(1), dim3(AN_BLOCK), 0, (hipStream_t)stream, flags, nb, ws, count);
    hipLaunchKernelGGL(k_ani_select_write, dim3(nb), dim3(AN_BLOCK), 0, (hipStream_t)stream, flags, n, ws, list);
    XR_LAUNCH_CHECK();
    return XR_OK;
}

extern "C" int xr_ani_blend_forward(const float* smpl_bw, const int32_t* idx, const float* logits, uint32_t n, float* bw, void* stream) {
    XR_REQUIRE(n <= AN_MAX_N, "too many points");
    if (n == 0) return XR_OK;
    XR_REQUIRE(smpl_bw && idx && logits && bw, "null pointer");
    XR_REQUIRE(AN_ALIGNED16(smpl_bw) && AN_ALIGNED16(logits) && AN_ALIGNED16(bw), "smpl_bw, logits and bw must be 16-byte aligned");
    hipLaunchKernelGGL(k_ani_blend_fwd, dim3(xr_div_up(n, AN_BLOCK)), dim3(AN_BLOCK), 0, (hipStream_t)stream, smpl_bw, idx, logits, n, bw);
    XR_LAUNCH_CHECK();
    return XR_OK;
}

extern "C" int xr_ani_blend_backward(const float* bw, const float* grad_bw, uint32_t n, float* grad_logits, void* stream) {
    XR_REQUIRE(n <= AN_MAX_N, "too many points");
    if (n == 0) return XR_OK;
    XR_REQUIRE(bw && grad_bw && grad_logits, "null pointer");
    XR_REQUIRE(AN_ALIGNED16(bw) && AN_ALIGNED16(grad_bw) && AN_ALIGNED16(grad_logits), "bw, grad_bw and grad_logits must be 16-byte aligned");
    hipLaunchKernelGGL(k_ani_blend_bwd, dim3(xr_div_up(n, AN_BLOCK)), dim3(AN_BLOCK), 0, (hipStream_t)stream, bw, grad_bw, n, grad_logits);
    XR_LAUNCH_CHECK();
    return XR_OK;
}

extern "C" int xr_ani_skin_forward(const float* pts, const float* dirs, const float* bw, const float* a_from, const float* a_to, uint32_t n,
                                   float* pts_out, float* dirs_out, void* stream) {
    XR_REQUIRE(n <= AN_MAX_N, "too many points");
    if (n == 0) return XR_OK;
    XR_REQUIRE(pts && bw && a_from && a_to && pts_out, "null pointer");
    XR_REQUIRE(dirs == nullptr || dirs_out != nullptr, "dirs given without dirs_out");
    XR_REQUIRE(AN_ALIGNED16(bw), "bw must be 16-byte aligned");
    hipLaunchKernelGGL(k_ani_skin_fwd, dim3(xr_div_up(n, AN_BLOCK)), dim3(AN_BLOCK), 0, (hipStream_t)stream, pts, dirs, bw, a_from, a_to, n,
                       pts_out, dirs_out);
    XR_LAUNCH_CHECK();
    return XR_OK;
}

extern "C" int xr_ani_skin_backward(const float* pts, const float* dirs, const float* bw, const float* a_from, const float* a_to, uint32_t n,
                                    const float* grad_pts, const float* grad_dirs, float* grad_bw, void* stream) {
    XR_REQUIRE(n <= AN_MAX_N, "too many points");
    if (n == 0) return XR_OK;
    XR_REQUIRE(pts && bw && a_from && a_to && grad_bw, "null pointer");
    XR_REQUIRE(grad_dirs == nullptr || dirs != nullptr, "grad_dirs given without dirs");
    XR_REQUIRE(AN_ALIGNED16(bw) && AN_ALIGNED16(grad_bw), "bw and grad_bw must be 16-byte aligned");
    hipLaunchKernelGGL(k_ani_skin_bwd, dim3(xr_div_up(n, AN_BLOCK)), dim3(AN_BLOCK), 0, (hipStream_t)stream, pts, dirs, bw, a_from, a_to, n,
                       grad_pts, grad_dirs, grad_bw);
    XR_LAUNCH_CHECK();
    return XR_OK;
}

extern "C" int xr_ani_encode_backward(const float* pts, const float* grad, uint32_t ld, uint32_t n, int multires, float* grad_pts,
                                      void* stream) {
    XR_REQUIRE(multires >= 0 && multires <= AN_MAX_FREQS, "multires must be in [0, 16]");
    const uint32_t cp = 3u + 6u * (uint32_t)multires;
    XR_REQUIRE(ld >= cp, "ld must be >= 3 + 6 multires");
    XR_REQUIRE(n <= AN_MAX_N, "too many points");
    if (n == 0) return XR_OK;
    XR_REQUIRE(pts && grad && grad_pts, "null pointer");
    hipLaunchKernelGGL(k_ani_encode_bwd, dim3(xr_div_up(n, AN_ENC_TILE)), dim3(AN_BLOCK), (size_t)AN_ENC_TILE * cp * sizeof(float),
                       (hipStream_t)stream, pts, grad, ld, n, multires, grad_pts);
    XR_LAUNCH_CHECK();
    return XR_OK;
}
