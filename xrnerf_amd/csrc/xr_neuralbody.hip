// NeuralBody (configs/neuralbody/nb_zjumocap_*.py) for gfx950: what `spconv` and the dense feature volumes are to the reference.
//   k_nb_mark0 / k_nb_mark_down   mark the active cells of a level in its index volume (level 0: the vertices' voxels; level l + 1: the
//                                 up to eight output cells every input row feeds).  All marks store the same value: no atomics
//   k_nb_count / _scan / _rank    count / scan / ranked write over the cells (xr_scan.h): rows in ascending linear index, the index
//                                 volume rewritten in place to the row of every cell
//   k_nb_subm_table, k_nb_down_tables   [N, 27] neighbour tables, one (row, tap) per thread
//   k_nb_conv       workgroup = 64 output rows.  Per tap that some row of the tile has (one ballot each), the gathered input rows
//                   (zero where -1) and W[k] pass through LDS in slices of 32 input channels to v_mfma_f32_32x32x2_f32: a wave owns
//                   32 rows x 32 output channels per accumulator, exact fp32 products; an fma chain per slice, the slices of a
//                   tap and then the taps summed in fp32 (three short sums instead of one chain of 27 Cin terms)
//   k_nb_wgrad      workgroup = (tap, row chunk): dW[k] = X_k^T G over the chunk on the same MFMA, written to a partial slab;
//                   k_nb_fold sums the slabs in chunk order
//   k_nb_sample_fwd thread = (point, float4 of channels): the pose transform and the normalisation, then the eight corners of the
//                   thread's level through its index volume, torch's grid_sample arithmetic and corner order
//   k_nb_sample_bwd the same walk, adding w g to the rows in 64-bit fixed point (xr_fixed.h: integer adds commute, repeatable bits)
// Compiled with -ffp-contract=off: every expression is fp32 in the written order.
#include "xr_common.h"
#include "xr_scan.h"
#include "xr_fixed.h"
#include "../../include/xrnerf_mi355_neuralbody.h"

#define NB_BLOCK 256
static_assert(NB_BLOCK == XR_SCAN_BLOCK && NB_BLOCK == XR_FIX_BLOCK, "the shared workgroup routines are written for 256 threads");
#define NB_SPAN 16                              // cells per thread of the count / rank kernels
#define NB_CELLS_PER_BLOCK (NB_BLOCK * NB_SPAN)
#define NB_TAPS XR_NB_TAPS
#define NB_TILE XR_NB_TILE
#define NB_KC 32                                // input channels per LDS slice of the convolution
#define NB_MARK (-2)

typedef float nb_f32x16 __attribute__((ext_vector_type(16)));
#define NB_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
__device__ __forceinline__ constexpr int nb_drow(int r) { return (r & 3) + 8 * (r >> 2); }

static inline bool nb_dims_ok(int D, int H, int W) {
    if (D <= 0 || H <= 0 || W <= 0 || (D & 31) || (H & 31) || (W & 31)) return false;
    return (uint64_t)D * (uint64_t)H * (uint64_t)W <= (uint64_t)XR_NB_MAX_CELLS;
}
static inline bool nb_channels_ok(int c) { return c == 16 || c == 32 || c == 64 || c == 128; }
static inline bool nb_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

extern "C" int xr_nb_layout(uint32_t V, int D, int H, int W, uint64_t* out) {
    XR_REQUIRE(out != nullptr, "null output");
    XR_REQUIRE(nb_dims_ok(D, H, W), "out_sh must be positive multiples of 32 with at most XR_NB_MAX_CELLS cells");
    uint64_t vo = 0, ro = 0;
    for (int l = 0; l < XR_NB_LEVELS; ++l) {
        const uint64_t cells = ((uint64_t)(D >> l) * (uint64_t)(H >> l)) * (uint64_t)(W >> l);
        const uint64_t grown = (uint64_t)V << (3 * l);
        out[l] = vo; out[5 + l] = ro;
        vo += cells; ro += grown < cells ? grown : cells;
    }
    out[10] = vo; out[11] = ro;
    return 0;
}

// ------------------------------------------------------------------------------------------ structure: marks
__global__ void __launch_bounds__(NB_BLOCK) k_nb_mark0(const int32_t* __restrict__ coord, uint32_t V, int D, int H, int W,
                                                       int32_t* __restrict__ vol) {
    const uint32_t i = blockIdx.x * NB_BLOCK + threadIdx.x;
    if (i >= V) return;
    const int z = coord[i * 3ull], y = coord[i * 3ull + 1], x = coord[i * 3ull + 2];
    if (z < 0 || z >= D || y < 0 || y >= H || x < 0 || x >= W) return;
    vol[((uint32_t)z * (uint32_t)H + (uint32_t)y) * (uint32_t)W + (uint32_t)x] = NB_MARK;
}

__global__ void __launch_bounds__(NB_BLOCK) k_nb_vert_row(const int32_t* __restrict__ coord, uint32_t V, int D, int H, int W,
                                                          const int32_t* __restrict__ vol, int32_t* __restrict__ vert_row) {
    const uint32_t i = blockIdx.x * NB_BLOCK + threadIdx.x;
    if (i >= V) return;
    const int z = coord[i * 3ull], y = coord[i * 3ull + 1], x = coord[i * 3ull + 2];
    const bool in = !(z < 0 || z >= D || y < 0 || y >= H || x < 0 || x >= W);
    vert_row[i] = in ? vol[((uint32_t)z * (uint32_t)H + (uint32_t)y) * (uint32_t)W + (uint32_t)x] : -1;
}

// output cells o (extent n_out) with 2 o - 1 + k = i for a tap k in {0, 1, 2}
static __device__ inline int nb_outs(int i, int n_out, int* o) {
    int n = 0;
    if (i & 1) {
        o[n++] = (i - 1) >> 1;                                  // k = 2
        if (((i + 1) >> 1) < n_out) o[n++] = (i + 1) >> 1;      // k = 0
    } else {
        o[n++] = i >> 1;                                        // k = 1
    }
    return n;
}

// (D, H, W): the INPUT level's dims; count_in: the input level's row count on the device
__global__ void __launch_bounds__(NB_BLOCK) k_nb_mark_down(const int32_t* __restrict__ rows_in, const int32_t* __restrict__ count_in,
                                                           uint32_t cap_in, int D, int H, int W, int32_t* __restrict__ vol_out) {
    const uint32_t r = blockIdx.x * NB_BLOCK + threadIdx.x;
    const uint32_t n_in = min((uint32_t)count_in[0], cap_in);
    if (r >= n_in) return;
    const uint32_t lin = (uint32_t)rows_in[r];
    const int x = (int)(lin % (uint32_t)W), y = (int)((lin / (uint32_t)W) % (uint32_t)H), z = (int)(lin / ((uint32_t)W * (uint32_t)H));
    if (z >= D) return;
    const int Do = D >> 1, Ho = H >> 1, Wo = W >> 1;
    int oz[2], oy[2], ox[2];
    const int nz = nb_outs(z, Do, oz), ny = nb_outs(y, Ho, oy), nx = nb_outs(x, Wo, ox);
    for (int a = 0; a < nz; ++a)
        for (int b = 0; b < ny; ++b)
            for (int c = 0; c < nx; ++c)
                vol_out[((uint32_t)oz[a] * (uint32_t)Ho + (uint32_t)oy[b]) * (uint32_t)Wo + (uint32_t)ox[c]] = NB_MARK;
}

// ------------------------------------------------------------------------------------------ structure: count / scan / rank
__global__ void __launch_bounds__(NB_BLOCK) k_nb_count(const int32_t* __restrict__ vol, uint32_t cells, uint32_t* __restrict__ cnt) {
    const uint32_t base = blockIdx.x * NB_CELLS_PER_BLOCK;
    uint32_t c = 0, sum;
    for (uint32_t s = 0; s < NB_SPAN; ++s) {
        const uint32_t cell = base + s * NB_BLOCK + threadIdx.x;
        if (cell < cells && vol[cell] == NB_MARK) ++c;
    }
    xr_block_excl(c, &sum);
    if (threadIdx.x == 0) cnt[blockIdx.x] = sum;
}

// exclusive scan of cnt [nb] -> off [nb], the total -> count[0]; one workgroup
__global__ void __launch_bounds__(NB_BLOCK) k_nb_scan(const uint32_t* __restrict__ cnt, uint32_t nb, uint32_t* __restrict__ off,
                                                      int32_t* __restrict__ count) {
    const uint64_t total = xr_scan_sweeps(nb, [&](uint32_t b) { return cnt[b]; }, [&](uint32_t b, uint32_t base) { off[b] = base; });
    if (threadIdx.x == 0) count[0] = xr_scan_total(total);
}

__global__ void __launch_bounds__(NB_BLOCK) k_nb_rank(int32_t* __restrict__ vol, uint32_t cells, const uint32_t* __restrict__ cnt,
                                                      const uint32_t* __restrict__ off, int32_t* __restrict__ rows, uint32_t cap) {
    if (cnt[blockIdx.x] == 0) return;                              // (the whole workgroup: nothing marked here, the cells stay -1)
    const uint32_t base = blockIdx.x * NB_CELLS_PER_BLOCK;
    uint32_t running = off[blockIdx.x];
    for (uint32_t s = 0; s < NB_SPAN; ++s) {
        const uint32_t cell = base + s * NB_BLOCK + threadIdx.x;
        const bool f = cell < cells && vol[cell] == NB_MARK;
        uint32_t total;
        const uint32_t before = xr_block_excl_flag(f, &total);
        if (f) {
            const uint32_t rank = running + before;
            vol[cell] = (int32_t)rank;
            if (rank < cap) rows[rank] = (int32_t)cell;
        }
        running += total;
    }
}

extern "C" size_t xr_nb_build_rows_workspace_bytes(int D, int H, int W) {
    if (!nb_dims_ok(D, H, W)) return 0;
    const uint64_t cells = (uint64_t)D * H * W;
    return (size_t)(2u * xr_div_up(cells, NB_CELLS_PER_BLOCK)) * sizeof(uint32_t);
}

extern "C" int xr_nb_build_rows(const int32_t* coord, uint32_t V, int D, int H, int W, int32_t* vol, int32_t* rows, int32_t* vert_row,
                                int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    XR_REQUIRE(nb_dims_ok(D, H, W), "out_sh must be positive multiples of 32 with at most XR_NB_MAX_CELLS cells");
    if (V == 0) {                                                  // no vertex: five empty levels (the outputs are consumed downstream)
        XR_REQUIRE(vol && counts, "null pointer");
        uint64_t lay0[12];
        xr_nb_layout(0, D, H, W, lay0);
        XR_HIP(hipMemsetAsync(vol, 0xff, (size_t)lay0[10] * sizeof(int32_t), (hipStream_t)stream));
        XR_HIP(hipMemsetAsync(counts, 0, XR_NB_LEVELS * sizeof(int32_t), (hipStream_t)stream));
        return 0;
    }
    XR_REQUIRE(coord && vol && rows && vert_row && counts && workspace, "null pointer");
    XR_REQUIRE(V <= (1u << 24), "too many vertices");
    if (workspace_bytes < xr_nb_build_rows_workspace_bytes(D, H, W)) { xr_set_error("%s: workspace too small", __func__); return XR_ENOMEM; }
    uint64_t lay[12];
    xr_nb_layout(V, D, H, W, lay);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nb0 = xr_div_up((uint64_t)D * H * W, NB_CELLS_PER_BLOCK);
    uint32_t* cnt = (uint32_t*)workspace;
    uint32_t* off = cnt + nb0;
    XR_HIP(hipMemsetAsync(vol, 0xff, (size_t)lay[10] * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_nb_mark0, dim3(xr_div_up(V, NB_BLOCK)), dim3(NB_BLOCK), 0, st, coord, V, D, H, W, vol);
    for (int l = 0; l < XR_NB_LEVELS; ++l) {
        const int Dl = D >> l, Hl = H >> l, Wl = W >> l;
        const uint32_t cells = (uint32_t)Dl * (uint32_t)Hl * (uint32_t)Wl;
        const uint32_t cap = (uint32_t)((l + 1 < XR_NB_LEVELS ? lay[5 + l + 1] : lay[11]) - lay[5 + l]);
        const uint32_t nb = xr_div_up(cells, NB_CELLS_PER_BLOCK);
        int32_t* vl = vol + lay[l];
        int32_t* rl = rows + lay[5 + l];
        hipLaunchKernelGGL(k_nb_count, dim3(nb), dim3(NB_BLOCK), 0, st, vl, cells, cnt);
        hipLaunchKernelGGL(k_nb_scan, dim3(1), dim3(NB_BLOCK), 0, st, cnt, nb, off, counts + l);
        hipLaunchKernelGGL(k_nb_rank, dim3(nb), dim3(NB_BLOCK), 0, st, vl, cells, cnt, off, rl, cap);
        if (l + 1 < XR_NB_LEVELS)
            hipLaunchKernelGGL(k_nb_mark_down, dim3(xr_div_up(cap, NB_BLOCK)), dim3(NB_BLOCK), 0, st, rl, counts + l, cap, Dl, Hl, Wl,
                               vol + lay[l + 1]);
    }
    hipLaunchKernelGGL(k_nb_vert_row, dim3(xr_div_up(V, NB_BLOCK)), dim3(NB_BLOCK), 0, st, coord, V, D, H, W, vol, vert_row);
    XR_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------ structure: neighbour tables
__global__ void __launch_bounds__(NB_BLOCK) k_nb_subm_table(const int32_t* __restrict__ vol, const int32_t* __restrict__ rows, uint32_t n,
                                                            int D, int H, int W, int32_t* __restrict__ nbr) {
    const uint64_t e = (uint64_t)blockIdx.x * NB_BLOCK + threadIdx.x;
    if (e >= (uint64_t)n * NB_TAPS) return;
    const uint32_t r = (uint32_t)(e / NB_TAPS), k = (uint32_t)(e - (uint64_t)r * NB_TAPS);
    const uint32_t lin = (uint32_t)rows[r];
    const int x = (int)(lin % (uint32_t)W), y = (int)((lin / (uint32_t)W) % (uint32_t)H), z = (int)(lin / ((uint32_t)W * (uint32_t)H));
    const int nz = z + (int)(k / 9) - 1, ny = y + (int)((k / 3) % 3) - 1, nx = x + (int)(k % 3) - 1;
    int32_t v = -1;
    if (nz >= 0 && nz < D && ny >= 0 && ny < H && nx >= 0 && nx < W) v = vol[((uint32_t)nz * (uint32_t)H + (uint32_t)ny) * (uint32_t)W + (uint32_t)nx];
    nbr[e] = v;
}

// (D, H, W): the INPUT level's dims
__global__ void __launch_bounds__(NB_BLOCK) k_nb_down_out_table(const int32_t* __restrict__ vol_in, const int32_t* __restrict__ rows_out,
                                                                uint32_t n_out, int D, int H, int W, int32_t* __restrict__ tab) {
    const uint64_t e = (uint64_t)blockIdx.x * NB_BLOCK + threadIdx.x;
    if (e >= (uint64_t)n_out * NB_TAPS) return;
    const uint32_t r = (uint32_t)(e / NB_TAPS), k = (uint32_t)(e - (uint64_t)r * NB_TAPS);
    const uint32_t Ho = (uint32_t)H >> 1, Wo = (uint32_t)W >> 1;
    const uint32_t lin = (uint32_t)rows_out[r];
    const int x = (int)(lin % Wo), y = (int)((lin / Wo) % Ho), z = (int)(lin / (Wo * Ho));
    const int iz = 2 * z - 1 + (int)(k / 9), iy = 2 * y - 1 + (int)((k / 3) % 3), ix = 2 * x - 1 + (int)(k % 3);
    int32_t v = -1;
    if (iz >= 0 && iz < D && iy >= 0 && iy < H && ix >= 0 && ix < W) v = vol_in[((uint32_t)iz * (uint32_t)H + (uint32_t)iy) * (uint32_t)W + (uint32_t)ix];
    tab[e] = v;
}

// o with 2 o - 1 + k = i, or -1
static __device__ inline int nb_out_of(int i, int k, int n_out) {
    const int t = i + 1 - k;
    if (t < 0 || (t & 1)) return -1;
    return (t >> 1) < n_out ? (t >> 1) : -1;
}

__global__ void __launch_bounds__(NB_BLOCK) k_nb_down_in_table(const int32_t* __restrict__ vol_out, const int32_t* __restrict__ rows_in,
                                                               uint32_t n_in, int D, int H, int W, int32_t* __restrict__ tab) {
    const uint64_t e = (uint64_t)blockIdx.x * NB_BLOCK + threadIdx.x;
    if (e >= (uint64_t)n_in * NB_TAPS) return;
    const uint32_t r = (uint32_t)(e / NB_TAPS), k = (uint32_t)(e - (uint64_t)r * NB_TAPS);
    const uint32_t lin = (uint32_t)rows_in[r];
    const int x = (int)(lin % (uint32_t)W), y = (int)((lin / (uint32_t)W) % (uint32_t)H), z = (int)(lin / ((uint32_t)W * (uint32_t)H));
    const int Do = D >> 1, Ho = H >> 1, Wo = W >> 1;
    const int oz = nb_out_of(z, (int)(k / 9), Do), oy = nb_out_of(y, (int)((k / 3) % 3), Ho), ox = nb_out_of(x, (int)(k % 3), Wo);
    int32_t v = -1;
    if (z < D && oz >= 0 && oy >= 0 && ox >= 0) v = vol_out[((uint32_t)oz * (uint32_t)Ho + (uint32_t)oy) * (uint32_t)Wo + (uint32_t)ox];
    tab[e] = v;
}

extern "C" int xr_nb_subm_table(const int32_t* vol, const int32_t* rows, uint32_t n, int D, int H, int W, int32_t* nbr, void* stream) {
    XR_REQUIRE(D > 0 && H > 0 && W > 0 && (uint64_t)D * H * W <= (uint64_t)XR_NB_MAX_CELLS, "bad level dims");
    if (n == 0) return 0;
    XR_REQUIRE(vol && rows && nbr, "null pointer");
    XR_REQUIRE((uint64_t)n <= (uint64_t)D * H * W, "more rows than cells");
    hipLaunchKernelGGL(k_nb_subm_table, dim3(xr_div_up((uint64_t)n * NB_TAPS, NB_BLOCK)), dim3(NB_BLOCK), 0, (hipStream_t)stream, vol, rows,
                       n, D, H, W, nbr);
    XR_LAUNCH_CHECK();
    return 0;
}

extern "C" int xr_nb_down_tables(const int32_t* vol_in, const int32_t* rows_in, uint32_t n_in, const int32_t* vol_out,
                                 const int32_t* rows_out, uint32_t n_out, int D, int H, int W, int32_t* out_tab, int32_t* in_tab,
                                 void* stream) {
    XR_REQUIRE(D > 0 && H > 0 && W > 0 && !(D & 1) && !(H & 1) && !(W & 1) && (uint64_t)D * H * W <= (uint64_t)XR_NB_MAX_CELLS,
               "bad level dims");
    XR_REQUIRE((uint64_t)n_in <= (uint64_t)D * H * W && (uint64_t)n_out * 8u <= (uint64_t)D * H * W, "more rows than cells");
    hipStream_t st = (hipStream_t)stream;
    if (n_out != 0) {
        XR_REQUIRE(vol_in && rows_out && out_tab, "null pointer");
        hipLaunchKernelGGL(k_nb_down_out_table, dim3(xr_div_up((uint64_t)n_out * NB_TAPS, NB_BLOCK)), dim3(NB_BLOCK), 0, st, vol_in, rows_out,
                           n_out, D, H, W, out_tab);
    }
    if (n_in != 0 && in_tab != nullptr) {
        XR_REQUIRE(vol_out && rows_in, "null pointer");
        hipLaunchKernelGGL(k_nb_down_in_table, dim3(xr_div_up((uint64_t)n_in * NB_TAPS, NB_BLOCK)), dim3(NB_BLOCK), 0, st, vol_out, rows_in,
                           n_in, D, H, W, in_tab);
    }
    XR_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------ convolution
struct NbConvArgs {
    const float* x; const int32_t* tab; const float* w;
    uint32_t n; int cin, cout, transposed, flip;
    float* out;
};
#define NB_XLD (NB_KC + 1)

__global__ void __launch_bounds__(NB_BLOCK) k_nb_conv(NbConvArgs a) {
    __shared__ int32_t s_tab[NB_TILE * NB_TAPS];
    __shared__ float s_x[NB_TILE * NB_XLD];
    __shared__ float s_w[NB_KC * (128 + 1)];
    __shared__ uint32_t s_has[NB_TAPS];
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63, col = lane & 31, hi = lane >> 5;
    const uint32_t row0 = blockIdx.x * NB_TILE;
    const int cin = a.cin, cout = a.cout;
    const int cout_pad = cout < 32 ? 32 : cout, kc = cin < NB_KC ? cin : NB_KC, ld = cout_pad + 1;
    const uint32_t n_tasks = 2u * (uint32_t)(cout_pad / 32);
    for (uint32_t e = t; e < NB_TILE * NB_TAPS; e += NB_BLOCK) {
        const uint32_t r = e / NB_TAPS;
        s_tab[e] = row0 + r < a.n ? a.tab[(uint64_t)row0 * NB_TAPS + e] : -1;
    }
    __syncthreads();
    if (wave == 0) {
        for (int k = 0; k < NB_TAPS; ++k) {
            const unsigned long long m = __ballot(s_tab[lane * NB_TAPS + (a.flip ? NB_TAPS - 1 - k : k)] >= 0);
            if (lane == 0) s_has[k] = m != 0ull ? 1u : 0u;
        }
    }
    __syncthreads();
    // three levels of summation, each an fp32 chain: the <= 32 channels of a slice (the MFMA's fma chain from zero), the slices of a
    // tap, the taps.  One chain over all 27 Cin terms would carry ~sqrt(27 Cin) roundings of the growing sum (6.7e-7 of max|ref| at
    // K = 1728 against 1.5e-7 for torch's blocked fp32 sum)
    nb_f32x16 acc[2], tap[2];
    nb_f32x16 zero;
#pragma unroll
    for (int r = 0; r < 16; ++r) zero[r] = 0.f;
    acc[0] = zero; acc[1] = zero;
    for (int k = 0; k < NB_TAPS; ++k) {
        if (!s_has[k]) continue;                                   // no row of this tile has the tap (the whole workgroup skips it)
        const int tk = a.flip ? NB_TAPS - 1 - k : k;
        tap[0] = zero; tap[1] = zero;
        for (int c0 = 0; c0 < cin; c0 += kc) {
            __syncthreads();                                       // the previous slice has been consumed
            const uint32_t q4 = (uint32_t)kc / 4u;
            for (uint32_t e = t; e < NB_TILE * q4; e += NB_BLOCK) {
                const uint32_t r = e / q4, q = e - r * q4;
                const int32_t src = s_tab[r * NB_TAPS + tk];
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (src >= 0) v = *reinterpret_cast<const float4*>(a.x + (uint64_t)(uint32_t)src * cin + c0 + 4u * q);
                float* d = s_x + r * NB_XLD + 4u * q;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
            const uint32_t total = (uint32_t)kc * (uint32_t)cout_pad;
            if (!a.transposed) {
                for (uint32_t e = t; e < total; e += NB_BLOCK) {
                    const uint32_t j = e / (uint32_t)kc, c = e - j * (uint32_t)kc;
                    s_w[c * ld + j] = (int)j < cout ? a.w[((uint64_t)j * NB_TAPS + k) * cin + c0 + c] : 0.f;
                }
            } else {
                for (uint32_t e = t; e < total; e += NB_BLOCK) {
                    const uint32_t c = e / (uint32_t)cout_pad, j = e - c * (uint32_t)cout_pad;
                    s_w[c * ld + j] = (int)j < cout ? a.w[((uint64_t)(c0 + c) * NB_TAPS + k) * cout + j] : 0.f;
                }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const uint32_t task = wave + 4u * q;
                if (task < n_tasks) {                              // (wave-uniform)
                    const uint32_t rb = task & 1u, cb = task >> 1;
                    const float* xa = s_x + (rb * 32u + col) * NB_XLD + hi;
                    const float* wb = s_w + hi * ld + cb * 32u + col;
                    nb_f32x16 part = zero;
                    for (int s = 0; s < kc; s += 2) part = NB_MFMA(xa[s], wb[s * ld], part);
                    tap[q] = tap[q] + part;
                }
            }
        }
        acc[0] = acc[0] + tap[0];
        acc[1] = acc[1] + tap[1];
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const uint32_t task = wave + 4u * q;
        if (task < n_tasks) {
            const uint32_t rb = task & 1u, cb = task >> 1;
            const uint32_t j = cb * 32u + col;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t row = row0 + rb * 32u + (uint32_t)nb_drow(r) + 4u * hi;
                if (row < a.n && (int)j < cout) a.out[(uint64_t)row * cout + j] = acc[q][r];
            }
        }
    }
}

extern "C" int xr_nb_conv(const float* x, const int32_t* tab, const float* w, uint32_t n, int cin, int cout, int transposed, int flip,
                          float* out, void* stream) {
    XR_REQUIRE(nb_channels_ok(cin) && nb_channels_ok(cout), "channels must be 16, 32, 64 or 128");
    if (n == 0) return 0;
    XR_REQUIRE(x && tab && w && out, "null pointer");
    XR_REQUIRE(nb_aligned16(x) && nb_aligned16(w) && nb_aligned16(out), "x, w and out must be 16-byte aligned");
    XR_REQUIRE(n <= XR_NB_MAX_CELLS, "too many rows");
    NbConvArgs a{x, tab, w, n, cin, cout, transposed ? 1 : 0, flip ? 1 : 0, out};
    hipLaunchKernelGGL(k_nb_conv, dim3(xr_div_up(n, NB_TILE)), dim3(NB_BLOCK), 0, (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------ weight gradient
#define NB_WG_ROWS 32
#define NB_WG_MAX_CHUNKS 32u
struct NbWgArgs {
    const float* x; const int32_t* tab; const float* g;
    uint32_t n; int cin, cout; uint32_t rows_per_chunk;
    float* part;
};
static inline void nb_wg_chunks(uint32_t n, uint32_t* chunks, uint32_t* rows_per_chunk) {
    uint32_t c = xr_div_up(n, 256u);
    if (c > NB_WG_MAX_CHUNKS) c = NB_WG_MAX_CHUNKS;
    if (c < 1) c = 1;
    uint32_t rpc = xr_div_up(n, c);
    rpc = (rpc + NB_WG_ROWS - 1) / NB_WG_ROWS * NB_WG_ROWS;
    *chunks = xr_div_up(n, rpc); *rows_per_chunk = rpc;
}

__global__ void __launch_bounds__(NB_BLOCK) k_nb_wgrad(NbWgArgs a) {
    __shared__ float s_g[NB_WG_ROWS * 128];
    __shared__ float s_x[NB_WG_ROWS * 128];
    __shared__ int32_t s_src[NB_WG_ROWS];
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63, col = lane & 31, hi = lane >> 5;
    const uint32_t k = blockIdx.x, chunk = blockIdx.y;
    const int cin = a.cin, cout = a.cout;
    const uint32_t cin_pad = cin < 32 ? 32u : (uint32_t)cin, cout_pad = cout < 32 ? 32u : (uint32_t)cout;
    const uint32_t nib = cout_pad / 32u, n_tasks = nib * (cin_pad / 32u);
    const uint32_t r_begin = chunk * a.rows_per_chunk;
    const uint32_t r_end = min(a.n, r_begin + a.rows_per_chunk);
    // two levels of summation: the 32 rows of a block (the MFMA's fma chain from zero), then the blocks of the chunk
    nb_f32x16 acc[4];
    nb_f32x16 zero;
#pragma unroll
    for (int r = 0; r < 16; ++r) zero[r] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = zero;
    for (uint32_t r0 = r_begin; r0 < r_end; r0 += NB_WG_ROWS) {
        __syncthreads();                                           // the previous rows have been consumed
        if (t < NB_WG_ROWS) s_src[t] = r0 + t < r_end ? a.tab[(uint64_t)(r0 + t) * NB_TAPS + k] : -1;
        __syncthreads();
        const unsigned long long m = __ballot(lane < NB_WG_ROWS && s_src[lane & (NB_WG_ROWS - 1)] >= 0);
        if (m == 0ull) continue;                                   // none of these rows has the tap (the same in every wave)
        for (uint32_t e = t; e < NB_WG_ROWS * cout_pad; e += NB_BLOCK) {
            const uint32_t rr = e / cout_pad, i = e - rr * cout_pad;
            s_g[e] = (s_src[rr] >= 0 && (int)i < cout) ? a.g[(uint64_t)(r0 + rr) * cout + i] : 0.f;
        }
        for (uint32_t e = t; e < NB_WG_ROWS * cin_pad; e += NB_BLOCK) {
            const uint32_t rr = e / cin_pad, j = e - rr * cin_pad;
            const int32_t src = s_src[rr];
            s_x[e] = (src >= 0 && (int)j < cin) ? a.x[(uint64_t)(uint32_t)src * cin + j] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t task = wave + 4u * q;
            if (task < n_tasks) {                                  // (wave-uniform)
                const uint32_t ib = task % nib, jb = task / nib;
                const float* ga = s_g + hi * cout_pad + ib * 32u + col;
                const float* xb = s_x + hi * cin_pad + jb * 32u + col;
                nb_f32x16 part = zero;
#pragma unroll 4
                for (uint32_t s = 0; s < NB_WG_ROWS; s += 2) part = NB_MFMA(ga[s * cout_pad], xb[s * cin_pad], part);
                acc[q] = acc[q] + part;
            }
        }
    }
    float* slab = a.part + (uint64_t)chunk * (uint64_t)cout * NB_TAPS * (uint64_t)cin;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t task = wave + 4u * q;
        if (task < n_tasks) {
            const uint32_t ib = task % nib, jb = task / nib;
            const uint32_t ci = jb * 32u + col;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t co = ib * 32u + (uint32_t)nb_drow(r) + 4u * hi;
                if ((int)co < cout && (int)ci < cin) slab[((uint64_t)co * NB_TAPS + k) * cin + ci] = acc[q][r];
            }
        }
    }
}

__global__ void __launch_bounds__(NB_BLOCK) k_nb_fold(const float* __restrict__ part, uint32_t chunks, uint32_t size, float* __restrict__ out) {
    const uint32_t e = blockIdx.x * NB_BLOCK + threadIdx.x;
    if (e >= size) return;
    float s = part[e];
    for (uint32_t c = 1; c < chunks; ++c) s += part[(uint64_t)c * size + e];
    out[e] = s;
}

extern "C" size_t xr_nb_conv_weight_grad_workspace_bytes(uint32_t n, int cin, int cout) {
    if (n == 0 || !nb_channels_ok(cin) || !nb_channels_ok(cout)) return 0;
    uint32_t chunks, rpc;
    nb_wg_chunks(n, &chunks, &rpc);
    return (size_t)chunks * (size_t)cout * NB_TAPS * (size_t)cin * sizeof(float);
}

extern "C" int xr_nb_conv_weight_grad(const float* x, const int32_t* tab, const float* g, uint32_t n, int cin, int cout, float* dw,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    XR_REQUIRE(nb_channels_ok(cin) && nb_channels_ok(cout), "channels must be 16, 32, 64 or 128");
    if (n == 0) return 0;
    XR_REQUIRE(x && tab && g && dw && workspace, "null pointer");
    XR_REQUIRE(n <= XR_NB_MAX_CELLS, "too many rows");
    if (workspace_bytes < xr_nb_conv_weight_grad_workspace_bytes(n, cin, cout)) { xr_set_error("%s: workspace too small", __func__); return XR_ENOMEM; }
    uint32_t chunks, rpc;
    nb_wg_chunks(n, &chunks, &rpc);
    NbWgArgs a{x, tab, g, n, cin, cout, rpc, (float*)workspace};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_nb_wgrad, dim3(NB_TAPS, chunks), dim3(NB_BLOCK), 0, st, a);
    const uint32_t size = (uint32_t)cout * NB_TAPS * (uint32_t)cin;
    hipLaunchKernelGGL(k_nb_fold, dim3(xr_div_up(size, NB_BLOCK)), dim3(NB_BLOCK), 0, st, (const float*)workspace, chunks, size, dw);
    XR_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------ sampling
#define NB_Q4 (XR_NB_FEATURES / 4)                 // float4 items per point
struct NbSampleGeom {
    const float* pts; const float* R; const float* T; const float* mn;
    float voxel; int D, H, W;
    const int32_t* vol[4];
    uint32_t n;
};
struct NbCorners { int32_t row[8]; float w[8]; };

// level (1..4), channels and column offset of float4 item q of a point's 352 features
static __device__ inline void nb_item(uint32_t q, int* l, int* C, uint32_t* coff, uint32_t* c4) {
    if (q < 8u) { *l = 1; *C = 32; *coff = 0u; *c4 = q; }
    else if (q < 24u) { *l = 2; *C = 64; *coff = 32u; *c4 = q - 8u; }
    else if (q < 56u) { *l = 3; *C = 128; *coff = 96u; *c4 = q - 24u; }
    else { *l = 4; *C = 128; *coff = 224u; *c4 = q - 56u; }
}

// the eight corners of point i in level l, in torch's order (x fastest, then y, then z), with their rows (-1: outside or empty)
static __device__ inline void nb_corners(const NbSampleGeom& g, uint32_t i, int l, NbCorners* o) {
    const float d0 = g.pts[i * 3ull] - g.T[0], d1 = g.pts[i * 3ull + 1] - g.T[1], d2 = g.pts[i * 3ull + 2] - g.T[2];
    const int dims[3] = {g.W, g.H, g.D};
    float f[3], lo[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float q = (d0 * g.R[j] + d1 * g.R[3 + j]) + d2 * g.R[6 + j];
        const float c = ((q - g.mn[j]) / g.voxel) / (float)dims[j] * 2.f - 1.f;
        f[j] = ((c + 1.f) / 2.f) * (float)((dims[j] >> l) - 1);
        lo[j] = floorf(f[j]);
    }
    const int Wl = g.W >> l, Hl = g.H >> l, Dl = g.D >> l;
    const int32_t* vol = g.vol[l - 1];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int bx = c & 1, by = (c >> 1) & 1, bz = c >> 2;
        const float cx = lo[0] + (float)bx, cy = lo[1] + (float)by, cz = lo[2] + (float)bz;
        const float wx = bx ? f[0] - lo[0] : (lo[0] + 1.f) - f[0];
        const float wy = by ? f[1] - lo[1] : (lo[1] + 1.f) - f[1];
        const float wz = bz ? f[2] - lo[2] : (lo[2] + 1.f) - f[2];
        o->w[c] = (wx * wy) * wz;
        int32_t row = -1;
        if (cx >= 0.f && cx <= (float)(Wl - 1) && cy >= 0.f && cy <= (float)(Hl - 1) && cz >= 0.f && cz <= (float)(Dl - 1))
            row = vol[((uint32_t)(int)cz * (uint32_t)Hl + (uint32_t)(int)cy) * (uint32_t)Wl + (uint32_t)(int)cx];
        o->row[c] = row;
    }
}

struct NbSampleFwd { NbSampleGeom g; const float* feat[4]; float* out; uint32_t ld; };

__global__ void __launch_bounds__(NB_BLOCK) k_nb_sample_fwd(NbSampleFwd a) {
    const uint64_t e = (uint64_t)blockIdx.x * NB_BLOCK + threadIdx.x;
    if (e >= (uint64_t)a.g.n * NB_Q4) return;
    const uint32_t i = (uint32_t)(e / NB_Q4), q = (uint32_t)(e - (uint64_t)i * NB_Q4);
    int l, C; uint32_t coff, c4;
    nb_item(q, &l, &C, &coff, &c4);
    NbCorners cn;
    nb_corners(a.g, i, l, &cn);
    const float* feat = a.feat[l - 1];
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if (cn.row[c] >= 0) {
            const float4 v = *reinterpret_cast<const float4*>(feat + (uint64_t)(uint32_t)cn.row[c] * C + 4u * c4);
            const float w = cn.w[c];
            s.x = s.x + v.x * w; s.y = s.y + v.y * w; s.z = s.z + v.z * w; s.w = s.w + v.w * w;
        }
    }
    *reinterpret_cast<float4*>(a.out + (uint64_t)i * a.ld + coff + 4u * c4) = s;
}

static int nb_sample_geom(NbSampleGeom* g, const float* pts, const float* R, const float* T, const float* mn, float voxel, int D, int H, int W,
                          const void* const* vols, uint32_t n) {
    if (!nb_dims_ok(D, H, W)) { xr_set_error("%s: out_sh must be positive multiples of 32 with at most XR_NB_MAX_CELLS cells", __func__); return XR_EINVAL; }
    if (!(voxel > 0.f)) { xr_set_error("%s: voxel size must be positive", __func__); return XR_EINVAL; }
    if (n > (1u << 24)) { xr_set_error("%s: too many points", __func__); return XR_EINVAL; }
    if (n == 0) return 0;
    if (!pts || !R || !T || !mn || !vols) { xr_set_error("%s: null pointer", __func__); return XR_EINVAL; }
    g->pts = pts; g->R = R; g->T = T; g->mn = mn; g->voxel = voxel; g->D = D; g->H = H; g->W = W; g->n = n;
    for (int l = 0; l < 4; ++l) {
        if (!vols[l]) { xr_set_error("%s: null index volume", __func__); return XR_EINVAL; }
        g->vol[l] = (const int32_t*)vols[l];
    }
    return 0;
}

extern "C" int xr_nb_sample_forward(const float* pts, const float* R, const float* T, const float* min_xyz, float voxel, int D, int H,
                                    int W, const void* const* vols, const void* const* feats, uint32_t n, float* out, uint32_t ld,
                                    void* stream) {
    NbSampleFwd a;
    const int rc = nb_sample_geom(&a.g, pts, R, T, min_xyz, voxel, D, H, W, vols, n);
    if (rc != 0) return rc;
    if (n == 0) return 0;
    XR_REQUIRE(feats && out, "null pointer");
    XR_REQUIRE(ld >= XR_NB_FEATURES && (ld & 3u) == 0 && nb_aligned16(out), "out must be 16-byte aligned with a row stride >= 352 that is a multiple of 4");
    for (int l = 0; l < 4; ++l) {
        XR_REQUIRE(nb_aligned16(feats[l]), "the rows must be 16-byte aligned");
        a.feat[l] = (const float*)feats[l];            // (may be null for a level without rows: its index volume is all -1)
    }
    a.out = out; a.ld = ld;
    hipLaunchKernelGGL(k_nb_sample_fwd, dim3(xr_div_up((uint64_t)n * NB_Q4, NB_BLOCK)), dim3(NB_BLOCK), 0, (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return 0;
}

// ---- backward: 64-bit fixed point
struct NbSampleBwd {
    NbSampleGeom g; const float* grad; uint32_t ld;
    const double* scale;
    unsigned long long* acc[4];
};

__global__ void __launch_bounds__(NB_BLOCK) k_nb_absmax(const float* __restrict__ grad, uint32_t ld, uint32_t n, float* __restrict__ bmax) {
    float m = 0.f;
    const uint64_t total = (uint64_t)n * NB_Q4;
    for (uint64_t e = (uint64_t)blockIdx.x * NB_BLOCK + threadIdx.x; e < total; e += (uint64_t)gridDim.x * NB_BLOCK) {
        const uint32_t i = (uint32_t)(e / NB_Q4), q = (uint32_t)(e - (uint64_t)i * NB_Q4);
        const float4 v = *reinterpret_cast<const float4*>(grad + (uint64_t)i * ld + 4u * q);
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
    xr_fix_block_max(m, bmax);
}

__global__ void __launch_bounds__(NB_BLOCK) k_nb_sample_bwd(NbSampleBwd a) {
    const uint64_t e = (uint64_t)blockIdx.x * NB_BLOCK + threadIdx.x;
    if (e >= (uint64_t)a.g.n * NB_Q4) return;
    const double scale = a.scale[0];
    const uint32_t i = (uint32_t)(e / NB_Q4), q = (uint32_t)(e - (uint64_t)i * NB_Q4);
    int l, C; uint32_t coff, c4;
    nb_item(q, &l, &C, &coff, &c4);
    NbCorners cn;
    nb_corners(a.g, i, l, &cn);
    const float4 gv = *reinterpret_cast<const float4*>(a.grad + (uint64_t)i * a.ld + coff + 4u * c4);
    const float ge[4] = {gv.x, gv.y, gv.z, gv.w};
    unsigned long long* acc = a.acc[l - 1];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if (cn.row[c] < 0) continue;
        unsigned long long* d = acc + (uint64_t)(uint32_t)cn.row[c] * C + 4u * c4;
        const double w = (double)cn.w[c];
#pragma unroll
        for (int k = 0; k < 4; ++k) xr_fix_add(d + k, w, ge[k], scale);
    }
}

struct NbSampleCvt { const double* scale; const unsigned long long* acc; uint64_t end[4]; float* out[4]; };

__global__ void __launch_bounds__(NB_BLOCK) k_nb_sample_cvt(NbSampleCvt a) {
    const uint64_t e = (uint64_t)blockIdx.x * NB_BLOCK + threadIdx.x;
    if (e >= a.end[3]) return;
    const double scale = a.scale[0];
    const int l = e < a.end[0] ? 0 : (e < a.end[1] ? 1 : (e < a.end[2] ? 2 : 3));
    const uint64_t first = l == 0 ? 0ull : a.end[l - 1];
    a.out[l][e - first] = xr_fix_to_float(a.acc[e], scale);
}

static inline int nb_level_channels(int l) { return l == 0 ? 32 : (l == 1 ? 64 : 128); }

extern "C" size_t xr_nb_sample_backward_workspace_bytes(const uint32_t* n_rows) {
    if (!n_rows) return 0;
    uint64_t el = 0;
    for (int l = 0; l < 4; ++l) el += (uint64_t)n_rows[l] * nb_level_channels(l);
    return (size_t)(XR_FIX_HEAD + el * sizeof(unsigned long long));
}

extern "C" int xr_nb_sample_backward(const float* pts, const float* R, const float* T, const float* min_xyz, float voxel, int D, int H,
                                     int W, const void* const* vols, const uint32_t* n_rows, const float* grad, uint32_t ld, uint32_t n,
                                     void* const* grad_feats, void* workspace, size_t workspace_bytes, void* stream) {
    NbSampleBwd a;
    const int rc = nb_sample_geom(&a.g, pts, R, T, min_xyz, voxel, D, H, W, vols, n);
    if (rc != 0) return rc;
    XR_REQUIRE(n_rows && grad_feats, "null pointer");
    uint64_t end[4], el = 0;
    for (int l = 0; l < 4; ++l) {
        XR_REQUIRE(n_rows[l] <= XR_NB_MAX_CELLS, "too many rows");
        XR_REQUIRE(n_rows[l] == 0 || grad_feats[l] != nullptr, "null gradient rows");
        el += (uint64_t)n_rows[l] * nb_level_channels(l);
        end[l] = el;
    }
    if (el == 0) return 0;
    XR_REQUIRE(workspace != nullptr && ((uintptr_t)workspace & 7u) == 0, "the workspace must be 8-byte aligned");
    if (workspace_bytes < xr_nb_sample_backward_workspace_bytes(n_rows)) { xr_set_error("%s: workspace too small", __func__); return XR_ENOMEM; }
    hipStream_t st = (hipStream_t)stream;
    const XrFixWs ws = xr_fix_ws(workspace);
    XR_HIP(hipMemsetAsync(workspace, 0, XR_FIX_HEAD + (size_t)el * sizeof(unsigned long long), st));
    uint32_t nbm = 1;
    if (n != 0) {
        XR_REQUIRE(grad != nullptr && nb_aligned16(grad) && ld >= XR_NB_FEATURES && (ld & 3u) == 0,
                   "grad must be 16-byte aligned with a row stride >= 352 that is a multiple of 4");
        nbm = xr_div_up((uint64_t)n * NB_Q4, NB_BLOCK);
        if (nbm > XR_FIX_MAX_BMAX) nbm = XR_FIX_MAX_BMAX;
        hipLaunchKernelGGL(k_nb_absmax, dim3(nbm), dim3(NB_BLOCK), 0, st, grad, ld, n, ws.bmax);
        hipLaunchKernelGGL(k_xr_fix_scale, dim3(1), dim3(XR_FIX_BLOCK), 0, st, (const float*)ws.bmax, nbm, n, ws.scale);
        a.grad = grad; a.ld = ld; a.scale = ws.scale;
        for (int l = 0; l < 4; ++l) a.acc[l] = ws.acc + (l == 0 ? 0ull : end[l - 1]);
        hipLaunchKernelGGL(k_nb_sample_bwd, dim3(xr_div_up((uint64_t)n * NB_Q4, NB_BLOCK)), dim3(NB_BLOCK), 0, st, a);
    }
    NbSampleCvt c;
    if (n == 0) hipLaunchKernelGGL(k_xr_fix_scale, dim3(1), dim3(XR_FIX_BLOCK), 0, st, (const float*)ws.bmax, nbm, n, ws.scale);
    c.scale = ws.scale; c.acc = ws.acc;
    for (int l = 0; l < 4; ++l) { c.end[l] = end[l]; c.out[l] = (float*)grad_feats[l]; }
    hipLaunchKernelGGL(k_nb_sample_cvt, dim3(xr_div_up(el, NB_BLOCK)), dim3(NB_BLOCK), 0, st, c);
    XR_LAUNCH_CHECK();
    return 0;
}
